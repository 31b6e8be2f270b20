"""The per-block phases of the exchange kernels (csrc/ise_scan.hpp: boot, threshold exchange, final phase filtered by the
exchange bound) change which keys a block ranks and writes, never the merged keys: D and I stay
bit-identical to the fp16 shadow ($ISE_NO_BYTE_FILTER=1) and to the float32 filter ($ISE_NO_HALF_FILTER=1), with the
route of every run asserted (tests/test_byte_filter_gpu.py, _three)."""
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.knn_checks import HUGE, assert_knn_identical, assert_nonfinite_range, brute_knn, decoy_ids, int_data, plant_ties
from tests.test_byte_filter_gpu import _three
from tests.test_exact_l2_gpu import _adversarial, env_knob, no_direct

pytestmark = pytest.mark.gpu
L2 = ko.METRIC_L2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 500_000  # long enough for every wave of a block to read the exchange (see _tiles_per_block)


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _tiles_per_block(n):
    """The streaming kernel's split of a long index at one query tile (make_plan, csrc/ise_knn.hip): two 8-wave
    blocks per CU, ceil(tiles / blocks) row tiles of 16 rows each."""
    import torch

    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (n + 15) // 16
    nb = min(slots, (tiles + 7) // 8)
    return (tiles + nb - 1) // nb


def _waves_reading_the_exchange(n):
    """Wave w of a block reads the exchange after its first tile iff 4 W = 32 or more of the block's tiles lie
    behind its next one: tiles_per_block - 8 - w >= 32."""
    tpb = _tiles_per_block(n)
    return sum(tpb - 8 - w >= 32 for w in range(8))


def test_bench_distribution_k1_k10_sampled_nq(faiss):
    """(a) the benchmark's index, k = 1 and 10, batches of 1 .. 16 queries: the byte route, the other filters' bits,
    nothing sent to the exact scan."""
    import torch

    sys.path.insert(0, ROOT)
    from bench import make_inputs

    n, d = 1_000_000, 512
    assert _waves_reading_the_exchange(n) == 8
    xb, xq16 = make_inputs(n, d, 16, 0, n)
    index = faiss.IndexFlatL2(d)
    index.add_torch(torch.from_numpy(xb).cuda())
    extra = _rng("bp", "a").random((16, d), dtype=np.float32)
    for k in (1, 10):
        for nq in (1, 2, 7, 15, 16):
            for xq in (xq16[:nq], extra[16 - nq:]):
                with no_direct():
                    _, _, exact = _three(index, np.ascontiguousarray(xq), k, "byte")
                assert exact == [0, 0, 0], (k, nq, exact)


@pytest.mark.parametrize("n", [262_145, 265_000, 270_000, 350_000])
def test_blocks_too_short_for_the_exchange(faiss, n):
    """(b) just above the shadows' threshold a block has 33 row tiles: after a wave's first tile fewer than 32 are
    left, no wave reads the exchange, no bound exists and the final phase is the unfiltered one.  At 350 000 rows
    (43 tiles per block) waves 0 .. 3 read it and waves 4 .. 7 do not: queries with and without a bound in one block."""
    d, k = 512, 10
    readers = _waves_reading_the_exchange(n)
    assert readers == (4 if n == 350_000 else 0), (n, _tiles_per_block(n), readers)
    rng = _rng("bp", "b", n)
    xb = rng.random((n, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    for kk in (1, k):
        xq = rng.random((16, d), dtype=np.float32)
        _, _, (xb8, xh, xf) = _three(index, xq, kk, "byte")
        # (a certificate may fail on any route -- the exact scan then gives the same bits; the byte route's lists
        # must not make it fail more often than the others')
        assert xb8 <= max(xh, xf), f"{n}, k = {kk}: exact scans byte {xb8}, fp16 {xh}, float32 {xf}"
    D, I, _ = _three(index, xb[1000:1016] + np.float32(0.001), k, "byte")
    assert np.array_equal(I[:, 0], np.arange(1000, 1016))


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import image_search_engine_amd.faiss_compat as fc
rng = np.random.default_rng(77)
xb = rng.random(({n}, {d}), dtype=np.float32)
xq = rng.random((16, {d}), dtype=np.float32)
index = fc.IndexFlatL2({d})
index.add(xb)
out = {{}}
for k in (1, 10):
    b0 = index.byte_stats()["byte_batches"]
    D, I = index.search(xq, k)
    assert index.byte_stats()["byte_batches"] == b0 + 1
    out["D%d" % k], out["I%d" % k] = D, I
np.savez({path!r}, **out)
"""


def test_without_the_exchange(faiss, tmp_path):
    """(c) $ISE_NO_XCHG=1 (read once per process, so a child process): no entry is published or read, every final
    phase is the unfiltered one, and the results are the bits of this process, where the exchange runs."""
    n, d = N, 128
    outs = {}
    for knob in ("0", "1"):
        path = str(tmp_path / f"xchg{knob}.npz")
        env = dict(os.environ, ISE_NO_XCHG=knob)
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, n=n, d=d, path=path)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[knob] = np.load(path)
    for key in ("D1", "I1", "D10", "I10"):
        a, b = outs["0"][key], outs["1"][key]
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b), key
    rng = np.random.default_rng(77)  # and both are the float32 filter's bits
    xb = rng.random((n, d), dtype=np.float32)
    xq = rng.random((16, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    for k in (1, 10):
        D, I, _ = _three(index, xq, k, "byte")
        assert np.array_equal(I, outs["1"]["I%d" % k]) and np.array_equal(D, outs["1"]["D%d" % k])


def test_adversarial_kinds_on_the_byte_route(faiss):
    """(d) the adversarial indexes of the byte filter's own test, long enough for the exchange: whichever route the
    build-time rule opens, the three filters agree; at least one of the kinds runs the byte kernel."""
    n, d, k, nq = N, 128, 10, 16
    routes = {}
    for kind in ("cluster_sorted", "two_far_clusters", "outlier_first", "huge_norm_rows"):
        rng = _rng("bp", "d", kind)
        xb = _adversarial(kind, rng, n, d)
        xq = (xb[rng.integers(0, n, nq)] + 0.03 * rng.standard_normal((nq, d))).astype(np.float32)
        index = faiss.IndexFlatL2(d)
        index.add(xb)
        _three(index, xq, k, "auto")
        routes[kind] = bool(index.byte_stats()["byte_route"])
        del index
    assert any(routes.values()), routes


def test_rows_and_queries_keyed_minus_flt_max(faiss):
    """(d) rows whose shifted norm overflows are keyed -FLT_MAX (always candidates), and for a query whose own norm
    overflows every row is: the exchange bound is then ord(-FLT_MAX) itself and every id at that score stays."""
    n, d, nq, k = N, 64, 8, 10
    rng = _rng("bp", "huge")
    xb, xq = int_data("small", rng, n, d), 20 + int_data("small", rng, nq, d)
    ids = decoy_ids(n)
    xb[ids] = xq[np.arange(len(ids)) % nq]
    xb[ids, :2] = HUGE
    assert_nonfinite_range(xb, xq, L2)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D, I, _ = _three(index, xq, k, "auto")
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(D, I, D_ref, I_ref, "rows keyed -FLT_MAX")
    xu = _rng("bp", "hugeq").random((n, d), dtype=np.float32)
    uni = faiss.IndexFlatL2(d)
    uni.add(xu)
    xq2 = xu[:8] + np.float32(0.001)
    xq2[4, :] = np.float32(3e38)  # x - mu stays finite, |x - mu|^2 overflows: every row keyed -FLT_MAX
    xq2[2, 0] = np.inf
    D2, I2, _ = _three(uni, xq2, k)
    assert np.isfinite(D2[[0, 1, 3, 5, 6, 7]]).all()


def test_integer_data_with_many_equal_distances(faiss):
    """(e) integer rows: distances tie in large groups, across blocks too (a planted group of copies of one row far
    apart in the index); ids and distance bits are those of the exact answer."""
    n, d, nq, k = N, 64, 16, 10
    rng = _rng("bp", "int")
    xb = int_data("small", rng, n, d)
    xq = int_data("small", rng, nq, d)
    plant_ties(xb, 5, [6, 7, 2047, 2048, n // 2, n - 1])
    xq[0] = xb[5]
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    for kk in (1, k):
        D, I, _ = _three(index, xq, kk, "auto")
        assert_knn_identical(D, I, D_ref[:, :kk], I_ref[:, :kk], f"integer data, k = {kk}")
    assert I_ref[0, :7].tolist() == [5, 6, 7, 2047, 2048, n // 2, n - 1]


def test_sixteen_streams_share_the_workspace_slots(faiss):
    """(f) 16 streams issue byte-route batches at once over the six workspace slots: every result equals the
    one-stream result.  An exchange entry an earlier launch left in the same slot carries another launch sequence and
    counts as absent, so no block filters by a bound that is not of its own launch."""
    import torch

    n, d, k = N, 128, 10
    rng = _rng("bp", "conc")
    xb = rng.random((n, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    # batches near rows (small distances: a bound of such a launch would empty the lists of a far batch) and far ones
    qs = [(xb[rng.integers(0, n, 16)] + np.float32(0.001)).astype(np.float32) if i % 2 else
          rng.random((16, d), dtype=np.float32) * np.float32(3.0) for i in range(16)]
    refs = [index.search(q, k) for q in qs]
    with env_knob("ISE_NO_HALF_FILTER"):
        for q, (D, I) in zip(qs, refs):
            Df, If = index.search(q, k)
            assert np.array_equal(I, If) and np.array_equal(D.view(np.uint32), Df.view(np.uint32))
    b0 = index.byte_stats()["byte_batches"]
    errors = []

    def work(i):
        try:
            st = torch.cuda.Stream()
            tq = torch.from_numpy(qs[i]).cuda()
            with torch.cuda.stream(st):
                outs = [index.search_torch(tq, k) for _ in range(6)]
            st.synchronize()
            for D, I in outs:
                assert np.array_equal(I.cpu().numpy(), refs[i][1]), i
                assert np.array_equal(D.cpu().numpy().view(np.uint32), refs[i][0].view(np.uint32)), i
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(16)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert index.byte_stats()["byte_batches"] == b0 + 16 * 6
