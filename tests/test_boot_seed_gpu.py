"""The seeded boot of the byte shadow scan on the GPU (csrc/ise_scan.hpp, NBOOT; model:
tests/test_boot_seed.py).  A block whose every wave reads the exchange keeps the keys of its first 256 rows (two row
tiles per wave) and seeds its list from the exchange bound instead of cutting; every other block boots with the cut.
Which keys a block holds changes, the merged keys never: D and I are the bits of the fp16 shadow and of the float32
filter, the route of every run is asserted (_three), and the byte route sends no more queries to the exact scan -- which
would hide a broken list -- than the other two."""
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.knn_checks import HUGE, assert_knn_identical, assert_nonfinite_range, brute_knn, decoy_ids, int_data, plant_ties
from tests.test_block_phases_gpu import _tiles_per_block, _waves_reading_the_exchange
from tests.test_byte_filter_gpu import _three
from tests.test_exact_l2_gpu import no_direct

pytestmark = pytest.mark.gpu
L2 = ko.METRIC_L2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_MIXED, D = 500_000, 350_000, 64
WINDOW = 256  # rows of a seeded block's boot window
KB = 32       # block-list slots of the byte route (kc = 32)


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _index(faiss, xb):
    index = faiss.IndexFlatL2(xb.shape[1])
    index.add(xb)
    return index


def _seeded(n):
    """Every wave of a full block has 4 W = 32 row tiles behind its two window tiles: the block takes the seeded boot."""
    return _tiles_per_block(n) - 7 - 16 >= 32


def _block_row0(n, b):
    return b * 16 * _tiles_per_block(n)


def _no_more_exact_scans(exact, what):
    xb8, xh, xf = exact
    assert xb8 <= max(xh, xf), f"{what}: exact scans byte {xb8}, fp16 {xh}, float32 {xf}"


@pytest.fixture(scope="module")
def uniform(faiss):
    out = {}
    for n in (N, N_MIXED):
        xb = _rng("bs", "uniform", n).random((n, D), dtype=np.float32)
        out[n] = (_index(faiss, xb), xb)
    return out


def test_shapes_take_the_paths_they_are_meant_to():
    assert _seeded(N) and _waves_reading_the_exchange(N) == 8
    assert not _seeded(N_MIXED) and _waves_reading_the_exchange(N_MIXED) == 4


@pytest.mark.parametrize("n", [N, N_MIXED])
@pytest.mark.parametrize("k", [1, 10])
def test_uniform_rows(uniform, n, k):
    """1. uniform rows: the three routes' bits, nothing sent to the exact scan on any of them."""
    index, xb = uniform[n]
    rng = _rng("bs", "q", n, k)
    for nq in (1, 2, 7, 15, 16):
        xq = rng.random((nq, D), dtype=np.float32)
        with no_direct():
            _, _, exact = _three(index, xq, k, "byte")
        assert exact == [0, 0, 0], (n, k, nq, exact)


@pytest.mark.parametrize("n", [N - 5, N_MIXED - 5])
def test_neighbours_planted_around_the_window(faiss, n):
    """2. the ten true neighbours of a query sit inside one block's boot window, end at the window's last row, start
    at the first row behind it, lie in the block's last tile, or in the index's last (partial) tile.  Planted at
    squared distances below 1e-3 among uniform rows (nearest ~ 3): the float32 route certifies them alone."""
    k = 10
    assert n % 16 and _seeded(n) == _seeded(n + 5)
    rng = _rng("bs", "plant", n)
    xb = rng.random((n, D), dtype=np.float32)
    tpb = _tiles_per_block(n)
    starts = [_block_row0(n, 3) + 40, _block_row0(n, 5) + WINDOW - k, _block_row0(n, 7) + WINDOW,
              _block_row0(n, 9) + 16 * tpb - k, n - k]
    xq = rng.random((len(starts), D), dtype=np.float32)
    want = []
    for j, s in enumerate(starts):
        order = rng.permutation(k)  # distance rank of the rows s .. s + k - 1
        for i in range(k):
            xb[s + i] = xq[j] + np.float32(0.001 * (1 + order[i])) * rng.standard_normal(D).astype(np.float32)
        want.append(np.arange(s, s + k))
    index = _index(faiss, xb)
    for kk in (1, k):
        with no_direct():
            Dk, Ik, exact = _three(index, xq, kk, "byte")
        _no_more_exact_scans(exact, f"planted, k = {kk}")
        D_ref, I_ref = brute_knn(xb, xq, kk, L2)
        assert np.array_equal(Ik, I_ref)
        for j in range(len(starts)):
            assert set(Ik[j]) <= set(want[j]), (j, Ik[j], want[j])


def test_more_window_keys_under_the_bound_than_the_list_holds(faiss):
    """3. integer data (ties are exact): 100 copies of a near row inside one boot window (more than kb: the block
    cuts exactly), exactly kb copies, and copies spread over two blocks' windows."""
    n, k = N, 10
    rng = _rng("bs", "overflow")
    xb = int_data("small", rng, n, D)
    srcs = [_block_row0(n, 4) + 3, _block_row0(n, 8) + 100, _block_row0(n, 12) + 200]
    xb[srcs] += np.float32(16)  # three rows apart from the rest and from each other
    xb[srcs[1], :8] += np.float32(5)
    xb[srcs[2], 8:16] += np.float32(5)
    plant_ties(xb, srcs[0], srcs[0] + 1 + np.arange(100))
    plant_ties(xb, srcs[1], srcs[1] + 1 + np.arange(KB - 1))
    plant_ties(xb, srcs[2], np.concatenate([srcs[2] + 1 + np.arange(50), _block_row0(n, 13) + 5 + np.arange(60)]))
    xq = xb[srcs].copy()
    index = _index(faiss, xb)
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert (D_ref == 0).all()
    for kk in (1, k):
        Dk, Ik, exact = _three(index, xq, kk, "byte")
        _no_more_exact_scans(exact, f"copies, k = {kk}")
        assert_knn_identical(Dk, Ik, D_ref[:, :kk], I_ref[:, :kk], f"copies in the boot window, k = {kk}")


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import image_search_engine_amd.faiss_compat as fc
xb = np.load({xb!r}); xq = np.load({xq!r})
index = fc.IndexFlatL2(xb.shape[1])
index.add(xb)
b0, e0 = index.byte_stats()["byte_batches"], index.exact_stats()["exact_scan"]
D, I = index.search(xq, 10)
assert index.byte_stats()["byte_batches"] == b0 + 1
np.savez({path!r}, D=D, I=I, exact=index.exact_stats()["exact_scan"] - e0)
"""


def test_without_the_exchange_in_a_child(uniform, tmp_path):
    """4. $ISE_NO_XCHG=1 (read once per process): every block boots with the cut; the bits are those of this process,
    and neither process sends a query to the exact scan."""
    index, xb = uniform[N]
    xq = _rng("bs", "noxchg").random((16, D), dtype=np.float32)
    np.save(tmp_path / "xb.npy", xb)
    np.save(tmp_path / "xq.npy", xq)
    path = str(tmp_path / "out.npz")
    src = _CHILD.format(root=ROOT, xb=str(tmp_path / "xb.npy"), xq=str(tmp_path / "xq.npy"), path=path)
    r = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, ISE_NO_XCHG="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(path)
    assert int(out["exact"]) == 0, "the byte route without the exchange sent queries to the exact scan"
    Dk, Ik, exact = _three(index, xq, 10, "byte")
    assert exact == [0, 0, 0]
    assert np.array_equal(Ik, out["I"]) and np.array_equal(Dk.view(np.uint32), out["D"].view(np.uint32))


def test_sixteen_streams_six_batches(uniform):
    """5. 16 streams x 6 batches over the six workspace slots, near and far batches alternating: an entry another
    launch left in a slot carries another sequence and seeds nothing.  A list emptied by a foreign bound would fail the
    certificate and come back with the right bits from the exact scan, so the count of queries sent there is bounded:
    the 96 threaded batches send no more than 6 x what the larger of the other two routes sent for the 16 batches."""
    import torch

    index, xb = uniform[N]
    k = 10
    rng = _rng("bs", "conc")
    qs = [(xb[rng.integers(0, N, 16)] + np.float32(0.001)).astype(np.float32) if i % 2 else
          rng.random((16, D), dtype=np.float32) * np.float32(3.0) for i in range(16)]
    refs, other = [], [0, 0]
    for q in qs:  # sequential: the byte route asserted, the three routes' bits equal, each route's exact scans
        Dr, Ir, (xb8, xh, xf) = _three(index, q, k, "byte")
        assert xb8 <= max(xh, xf), f"sequential batch: exact scans byte {xb8}, fp16 {xh}, float32 {xf}"
        refs.append((Dr, Ir))
        other[0] += xh
        other[1] += xf
    b0, e0 = index.byte_stats()["byte_batches"], index.exact_stats()["exact_scan"]
    errors = []

    def work(i):
        try:
            st = torch.cuda.Stream()
            tq = torch.from_numpy(qs[i]).cuda()
            with torch.cuda.stream(st):
                outs = [index.search_torch(tq, k) for _ in range(6)]
            st.synchronize()
            for Do, Io in outs:
                assert np.array_equal(Io.cpu().numpy(), refs[i][1]), i
                assert np.array_equal(Do.cpu().numpy().view(np.uint32), refs[i][0].view(np.uint32)), i
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(16)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert index.byte_stats()["byte_batches"] == b0 + 16 * 6
    sent = index.exact_stats()["exact_scan"] - e0
    assert sent <= 6 * max(other), f"threaded byte batches sent {sent} queries to the exact scan, fp16 / float32 {other}"


def test_rows_keyed_minus_flt_max_and_an_overflowing_query(faiss, uniform):
    """6. rows whose shifted norm overflows are keyed -FLT_MAX; for a query whose own norm overflows every row is:
    the bound is ord(-FLT_MAX) and every id at that score stays (far more than kb of them in every window).
    The first half runs whichever shadow the index's build-time rule opens for the HUGE rows (_three asserts that
    route; the seeded kernel runs only if it is the byte one); the second half, the overflowing query on uniform rows,
    is asserted to take the byte route, hence the seeded boot.  That query's own row is checked for the three routes'
    equal bits only."""
    n, nq, k = N, 8, 10
    rng = _rng("bs", "huge")
    xb, xq = int_data("small", rng, n, D), 20 + int_data("small", rng, nq, D)
    ids = decoy_ids(n)
    xb[ids] = xq[np.arange(len(ids)) % nq]
    xb[ids, :2] = HUGE
    assert_nonfinite_range(xb, xq, L2)
    index = _index(faiss, xb)
    Dk, Ik, exact = _three(index, xq, k, "auto")
    _no_more_exact_scans(exact, "rows keyed -FLT_MAX")
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(Dk, Ik, D_ref, I_ref, "rows keyed -FLT_MAX")
    uni, xu = uniform[N]
    xq2 = xu[:8] + np.float32(0.001)
    xq2[4, :] = np.float32(3e38)  # x - mu stays finite, |x - mu|^2 overflows: every row keyed -FLT_MAX
    D2, I2, exact = _three(uni, xq2, k, "byte")
    _no_more_exact_scans(exact, "a query whose norm overflows")
    assert np.isfinite(D2[[0, 1, 2, 3, 5, 6, 7]]).all()
    assert np.array_equal(I2[[0, 1, 2, 3, 5, 6, 7], 0], np.array([0, 1, 2, 3, 5, 6, 7]))
