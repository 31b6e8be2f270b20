"""The byte shadow-row filter of long float32 L2 indexes (csrc/ise_scan.hpp BYTE).

Like the fp16 shadow, the byte shadow only changes which rows the scan hands to the re-rank: D and I must be
bit-identical to the fp16 shadow ($ISE_NO_BYTE_FILTER=1) and to the float32 filter ($ISE_NO_HALF_FILTER=1).  Every
case asserts the route of each of the three runs (ise_index_byte_stats, ise_index_half_stats) so that a silent
fall-back cannot pass, and bounds the queries each route sends to the exact scan."""
import threading
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests import byte_filter_ref as br
from tests.knn_checks import (HUGE, assert_knn_identical, assert_nonfinite_range, brute_knn, decoy_ids, int_data,
                              plant_decoys)
from tests.test_exact_l2_gpu import _adversarial, env_knob, no_direct

pytestmark = pytest.mark.gpu
L2 = ko.METRIC_L2
N = 300_000  # past the shadows' threshold (262144 rows)


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _exact(index):
    return index.exact_stats()["exact_scan"]


def _counts(index):
    return index.byte_stats()["byte_batches"], index.half_stats()["half_batches"], _exact(index)


def _three(index, xq, k, route="byte"):
    """(D, I) through the default route, then $ISE_NO_BYTE_FILTER=1, then $ISE_NO_HALF_FILTER=1; asserts that the
    default run took `route` ("byte", "half" or "f32"), that the second read no byte shadow and the third no shadow
    at all, that all three give the same bits, and returns the queries each sent to the exact scan."""
    if route == "auto":  # whichever the index's build-time rule opens: the first search builds it
        index.search(xq, k)
        route = "byte" if index.byte_stats()["byte_route"] else "half"
    outs, exact = [], []
    knobs = (None, "ISE_NO_BYTE_FILTER", "ISE_NO_HALF_FILTER")
    expect = {"byte": [(1, 1), (0, 1), (0, 0)], "half": [(0, 1), (0, 1), (0, 0)], "f32": [(0, 0)] * 3}[route]
    for knob, (want_b, want_h) in zip(knobs, expect):
        b0, h0, e0 = _counts(index)
        if knob is None:
            outs.append(index.search(xq, k))
        else:
            with env_knob(knob):
                outs.append(index.search(xq, k))
        b1, h1, e1 = _counts(index)
        assert (b1 > b0, h1 > h0) == (bool(want_b), bool(want_h)), (route, knob, b1 - b0, h1 - h0)
        exact.append(e1 - e0)
    (D, I), (Dh, Ih), (Df, If) = outs
    for Do, Io, what in ((Dh, Ih, "fp16 shadow"), (Df, If, "float32 filter")):
        assert np.array_equal(I, Io), f"ids differ from the {what}"
        assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), f"distances differ from the {what}"
    return D, I, exact


@pytest.fixture(scope="module")
def uniform_indexes(faiss):
    out = {}
    for d in (64, 100, 512):
        xb = _rng("bu", d).random((N, d), dtype=np.float32)
        index = faiss.IndexFlatL2(d)
        index.add(xb)
        out[d] = (index, xb)
    return out


@pytest.mark.parametrize("d", [64, 100, 512])
@pytest.mark.parametrize("k", [1, 5, 10, 11, 12])
def test_uniform_bit_identical_and_routes(faiss, uniform_indexes, d, k):
    index, xb = uniform_indexes[d]
    rng = _rng("bq", d, k)
    for nq in (1, 16, 48, 128):
        xq = rng.random((nq, d), dtype=np.float32)
        with no_direct():  # k <= 10 and one query tile: the byte shadow; else the fp16 one
            _, _, exact = _three(index, xq, k, "byte" if k <= 10 and nq <= 16 else "half")
        assert exact == [0, 0, 0], ("exact scans (byte, fp16, float32)", d, k, nq, exact)


def test_large_k_and_long_rows_take_no_byte_route(faiss, uniform_indexes):
    index, xb = uniform_indexes[64]
    xq = _rng("bk").random((16, 64), dtype=np.float32)
    _three(index, xq, 32, "f32")
    d = 2048  # rows of more than 1024 floats: no shadow of either kind
    xb = _rng("blong", d).random((N, d), dtype=np.float32)
    long_index = faiss.IndexFlatL2(d)
    long_index.add(xb)
    _, _, exact = _three(long_index, xb[:16] + np.float32(0.01), 10, "f32")
    assert exact == [0, 0, 0]
    with pytest.raises(Exception):
        long_index.byte_row(0)


def test_integer_data_identical_to_exact(faiss):
    n, d, nq, k = N, 64, 16, 10
    rng = _rng("bint")
    xb = int_data("small", rng, n, d)
    xq = int_data("small", rng, nq, d)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D, I, _ = _three(index, xq, k, "auto")
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(D, I, D_ref, I_ref, "byte shadow")


@pytest.mark.parametrize("kind", ["cluster_sorted", "two_far_clusters", "outlier_first", "huge_norm_rows"])
def test_adversarial_bit_identical(faiss, kind):
    rng = _rng("badv", kind)
    n, d, k, nq = N, 128, 10, 16
    xb = _adversarial(kind, rng, n, d)
    xq = (xb[rng.integers(0, n, nq)] + 0.03 * rng.standard_normal((nq, d))).astype(np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    _, _, (xb8, xh, xf) = _three(index, xq, k, "auto")
    assert xb8 <= max(xh, xf), f"{kind}: exact scans byte {xb8}, fp16 {xh}, float32 {xf}"


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf", "all_nan", "huge"])
def test_nonfinite_and_overflowing_rows(faiss, kind):
    n, d, nq, k = N, 64, 8, 10
    rng = _rng("bnf", kind)
    xb, xq = int_data("small", rng, n, d), 20 + int_data("small", rng, nq, d)
    ids = decoy_ids(n)
    if kind == "huge":
        xb[ids] = xq[np.arange(len(ids)) % nq]
        xb[ids, :2] = HUGE
    else:
        plant_decoys(xb, xq, ids, kind)
    assert_nonfinite_range(xb, xq, L2)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D, I, _ = _three(index, xq, k, "auto")
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(D, I, D_ref, I_ref, kind)
    ci, cj = int(ids[0]), 17  # a non-finite row: zero shadow, c_r = e_r = 0
    if kind != "huge":
        assert index.byte_row(ci) == (0.0, 0.0)
    assert index.byte_row(cj)[0] > 0


def test_nonfinite_queries(faiss, uniform_indexes):
    index, xb = uniform_indexes[64]
    xq = xb[:8] + np.float32(0.001)
    xq[1, 3] = np.nan
    xq[2, 0] = np.inf
    xq[3, 5] = -np.inf
    xq[4, :] = np.float32(3e38)  # x - mu stays finite, |x - mu|^2 overflows: every row keyed -FLT_MAX
    D, I, _ = _three(index, xq, 10)  # the same bits as the float32 filter (tests/test_nonfinite_gpu.py checks that one)
    assert np.isfinite(D[[0, 5, 6, 7]]).all()


@pytest.mark.parametrize("kind", ["clustered_uniform", "sparse_relu"])
def test_rule_keeps_the_fp16_route(faiss, kind):
    """Indexes whose rows the byte bound does not suit (bounded clusters: neighbours far closer than typical pairs;
    sparse ReLU-like rows: coarse per-row steps) keep the fp16 shadow by the build-time rule, with the same bits."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from scripts.byte_hard_probe import make

    rng = _rng("brule", kind)
    d = 128
    scale = rng.gamma(2.0, 0.5, d)
    xb = make(kind, rng, N, d, scale)
    xq = make(kind, rng, 16, d, scale)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    index.search(xq, 10)
    assert not index.byte_stats()["byte_route"]
    index.byte_row(0)  # the byte shadow exists; the rule closed its route
    _three(index, xq, 10, "half")


def test_allocation_fallback(faiss, uniform_indexes):
    """A byte shadow that cannot be allocated leaves the fp16 route serving, with the same bits, until reset."""
    _, xb = uniform_indexes[64]
    xq = _rng("balloc").random((16, 64), dtype=np.float32)
    index = faiss.IndexFlatL2(64)
    index.add(xb)
    with env_knob("ISE_FAIL_BYTE_ALLOC"):
        index.search(xq, 10)  # the shadows are allocated here
    assert not index.byte_stats()["byte_route"]
    with pytest.raises(Exception):
        index.byte_row(0)
    index.shadow_row(0)
    _, _, exact = _three(index, xq, 10, "half")
    assert exact == [0, 0, 0]
    index.reset()
    index.add(xb)
    _three(index, xq, 10, "byte")


def test_byte_row_matches_cpu_restatement(faiss):
    n, d = N, 100
    rng = _rng("bmeta")
    xb = rng.random((n, d), dtype=np.float32) * np.float32(3.0)
    xb[7] = xb[:1000].mean(0).astype(np.float32)  # a row next to mu: a small c_r
    xb[8] = xb[8] * np.float32(1e6)  # large entries
    xb[9] = np.float32(1e-41)  # subnormal entries
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    index.search(xb[:16], 5)  # the shadows are built at the first search past the threshold
    mu = np.asarray(index.get_shift(), np.float32)
    for i in (0, 7, 8, 9, 12345, n - 1):
        cr, er = index.byte_row(i)
        cr_r, er_r = br.byte_meta(xb[i], mu)
        assert cr == np.float32(cr_r), (i, cr, cr_r)
        assert er == np.float32(er_r), (i, er, er_r)
    index.shadow_row(0)  # the fp16 shadow is still there


def test_adds_shift_refresh_pinned_and_reset(faiss):
    n, d, k, nq = N, 96, 10, 16
    rng = _rng("blife")
    xb = (rng.random((n + 120_000, d), dtype=np.float32) + np.float32(5.0)).astype(np.float32)
    xq = (xb[rng.integers(0, n, nq)] + 0.01).astype(np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb[:n])
    D, I, exact = _three(index, xq, k)
    assert exact == [0, 0, 0]
    index.add(xb[n:n + 7])                 # rows behind a fixed mu: their byte rows are taken with their norms
    _three(index, xq, k)
    cr, er = index.byte_row(n + 3)
    assert (cr, er) == tuple(np.float32(br.byte_meta(xb[n + 3], np.asarray(index.get_shift(), np.float32))))
    index.add(xb[n + 7:])                  # grown by more than a quarter: new mu, storage growth, everything retaken
    D, I, exact = _three(index, xq, k)
    assert exact == [0, 0, 0]
    D_ref, I_ref = ko.knn_exact(xb, xq, k, L2)
    assert np.array_equal(I, I_ref)
    mu = np.asarray(index.get_shift(), np.float32)
    assert index.byte_row(n + 50_000) == tuple(np.float32(br.byte_meta(xb[n + 50_000], mu)))
    for mu in (np.zeros(d, np.float32), np.full(d, 1e3, np.float32)):  # pinned, and a bad pinned shift
        index.set_shift(mu)
        D2, I2, _ = _three(index, xq, k)
        assert np.array_equal(I2, I) and np.array_equal(D2, D)
        assert index.byte_row(5) == tuple(np.float32(br.byte_meta(xb[5], mu)))
    index.reset()
    index.add(xb[:1000])
    index.search(xq, k)                    # short again: no shadow
    with pytest.raises(Exception):
        index.byte_row(0)
    index.add(xb[1000:])
    D4, I4, _ = _three(index, xq, k)
    assert np.array_equal(I4, I) and np.array_equal(D4, D)


def test_concurrent_streams_and_sharded_keys(faiss):
    import torch

    n, d, k = N, 128, 10
    rng = _rng("bconc")
    xb = rng.random((n, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    qs = [rng.random((nq, d), dtype=np.float32) for nq in (16, 16, 32, 48) * 4]
    with env_knob("ISE_NO_HALF_FILTER"):
        refs = [index.search(q, k) for q in qs]
    b0 = index.byte_stats()["byte_batches"]
    errors = []

    def work(i):
        try:
            st = torch.cuda.Stream()
            tq = torch.from_numpy(qs[i]).cuda()
            with torch.cuda.stream(st):
                outs = [index.search_torch(tq, k) for _ in range(3)]
            st.synchronize()
            for D, I in outs:
                assert np.array_equal(I.cpu().numpy(), refs[i][1]), i
                assert np.array_equal(D.cpu().numpy().view(np.uint32), refs[i][0].view(np.uint32)), i
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(qs))]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert index.byte_stats()["byte_batches"] >= b0 + 3 * sum(len(q) <= 16 for q in qs)  # nq > 16: the fp16 shadow
    whole = faiss.IndexFlatL2(d)
    xb2 = rng.random((2 * N, d), dtype=np.float32)
    whole.add(xb2)
    xq = rng.random((16, d), dtype=np.float32)
    D0, I0 = whole.search(xq, k)
    tq = torch.from_numpy(xq).cuda()
    keys = []
    for r in range(2):
        sh = faiss.IndexFlatL2(d)
        sh.add(xb2[r * N:(r + 1) * N])
        keys.append(sh.search_keys_torch(tq, k, id_base=r * N))
        assert sh.byte_stats()["byte_batches"] == 1
    D1, I1 = faiss.merge_keys_torch(torch.stack(keys), L2)
    assert np.array_equal(I0, I1.cpu().numpy()) and np.array_equal(D0, D1.cpu().numpy())


def test_bench_distribution_needs_no_exact_scan(faiss):
    """The benchmark's own index (1M x 512 uniform) and the same 256 queries as the fp16 shadow's test: every
    certificate holds through the byte shadow at kc = 32, and the results are the other filters' bits."""
    import os
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_inputs

    n, d, k = 1_000_000, 512, 10
    xb, xq16 = make_inputs(n, d, 16, 0, n)
    xq = np.concatenate([xq16, np.random.default_rng(4322).random((240, d), dtype=np.float32)])
    index = faiss.IndexFlatL2(d)
    index.add_torch(torch.from_numpy(xb).cuda())
    tot = np.zeros(3, int)
    for q0 in range(0, 256, 16):
        _, _, exact = _three(index, xq[q0:q0 + 16], k)
        tot += exact
    assert index.byte_stats()["byte_batches"] == 16
    assert tot.tolist() == [0, 0, 0], f"queries sent to the exact scan: byte, fp16, float32 {tot.tolist()}"
