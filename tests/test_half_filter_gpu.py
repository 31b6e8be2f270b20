"""The fp16 shadow-row filter of long float32 L2 indexes (csrc/ise_scan.hpp HALF).

The shadow only changes which rows the scan hands to the re-rank: D and I must be bit-identical to the float32
filter ($ISE_NO_HALF_FILTER=1) and, on integer-valued data, to the exact answer.  Every case asserts the route
(ise_index_half_stats) so that a silent fall-back to the float32 filter cannot pass."""
import threading
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests import half_filter_ref as hr
from tests.knn_checks import (HUGE, assert_knn_identical, assert_knn_matches, assert_nonfinite_range, brute_knn, decoy_ids, int_data,
                              plant_decoys)
from tests.test_exact_l2_gpu import _adversarial, env_knob, no_direct

pytestmark = pytest.mark.gpu
L2 = ko.METRIC_L2
N = 300_000  # past the shadow's threshold (262144 rows)


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def no_half():
    return env_knob("ISE_NO_HALF_FILTER")


def _exact(index):
    return index.exact_stats()["exact_scan"]


def _both(index, xq, k, half=True):
    """(D, I) through the shadow (half=False: the batch must keep the float32 filter by the plan's own rule), then
    through the float32 filter ($ISE_NO_HALF_FILTER=1); asserts the route of each.  Also returns the
    queries each route sent to the exact scan (the filters differ only in how tight their keys are: a loose one
    gives the same bits through the exact scan, so the tests bound these counts too)."""
    h0, e0 = index.half_stats()["half_batches"], _exact(index)
    D, I = index.search(xq, k)
    h1, e1 = index.half_stats()["half_batches"], _exact(index)
    assert (h1 > h0) == half, "the batch did not read the shadow rows" if half else "the batch read the shadow rows"
    with no_half():
        Df, If = index.search(xq, k)
    assert index.half_stats()["half_batches"] == h1, "ISE_NO_HALF_FILTER=1 still read the shadow rows"
    return D, I, Df, If, e1 - e0, _exact(index) - e1


def _same(D, I, Df, If, what=""):
    assert np.array_equal(I, If), f"ids differ from the float32 filter {what}"
    assert np.array_equal(D.view(np.uint32), Df.view(np.uint32)), f"distances differ from the float32 filter {what}"


@pytest.fixture(scope="module")
def uniform_indexes(faiss):
    out = {}
    for d in (64, 100, 512):
        xb = _rng("u", d).random((N, d), dtype=np.float32)
        index = faiss.IndexFlatL2(d)
        index.add(xb)
        out[d] = (index, xb)
    return out


@pytest.mark.parametrize("d", [64, 100, 512])
@pytest.mark.parametrize("k", [1, 10, 32, 100])
def test_uniform_bit_identical_to_float32_filter(faiss, uniform_indexes, d, k):
    index, xb = uniform_indexes[d]
    rng = _rng("q", d, k)
    for nq in (1, 5, 16, 48, 128):
        xq = rng.random((nq, d), dtype=np.float32)
        with no_direct():  # k + 4 <= 16: the shadow; larger k keeps the float32 filter
            D, I, Df, If, xh, xf = _both(index, xq, k, half=k + 4 <= 16)
        _same(D, I, Df, If, (d, k, nq))
        assert (xh, xf) == (0, 0), ("exact scans (shadow, float32 filter)", d, k, nq, xh, xf)


def test_long_rows_keep_the_float32_filter(faiss):
    """Rows of more than 1024 floats get no shadow (its bound is too loose there: DESIGN.md 5.0a)."""
    n, d, k = N, 2048, 10
    rng = _rng("long", d)
    xb = rng.random((n, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    xq = rng.random((16, d), dtype=np.float32)
    D, I, Df, If, xh, xf = _both(index, xq, k, half=False)
    _same(D, I, Df, If)
    assert (xh, xf) == (0, 0)
    with pytest.raises(Exception):
        index.shadow_row(0)


def test_lds_limit_rows_keep_the_float32_filter(faiss):
    """d = 2177 .. 2240: the float32 filter's one-tile image fits the 160 KiB LDS, a shadow kernel's (hi | lo query
    halves padded to 32-half steps, e_q, sh) would not.  Such an index builds no shadow and keeps searching."""
    n, d, k = 270_000, 2240, 10
    rng = _rng("ldslimit", d)
    xb = rng.random((n, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    xq = rng.random((16, d), dtype=np.float32)
    e0 = _exact(index)
    D, I = index.search(xq, k)
    assert index.half_stats()["half_batches"] == 0
    with pytest.raises(Exception):
        index.shadow_row(0)
    with no_half():
        Df, If = index.search(xq, k)
    _same(D, I, Df, If)
    assert _exact(index) == e0
    D1, I1 = index.search(xq[:3], 10)  # and a sample against float64 brute force
    rows = xb[I1.reshape(-1)].astype(np.float64).reshape(3, k, d)
    assert np.allclose(((rows - xq[:3, None, :].astype(np.float64)) ** 2).sum(-1), D1, rtol=1e-5)


def test_integer_data_identical_to_exact(faiss):
    n, d, nq, k = N, 64, 40, 12  # kc = 16: the largest k the shadow takes, block lists without a cut window
    rng = _rng("int")
    xb = int_data("small", rng, n, d)
    xq = int_data("small", rng, nq, d)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D, I, Df, If, xh, xf = _both(index, xq, k)
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(D, I, D_ref, I_ref, "shadow")
    assert_knn_identical(Df, If, D_ref, I_ref, "float32 filter")


@pytest.mark.parametrize("kind", ["cluster_sorted", "two_far_clusters", "outlier_first", "huge_norm_rows"])
def test_adversarial_bit_identical(faiss, kind):
    rng = _rng("adv", kind)
    n, d, k, nq = N, 128, 10, 16
    xb = _adversarial(kind, rng, n, d)
    xq = (xb[rng.integers(0, n, nq)] + 0.03 * rng.standard_normal((nq, d))).astype(np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D, I, Df, If, xh, xf = _both(index, xq, k)
    _same(D, I, Df, If, kind)
    assert xh <= xf, f"{kind}: the shadow sent {xh} queries to the exact scan, the float32 filter {xf}"
    D_ref, I_ref = ko.knn_exact(xb, xq, k, L2)
    n_mism = assert_knn_matches(D, I, D_ref, I_ref, xb, xq, L2, gap=ko.kth_gap(xb, xq, k, L2))
    assert n_mism == 0 or kind == "two_far_clusters"  # as test_exact_l2_gpu: only float32 near-ties may differ there


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf", "all_nan", "huge"])
def test_nonfinite_and_overflowing_rows(faiss, kind):
    n, d, nq, k = N, 64, 8, 10
    rng = _rng("nf", kind)
    xb, xq = int_data("small", rng, n, d), 20 + int_data("small", rng, nq, d)
    ids = decoy_ids(n)
    if kind == "huge":
        xb[ids] = xq[np.arange(len(ids)) % nq]
        xb[ids, :2] = HUGE  # ~2^129 from every query: overflows in any order (assert_nonfinite_range)
    else:
        plant_decoys(xb, xq, ids, kind)
    assert_nonfinite_range(xb, xq, L2)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    D, I, Df, If, xh, xf = _both(index, xq, k)
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(D, I, D_ref, I_ref, kind)
    _same(D, I, Df, If, kind)


def test_shadow_row_matches_cpu_restatement(faiss):
    n, d = N, 100
    rng = _rng("meta")
    xb = rng.random((n, d), dtype=np.float32) * np.float32(3.0)
    xb[7] = xb[:1000].mean(0).astype(np.float32)  # a row next to mu: small |y - mu|, a large s_r
    xb[8] = xb[8] * np.float32(1e6)  # large entries: a negative s_r
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    index.search(xb[:16], 5)  # the shadow is built at the first search past the threshold
    mu = index.get_shift()
    for i in (0, 7, 8, 12345, n - 1):
        nu, e, s = index.shadow_row(i)
        nu_r, e_r, s_r = hr.shadow_meta(xb[i], np.asarray(mu, np.float32))
        assert s == s_r, (i, s, s_r)
        assert abs(nu - nu_r) <= 2.0 ** -23 * nu_r, (i, nu, nu_r)  # float64 sums in another order, rounded once
        assert e >= e_r and e <= e_r * (1 + 1e-6) + 1e-44, (i, e, e_r)


def test_adds_shift_refresh_pinned_and_reset(faiss):
    n, d, k, nq = N, 96, 10, 16
    rng = _rng("life")
    xb = (rng.random((n + 120_000, d), dtype=np.float32) + np.float32(5.0)).astype(np.float32)
    xq = (xb[rng.integers(0, n, nq)] + 0.01).astype(np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb[:n])
    D, I, Df, If, xh, xf = _both(index, xq, k)
    _same(D, I, Df, If, "first")
    assert (xh, xf) == (0, 0)
    index.add(xb[n:n + 7])                 # rows behind a fixed mu: their shadow is taken with their norms
    D, I, Df, If, xh, xf = _both(index, xq, k)
    _same(D, I, Df, If, "small add")
    index.add(xb[n + 7:])                  # grown by more than a quarter: new mu, every norm and shadow row retaken
    up0 = index.exact_stats()["shift_updates"]
    D, I, Df, If, xh, xf = _both(index, xq, k)
    _same(D, I, Df, If, "large add")
    assert (xh, xf) == (0, 0)
    D_ref, I_ref = ko.knn_exact(xb, xq, k, L2)
    assert np.array_equal(I, I_ref)
    assert index.exact_stats()["shift_updates"] >= up0
    for mu in (np.zeros(d, np.float32), np.full(d, 1e3, np.float32)):  # pinned, and a bad pinned shift
        index.set_shift(mu)
        D2, I2, Df2, If2, xh, xf = _both(index, xq, k)
        _same(D2, I2, Df2, If2, "pinned")
        assert np.array_equal(I2, I) and np.array_equal(D2, D)
    index.reset()
    index.add(xb[:1000])
    D3, I3 = index.search(xq, k)           # short again: no shadow
    with pytest.raises(Exception):
        index.shadow_row(0)
    index.add(xb[1000:])
    D4, I4, Df4, If4, xh, xf = _both(index, xq, k)
    assert np.array_equal(I4, I) and np.array_equal(D4, D)


def test_concurrent_streams_and_sharded_keys(faiss):
    import torch

    n, d, k = N, 128, 10
    rng = _rng("conc")
    xb = rng.random((n, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    qs = [rng.random((nq, d), dtype=np.float32) for nq in (16, 16, 32, 48) * 4]
    with no_half():
        refs = [index.search(q, k) for q in qs]
    h0 = index.half_stats()["half_batches"]
    errors = []

    def work(i):
        try:
            st = torch.cuda.Stream()
            tq = torch.from_numpy(qs[i]).cuda()
            with torch.cuda.stream(st):
                outs = [index.search_torch(tq, k) for _ in range(3)]
            st.synchronize()
            for D, I in outs:
                _same(D.cpu().numpy(), I.cpu().numpy(), refs[i][0], refs[i][1], i)
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(qs))]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert index.half_stats()["half_batches"] >= h0 + 3 * len(qs)
    # sharded keys path: two shards past the threshold, merged == one index
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
        assert sh.half_stats()["half_batches"] == 1
    D1, I1 = faiss.merge_keys_torch(torch.stack(keys), L2)
    assert np.array_equal(I0, I1.cpu().numpy()) and np.array_equal(D0, D1.cpu().numpy())


def test_bench_distribution_needs_no_exact_scan(faiss):
    """The benchmark's own index (1M x 512 uniform, default_rng 1234) and 256 queries: every certificate holds
    through the shadow, and the results are the float32 filter's bits."""
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
    outs = []
    e0 = index.exact_stats()["exact_scan"]
    for q0 in range(0, 256, 16):
        outs.append(index.search(xq[q0:q0 + 16], k))
    e_half = index.exact_stats()["exact_scan"] - e0
    with no_half():
        for j, q0 in enumerate(range(0, 256, 16)):
            _same(*outs[j], *index.search(xq[q0:q0 + 16], k), q0)
    e_f32 = index.exact_stats()["exact_scan"] - e0 - e_half
    assert index.half_stats()["half_batches"] == 16
    assert (e_half, e_f32) == (0, 0), f"queries sent to the exact scan: shadow {e_half}, float32 filter {e_f32}"
