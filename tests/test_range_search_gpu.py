"""GPU tests of range search (csrc/ise_range.hpp): every result is checked for shape (lims monotone, ids
ascending and unique per query), every case asserts the range counters, and the distances are compared bit
for bit -- with the passing rows of search() on the same index, or with an exact brute force on integer data."""
import os
import threading

import numpy as np
import pytest

from image_search_engine_amd import _native
from image_search_engine_amd import faiss_compat as faiss
from tests.knn_checks import HUGE, int_data, poison
from tests.range_ref import IP, L2, assert_range_identical, assert_range_shape, filter_search

pytestmark = pytest.mark.gpu

STORAGES = [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")]


def make_index(xb, metric, storage):
    idx = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    idx.add(xb)
    return idx


def checked_range(idx, xq, radius, overflow=False):
    before = idx.range_stats()
    lims, D, I = idx.range_search(xq, radius)
    after = idx.range_stats()
    assert_range_shape(lims, D, I, len(xq), idx.ntotal)
    nb = (len(xq) + 255) // 256 if (len(xq) and idx.ntotal) else 0
    assert after["range_batches"] - before["range_batches"] == nb
    if overflow:
        assert after["range_overflow_batches"] - before["range_overflow_batches"] >= 1
    return lims, D, I


SHAPES = [(1000, 2048, 1), (2048, 512, 16), (777, 100, 5), (1, 1, 1), (2000, 64, 70)]


@pytest.mark.parametrize("metric,storage", STORAGES)
@pytest.mark.parametrize("n,d,nq", SHAPES)
def test_consistent_with_search(metric, storage, n, d, nq):
    rng = np.random.default_rng(n + d + nq)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    if metric == IP and storage == "bf16":
        faiss.normalize_L2(xb)
        faiss.normalize_L2(xq)
    idx = make_index(xb, metric, storage)
    Ds, Is = idx.search(xq, n)
    assert (Is >= 0).all()
    flat = Ds.ravel()
    radii = [float(np.quantile(flat, qq)) for qq in (0.01, 0.1, 0.5)]
    radii += [float(flat[len(flat) // 3]), np.inf, -np.inf, np.nan]
    for r in radii:
        got = checked_range(idx, xq, r)
        want = filter_search(Ds, Is, r, metric)
        assert_range_identical(got, want, f"radius {r}")
    # an attained distance is excluded (strict comparison)
    r = float(Ds[0, min(3, n - 1)])
    lims, D, I = checked_range(idx, xq, r)
    assert not (D[: int(lims[1])] == np.float32(r)).any()


def _int_brute(xb, xq, radius, metric):
    a, b = xb.astype(np.int64), xq.astype(np.int64)
    s = ((b[:, None, :] - a[None]) ** 2).sum(-1) if metric == L2 else b @ a.T
    lims, Ds, Is = [0], [], []
    for row in s:
        ids = np.nonzero(row < radius if metric == L2 else row > radius)[0]
        Ds.append(row[ids].astype(np.float32))
        Is.append(ids)
        lims.append(lims[-1] + len(ids))
    return np.asarray(lims, np.uint64), np.concatenate(Ds), np.concatenate(Is).astype(np.int64)


@pytest.mark.parametrize("metric,storage", STORAGES)
@pytest.mark.parametrize("kind", ["binary", "small", "signed"])
def test_integer_data_exact(metric, storage, kind):
    rng = np.random.default_rng(11)
    xb = int_data(kind, rng, 6000, 48)
    xq = int_data(kind, rng, 20, 48)
    xb[100:3100] = xq[0]  # thousands of rows tied with query 0 at distance 0 / its norm
    idx = make_index(xb, metric, storage)
    a, b = xb.astype(np.int64), xq.astype(np.int64)
    s = ((b[:, None, :] - a[None]) ** 2).sum(-1) if metric == L2 else b @ a.T
    for r in (float(np.median(s)), float(s[0, 100]), float(s[0, 100]) + 0.5):
        got = checked_range(idx, xq, r)
        assert_range_identical(got, _int_brute(xb, xq, r, metric), f"{kind} radius {r}")


@pytest.mark.parametrize("metric,storage,n", [(L2, "f32", 1 << 20), (IP, "f32", 1 << 20), (IP, "bf16", 100_000)])
def test_large_index_prefix_of_search(metric, storage, n):
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((n, 512)).astype(np.float32)
    xq = rng.standard_normal((16, 512)).astype(np.float32)
    if storage == "bf16":
        faiss.normalize_L2(xb)
        faiss.normalize_L2(xq)
    idx = make_index(xb, metric, storage)
    D0, _ = idx.search(xq, 100)
    # at most 60 rows for every query: D < (L2) / > (IP) every query's 61st distance
    r = float(D0[:, 60].min() if metric == L2 else D0[:, 60].max())
    lims, D, I = checked_range(idx, xq, r)
    counts = np.diff(lims.astype(np.int64))
    assert counts.max() <= 60 and counts.sum() > 16
    Ds, Is = idx.search(xq, int(counts.max()) + 1)
    assert_range_identical((lims, D, I), filter_search(Ds, Is, r, metric), "large")


def test_nonfinite_l2():
    rng = np.random.default_rng(9)
    xb = int_data("small", rng, 3000, 32)
    xq = int_data("small", rng, 4, 32)
    poison(xb, [5, 77], "nan")
    poison(xb, [9], "inf")
    poison(xq, [1], "nan")
    xb[200] = xq[2]
    xb[200, 3] = HUGE  # |y - mu|^2 overflows; the direct distance is HUGE^2 = inf: out
    xb[201] = xq[2]
    xb[201, 3] += 1  # a finite near row
    idx = make_index(xb, L2, "f32")
    mu = np.zeros(32, np.float32)
    mu[3] = -HUGE  # |y - mu|^2 of every row overflows: their lower bounds are keyed -FLT_MAX, d decides
    for pin in (False, True):
        if pin:
            idx.set_shift(mu)
        lims, D, I = checked_range(idx, xq, np.inf)
        assert not np.isin(I, [5, 77, 9]).any(), "a NaN / inf row was returned"
        assert lims[2] == lims[1], "a NaN query got results"
        q2 = I[int(lims[2]):int(lims[3])]
        assert 201 in q2 and 200 not in q2
        l2, D2, I2 = checked_range(idx, xq[2:3], 2.0)
        assert list(I2) == [201] and D2[0] == 1.0


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_staging_overflow_pass(metric, storage, monkeypatch):
    rng = np.random.default_rng(13)
    xb = rng.standard_normal((20000, 64)).astype(np.float32)
    xq = rng.standard_normal((16, 64)).astype(np.float32)
    idx = make_index(xb, metric, storage)
    D0, _ = idx.search(xq, 500)
    r = float(np.median(D0[:, 400]))
    base = checked_range(idx, xq, r)
    monkeypatch.setenv("ISE_RANGE_STAGE_CAP", "1")
    _native.lib.ise_refresh_env_knobs()
    try:
        got = checked_range(idx, xq, r, overflow=True)
    finally:
        monkeypatch.delenv("ISE_RANGE_STAGE_CAP")
        _native.lib.ise_refresh_env_knobs()
    assert_range_identical(got, base, "overflow pass")


def test_everything_100k_x_16():
    rng = np.random.default_rng(17)
    xb = rng.standard_normal((100_000, 32)).astype(np.float32)
    xq = rng.standard_normal((16, 32)).astype(np.float32)
    idx = make_index(xb, L2, "f32")
    lims, D, I = checked_range(idx, xq, np.inf)
    assert int(lims[-1]) == 1_600_000
    assert np.array_equal(I[:100_000], np.arange(100_000))
    Ds, Is = idx.search(xq[:2], 2048)
    sel = np.argsort(Is[0])
    assert np.array_equal(D[Is[0][sel]].view(np.uint32), Ds[0][sel].view(np.uint32))


def test_edges(tmp_path):
    rng = np.random.default_rng(19)
    xb = rng.standard_normal((1500, 40)).astype(np.float32)
    xq = rng.standard_normal((3, 40)).astype(np.float32)
    idx = faiss.IndexFlatL2(40)
    lims, D, I = checked_range(idx, xq, np.inf)  # empty index
    assert list(lims) == [0, 0, 0, 0]
    lims, D, I = checked_range(idx, xq[:0], 1.0)  # nq = 0
    assert list(lims) == [0]
    for a, b in ((0, 400), (400, 401), (401, 1500)):
        idx.add(xb[a:b])
    r = 60.0
    Ds, Is = idx.search(xq, 1500)
    want = filter_search(Ds, Is, r, L2)
    assert_range_identical(checked_range(idx, xq, r), want, "several adds")
    assert_range_identical(checked_range(idx, np.matrix(xq), r), want, "np.matrix")
    idx.reset()
    idx.add(xb)
    assert_range_identical(checked_range(idx, xq, r), want, "reset + re-add")
    path = str(tmp_path / "i.faiss")
    faiss.write_index(idx, path)
    idx2 = faiss.read_index(path)
    assert_range_identical(checked_range(idx2, xq, r), want, "read_index")
    idx.set_shift(np.full(40, 1e3, np.float32))
    assert_range_identical(checked_range(idx, xq, r), want, "far shift")


def test_concurrent_callers():
    rng = np.random.default_rng(23)
    xb = rng.standard_normal((30000, 128)).astype(np.float32)
    idx = make_index(xb, L2, "f32")
    qs = [rng.standard_normal((1 + i % 3, 128)).astype(np.float32) for i in range(8)]
    D0, _ = idx.search(qs[0], 200)
    r = float(D0[0, 150])
    solo = [idx.range_search(q, r) for q in qs]
    solo_knn = [idx.search(q, 10) for q in qs]
    errs = []

    def work(i):
        try:
            for _ in range(5):
                got = idx.range_search(qs[i], r)
                assert_range_identical(got, solo[i], f"thread {i}")
                Dk, Ik = idx.search(qs[i], 10)
                assert np.array_equal(Ik, solo_knn[i][1]) and np.array_equal(Dk, solo_knn[i][0])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs[0]
