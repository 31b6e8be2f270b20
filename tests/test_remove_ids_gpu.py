"""GPU tests of remove_ids (csrc/ise_remove.hpp; its host planning: csrc/ise_remove_plan.hpp).  The yardstick
everywhere: after remove_ids the index must be indistinguishable from a FRESH index built with add(x[keep]) from the
original float32 rows -- ntotal, reconstruct_n, search and range_search bit for bit.  Results do not depend on the shift
vector or on the path, so no comparison here has a tolerance."""
import ctypes
import threading

import numpy as np
import pytest

from image_search_engine_amd import _native
from image_search_engine_amd import faiss_compat as faiss
from tests import remove_ref as rr
from tests.knn_checks import HUGE, assert_knn_identical, brute_knn, int_data, plant_ties, poison
from tests.range_ref import IP, L2, assert_range_identical
from tests.test_range_search_gpu import STORAGES

pytestmark = pytest.mark.gpu

K = 10
NQS = (1, 16, 40)


@pytest.fixture
def small_slabs(monkeypatch):
    """48 destination rows per slab: every case crosses slabs."""
    monkeypatch.setenv("ISE_REMOVE_SLAB_ROWS", "48")
    _native.lib.ise_refresh_env_knobs()
    yield
    monkeypatch.delenv("ISE_REMOVE_SLAB_ROWS")
    _native.lib.ise_refresh_env_knobs()


def make_index(xb, metric, storage="f32"):
    idx = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    if len(xb):
        idx.add(xb)
    return idx


def data(rng, n, d, nq, metric, storage):
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    if metric == IP and storage == "bf16":
        faiss.normalize_L2(xb)
        faiss.normalize_L2(xq)
    return xb, xq


def assert_same_as_fresh(idx, rows, xq, metric, storage, what):
    """idx against a fresh index of ``rows`` (the original float32 rows that are left)."""
    fresh = make_index(rows, metric, storage)
    assert idx.ntotal == fresh.ntotal == len(rows), what
    assert np.array_equal(idx.reconstruct_n().view(np.uint32), fresh.reconstruct_n().view(np.uint32)), what
    Dw = None
    for nq in NQS:
        Dw, Iw = fresh.search(xq[:nq], K)
        D, I = idx.search(xq[:nq], K)
        assert_knn_identical(D, I, Dw, Iw, f"{what} nq={nq}")
    ok = np.isfinite(Dw) & (np.abs(Dw) < 3e38)
    r = float(np.median(Dw[ok])) if ok.any() else 1.0
    assert_range_identical(idx.range_search(xq[:16], r), fresh.range_search(xq[:16], r), what)
    return fresh


def checked_remove(idx, arg, want_removed, n):
    """remove_ids(arg) with its return value and the counters asserted; -> keep mask."""
    gone = np.zeros(n, dtype=bool)
    gone[sorted(want_removed)] = True
    before = idx.remove_stats()
    got = idx.remove_ids(arg)
    after = idx.remove_stats()
    assert got == int(gone.sum())
    n_new = n - got
    first = int(np.flatnonzero(gone)[0]) if got else n
    assert after["rows_removed"] - before["rows_removed"] == got
    assert after["remove_calls"] - before["remove_calls"] == (1 if got else 0)
    assert after["rows_moved"] - before["rows_moved"] == (n_new - first if got else 0)
    return ~gone


def patterns(rng, n):
    """(name, argument of remove_ids, the rows that must go)."""
    tenth = rng.choice(n, max(1, n // 10), replace=False)
    some = rng.integers(0, n, 7)
    messy = np.concatenate((some, some[:3], [n, n + 3, -1, -(1 << 40), 1 << 40, int(some[0])]))
    return [
        ("first row", [0], {0}),
        ("middle row", faiss.IDSelectorBatch([n // 2]), {n // 2}),
        ("last row", faiss.IDSelectorArray([n - 1]), {n - 1}),
        ("every second row", np.arange(0, n, 2), set(range(0, n, 2))),
        ("300-row run", faiss.IDSelectorRange(10, 310), set(range(10, min(310, n)))),
        ("random tenth", rng.permutation(tenth), set(tenth.tolist())),
        ("all but row 0", faiss.IDSelectorNot(faiss.IDSelectorBatch([0])), set(range(1, n))),
        ("all rows", faiss.IDSelectorRange(-5, n + 5), set(range(n))),
        ("messy id list", messy, set(int(i) for i in some)),
    ]


SHAPES = [(1000, 2048), (2048, 512), (777, 100), (50, 1), (5000, 33)]


@pytest.mark.parametrize("metric,storage", STORAGES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_equals_fresh_index(metric, storage, n, d, small_slabs):
    rng = np.random.default_rng(n + d)
    xb, xq = data(rng, n, d, max(NQS), metric, storage)
    for name, arg, gone in patterns(rng, n):
        idx = make_index(xb, metric, storage)
        if name in ("every second row", "messy id list"):
            idx.search(xq[:1], K)  # norms (and the shift vector) taken before the removal: they move with the rows
        keep = checked_remove(idx, arg, gone, n)
        assert_same_as_fresh(idx, xb[keep], xq, metric, storage, f"{name} n={n} d={d}")


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_default_slab(metric, storage):
    rng = np.random.default_rng(1)
    n = 3000
    xb, xq = data(rng, n, 96, max(NQS), metric, storage)
    idx = make_index(xb, metric, storage)
    idx.search(xq[:1], K)
    gone = set(rng.choice(n, 400, replace=False).tolist())
    keep = checked_remove(idx, np.asarray(sorted(gone)), gone, n)
    assert_same_as_fresh(idx, xb[keep], xq, metric, storage, "default slab")


@pytest.mark.parametrize("metric", [L2, IP])
def test_tail_is_zeroed(metric, small_slabs):
    rng = np.random.default_rng(2)
    n, d = 1030, 40
    xb, xq = data(rng, n, d, max(NQS), metric, "f32")
    tail = np.arange(n - 21, n)
    poison(xb, tail[:7], "nan")
    poison(xb, tail[7:14], "inf", col=3)
    xb[tail[14:], 5] = HUGE
    idx = make_index(xb, metric)
    idx.search(xq[:16], K)  # norms of the poisoned rows exist
    keep = checked_remove(idx, faiss.IDSelectorRange(n - 21, n), set(tail.tolist()), n)
    assert idx.ntotal % 16 != 0
    assert_same_as_fresh(idx, xb[keep], xq, metric, "f32", "poisoned tail removed")
    more = rng.standard_normal((40, d)).astype(np.float32)
    idx.add(more)
    assert_same_as_fresh(idx, np.concatenate((xb[keep], more)), xq, metric, "f32", "add behind the removal")


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_remove_add_remove(metric, storage, small_slabs):
    rng = np.random.default_rng(3)
    d = 72
    cur, xq = data(rng, 1000, d, max(NQS), metric, storage)
    idx = make_index(cur, metric, storage)
    for step, (n_rm, n_add) in enumerate(((100, 500), (333, 17), (1, 2000))):  # 900 + 500 outgrows the 1008-row capacity
        gone = set(rng.choice(len(cur), n_rm, replace=False).tolist())
        keep = checked_remove(idx, rng.permutation(sorted(gone)), gone, len(cur))
        cur = cur[keep]
        assert_same_as_fresh(idx, cur, xq, metric, storage, f"step {step} removed")
        more, _ = data(rng, n_add, d, 1, metric, storage)
        idx.add(more)
        cur = np.concatenate((cur, more))
        assert_same_as_fresh(idx, cur, xq, metric, storage, f"step {step} added")


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_integer_ties_come_back_in_new_id_order(metric, storage, small_slabs):
    rng = np.random.default_rng(4)
    n, d = 3000, 32
    xb = int_data("small", rng, n, d)
    group = [101, 102, 500, 1500, 1501, 2200, 2999]
    plant_ties(xb, 100, group)
    xq = np.concatenate((xb[100:101], int_data("small", rng, 15, d)))
    idx = make_index(xb, metric, storage)
    idx.search(xq, K)
    gone = {7, 50, 101, 1500, 2500}  # two members of the tie group, and rows in front of the others
    keep = checked_remove(idx, sorted(gone), gone, n)
    rows = xb[keep]
    D, I = idx.search(xq, K)
    Dw, Iw = brute_knn(rows, xq, K, metric)
    assert_knn_identical(D, I, Dw, Iw, "integer data")
    new_id = np.cumsum(keep) - 1
    left = [int(new_id[i]) for i in [100] + group if i not in gone]
    if metric == L2:  # the group is at distance 0 from query 0: its members fill the first ranks in ascending new id
        assert I[0, :len(left)].tolist() == left and not D[0, :len(left)].any()
    else:  # equal inner products: wherever they rank, the members present appear in ascending new id
        pos = [int(np.flatnonzero(I[0] == i)[0]) for i in left if i in I[0]]
        assert pos == sorted(pos)
    assert_same_as_fresh(idx, rows, xq, metric, storage, "integer data")


def test_shadow_rows_move_with_the_rows(small_slabs):
    rng = np.random.default_rng(5)
    n, d = 262144 + 3000, 32
    xb = rng.random((n, d), dtype=np.float32)
    xq = rng.random((max(NQS), d), dtype=np.float32)
    idx = make_index(xb, L2)
    idx.search(xq[:16], K)  # both shadows exist
    idx.shadow_row(0), idx.byte_row(0)
    gone = np.sort(rng.choice(n, 1000, replace=False))
    runs = rr.runs_of(gone.tolist(), n)
    src = rr.source_map(n, runs)
    sample = np.unique(np.concatenate(([0, int(gone[0]), len(src) - 1], rng.integers(int(gone[0]), len(src), 47))))
    before = {int(j): (idx.shadow_row(int(src[j])), idx.byte_row(int(src[j]))) for j in sample}
    shifts = idx.exact_stats()["shift_updates"]
    keep = checked_remove(idx, gone, set(gone.tolist()), n)
    for j, (sh, by) in before.items():
        assert idx.shadow_row(j) == sh and idx.byte_row(j) == by, j
    halves = idx.half_stats()["half_batches"]
    idx.search(xq[:16], K)
    assert idx.half_stats()["half_batches"] == halves + 1
    assert idx.exact_stats()["shift_updates"] == shifts
    cur = xb[keep]
    assert_same_as_fresh(idx, cur, xq, L2, "f32", "above the shadow threshold")
    assert idx.exact_stats()["shift_updates"] == shifts
    # ... then to or below the threshold: the shadows go, as a fresh index of that size has none
    gone2 = set(rng.choice(len(cur), 5000, replace=False).tolist())
    keep2 = checked_remove(idx, np.asarray(sorted(gone2)), gone2, len(cur))
    assert idx.ntotal <= 262144
    with pytest.raises(RuntimeError, match="no shadow rows"):
        idx.shadow_row(0)
    halves = idx.half_stats()["half_batches"]
    assert_same_as_fresh(idx, cur[keep2], xq, L2, "f32", "below the shadow threshold")
    assert idx.half_stats()["half_batches"] == halves


def test_shift_refresh_rules(small_slabs):
    rng = np.random.default_rng(6)
    n, d = 4000, 64
    xb = rng.standard_normal((n, d)).astype(np.float32) + 3.0
    xq = rng.standard_normal((max(NQS), d)).astype(np.float32) + 3.0
    updates = lambda i: i.exact_stats()["shift_updates"]
    idx = make_index(xb, L2)
    idx.search(xq[:16], K)
    assert updates(idx) == 1
    assert idx.remove_ids(faiss.IDSelectorRange(0, n // 2)) == n // 2
    assert updates(idx) == 1
    idx.search(xq[:16], K)
    assert updates(idx) == 2  # shrunk below three quarters: refreshed once, at the next search
    idx.search(xq[:16], K)
    assert updates(idx) == 2
    assert_same_as_fresh(idx, xb[n // 2:], xq, L2, "f32", "half removed")

    idx = make_index(xb, L2)
    idx.search(xq[:16], K)
    assert idx.remove_ids(np.arange(0, n, 100)) == n // 100
    idx.search(xq[:16], K)
    assert updates(idx) == 1  # one per cent: the shift vector stays

    idx = make_index(xb, L2)
    mu = rng.standard_normal(d).astype(np.float32)
    idx.set_shift(mu)
    idx.search(xq[:16], K)
    u0 = updates(idx)
    assert idx.remove_ids(faiss.IDSelectorRange(0, n // 2)) == n // 2
    idx.search(xq[:16], K)
    assert updates(idx) == u0 and np.array_equal(idx.get_shift(), mu)  # a pinned shift stays pinned
    assert_same_as_fresh(idx, xb[n // 2:], xq, L2, "f32", "pinned shift")


def test_concurrent_searches_see_before_or_after(small_slabs):
    rng = np.random.default_rng(7)
    n, d = 20000, 64
    xb = rng.standard_normal((n, d)).astype(np.float32)
    gone = np.sort(rng.choice(n, 100, replace=False))
    qs = [xb[int(i)][None, :].copy() for i in gone[:4]]  # a removed row as the query: its results must change
    idx = make_index(xb, L2)
    before = [idx.search(q, K) for q in qs]
    keep = np.ones(n, dtype=bool)
    keep[gone] = False
    fresh = make_index(xb[keep], L2)
    after = [fresh.search(q, K) for q in qs]
    for b, a in zip(before, after):
        assert not np.array_equal(b[1], a[1])
    same = lambda x, y: np.array_equal(x[1], y[1]) and np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))
    errs, seen = [], [set() for _ in qs]
    start = threading.Barrier(5)

    def searcher(t):
        try:
            start.wait()
            for _ in range(50):
                got = idx.search(qs[t], K)
                which = "before" if same(got, before[t]) else ("after" if same(got, after[t]) else None)
                assert which, f"thread {t}: a result that is neither the before- nor the after-result"
                assert not (which == "before" and "after" in seen[t]), "a before-result behind an after-result"
                seen[t].add(which)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def remover():
        try:
            start.wait()
            assert idx.remove_ids(gone) == 100
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=searcher, args=(t,)) for t in range(4)] + [threading.Thread(target=remover)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs[0]
    for t, q in enumerate(qs):
        assert same(idx.search(q, K), after[t])


def test_index_id_map(tmp_path, small_slabs):
    rng = np.random.default_rng(8)
    n, d = 1500, 24
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((16, d)).astype(np.float32)
    ext = rng.permutation(np.arange(n, dtype=np.int64) * 7919 + (1 << 40))  # scattered 64-bit ids
    m = faiss.IndexIDMap(faiss.IndexFlatL2(d))
    with pytest.raises(RuntimeError):
        m.add(xb)
    m.add_with_ids(xb[:1000], ext[:1000])
    m.add_with_ids(xb[1000:], ext[1000:])
    assert (m.ntotal, m.d, m.metric_type, m.is_trained) == (n, d, L2, True) and np.array_equal(m.id_map, ext)
    plain = make_index(xb, L2)
    Dp, Ip = plain.search(xq, K)
    D, I = m.search(xq, K)
    assert np.array_equal(D, Dp) and np.array_equal(I, ext[Ip])
    r = float(np.median(Dp))
    lp, Drp, Irp = plain.range_search(xq, r)
    assert_range_identical(m.range_search(xq, r), (lp, Drp, ext[Irp]), "mapped range search")
    assert m.search(xq[:1], n + 5)[1][0, -1] == -1  # -1 stays -1

    rows = np.sort(rng.choice(n, 200, replace=False))
    assert m.remove_ids(faiss.IDSelectorBatch(np.concatenate((ext[rows][::-1], [12345, -1])))) == 200
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    assert m.ntotal == n - 200 and np.array_equal(m.id_map, ext[keep])
    fresh = make_index(xb[keep], L2)
    Df, If = fresh.search(xq, K)
    D, I = m.search(xq, K)
    assert_knn_identical(D, I, Df, ext[keep][If], "after remove_ids")  # the other ids are still valid
    assert not np.isin(I, ext[rows]).any()
    assert m.remove_ids(ext[rows]) == 0

    path = str(tmp_path / "m.faiss")
    faiss.write_index(m, path)
    m2 = faiss.read_index(path)
    assert isinstance(m2, faiss.IndexIDMap) and np.array_equal(m2.id_map, m.id_map)
    D2, I2 = m2.search(xq, K)
    assert_knn_identical(D2, I2, D, I, "read_index")
    m.reset()
    assert m.ntotal == 0 and m.id_map.size == 0


def test_abi_errors_and_noop():
    lib = _native.lib
    out = ctypes.c_int64(-7)
    ids = (ctypes.c_int64 * 2)(1, 2)
    assert lib.ise_index_remove_ids_host(None, ids, 2, ctypes.byref(out)) == _native.E_INVALID
    assert lib.ise_last_error()
    assert lib.ise_index_remove_range(None, 0, 1, None) == _native.E_INVALID
    assert lib.ise_last_error()
    assert lib.ise_index_remove_stats(None, None) == _native.E_INVALID
    rng = np.random.default_rng(9)
    idx = make_index(rng.standard_normal((100, 8)).astype(np.float32), L2)
    assert lib.ise_index_remove_ids_host(idx._h, None, 3, ctypes.byref(out)) == _native.E_INVALID
    assert b"ids" in lib.ise_last_error() and out.value == 0
    s0 = idx.remove_stats()
    assert s0 == {"remove_calls": 0, "rows_removed": 0, "rows_moved": 0}
    assert idx.remove_ids([]) == 0 and idx.remove_ids([100, -1, 1 << 50]) == 0
    assert idx.remove_ids(faiss.IDSelectorRange(40, 40)) == 0 and idx.remove_ids(faiss.IDSelectorRange(100, 900)) == 0
    assert lib.ise_index_remove_ids_host(idx._h, None, 0, None) == 0
    assert idx.remove_stats() == s0 and idx.ntotal == 100
    assert lib.ise_index_remove_ids_host(idx._h, ids, 2, None) == 0  # n_removed may be NULL
    assert idx.ntotal == 98 and idx.remove_stats() == {"remove_calls": 1, "rows_removed": 2, "rows_moved": 97}
