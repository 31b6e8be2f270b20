"""GPU tests of remove_ids on IndexBinaryFlat and of IndexBinaryIDMap (include/ise_knn.h, ise_binary_index_remove_*; the
compaction kernels of csrc/ise_remove.hpp and csrc/ise_binary_scan.hpp).  The yardstick everywhere: after remove_ids the
index must be indistinguishable from a FRESH index built with add(xb[keep]) -- ntotal, reconstruct_n, search and
range_search, compared exactly (every score is an integer)."""
import threading

import numpy as np
import pytest

from image_search_engine_amd import _native
from image_search_engine_amd import faiss_compat as faiss
from tests import binary_ref as ref
from tests import binary_sel_ref as sref
from tests.test_binary_flat_gpu import assert_range_same, assert_same, make_index
from tests.test_remove_ids_gpu import patterns

pytestmark = pytest.mark.gpu

K = 40
NQS = (1, 16, 40)


@pytest.fixture
def small_slabs(monkeypatch):
    """48 destination rows per slab: every case crosses slabs."""
    monkeypatch.setenv("ISE_REMOVE_SLAB_ROWS", "48")
    _native.lib.ise_refresh_env_knobs()
    yield
    monkeypatch.delenv("ISE_REMOVE_SLAB_ROWS")
    _native.lib.ise_refresh_env_knobs()


def data(rng, n, code_size, nq=max(NQS)):
    xb = rng.integers(0, 256, (n, code_size), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, code_size), dtype=np.uint8)
    return xb, xq


def assert_same_as_fresh(idx, rows, xq, what):
    """idx against a fresh index of ``rows`` (the original codes that are left), and both against numpy."""
    fresh = faiss.IndexBinaryFlat(8 * xq.shape[1])
    if len(rows):
        fresh.add(rows)
    assert idx.ntotal == fresh.ntotal == len(rows), what
    back = idx.reconstruct_n()
    assert back.dtype == np.uint8 and np.array_equal(back, rows), what
    dist = ref.distances(rows, xq)
    want = ref.search(rows, xq, K, dist)
    for nq in NQS:
        got = idx.search(xq[:nq], K)
        assert_same(got, fresh.search(xq[:nq], K))
        assert_same(got, (want[0][:nq], want[1][:nq]))
    r = int(np.median(dist)) if dist.size else 1
    got = idx.range_search(xq[:16], r)
    assert_range_same(got, fresh.range_search(xq[:16], r))
    assert_range_same(got, ref.range_search(rows, xq[:16], r, dist[:16]))


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


# ws = 1 (the 8-byte kernel), ws = 1 with pad, ws = 2, an odd word count stored as 4, 128 words, 5 words stored as 6
SHAPES = [(1000, 8), (777, 1), (2048, 16), (600, 24), (50, 1024), (5000, 40)]


@pytest.mark.parametrize("n,code_size", SHAPES)
def test_equals_fresh_index(n, code_size, small_slabs):
    rng = np.random.default_rng(n + code_size)
    xb, xq = data(rng, n, code_size)
    for name, arg, gone in patterns(rng, n):
        idx = make_index(xb)
        keep = checked_remove(idx, arg, gone, n)
        assert_same_as_fresh(idx, xb[keep], xq, f"{name} n={n} code_size={code_size}")


@pytest.mark.parametrize("code_size", (8, 16))
def test_default_slab(code_size):
    rng = np.random.default_rng(1)
    n = 3000
    xb, xq = data(rng, n, code_size)
    idx = make_index(xb)
    gone = set(rng.choice(n, 400, replace=False).tolist())
    keep = checked_remove(idx, np.asarray(sorted(gone)), gone, n)
    assert_same_as_fresh(idx, xb[keep], xq, "default slab")


@pytest.mark.parametrize("code_size", (8, 24))
def test_remove_add_remove(code_size, small_slabs):
    rng = np.random.default_rng(3)
    cur, xq = data(rng, 1000, code_size)
    idx = make_index(cur)
    for step, (n_rm, n_add) in enumerate(((100, 500), (333, 17), (1, 2000))):  # 900 + 500 outgrows the capacity
        gone = set(rng.choice(len(cur), n_rm, replace=False).tolist())
        keep = checked_remove(idx, rng.permutation(sorted(gone)), gone, len(cur))
        cur = cur[keep]
        assert_same_as_fresh(idx, cur, xq, f"step {step} removed")
        more, _ = data(rng, n_add, code_size, 1)
        idx.add(more)  # over the stale rows the removal left behind its new end
        cur = np.concatenate((cur, more))
        assert_same_as_fresh(idx, cur, xq, f"step {step} added")


def test_nothing_removed_leaves_counters_and_epoch_alone():
    rng = np.random.default_rng(9)
    xb, xq = data(rng, 100, 8)
    idx = make_index(xb)
    ds = idx.make_selector(faiss.IDSelectorRange(0, 50))
    s0 = idx.remove_stats()
    assert s0 == {"remove_calls": 0, "rows_removed": 0, "rows_moved": 0}
    assert idx.remove_ids([]) == 0 and idx.remove_ids([100, -1, 1 << 50]) == 0
    assert idx.remove_ids(faiss.IDSelectorRange(40, 40)) == 0 and idx.remove_ids(faiss.IDSelectorRange(100, 900)) == 0
    assert idx.remove_ids(faiss.IDSelectorBatch([200, 300])) == 0
    assert idx.remove_stats() == s0 and idx.ntotal == 100
    members = sref.members_of(faiss.IDSelectorRange(0, 50), 100)
    assert_same(idx.search(xq, 5, params=faiss.SearchParameters(sel=ds)), sref.search(xb, xq, 5, members))  # still valid
    assert idx.remove_ids([7, 7, 99]) == 2
    assert idx.ntotal == 98 and idx.remove_stats() == {"remove_calls": 1, "rows_removed": 2, "rows_moved": 91}
    with pytest.raises(_native.IseError, match="row epoch"):
        idx.search(xq, 5, params=faiss.SearchParameters(sel=ds))


def test_integer_ties_come_back_in_new_id_order(small_slabs):
    rng = np.random.default_rng(4)
    n = 3000
    xb, xq = data(rng, n, 8, 16)
    group = [100, 101, 102, 500, 1500, 1501, 2200, 2999]
    xb[group] = xq[0]
    idx = make_index(xb)
    gone = {7, 50, 101, 1500, 2500}  # two members of the tie group, and rows in front of the others
    keep = checked_remove(idx, sorted(gone), gone, n)
    new_id = np.cumsum(keep) - 1
    left = [int(new_id[i]) for i in group if i not in gone]
    D, I = idx.search(xq, 10)
    assert I[0, :len(left)].tolist() == left and not D[0, :len(left)].any()
    assert_same((D, I), ref.search(xb[keep], xq, 10))


def test_concurrent_searches_see_before_or_after(small_slabs):
    rng = np.random.default_rng(7)
    n = 20000
    xb, _ = data(rng, n, 8, 1)
    gone = np.sort(rng.choice(n, 100, replace=False))
    qs = [xb[int(i)][None, :].copy() for i in gone[:2]]  # a removed row as the query: its results must change
    idx = make_index(xb)
    keep = np.ones(n, dtype=bool)
    keep[gone] = False
    before = [ref.search(xb, q, 10) for q in qs]
    after = [ref.search(xb[keep], q, 10) for q in qs]
    for t, (b, a) in enumerate(zip(before, after)):
        assert not np.array_equal(b[1], a[1])
        assert_same(idx.search(qs[t], 10), b)
    same = lambda x, y: np.array_equal(x[1], y[1]) and np.array_equal(x[0], y[0])
    errs, seen = [], [set() for _ in qs]
    start = threading.Barrier(3)

    def searcher(t):
        try:
            start.wait()
            for _ in range(50):
                got = idx.search(qs[t], 10)
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

    ts = [threading.Thread(target=searcher, args=(t,)) for t in range(2)] + [threading.Thread(target=remover)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs[0]
    for t, q in enumerate(qs):
        assert same(idx.search(q, 10), after[t])


def test_index_binary_id_map(tmp_path, small_slabs):
    rng = np.random.default_rng(8)
    n, cs = 1500, 8
    xb, xq = data(rng, n, cs, 16)
    ext = rng.permutation(np.arange(n, dtype=np.int64) * 7919 + (1 << 40))  # scattered 64-bit ids, all above 2^32
    ext[:3] = [5, (1 << 32) + 1, 1 << 31]
    m = faiss.IndexBinaryIDMap(faiss.IndexBinaryFlat(8 * cs))
    with pytest.raises(RuntimeError):
        m.add(xb)
    m.add_with_ids(xb[:1000], ext[:1000])
    m.add_with_ids(xb[1000:], ext[1000:])
    assert (m.ntotal, m.d, m.code_size, m.is_trained) == (n, 8 * cs, cs, True) and np.array_equal(m.id_map, ext)
    dist = ref.distances(xb, xq)
    Dw, Iw = ref.search(xb, xq, 10, dist)
    D, I = m.search(xq, 10)
    assert_same((D, I), (Dw, ext[Iw]))
    r = int(np.median(dist))
    lw, Drw, Irw = ref.range_search(xb, xq, r, dist)
    assert_range_same(m.range_search(xq, r), (lw, Drw, ext[Irw]))
    last = m.search(xq[:1], n + 5)
    assert (last[1][0, n:] == -1).all() and (last[0][0, n:] == ref.INT32_MAX).all()  # -1 stays -1
    assert sorted(last[1][0, :n].tolist()) == sorted(ext.tolist())

    # params= selectors are over EXTERNAL ids
    chosen = ext[rng.choice(n, 300, replace=False)]
    for sel in (faiss.IDSelectorBatch(chosen), faiss.IDSelectorRange(1 << 40, (1 << 40) + 7919 * 200),
                faiss.IDSelectorNot(faiss.IDSelectorBatch(ext[Iw[:, 0]]))):
        members = sel.members(ext)
        p = faiss.SearchParameters(sel=sel)
        Ds, Is = sref.search(xb, xq, 10, members, dist)
        assert_same(m.search(xq, 10, params=p), (Ds, np.where(Is >= 0, ext[Is], -1)))
        ls, Drs, Irs = sref.range_search(xb, xq, r, members, dist)
        assert_range_same(m.range_search(xq, r, params=p), (ls, Drs, ext[Irs]))
    with pytest.raises(TypeError):
        m.search(xq, 10, params=faiss.SearchParameters(sel=m.index.make_selector(faiss.IDSelectorRange(0, 5))))

    # remove_ids by external ids: a batch, a range, a Not
    keep = np.ones(n, dtype=bool)
    rows = np.sort(rng.choice(n, 200, replace=False))
    assert m.remove_ids(faiss.IDSelectorBatch(np.concatenate((ext[rows][::-1], [12345, -1])))) == 200
    keep[rows] = False
    assert m.ntotal == n - 200 and np.array_equal(m.id_map, ext[keep])
    assert m.remove_ids(ext[rows]) == 0
    in_range = (ext >= (1 << 40)) & (ext < (1 << 40) + 7919 * 100) & keep
    assert m.remove_ids(faiss.IDSelectorRange(1 << 40, (1 << 40) + 7919 * 100)) == int(in_range.sum()) > 0
    keep &= ~in_range
    stay = ext[keep][::2]
    assert m.remove_ids(faiss.IDSelectorNot(faiss.IDSelectorBatch(stay))) == int(keep.sum()) - stay.size
    keep &= np.isin(ext, stay)
    assert m.ntotal == stay.size and np.array_equal(m.id_map, ext[keep])
    Df, If = ref.search(xb[keep], xq, 10)
    D, I = m.search(xq, 10)
    assert_same((D, I), (Df, ext[keep][If]))  # surviving ids still find their codes
    for j in (0, stay.size // 2, stay.size - 1):  # ... each its own: the code of an id is its nearest neighbour
        Dj, Ij = m.search(xb[keep][j:j + 1], 1)
        assert Dj[0, 0] == 0 and Ij[0, 0] == ext[keep][j]

    path = str(tmp_path / "m.index")
    faiss.write_index_binary(m, path)
    m2 = faiss.read_index_binary(path)
    assert isinstance(m2, faiss.IndexBinaryIDMap) and np.array_equal(m2.id_map, m.id_map)
    assert m2.ntotal == m.ntotal and np.array_equal(m2.index.reconstruct_n(), m.index.reconstruct_n())
    assert_same(m2.search(xq, 10), (D, I))
    assert_range_same(m2.range_search(xq, r), m.range_search(xq, r))
    m.reset()
    assert m.ntotal == 0 and m.id_map.size == 0
