"""GPU tests of IndexIVFScalarQuantizer (include/ise_knn.h, ise_ivfsq_*; csrc/ise_ivfsq.hpp).  On the integer
construction of tests/sq_ref.py every comparison is bit for bit: against the float64 ranking over the decoded rows cut
to each query's probed members (tests/ivfsq_ref.py) and against an IndexScalarQuantizer with the same trained state over
the same rows.  Every search also asserts what it adds to ``ivfsq_stats``: one batch, the passes, and the 64-row tiles
of the probed lists and no others."""
import numpy as np
import pytest

from image_search_engine_amd import _native as native
from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref, ivfsq_ref, sq_ref
from tests.knn_checks import RTOL, assert_exact_range, assert_knn_identical, assert_knn_matches, int_data
from tests.sel_ref import IP, L2, pad_value
from tests.sq_ref import exact_top

pytestmark = pytest.mark.gpu

SQ = faiss.ScalarQuantizer
QTYPES = [SQ.QT_8bit, SQ.QT_8bit_uniform]
CHUNKS = [250, 1, 349]  # the three add calls


def new_index(d, qtype, metric, cent, t):
    qz = faiss.IndexFlatL2(d)
    qz.add(np.ascontiguousarray(cent, dtype=np.float32))
    index = faiss.IndexIVFScalarQuantizer(qz, d, len(cent), qtype, metric, by_residual=False)
    assert not index.is_trained and index.ntotal == 0 and index.nprobe == 1 and index.quantizer is qz
    assert (index.nlist, index.by_residual, index.code_size, index.sa_code_size()) == (len(cent), False, d, d)
    assert index.sq.trained.size == 0
    index.sq.set_trained(t)
    assert index.is_trained and np.array_equal(index.sq.trained.view(np.uint32), np.asarray(t, np.float32).view(np.uint32))
    return qz, index


def sq_index(d, qtype, metric, t, xb):
    sqi = faiss.IndexScalarQuantizer(d, qtype, metric)
    sqi.sq.set_trained(t)
    if len(xb):
        sqi.add(xb)
    return sqi


def force_add(index, x, lists):
    """Rows into the lists the test names (the library takes list numbers; the class asks its quantiser)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lists = np.ascontiguousarray(lists, dtype=np.int64)
    native.check(native.lib.ise_ivfsq_add_host(index._h, x.ctypes.data, lists.ctypes.data, len(x)))


def sizes_of(index):
    return [index.list_size(l) for l in range(index.nlist)]


def counted(index, probes, k, call):
    """call() -> (D, I), with the statistics it adds asserted against the reference's count."""
    sizes = sizes_of(index)
    want = ivfsq_ref.stats_of(probes, sizes, index.d, k) if index.ntotal and len(probes) else \
        {"batches": 1 if len(probes) else 0, "passes": 0, "tiles_loaded": 0}
    before = index.ivfsq_stats()
    out = call()
    after = index.ivfsq_stats()
    got = {key: after[key] - before[key] for key in want}
    assert got == want, (got, want)
    return out


def search_pre(index, xq, k, probes):
    return counted(index, probes, k, lambda: index.search_preassigned(xq, k, probes))


def check_lists(index, assign, codes):
    for l, want in enumerate(ivf_ref.list_members(assign, index.nlist)):
        ids, got = index.get_list(l)
        assert ids.dtype == np.int64 and got.dtype == np.uint8 and got.shape == (len(want), index.d)
        assert np.array_equal(ids, want) and (np.diff(ids) > 0).all() and index.list_size(l) == len(want)
        assert np.array_equal(got, codes[want])


# ---------------------------------------------------------------- 1. sweep
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("d", [1, 17, 64, 100, 512])
def test_sweep(d, qtype, metric):
    n, nlist = 600, 5
    rng = np.random.default_rng(4000 + 7 * d + qtype)
    t, m, s = sq_ref.integer_trained(rng, d, qtype)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, 40, d)
    cent = np.full((nlist, d), 1000.0, np.float32)  # the last list stays empty
    cent[:4] = (m[None, :] + s[None, :] * np.array([[1.0], [5.0], [9.0], [13.0]])) if d == 1 else xb[:4]
    qz, index = new_index(d, qtype, metric, cent, t)
    index.train(xb)  # a no-op: both halves are trained
    assert qz.ntotal == nlist and np.array_equal(index.sq.trained.view(np.uint32), t.view(np.uint32))
    i0 = 0
    for c in CHUNKS:
        index.add(xb[i0:i0 + c])
        i0 += c
        assert index.ntotal == i0
    assign = qz.search(xb, 1)[1].reshape(-1)
    sizes = sizes_of(index)
    assert sizes == np.bincount(assign, minlength=nlist).tolist() and 0 in sizes
    vmin, vdiff = sq_ref.expand(t, d, qtype)
    codes = sq_ref.encode(xb, vmin, vdiff)
    dec = sq_ref.decode(codes, vmin, vdiff)
    assert np.array_equal(codes, base) and np.array_equal(dec, xb)
    assert np.array_equal(index.sq.compute_codes(xb[:3]), codes[:3])
    assert np.array_equal(index.sq.decode(codes[:3]).view(np.uint32), dec[:3].view(np.uint32))
    assert_exact_range(dec, xq)
    check_lists(index, assign, codes)
    sqi = sq_index(d, qtype, metric, t, xb)
    full_ref = sq_ref.expected(xq, dec, n, metric)  # the complete rankings, computed once
    full_sq = sqi.search(xq, n)
    assert_knn_identical(*full_sq, *full_ref, "the flat scalar-quantised index")
    for nq in (1, 16, 17, 40):
        for nprobe in (1, 2, nlist):
            index.nprobe = nprobe
            probes = qz.search(xq[:nq], nprobe)[1]
            members = ivf_ref.probed_members(probes, assign, nlist)
            for k in (1, 10, 33, 70):
                what = f"nq={nq} nprobe={nprobe} k={k}"
                D, I = counted(index, probes, k, lambda: index.search(xq[:nq], k))
                assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full_ref[0][:nq], full_ref[1][:nq], members, k, metric), what)
                assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full_sq[0][:nq], full_sq[1][:nq], members, k, metric),
                                     "IndexScalarQuantizer's bits " + what)
                if nprobe == nlist:
                    assert_knn_identical(D, I, *sqi.search(xq[:nq], k), "all lists " + what)
    check_lists(index, assign, codes)


# ---------------------------------------------------------------- 2. list and tile edges
EDGE_SIZES = [0, 1, 63, 64, 65, 128, 129]


@pytest.mark.parametrize("metric", [L2, IP])
def test_list_and_tile_edges(metric):
    d, nlist, n = 24, len(EDGE_SIZES), sum(EDGE_SIZES)
    rng = np.random.default_rng(61)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, 9, d)
    assign = rng.permutation(np.repeat(np.arange(nlist), EDGE_SIZES))
    qz, index = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    # an empty index: padding, one batch, no pass, no tile
    D, I = search_pre(index, xq, 5, np.zeros((9, 1), np.int64))
    assert (I == -1).all() and (D == pad_value(metric)).all() and D.dtype == np.float32 and I.dtype == np.int64
    force_add(index, xb, assign)
    assert sizes_of(index) == EDGE_SIZES and index.ntotal == n
    check_lists(index, assign, base)
    full = sq_ref.expected(xq, xb, n, metric)
    tables = [np.tile(np.arange(nlist), (9, 1)),                                           # every list: 10 tiles
              np.array([[l] for l in (0, 1, 2, 3, 4, 5, 6, 1, 4)], np.int64),              # one list each
              np.array([[4, -1, 4], [nlist, -1, nlist], [-1, -1, -1], [0, 0, -1], [6, 5, 6], [2, nlist + 5, 3], [-7, 1, 1],
                        [5, 5, 5], [3, 2, -1]], np.int64)]                                  # -1, nlist, duplicates, the empty list
    for probes in tables:
        members = ivf_ref.probed_members(probes, assign, nlist)
        for k in (1, 5, 66, 200):  # 200 exceeds every member set but the first table's: the tail is padding
            D, I = search_pre(index, xq, k, probes)
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(*full, members, k, metric), f"k={k}")
            for q, mem in enumerate(members):
                assert (I[q, len(mem):] == -1).all() and (I[q, :min(k, len(mem))] >= 0).all()
    # rows of only -1: padding, and the pass costs no tile (counted asserts tiles_loaded == 0)
    D, I = search_pre(index, xq, 40, np.full((9, 2), -1, np.int64))
    assert (I == -1).all() and (D == pad_value(metric)).all()
    assert ivfsq_ref.stats_of(np.full((9, 2), -1), EDGE_SIZES, d, 40)["tiles_loaded"] == 0
    # one list, one query: exactly that list's tiles
    for l, size in enumerate(EDGE_SIZES):
        t0 = index.ivfsq_stats()["tiles_loaded"]
        index.search_preassigned(xq[:1], 3, np.array([[l]]))
        assert index.ivfsq_stats()["tiles_loaded"] - t0 == -(-size // 64)
    D, I = index.search(xq[:0], 4)
    assert D.shape == (0, 4) and I.shape == (0, 4) and D.dtype == np.float32 and I.dtype == np.int64
    D, I = index.search_preassigned(xq[:0], 4, np.zeros((0, 1), np.int64))
    assert D.shape == (0, 4) and I.shape == (0, 4)


# ---------------------------------------------------------------- 3. widest rows: 8 queries per pass
@pytest.mark.parametrize("metric", [L2, IP])
def test_widest_rows(metric):
    d, n, nlist = 2048, 300, 3
    assert sq_ref.qt_of(d) == 8
    rng = np.random.default_rng(2048)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s, "binary")
    xq = int_data("binary", rng, 17, d)
    assert_exact_range(xb, xq)
    assign = np.repeat(np.arange(nlist), [100, 130, 70])
    qz, index = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    force_add(index, xb, assign)
    check_lists(index, assign, base)
    # queries 8 .. 15 probe another list than queries 0 .. 7: a mask grouped by 16 hands them the wrong rows
    probes = np.array([[0]] * 8 + [[1]] * 8 + [[2]], np.int64)
    members = ivf_ref.probed_members(probes, assign, nlist)
    full = sq_ref.expected(xq, xb, n, metric)
    for nq in (1, 8, 9, 17):
        for k in (1, 33):
            D, I = search_pre(index, xq[:nq], k, probes[:nq])
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full[0][:nq], full[1][:nq], members[:nq], k, metric),
                                 f"nq={nq} k={k}")
    sqi = sq_index(d, SQ.QT_8bit, metric, t, xb)
    assert_knn_identical(*search_pre(index, xq, 33, np.tile(np.arange(nlist), (17, 1))), *sqi.search(xq, 33), "all lists")
    with pytest.raises(RuntimeError, match="ISE_SQ_MAX_D"):
        faiss.IndexIVFScalarQuantizer(faiss.IndexFlatL2(d + 1), d + 1, nlist, SQ.QT_8bit, metric, by_residual=False)


# ---------------------------------------------------------------- 4. more than two staging chunks
@pytest.mark.parametrize("metric", [L2, IP])
def test_chunks(metric):
    d, n, nlist, nq = 17, 700, 6, 130
    rng = np.random.default_rng(17)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit_uniform)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, nq, d)
    assign = rng.integers(0, nlist, n)
    qz, index = new_index(d, SQ.QT_8bit_uniform, metric, rng.standard_normal((nlist, d)), t)
    force_add(index, xb, assign)
    probes = rng.integers(0, nlist, (nq, 1))  # every query one list of its own choosing
    members = ivf_ref.probed_members(probes, assign, nlist)
    full = sq_ref.expected(xq, xb, n, metric)
    for k in (10, 40):
        D, I = search_pre(index, xq, k, probes)
        assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(*full, members, k, metric), f"k={k}")


# ---------------------------------------------------------------- 5. interleaved build
@pytest.mark.parametrize("metric", [L2, IP])
def test_interleaved_build(metric):
    d, nlist = 20, 4
    rng = np.random.default_rng(5)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, 601, d, m, s)
    xq = int_data("small", rng, 20, d)
    qz, index = new_index(d, SQ.QT_8bit, metric, xb[[3, 50, 200, 400]], t)
    assign = qz.search(xb, 1)[1].reshape(-1)
    index.nprobe = 2
    probes = qz.search(xq, 2)[1]
    have = 0
    for c in (100, 1, 500):  # each rebuild moves the old tiles to where their lists now start
        index.add(xb[have:have + c])
        have += c
        assert index.ntotal == have
        for k in (10, 40):
            D, I = counted(index, probes, k, lambda: index.search(xq, k))
            assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb[:have], probes, assign[:have], nlist, k, metric), f"n={have} k={k}")
        check_lists(index, assign[:have], base)
    # a NaN or inf row in the middle of an add: refused whole, by the class (no nearest centroid) and by the library (the encoder's flag)
    rows = xb[:9].copy()
    rows[4, 7] = np.nan
    with pytest.raises(ValueError, match="row 4"):
        index.add(rows)
    for bad in (np.nan, np.inf, -np.inf):
        rows[4, 7] = bad
        lists = np.ascontiguousarray(assign[:9], dtype=np.int64)
        assert native.lib.ise_ivfsq_add_host(index._h, rows.ctypes.data, lists.ctypes.data, 9) == native.E_INVALID
        assert b"NaN or inf" in native.lib.ise_last_error()
    lists = np.array([0, 1, nlist, 2], np.int64)
    assert native.lib.ise_ivfsq_add_host(index._h, xb[:4].ctypes.data, lists.ctypes.data, 4) == native.E_INVALID
    assert b"nothing was added" in native.lib.ise_last_error()
    assert index.ntotal == 601 and sizes_of(index) == np.bincount(assign, minlength=nlist).tolist()
    D, I = counted(index, probes, 10, lambda: index.search(xq, 10))
    assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb, probes, assign, nlist, 10, metric), "after the refused adds")
    index.add(xb[:30])  # a following add works
    xb2, assign2 = np.concatenate([xb, xb[:30]]), np.concatenate([assign, assign[:30]])
    D, I = counted(index, probes, 40, lambda: index.search(xq, 40))
    assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb2, probes, assign2, nlist, 40, metric), "after the next add")
    check_lists(index, assign2, np.concatenate([base, base[:30]]))
    # reset keeps the trained state and the quantiser
    index.reset()
    assert index.ntotal == 0 and index.is_trained and qz.ntotal == nlist and sizes_of(index) == [0] * nlist
    assert np.array_equal(index.sq.trained.view(np.uint32), t.view(np.uint32))
    D, I = counted(index, probes, 3, lambda: index.search(xq, 3))
    assert (I == -1).all() and (D == pad_value(metric)).all()
    index.add(xb[:70])
    D, I = counted(index, probes, 10, lambda: index.search(xq, 10))
    assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb[:70], probes, assign[:70], nlist, 10, metric), "after reset")
    with pytest.raises(RuntimeError):
        index.sq.set_trained(t)  # the index holds rows


# ---------------------------------------------------------------- 6. ties
@pytest.mark.parametrize("metric", [L2, IP])
def test_tie_group_over_five_lists(metric):
    """60 all-ones rows at ids 0 .. 59 tie at the top for the all-ones query (distance 0, score d); every other row has
    at most d - 4 ones.  Ids 0 .. 11 go to list 4, 12 .. 23 to list 3, ... 48 .. 59 to list 0: the smaller id sits in a
    LATER slot, in a higher list.  k = 5 and 20 cut inside the group; k = 40 puts the second pass's floor inside it."""
    d, n, nlist, ties = 24, 400, 5, 60
    rng = np.random.default_rng(66)
    t = np.concatenate([np.full(d, -0.5), np.full(d, 255.0)]).astype(np.float32)  # s = 1, m = 0: a row is its code
    xb = (rng.random((n, d)) < 0.6).astype(np.float32)
    xb[:, :4] = 0.0
    xb[:ties] = 1.0
    xq = np.ones((3, d), np.float32)
    xq[1, 0] = 0.0  # a second query that still ranks the group first: distance 1, score d - 1
    assert_exact_range(xb, xq)
    assign = np.concatenate([4 - np.arange(ties) // 12, rng.integers(0, nlist, n - ties)])
    qz, index = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    force_add(index, xb, assign)
    assert index.get_list(4)[0][0] == 0 and index.get_list(0)[0][0] == 48
    check_lists(index, assign, xb.astype(np.uint8))
    full = sq_ref.expected(xq, xb, n, metric)
    for probes in (np.tile(np.arange(nlist), (3, 1)), np.tile([4, 2, 0], (3, 1)), np.tile([1, 3], (3, 1))):
        members = ivf_ref.probed_members(probes, assign, nlist)
        for k in (1, 5, 20, 31, 32, 40, 70):
            D, I = search_pre(index, xq, k, probes)
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(*full, members, k, metric), f"k={k}")
        if probes.shape[1] == nlist:
            assert I[0, :ties].tolist() == list(range(ties)) and (D[0, :ties] == (0.0 if metric == L2 else d)).all()


# ---------------------------------------------------------------- 7. many entries per wave
def pass_blocks(tiles, d, device):
    """The grid of a pass (csrc/ise_ivfsq.hip, pass_grid): two tiles per wave of four, at most the blocks the CUs' LDS
    holds at once, at most the merge's 1024 lists."""
    import torch

    cu = torch.cuda.get_device_properties(device).multi_processor_count
    dpad = -(-d // 64) * 64
    qt = sq_ref.qt_of(d)
    lds = qt * (2 * (2 * dpad + 16) + 4 * 128 * 8 + 16)
    return max(1, min(-(-tiles // 8), max(1, sq_ref.LDS_LIMIT // lds) * cu, 1024))


@pytest.mark.parametrize("metric", [L2, IP])
def test_many_entries_per_wave(metric):
    """786 432 rows in 7 lists: every wave of the largest grid walks three entries or more, of several lists, so the
    ring of code bytes crosses entries and lists and the prefetch runs past a wave's last entry."""
    d, n, nlist, nq = 24, 786_432, 7, 20
    rng = np.random.default_rng(786)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    base = rng.integers(0, 2, (n, d)).astype(np.float32)
    xb = (m[None, :] + s[None, :] * base).astype(np.float32)
    xq = int_data("small", rng, nq, d)
    assign = rng.integers(0, nlist, n)
    qz, index = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    force_add(index, xb, assign)
    sizes = sizes_of(index)
    tiles = ivfsq_ref.tiles_of(sizes)
    blocks = pass_blocks(tiles, d, index.device)
    assert 12_288 <= tiles <= 12_288 + nlist and blocks <= 1024 and tiles >= 3 * 4 * 1024 >= 3 * 4 * blocks, (tiles, blocks)
    xb64 = xb.astype(np.float64)
    norms = (xb64 * xb64).sum(1)
    assert norms.max() + 2 * 15 * 24 * np.abs(xb64).max() + 15 * 15 * 24 < 1 << 24  # every partial sum is an exact float32
    every = np.arange(n, dtype=np.int64)
    sqi = sq_index(d, SQ.QT_8bit, metric, t, xb)
    probes2 = rng.integers(0, nlist, (nq, 2))
    members2 = ivf_ref.probed_members(probes2, assign, nlist)
    all_lists = np.tile(np.arange(nlist), (nq, 1))
    for k in (10, 33):
        D, I = search_pre(index, xq, k, all_lists)
        for q in (0, 7, 19):
            Dw, Iw = exact_top(xb64, norms, xq[q].astype(np.float64), every, k, metric)
            assert_knn_identical(D[q:q + 1], I[q:q + 1], Dw[None, :], Iw[None, :], f"all lists k={k} q={q}")
        assert_knn_identical(D, I, *sqi.search(xq, k), f"IndexScalarQuantizer.search k={k}")
        D, I = search_pre(index, xq, k, probes2)
        for q in range(nq):
            Dw, Iw = exact_top(xb64, norms, xq[q].astype(np.float64), members2[q], k, metric)
            assert_knn_identical(D[q:q + 1], I[q:q + 1], Dw[None, :], Iw[None, :], f"two lists k={k} q={q}")


@pytest.mark.parametrize("d", [130, 1473])  # QT = 16, 8
def test_one_block_cut_then_short_lists(d):
    """``sq_ref.one_block_case``: 512 rows in two lists of four full tiles, every list probed -- eight entries in one
    block, in row order.  Wave 0 streams entries 0 and 4 and cuts after the second (the rows lie in descending distance
    to query 0), k = 33 runs the floor-keyed second pass, and the last three queries are far from all rows: their lists
    end without a key in either pass."""
    assert sq_ref.qt_of(d) == (16 if d == 130 else 8)
    t, xb, base, plain, xq, Dw, Iw = sq_ref.one_block_case(d)
    assign = np.repeat(np.arange(2), 256)
    qz, index = new_index(d, SQ.QT_8bit, L2, np.random.default_rng(d).standard_normal((2, d)), t)
    force_add(index, xb, assign)
    check_lists(index, assign, base)
    D, I = search_pre(index, xq, 33, np.tile(np.arange(2), (16, 1)))
    assert_knn_identical(D, I, Dw, Iw, f"d={d}")
    assert (D[13:] == pad_value(L2)).all()


# ---------------------------------------------------------------- 8. real-valued data
def sq_scores_of(sqi, xq, I):
    """IndexScalarQuantizer's D for the pairs (q, I[q, r]), read out of its own deepest search."""
    Df, If = sqi.search(xq, min(sqi.ntotal, native.MAX_K))
    out = np.empty(I.shape, np.float32)
    for q in range(len(I)):
        order = np.argsort(If[q])
        pos = np.searchsorted(If[q][order], I[q])
        assert (If[q][order][np.minimum(pos, len(order) - 1)] == I[q]).all(), "a returned row lies beyond the flat search's depth"
        out[q] = Df[q][order][pos]
    return out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [100, 512])
def test_real_valued_data(d, metric):
    n, nlist, nq = 3000, 8, 33
    rng = np.random.default_rng(3000 + d)
    xb = (3.0 + rng.standard_normal((n, d))).astype(np.float32)
    xq = (3.0 + rng.standard_normal((nq, d))).astype(np.float32)
    qz = faiss.IndexFlatL2(d)
    index = faiss.IndexIVFScalarQuantizer(qz, d, nlist, SQ.QT_8bit, metric, by_residual=False)
    assert not index.is_trained
    with pytest.raises(RuntimeError):
        index.add(xb[:4])
    with pytest.raises(RuntimeError):
        index.search(xq, 3)
    index.train(xb)
    assert index.is_trained and qz.ntotal == nlist
    t = index.sq.trained
    assert np.array_equal(t.view(np.uint32), sq_ref.train_minmax(xb, SQ.QT_8bit).view(np.uint32))
    index.add(xb)
    assign = qz.search(xb, 1)[1].reshape(-1)
    vmin, vdiff = sq_ref.expand(t, d, SQ.QT_8bit)
    sqi = sq_index(d, SQ.QT_8bit, metric, t, xb)
    codes = sqi.codes
    dec = sq_ref.decode(codes, vmin, vdiff)
    check_lists(index, assign, codes)
    for nprobe, k in ((1, 10), (3, 10), (3, 70), (nlist, 33)):
        index.nprobe = nprobe
        probes = qz.search(xq, nprobe)[1]
        members = ivf_ref.probed_members(probes, assign, nlist)
        D, I = counted(index, probes, k, lambda: index.search(xq, k))
        D_ref, I_ref = ivf_ref.expected_brute(dec, xq, members, k, metric)
        err = np.abs(D.astype(np.float64) - D_ref) / np.maximum(1.0, np.abs(D_ref))
        print(f"d={d} metric={metric} nprobe={nprobe} k={k}: largest relative error {err[I_ref >= 0].max():.3e} (bound {RTOL:g})")
        assert_knn_matches(D, I, D_ref, I_ref, dec, xq, metric)
        # the bits IndexScalarQuantizer reports for the same (query, row) pairs
        assert np.array_equal(D.view(np.uint32), sq_scores_of(sqi, xq, I).view(np.uint32)), f"nprobe={nprobe} k={k}"
        if nprobe == nlist:
            assert_knn_identical(D, I, *sqi.search(xq, k), "all lists")


# ---------------------------------------------------------------- 9. device forms
def test_device_forms():
    import torch

    d, n, nlist = 40, 900, 6
    rng = np.random.default_rng(9)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, 70, d)
    cent = xb[[1, 2, 3, 5, 8, 13]]
    qz, index = new_index(d, SQ.QT_8bit, L2, cent, t)
    qz2, index2 = new_index(d, SQ.QT_8bit, L2, cent, t)
    dev = torch.device("cuda", index.device)
    index.add(xb)
    index2.add_torch(torch.from_numpy(xb[:300]).to(dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        index2.add_torch(torch.from_numpy(xb[300:]).to(dev))
    assert index2.ntotal == n
    assign = qz.search(xb, 1)[1].reshape(-1)
    check_lists(index2, assign, base)
    xq_t = torch.from_numpy(xq).to(dev)
    for nprobe, k in ((1, 10), (3, 33), (nlist, 5), (50, 70)):  # nprobe beyond nlist is clipped
        index.nprobe = index2.nprobe = nprobe
        probes = qz.search(xq, min(nprobe, nlist))[1]
        D, I = counted(index, probes, k, lambda: index.search(xq, k))
        assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb, probes, assign, nlist, k, L2), f"host nprobe={nprobe}")
        Dt, It = counted(index2, probes, k, lambda: index2.search_torch(xq_t, k))
        assert Dt.is_cuda and Dt.dtype == torch.float32 and It.dtype == torch.int64
        assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D, I, f"torch nprobe={nprobe}")
        with torch.cuda.stream(side):  # the same handle from another stream: ordered behind the call before
            Ds, Is = index2.search_torch(xq_t, k)
        side.synchronize()
        assert_knn_identical(Ds.cpu().numpy(), Is.cpu().numpy(), D, I, f"side stream nprobe={nprobe}")
    # a query with a NaN or inf entry is padding, in both forms
    bad = xq[:5].copy()
    bad[1, 4] = np.nan
    bad[3, 0] = np.inf
    index.nprobe = index2.nprobe = 2
    D, I = index.search(bad, 5)
    assert (I[[1, 3]] == -1).all() and (D[[1, 3]] == pad_value(L2)).all() and (I[[0, 2, 4]] >= 0).all()
    assert_knn_identical(D[[0, 2, 4]], I[[0, 2, 4]], *index.search(xq[[0, 2, 4]], 5), "beside a NaN query")
    Dt, It = index2.search_torch(torch.from_numpy(bad).to(dev), 5)
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D, I, "NaN query, torch")
    rows = xb[:6].copy()
    rows[4, 0] = np.nan
    with pytest.raises(ValueError, match="row 4"):
        index2.add_torch(torch.from_numpy(rows).to(dev))
    rows_t, lists_t = torch.from_numpy(rows).to(dev), torch.zeros(6, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    rc = native.lib.ise_ivfsq_add_device(index2._h, rows_t.data_ptr(), lists_t.data_ptr(), 6, None)
    assert rc == native.E_INVALID and b"NaN or inf" in native.lib.ise_last_error() and index2.ntotal == n
    Dt, It = index2.search_torch(xq_t, 10)
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), *index.search(xq, 10), "after the refused adds")
    Dt, It = index2.search_torch(xq_t[:0], 4)
    assert tuple(Dt.shape) == (0, 4) and tuple(It.shape) == (0, 4)


# ---------------------------------------------------------------- 10. composition
def test_composition(tmp_path):
    from image_search_engine_amd.utils import create_search_index

    d, n, k = 32, 2000, 10
    rng = np.random.default_rng(10)
    x = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((17, d)).astype(np.float32)
    # the reference's call (backend/utils.py:311-325) with the scalar quantiser in the product quantiser's place
    index = create_search_index(x.copy(), "cell-probe-sq8")
    assert isinstance(index, faiss.IndexIVFScalarQuantizer) and (index.nprobe, index.nlist, index.ntotal) == (5, 8, n)
    assert index.quantizer.metric_type == L2 and index.quantizer.ntotal == 8 and index.qtype == SQ.QT_8bit and not index.by_residual
    assign = index.quantizer.search(x, 1)[1].reshape(-1)
    t = index.sq.trained
    vmin, vdiff = sq_ref.expand(t, d, SQ.QT_8bit)
    codes = index.sq.compute_codes(x)
    dec = sq_ref.decode(codes, vmin, vdiff)
    check_lists(index, assign, codes)
    probes = index.quantizer.search(xq, 5)[1]
    D, I = counted(index, probes, k, lambda: index.search(xq, k))
    D_ref, I_ref = ivf_ref.expected_brute(dec, xq, ivf_ref.probed_members(probes, assign, 8), k, L2)
    assert_knn_matches(D, I, D_ref, I_ref, dec, xq, L2)
    # write_index -> read_index: identical lists, identical search bits
    path = tmp_path / "ivfsq.index"
    faiss.write_index(index, str(path))
    back = faiss.read_index(str(path))
    assert isinstance(back, faiss.IndexIVFScalarQuantizer) and back.is_trained and not back.by_residual
    assert (back.d, back.nlist, back.nprobe, back.ntotal, back.qtype, back.metric_type) == (d, 8, 5, n, SQ.QT_8bit, L2)
    assert np.array_equal(back.sq.trained.view(np.uint32), t.view(np.uint32))
    assert np.array_equal(back.quantizer.reconstruct_n(0, 8).view(np.uint32), index.quantizer.reconstruct_n(0, 8).view(np.uint32))
    check_lists(back, assign, codes)
    for kk in (k, 40):
        assert_knn_identical(*back.search(xq, kk), *index.search(xq, kk), f"read back k={kk}")
    empty = faiss.IndexIVFScalarQuantizer(faiss.IndexFlatL2(d), d, 3, SQ.QT_8bit_uniform, IP, by_residual=False)
    with pytest.raises(RuntimeError):
        faiss.write_index(empty, str(path))  # untrained
    empty.train(x[:50])
    faiss.write_index(empty, str(path))
    back0 = faiss.read_index(str(path))
    assert (back0.ntotal, back0.nlist, back0.qtype, back0.metric_type, back0.is_trained) == (0, 3, SQ.QT_8bit_uniform, IP, True)
    buf = bytearray(path.read_bytes())
    buf[-(3 * 8 + 4 + 8 + 16 + 4 + 1)] = 1  # the by_residual byte in front of the (empty) lists
    path.write_bytes(bytes(buf))
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.read_index(str(path))
    # IndexRefineFlat over it, every list probed: the candidates needed are the worst rank, in the base's order, of a row
    # of the exact answer (one more for a float32 near-tie at the cut)
    flat = faiss.IndexFlatL2(d)
    flat.add(x)
    De, Ie = flat.search(xq, k)
    base_rank = sq_ref.expected(xq, dec, n, L2)[1]
    worst = max(int(np.flatnonzero(np.isin(base_rank[q], Ie[q])).max()) for q in range(len(xq)))
    k_factor = (worst + 2 + k - 1) // k
    assert k * k_factor < n // 4, "the derived depth is a small part of the index"
    qz = faiss.IndexFlatL2(d)
    qz.add(index.quantizer.reconstruct_n(0, 8))
    refine = faiss.IndexRefineFlat(faiss.IndexIVFScalarQuantizer(qz, d, 8, SQ.QT_8bit, L2, by_residual=False))
    refine.train(x)
    refine.add(x)
    refine.base_index.nprobe = 8
    refine.k_factor = k_factor
    assert_knn_identical(*refine.search(xq, k), De, Ie, f"refined at k_factor={k_factor}")
    import torch

    Dt, It = refine.search_torch(torch.from_numpy(xq).to(torch.device("cuda", refine.device)), k)
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), De, Ie, "refined, torch")


# ---------------------------------------------------------------- 11. what raises
def test_what_raises():
    d, nlist = 16, 4
    rng = np.random.default_rng(11)
    x = rng.standard_normal((200, d)).astype(np.float32)
    qz = faiss.IndexFlatL2(d)
    index = faiss.IndexIVFScalarQuantizer(qz, d, nlist, SQ.QT_8bit, L2, by_residual=False)
    assert not index.is_trained
    for call in (lambda: index.add(x), lambda: index.search(x[:2], 3), lambda: index.search_preassigned(x[:2], 3, np.zeros((2, 1))),
                 lambda: faiss.write_index(index, "/nonexistent/never-written")):
        with pytest.raises(RuntimeError, match="before train"):
            call()
    index.sq.set_trained(sq_ref.train_minmax(x, SQ.QT_8bit))
    assert not index.is_trained  # the quantiser is still empty
    with pytest.raises(RuntimeError, match="before train"):
        index.add(x)
    with pytest.raises(RuntimeError):
        index.train(x[:3])  # fewer rows than lists
    with pytest.raises(AssertionError, match="dimension mismatch"):
        faiss.IndexIVFScalarQuantizer(faiss.IndexFlatL2(d + 1), d, nlist, SQ.QT_8bit, L2, by_residual=False)
    with pytest.raises(AssertionError):
        faiss.IndexIVFScalarQuantizer(faiss.IndexPQ(d, 4), d, nlist, SQ.QT_8bit, L2, by_residual=False)
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFScalarQuantizer(qz, d, nlist, SQ.QT_8bit)
    with pytest.raises(NotImplementedError, match="qtype"):
        faiss.IndexIVFScalarQuantizer(qz, d, nlist, SQ.QT_fp16, L2, by_residual=False)
    index.train(x)
    assert index.is_trained and qz.ntotal == nlist
    index.add(x)
    with pytest.raises(NotImplementedError):
        index.search(x[:2], 3, params=faiss.SearchParameters())
    import torch

    with pytest.raises(NotImplementedError):
        index.search_torch(torch.from_numpy(x[:2]).to(torch.device("cuda", index.device)), 3, params=faiss.SearchParameters())
    with pytest.raises(NotImplementedError, match="IndexIVFScalarQuantizer"):
        index.range_search(x[:2], 1.0)
    with pytest.raises(NotImplementedError, match="IndexIVFScalarQuantizer"):
        index.remove_ids([1])
    with pytest.raises(NotImplementedError, match="IndexIVFScalarQuantizer"):
        faiss.IndexIDMap(index)
    with pytest.raises(AssertionError):
        faiss.IndexRefineFlat(index)  # wraps an empty index only
    for k in (0, native.MAX_K + 1):
        with pytest.raises((AssertionError, RuntimeError)):
            index.search(x[:2], k)
