"""GPU tests of IndexIVFPQ with by_residual=False (include/ise_knn.h, ise_ivfpq_*; csrc/ise_ivfpq.hpp).  On integer
codebooks, rows and queries (the construction of tests/test_pq_gpu.py) every comparison is bit for bit: against the
float64 ranking over the decoded rows cut to each query's probed members (tests/ivfpq_ref.py) and against an IndexPQ with
the same centroids over the same rows.  Every search also asserts what it adds to ``ivfpq_stats``: one batch, the
passes, the 64-row tiles of the probed lists and no others, and the table builds."""
import numpy as np
import pytest

from image_search_engine_amd import _native as native
from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref, ivfpq_ref, pq_ref
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data
from tests.sel_ref import IP, L2, pad_value

pytestmark = pytest.mark.gpu

CHUNKS = [250, 1, 349]  # the three add calls
STAT_KEYS = ("batches", "passes", "tiles_loaded", "table_builds")
PAD_ID = 0xFFFFFFFF


def new_index(d, M, metric, cent, C):
    qz = faiss.IndexFlatL2(d)
    qz.add(np.ascontiguousarray(cent, dtype=np.float32))
    index = faiss.IndexIVFPQ(qz, d, len(cent), M, 8, metric, by_residual=False)
    assert not index.is_trained and index.ntotal == 0 and index.nprobe == 1 and index.quantizer is qz
    assert (index.nlist, index.by_residual, index.code_size, index.sa_code_size(), index.M) == (len(cent), False, M, M, M)
    pq = index.pq
    assert (pq.d, pq.M, pq.nbits, pq.dsub, pq.ksub, pq.code_size) == (d, M, 8, d // M, 256, M)
    pq.set_centroids(C)
    assert index.is_trained and np.array_equal(pq.centroids.view(np.uint32), np.asarray(C, np.float32).view(np.uint32))
    return qz, index


def pq_index(d, M, metric, C, codes=None):
    pqi = faiss.IndexPQ(d, M, 8, metric)
    pqi.pq.set_centroids(C)
    if codes is not None and len(codes):
        pqi._add_codes(codes)
    return pqi


def force_add(index, x, lists):
    """Rows into the lists the test names (the library takes list numbers; the class asks its quantiser)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lists = np.ascontiguousarray(lists, dtype=np.int64)
    faiss._check_rows(native.lib.ise_ivfpq_add_host(index._h, x.ctypes.data, lists.ctypes.data, len(x)))


def sizes_of(index):
    return [index.list_size(l) for l in range(index.nlist)]


def counted(index, probes, k, call):
    """call() -> (D, I), with the statistics it adds asserted against the reference's count."""
    nq = len(probes)
    want = ivfpq_ref.stats_of(probes, sizes_of(index), index.M, k, nq) if index.ntotal and nq else \
        {"batches": 1 if nq else 0, "passes": 0, "tiles_loaded": 0, "table_builds": 0}
    before = index.ivfpq_stats()
    out = call()
    after = index.ivfpq_stats()
    got = {key: after[key] - before[key] for key in STAT_KEYS}
    assert got == want, (got, want)
    return out


def search_pre(index, xq, k, probes):
    return counted(index, probes, k, lambda: index.search_preassigned(xq, k, probes))


def check_lists(index, assign, codes):
    for l, want in enumerate(ivf_ref.list_members(assign, index.nlist)):
        ids, got = index.get_list(l)
        assert ids.dtype == np.int64 and got.dtype == np.uint8 and got.shape == (len(want), index.M)
        assert np.array_equal(ids, want) and (np.diff(ids) > 0).all() and index.list_size(l) == len(want)
        assert np.array_equal(got, codes[want])


def integer_case(M, dsub, kind, n, nq, nlist, seed):
    rng = np.random.default_rng(seed)
    d = M * dsub
    C = int_data(kind, rng, M * 256, dsub).reshape(M, 256, dsub)
    xb, xq = int_data(kind, rng, n, d), int_data(kind, rng, nq, d)
    cent = int_data(kind, rng, nlist, d)
    return d, C, xb, xq, cent


# ---------------------------------------------------------------- 1. the grid of cases
# every QT (16: M <= 5, 8: <= 15, 4: <= 35, 2: above) and strides of one to four 16-byte pieces (M = 17: two, 36: three)
SHAPES = [(1, 4, "small"), (4, 1, "small"), (4, 4, "binary"), (8, 4, "small"), (8, 1, "signed"), (16, 1, "small"),
          (16, 4, "signed"), (17, 4, "signed"), (36, 1, "signed"), (36, 4, "signed"), (64, 1, "signed"), (64, 4, "signed")]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M,dsub,kind", SHAPES)
def test_sweep(M, dsub, kind, metric):
    n, nlist = 600, 8
    d, C, xb, xq, cent = integer_case(M, dsub, kind, n, 40, nlist, 5000 + 7 * M + dsub)
    qz, index = new_index(d, M, metric, cent, C)
    index.train(xb)  # a no-op: both halves are trained
    assert qz.ntotal == nlist and np.array_equal(index.pq.centroids.view(np.uint32), C.view(np.uint32))
    i0 = 0
    for c in CHUNKS:
        index.add(xb[i0:i0 + c])
        i0 += c
        assert index.ntotal == i0
    assign = qz.search(xb, 1)[1].reshape(-1)
    assert sizes_of(index) == np.bincount(assign, minlength=nlist).tolist()
    codes = pq_ref.encode(xb, C)
    dec = pq_ref.decode(codes, C)
    assert np.array_equal(index.sa_encode(xb[:70]), codes[:70]) and np.array_equal(index.pq.compute_codes(xb[:3]), codes[:3])
    assert np.array_equal(index.sa_decode(codes[:70]).view(np.uint32), dec[:70].view(np.uint32))
    assert_exact_range(dec, xq)
    check_lists(index, assign, codes)
    pqi = pq_index(d, M, metric, C, codes)
    full_ref = ivfpq_ref.full_ranking(xq, C, codes, metric)  # the complete rankings, computed once
    full_pq = pqi.search(xq, n)
    assert_knn_identical(*full_pq, *full_ref, "the flat product-quantised index")
    qt = pq_ref.qt_of(M)
    for nq in sorted({1, qt, qt + 1, 40}):
        for nprobe in (1, 2, nlist):
            index.nprobe = nprobe
            probes = qz.search(xq[:nq], nprobe)[1]
            members = ivf_ref.probed_members(probes, assign, nlist)
            for k in (1, 10, 33, 70):
                what = f"nq={nq} nprobe={nprobe} k={k}"
                D, I = counted(index, probes, k, lambda: index.search(xq[:nq], k))
                assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full_ref[0][:nq], full_ref[1][:nq], members, k, metric), what)
                assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full_pq[0][:nq], full_pq[1][:nq], members, k, metric),
                                     "IndexPQ's bits " + what)
                if nprobe == nlist:
                    assert_knn_identical(D, I, *pqi.search(xq[:nq], k), "all lists " + what)
    check_lists(index, assign, codes)


# ---------------------------------------------------------------- 2. list and tile edges
EDGE_SIZES = [0, 1, 63, 64, 65, 128, 129]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M", [4, 16])
def test_list_and_tile_edges(M, metric):
    nlist, n, nq = len(EDGE_SIZES), sum(EDGE_SIZES), 9
    d, C, xb, xq, cent = integer_case(M, 2, "signed", n, nq, nlist, 61 + M)
    rng = np.random.default_rng(62)
    assign = rng.permutation(np.repeat(np.arange(nlist), EDGE_SIZES))
    qz, index = new_index(d, M, metric, cent, C)
    # an empty index: padding, one batch, no pass, no tile, no table
    D, I = search_pre(index, xq, 5, np.zeros((nq, 1), np.int64))
    assert (I == -1).all() and (D == pad_value(metric)).all() and D.dtype == np.float32 and I.dtype == np.int64
    force_add(index, xb, assign)
    assert sizes_of(index) == EDGE_SIZES and index.ntotal == n
    codes = pq_ref.encode(xb, C)
    check_lists(index, assign, codes)
    full = ivfpq_ref.full_ranking(xq, C, codes, metric)
    tables = [np.tile(np.arange(nlist), (nq, 1)),                                         # every list: 10 tiles
              np.array([[l] for l in (0, 1, 2, 3, 4, 5, 6, 1, 4)], np.int64),            # one list each: the queries of
              np.array([[4, -1, 4], [nlist, -1, nlist], [-1, -1, -1], [0, 0, -1], [6, 5, 6], [2, nlist + 5, 3], [-7, 1, 1],
                        [5, 5, 5], [3, 2, -1]], np.int64)]                                # a group probe disjoint lists
    for probes in tables:
        members = ivf_ref.probed_members(probes, assign, nlist)
        for k in (1, 5, 66, 200):  # 200 exceeds every member set but the first table's: the tail is padding
            D, I = search_pre(index, xq, k, probes)
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(*full, members, k, metric), f"k={k}")
            for q, mem in enumerate(members):
                assert (I[q, len(mem):] == -1).all() and (I[q, :min(k, len(mem))] >= 0).all()
    # rows of only -1: padding, and the pass costs no tile (counted asserts tiles_loaded == 0)
    D, I = search_pre(index, xq, 40, np.full((nq, 2), -1, np.int64))
    assert (I == -1).all() and (D == pad_value(metric)).all()
    # one list, one query: exactly that list's tiles
    for l, size in enumerate(EDGE_SIZES):
        t0 = index.ivfpq_stats()["tiles_loaded"]
        index.search_preassigned(xq[:1], 3, np.array([[l]]))
        assert index.ivfpq_stats()["tiles_loaded"] - t0 == -(-size // 64)
    D, I = index.search(xq[:0], 4)
    assert D.shape == (0, 4) and I.shape == (0, 4)


# ---------------------------------------------------------------- 3. the pad-slot trap
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M", [4, 16, 36])
def test_pad_slots_never_enter(M, metric):
    """The all-zero code -- what a pad slot holds -- scores strictly best for every query, and no stored row has it: only
    the position mask keeps the pad slots (id 0xFFFFFFFF) out.  The lists are built in three adds with a search after
    each; the first list grows by a tile each time, so every rebuild moves the old tiles of the others."""
    dsub, nlist, nq = 2, 4, 5
    d = M * dsub
    rng = np.random.default_rng(300 + M)
    C = rng.integers(1, 3, (M, 256, dsub)).astype(np.float32)
    if metric == L2:
        C[:, 0, :] = 0.0   # centroid 0 of every sub-quantiser is the query itself: the zero code scores 0, all others > 0
        xq = np.zeros((nq, d), np.float32)
        zero_score = 0.0
    else:
        C[:, 0, :] = 3.0   # ... or the longest centroid along an all-ones query
        xq = np.ones((nq, d), np.float32)
        zero_score = 3.0 * d
    stages = [[60, 1, 20, 30], [70, 1, 63, 40], [130, 1, 63, 65]]  # tiles 1 1 1 1 | 2 1 1 1 | 3 1 1 2
    n = sum(stages[-1])
    raw = rng.integers(0, 256, (n, M)).astype(np.uint8)
    raw[:, 0] = np.maximum(raw[:, 0], 1)
    xb = pq_ref.decode(raw, C)
    codes = pq_ref.encode(xb, C)  # (the lowest number among equal centroids: what the index stores)
    assert codes.any(axis=1).all() and (codes[:, 0] > 0).all()  # no stored row has the zero code
    scores = pq_ref.adc_scores(xq, C, np.zeros((1, M), np.uint8), metric)
    assert (scores == zero_score).all()
    best_row = pq_ref.adc_scores(xq, C, codes, metric)
    assert (best_row > zero_score).all() if metric == L2 else (best_row < zero_score).all()
    qz, index = new_index(d, M, metric, rng.standard_normal((nlist, d)), C)
    assign = np.zeros(0, np.int64)
    have = [0] * nlist
    probes = np.tile(np.arange(nlist), (nq, 1))
    for stage in stages:
        new = np.concatenate([np.full(s - h, l, np.int64) for l, (s, h) in enumerate(zip(stage, have))])
        new = rng.permutation(new)
        i0 = len(assign)
        force_add(index, xb[i0:i0 + len(new)], new)
        assign = np.concatenate([assign, new])
        have = stage
        for poison in (np.nan, np.inf):  # a refused add in between changes nothing
            bad = xb[:3].copy()
            bad[1, d - 1] = poison
            with pytest.raises(ValueError, match="NaN or inf"):
                force_add(index, bad, np.zeros(3, np.int64))
            assert index.ntotal == len(assign) and sizes_of(index) == stage
        m = len(assign)
        full = ivfpq_ref.full_ranking(xq, C, codes[:m], metric)
        for k in (1, 40, m + 7):
            D, I = search_pre(index, xq, k, probes)
            assert not (I == PAD_ID).any() and not (D == np.float32(zero_score)).any()
            assert I.max() < m and ((I >= 0).sum(1) == min(k, m)).all()
            assert_knn_identical(D, I, full[0][:, :k] if k <= m else np.pad(full[0], ((0, 0), (0, k - m)), constant_values=pad_value(metric)),
                                 full[1][:, :k] if k <= m else np.pad(full[1], ((0, 0), (0, k - m)), constant_values=-1), f"m={m} k={k}")
        check_lists(index, assign, codes[:m])
    assert sizes_of(index) == stages[-1]


# ---------------------------------------------------------------- 4. a tie group over five lists
@pytest.mark.parametrize("metric", [L2, IP])
def test_tie_group_over_five_lists(metric):
    """80 rows with one code -- query 0's best -- spread over the five lists, the smaller ids in the later lists (so in
    later slots): ranks 0 .. 79 of query 0 are the group in ascending id, and with k = 33 the second pass's floor key (rank
    31) falls inside it."""
    M, dsub, nlist = 16, 1, 5
    d, C, xb, xq, cent = integer_case(M, dsub, "small", 400, 6, nlist, 77)
    rng = np.random.default_rng(78)
    codes = pq_ref.encode(xb, C)
    group = np.arange(10, 90)
    tables = pq_ref.adc_tables(xq[:1], C, metric)[0]  # (M, 256): the group's code is query 0's best in every sub-quantiser
    codes[group] = (np.argmin(tables, axis=1) if metric == L2 else np.argmax(tables, axis=1)).astype(np.uint8)
    assign = rng.integers(0, nlist, len(codes))
    assign[group] = 4 - (group - 10) // 16
    qz, index = new_index(d, M, metric, cent, C)
    index._add_codes(codes, assign)
    pqi = pq_index(d, M, metric, C, codes)
    check_lists(index, assign, codes)
    full = ivfpq_ref.full_ranking(xq, C, codes, metric)
    assert np.array_equal(full[1][0][:80], group) and len(set(full[0][0][:80].tolist())) == 1
    assert full[0][0][80] != full[0][0][79]
    probes = np.tile(np.arange(nlist), (len(xq), 1))
    for k in (1, 33, 64, 70, 120):
        D, I = search_pre(index, xq, k, probes)
        assert_knn_identical(D, I, full[0][:, :k], full[1][:, :k], f"k={k}")
        assert_knn_identical(D, I, *pqi.search(xq, k), f"IndexPQ k={k}")
    # lists 4 and 3 alone: the group's ids 10 .. 41
    probes = np.tile(np.array([4, 3]), (len(xq), 1))
    D, I = search_pre(index, xq, 33, probes)
    assert_knn_identical(D, I, *ivfpq_ref.expected(xq, C, codes, probes, assign, nlist, 33, metric, full), "two lists")


# ---------------------------------------------------------------- 5. three staging chunks
@pytest.mark.parametrize("M", [4, 17, 64])
def test_130_queries(M):
    n, nlist, nq = 500, 8, 130
    d, C, xb, xq, cent = integer_case(M, 2, "signed", n, nq, nlist, 900 + M)
    qz, index = new_index(d, M, L2, cent, C)
    index.add(xb)
    assign = qz.search(xb, 1)[1].reshape(-1)
    codes = pq_ref.encode(xb, C)
    full = ivfpq_ref.full_ranking(xq, C, codes, L2)
    for nprobe, k in ((2, 10), (3, 40)):
        index.nprobe = nprobe
        probes = qz.search(xq, nprobe)[1]
        D, I = counted(index, probes, k, lambda: index.search(xq, k))
        assert_knn_identical(D, I, *ivfpq_ref.expected(xq, C, codes, probes, assign, nlist, k, L2, full), f"nprobe={nprobe}")


# ---------------------------------------------------------------- 6. three entries per wave at the largest grid
def test_long_lists_equal_the_flat_index():
    """393 216 rows at M = 16 in 64 lists: 6144 tiles and more, so three or more entries per wave at the 512 blocks of
    four waves a 256-CU device launches (two blocks of 80 KiB per CU)."""
    M, dsub, nlist, n, nq = 16, 1, 64, 393216, 5
    rng = np.random.default_rng(6)
    d = M * dsub
    C = int_data("small", rng, M * 256, dsub).reshape(M, 256, dsub)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    assign = rng.integers(0, nlist, n)
    xq = int_data("small", rng, nq, d)
    qz, index = new_index(d, M, L2, int_data("small", rng, nlist, d), C)
    index._add_codes(codes, assign)
    pqi = pq_index(d, M, L2, C, codes)
    index.nprobe = nlist
    probes = np.tile(np.arange(nlist), (nq, 1))
    want = pq_ref.adc_topk(pq_ref.adc_scores(xq, C, codes, L2), 40, L2)
    for k in (10, 40):
        D, I = counted(index, probes, k, lambda: index.search(xq, k))
        assert_knn_identical(D, I, *pqi.search(xq, k), f"IndexPQ k={k}")
        assert_knn_identical(D, I, want[0][:, :k], want[1][:, :k], f"k={k}")
    assert sum(-(-s // 64) for s in sizes_of(index)) >= 3 * 512 * 4


# ---------------------------------------------------------------- 7. real-valued data: the construction claim
@pytest.mark.parametrize("metric", [L2, IP])
def test_real_data_has_the_flat_index_bits(metric):
    d, M, n, nlist, nq = 64, 16, 2000, 8, 23  # n <= ISE_MAX_K: IndexPQ ranks every row
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    qz, index = new_index(d, M, metric, xb[:nlist], C)
    index.add(xb)
    pqi = pq_index(d, M, metric, C)
    pqi.add(xb)
    Dp, Ip = pqi.search(xq, n)
    by_id = np.empty((nq, n), np.uint32)  # IndexPQ's bits of every (query, row) pair
    np.put_along_axis(by_id, Ip, Dp.view(np.uint32), axis=1)
    assert (Ip >= 0).all()
    assign = qz.search(xb, 1)[1].reshape(-1)
    check_lists(index, assign, pqi.codes)
    for nprobe in (1, 3, nlist):
        index.nprobe = nprobe
        probes = qz.search(xq, nprobe)[1]
        for k in (10, 40):
            D, I = counted(index, probes, k, lambda: index.search(xq, k))
            assert (I >= 0).all()
            assert np.array_equal(D.view(np.uint32), np.take_along_axis(by_id, I, axis=1)), f"nprobe={nprobe} k={k}"
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(Dp, Ip, ivf_ref.probed_members(probes, assign, nlist), k, metric),
                                 f"cut of IndexPQ's ranking nprobe={nprobe} k={k}")
            if nprobe == nlist:
                assert_knn_identical(D, I, Dp[:, :k], Ip[:, :k], f"all lists k={k}")


# ---------------------------------------------------------------- 8. the device forms
def test_device_forms_on_two_streams():
    import torch

    M, dsub, nlist, n = 16, 2, 8, 700
    d, C, xb, xq, cent = integer_case(M, dsub, "signed", n, 21, nlist, 88)
    qz, index = new_index(d, M, L2, cent, C)
    dev = torch.device("cuda", index.device)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        xb_dev = torch.from_numpy(xb).to(dev)
        index.add_torch(xb_dev[:300])
        index.add_torch(xb_dev[300:])
    assert index.ntotal == n
    s1.synchronize()
    assign = qz.search(xb, 1)[1].reshape(-1)
    codes = pq_ref.encode(xb, C)
    check_lists(index, assign, codes)
    full = ivfpq_ref.full_ranking(xq, C, codes, L2)
    index.nprobe = 3
    probes = qz.search(xq, 3)[1]
    want = ivfpq_ref.expected(xq, C, codes, probes, assign, nlist, 40, L2, full)
    outs = []
    for s in (s2, s1, s2):
        with torch.cuda.stream(s):
            xq_dev = torch.from_numpy(xq).to(dev)
            outs.append((s, counted(index, probes, 40, lambda: index.search_torch(xq_dev, 40))))
    for s, (D, I) in outs:
        s.synchronize()
        assert D.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64
        assert_knn_identical(D.cpu().numpy(), I.cpu().numpy(), *want, "search_torch")
    # an add on one stream, the search that rebuilds on the other
    extra = int_data("signed", np.random.default_rng(89), 70, d)
    with torch.cuda.stream(s1):
        index.add_torch(torch.from_numpy(extra).to(dev))
    with torch.cuda.stream(s2):
        D, I = index.search_torch(torch.from_numpy(xq).to(dev), 10)
    s2.synchronize()
    xb2, codes2 = np.concatenate([xb, extra]), np.concatenate([codes, pq_ref.encode(extra, C)])
    assign2 = qz.search(xb2, 1)[1].reshape(-1)
    assert_knn_identical(D.cpu().numpy(), I.cpu().numpy(), *ivfpq_ref.expected(xq, C, codes2, probes, assign2, nlist, 10, L2), "after add")
    # reset keeps the trained state
    index.reset()
    assert index.ntotal == 0 and index.is_trained and sizes_of(index) == [0] * nlist
    D, I = index.search(xq, 3)
    assert (I == -1).all() and (D == pad_value(L2)).all()
    index.add(xb[:100])
    D, I = index.search(xq, 3)
    assert_knn_identical(D, I, *ivfpq_ref.expected(xq, C, codes[:100], probes, assign[:100], nlist, 3, L2), "after reset")


# ---------------------------------------------------------------- 9. the rest of the interface
def clustered(rng, n, d, nclusters):
    centres = rng.standard_normal((nclusters, d)).astype(np.float32) * 4.0
    return (centres[rng.integers(0, nclusters, n)] + rng.standard_normal((n, d)).astype(np.float32) * 0.5).astype(np.float32)


def test_train_gives_the_flat_index_codebook():
    """Integer rows: every centroid update of ``Kmeans`` is then a sum of integers below 2^24 -- exact in float32 in any
    order -- divided once, so two trainings from the same seed agree bit for bit (on real-valued rows the device's
    scatter-add sums in no fixed order, for ``IndexPQ.train`` against itself too)."""
    d, M, nlist, n = 16, 4, 6, 1200
    rng = np.random.default_rng(91)
    xb = int_data("small", rng, n, d)
    # an empty quantiser: k-means, then the codebook
    index = faiss.IndexIVFPQ(faiss.IndexFlatL2(d), d, nlist, M, 8, faiss.METRIC_L2, by_residual=False)
    assert not index.is_trained
    with pytest.raises(RuntimeError, match="before train"):
        index.add(xb)
    index.pq.cp.niter = 3
    index.train(xb)
    assert index.is_trained and index.quantizer.ntotal == nlist
    pqi = faiss.IndexPQ(d, M, 8)
    pqi.cp.niter = 3
    pqi.train(xb)
    assert np.array_equal(index.pq.centroids.view(np.uint32), pqi.pq.centroids.view(np.uint32))
    cent, cb = index.quantizer.reconstruct_n(0, nlist), index.pq.centroids
    index.train(xb[::-1])  # trained: nothing
    assert np.array_equal(index.quantizer.reconstruct_n(0, nlist), cent) and np.array_equal(index.pq.centroids, cb)
    # a given quantiser is left as it is
    qz = faiss.IndexFlatL2(d)
    qz.add(xb[:nlist])
    given = faiss.IndexIVFPQ(qz, d, nlist, M, by_residual=False)
    assert not given.is_trained
    given.pq.cp.niter = 3
    given.train(xb)
    assert given.is_trained and np.array_equal(qz.reconstruct_n(0, nlist), xb[:nlist])
    assert np.array_equal(given.pq.centroids.view(np.uint32), pqi.pq.centroids.view(np.uint32))
    # the codebook alone does not make the index trained
    half = faiss.IndexIVFPQ(faiss.IndexFlatL2(d), d, nlist, M, by_residual=False)
    half.pq.set_centroids(cb)
    assert not half.is_trained


def test_files_wrappers_and_raises(tmp_path):
    from image_search_engine_amd.utils import create_search_index

    d, M, nlist, n = 32, 16, 8, 1500
    rng = np.random.default_rng(92)
    xb, xq = clustered(rng, n, d, 20), clustered(rng, 15, d, 20)
    index = create_search_index(xb.copy(), "cell-probe-pq")
    assert isinstance(index, faiss.IndexIVFPQ) and (index.nprobe, index.nlist, index.ntotal, index.M) == (5, 8, n, 16)
    assert index.is_trained and index.quantizer.metric_type == L2 and index.quantizer.ntotal == 8 and not index.by_residual
    assign = index.quantizer.search(xb, 1)[1].reshape(-1)
    codes = index.sa_encode(xb)
    check_lists(index, assign, codes)
    D, I = index.search(xq, 10)
    # write_index -> read_index: the same lists and results
    path = tmp_path / "ivfpq.index"
    faiss.write_index(index, path)
    back = faiss.read_index(path)
    assert isinstance(back, faiss.IndexIVFPQ) and (back.nprobe, back.nlist, back.ntotal, back.M, back.d) == (5, 8, n, 16, d)
    check_lists(back, assign, codes)
    assert_knn_identical(*back.search(xq, 10), D, I, "read_index")
    parts = faiss.parse_ivfpq(path.read_bytes())
    residual = tmp_path / "residual.index"
    residual.write_bytes(faiss.serialize_ivfpq(*parts[:6], parts[8], parts[9], by_residual=True))
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.read_index(residual)
    renumbered = [(ids + 1, c) for ids, c in parts[9]]
    other = tmp_path / "renumbered.index"
    other.write_bytes(faiss.serialize_ivfpq(*parts[:6], parts[8], renumbered))
    with pytest.raises(RuntimeError, match="insertion numbers"):
        faiss.read_index(other)
    # IndexRefineFlat over it: with k_factor large enough, the exact result
    flat = faiss.IndexFlatL2(d)
    flat.add(xb)
    base = faiss.IndexIVFPQ(faiss.IndexFlatL2(d), d, nlist, M, by_residual=False)
    refine = faiss.IndexRefineFlat(base)
    refine.train(xb)
    refine.add(xb)
    base.nprobe = nlist
    refine.k_factor = 100
    assert_knn_identical(*refine.search(xq, 10), *flat.search(xq, 10), "IndexRefineFlat")
    rpath = tmp_path / "refine.index"
    faiss.write_index(refine, rpath)
    rback = faiss.read_index(rpath)
    assert isinstance(rback, faiss.IndexRefineFlat) and isinstance(rback.base_index, faiss.IndexIVFPQ) and rback.k_factor == 100
    assert rback.base_index.nprobe == nlist and rback.ntotal == n
    assert_knn_identical(*rback.search(xq, 10), *refine.search(xq, 10), "IxRF")
    # Faiss's OPQ,IVF,PQ chain
    opq = faiss.OPQMatrix(d, M)
    opq.niter, opq.niter_pq, opq.niter_pq_0 = 2, 2, 4
    sub = faiss.IndexIVFPQ(faiss.IndexFlatL2(d), d, nlist, M, by_residual=False)
    sub.pq.cp.niter = 4
    chain = faiss.IndexPreTransform(opq, sub)
    assert not chain.is_trained
    chain.train(xb)
    assert chain.is_trained and sub.is_trained
    chain.add(xb)
    sub.nprobe = 3
    Dc, Ic = chain.search(xq, 10)
    assert_knn_identical(Dc, Ic, *sub.search(chain.apply_chain(xq), 10), "IndexPreTransform")
    cpath = tmp_path / "chain.index"
    faiss.write_index(chain, cpath)
    cback = faiss.read_index(cpath)
    assert isinstance(cback, faiss.IndexPreTransform) and isinstance(cback.index, faiss.IndexIVFPQ) and cback.index.nprobe == 3
    assert_knn_identical(*cback.search(xq, 10), Dc, Ic, "IxPT")
    # what is not provided
    with pytest.raises(NotImplementedError, match="by_residual"):
        index.by_residual = True
    index.by_residual = False
    with pytest.raises((AssertionError, NotImplementedError, TypeError)):
        faiss.IndexIDMap(index)
    with pytest.raises(NotImplementedError):
        index.range_search(xq, 1.0)
    with pytest.raises(NotImplementedError):
        index.remove_ids(np.arange(3))
    with pytest.raises(NotImplementedError):
        index.search(xq, 3, params=faiss.SearchParameters())
    with pytest.raises(NotImplementedError, match="nbits"):
        faiss.IndexIVFPQ(faiss.IndexFlatL2(d), d, nlist, M, 4, by_residual=False)
    with pytest.raises(AssertionError):
        faiss.IndexIVFPQ(faiss.IndexFlatL2(d), d, nlist, 5, by_residual=False)  # 5 does not divide 32
    with pytest.raises(AssertionError):
        faiss.IndexIVFPQ(faiss.IndexFlatL2(d), 130, nlist, 65, by_residual=False)  # M above ISE_PQ_MAX_M
    with pytest.raises(AssertionError):
        faiss.IndexIVFPQ(faiss.IndexFlatL2(d + 1), d, nlist, M, by_residual=False)
    with pytest.raises(ValueError):  # a query-side poison gives padding, a row-side one refuses the add
        bad = xb[:4].copy()
        bad[2, 3] = np.nan
        index.add(bad)
    assert index.ntotal == n
    q = xq[:3].copy()
    q[1, 0] = np.inf
    D, I = index.search(q, 4)
    assert (I[1] == -1).all() and (D[1] == pad_value(L2)).all() and (I[[0, 2]] >= 0).all()
