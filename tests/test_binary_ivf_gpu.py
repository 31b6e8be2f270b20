"""GPU tests of IndexBinaryIVF (include/ise_knn.h, ise_binary_ivf_*; csrc/ise_binary_ivf.hpp).  Everything is integer,
so every comparison is exact: against the numpy reference over each query's probed lists (tests/binary_ivf_ref.py) and,
where every list is probed, against IndexBinaryFlat over the same rows.  Every counted search also asserts what it adds
to ``binary_ivf_stats``: one batch, groups x ceil(k / 32) passes, and the 64-row tiles of the lists that a query of the
group probes and no others."""
import numpy as np
import pytest

from image_search_engine_amd import _native as native
from image_search_engine_amd import faiss_compat as faiss
from tests import binary_ivf_ref as ref
from tests import binary_ref

pytestmark = pytest.mark.gpu

INT32_MAX = binary_ref.INT32_MAX


def new_index(C):
    """An IndexBinaryIVF over a quantiser that already holds the centroid codes ``C``."""
    C = np.ascontiguousarray(C, dtype=np.uint8)
    d = C.shape[1] * 8
    qz = faiss.IndexBinaryFlat(d)
    qz.add(C)
    index = faiss.IndexBinaryIVF(qz, d, len(C))
    assert index.is_trained and index.ntotal == 0 and index.nprobe == 1 and index.quantizer is qz
    assert (index.d, index.code_size, index.nlist, index.device) == (d, d // 8, len(C), qz.device)
    assert isinstance(index.cp, faiss.ClusteringParameters)
    return index


def flat_index(xb):
    flat = faiss.IndexBinaryFlat(xb.shape[1] * 8)
    if len(xb):
        flat.add(xb)
    return flat


def sizes_of(index):
    return [index.list_size(l) for l in range(index.nlist)]


def counted(index, table, k, call):
    """call() -> (D, I), with the statistics it adds asserted against the reference's count."""
    want = ref.stats_of(table, sizes_of(index), k) if index.ntotal else {"batches": 1, "passes": 0, "tiles_loaded": 0}
    before = index.binary_ivf_stats()
    out = call()
    after = index.binary_ivf_stats()
    got = {key: after[key] - before[key] for key in want}
    assert got == want, (got, want)
    return out


def search_pre(index, xq, k, table):
    table = np.asarray(table, dtype=np.int64)
    return counted(index, table, k, lambda: index.search_preassigned(xq, k, table))


def assert_same(got, want):
    (D, I), (Dw, Iw) = got, want
    assert D.dtype == np.int32 and I.dtype == np.int64 and D.shape == Dw.shape and I.shape == Iw.shape
    bad = np.flatnonzero((D != Dw).any(axis=1) | (I != Iw).any(axis=1))
    assert bad.size == 0, f"query {bad[0]}: D {D[bad[0]][:8]} I {I[bad[0]][:8]}, want D {Dw[bad[0]][:8]} I {Iw[bad[0]][:8]}"


def assert_ordered(D, I):
    """Ascending (distance, id), padding INT32_MAX / -1 behind the last result, no id twice."""
    for d_row, i_row in zip(D, I):
        m = int((i_row >= 0).sum())
        assert (i_row[m:] == -1).all() and (d_row[m:] == INT32_MAX).all() and (i_row[:m] >= 0).all()
        keys = d_row[:m].astype(np.int64) << 32 | i_row[:m]
        assert (np.diff(keys) > 0).all()


def check_lists(index, list_no, xb):
    total = 0
    for l in range(index.nlist):
        want = np.flatnonzero(list_no == l)
        ids, codes = index.get_list(l)
        assert ids.dtype == np.int64 and codes.dtype == np.uint8 and codes.shape == (len(want), index.code_size)
        assert np.array_equal(ids, want) and (np.diff(ids) > 0).all() and index.list_size(l) == len(want)
        assert np.array_equal(codes, xb[want])
        total += len(want)
    assert total == index.ntotal == len(xb)


def sweep(index, flat, C, xb, xq, ks, nprobes):
    """Case 1's comparison: the reference at every (k, nprobe), IndexBinaryFlat where every list is probed."""
    nlist = len(C)
    dist = binary_ref.distances(xb, xq)
    list_no = ref.assign(C, xb)
    check_lists(index, list_no, xb)
    for nprobe in nprobes:
        index.nprobe = nprobe
        table = ref.probes(C, xq, min(nprobe, nlist))
        for k in ks:
            want = ref.search_preassigned(xb, list_no, xq, k, table, nlist, dist)
            got = counted(index, table, k, lambda: index.search(xq, k))
            assert_same(got, want)
            assert_ordered(*got)
            if nprobe >= nlist:
                assert_same(got, flat.search(xq, k))


# ---------------------------------------------------------------- 1. row-length classes
@pytest.mark.parametrize("d", [8, 64, 72, 128, 136, 256, 1024])
def test_row_length_classes(d):
    """ws = 1 (8, 64), the padded ws = 2 (72), the exact ws = 2 (128), the odd word count rounded up (136: three words in
    four), ws = 4 (256) and the LDS query path at its longest here (1024); nq = 37 is two full groups and one of 5."""
    nlist, n, nq, cs = 7, 3000, 37, d // 8
    rng = np.random.default_rng(100 + d)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
    xq[:5] = xb[[0, 1, 63, 64, n - 1]]  # distance 0, also to id 0
    index = new_index(C)
    index.add(xb)
    assert index.ntotal == n
    sweep(index, flat_index(xb), C, xb, xq, (1, 32, 33, 70), (1, 3, nlist))


# ---------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("k", [5, 32, 40])
def test_ties_go_by_ascending_id(k):
    """Codes drawn from 20 values: equal distances span lists, tiles and the k-cut."""
    d, nlist, n, nq = 64, 5, 2000, 20
    rng = np.random.default_rng(7)
    values = rng.integers(0, 256, (20, d // 8), dtype=np.uint8)
    C = rng.integers(0, 256, (nlist, d // 8), dtype=np.uint8)
    xb = values[rng.integers(0, 20, n)]
    xq = np.concatenate([values[:10], rng.integers(0, 256, (nq - 10, d // 8), dtype=np.uint8)])
    index = new_index(C)
    index.add(xb)
    list_no = ref.assign(C, xb)
    assert len(set(list_no.tolist())) >= 3  # the values are spread over several lists
    for nprobe in (2, nlist):
        index.nprobe = nprobe
        got = index.search(xq, k)
        assert_same(got, ref.search(C, xb, xq, k, nprobe))
        assert_ordered(*got)
        assert (np.diff(got[0], axis=1) == 0).sum() > nq  # ties inside the results
    assert_same(got, flat_index(xb).search(xq, k))


# ---------------------------------------------------------------- 3. / 4. list sizes and probe tables
SIZES = (0, 1, 63, 64, 65, 128, 129)


@pytest.fixture(scope="module")
def sized():
    """Lists of SIZES rows, steered through the public interface: every row is its list's centroid with at most two
    bits flipped, added in shuffled order so that the ids of a list are spread over the whole range."""
    d, nlist = 64, len(SIZES)
    rng = np.random.default_rng(11)
    C = rng.integers(0, 256, (nlist, d // 8), dtype=np.uint8)
    want = rng.permutation(np.repeat(np.arange(nlist), SIZES))
    xb = ref.near_centroids(rng, C, want)
    assert np.array_equal(ref.assign(C, xb), want)  # the assignment came out as intended
    index = new_index(C)
    index.add(xb)
    assert sizes_of(index) == list(SIZES)
    xq = rng.integers(0, 256, (19, d // 8), dtype=np.uint8)
    xq[:7] = C
    return index, C, xb, want, xq, binary_ref.distances(xb, xq)


def test_list_sizes(sized):
    index, C, xb, list_no, xq, dist = sized
    nlist, nq = len(C), len(xq)
    check_lists(index, list_no, xb)
    for k in (1, 70, 200):  # 200: more than any list holds, a padded tail
        for l in range(nlist):  # each list alone
            table = np.full((nq, 1), l, dtype=np.int64)
            got = search_pre(index, xq, k, table)
            assert_same(got, ref.search_preassigned(xb, list_no, xq, k, table, nlist, dist))
            assert (got[1][:, :min(k, SIZES[l])] >= 0).all() and (got[1][:, SIZES[l]:] == -1).all()
        table = np.tile(np.arange(nlist, dtype=np.int64), (nq, 1))  # all of them
        got = search_pre(index, xq, k, table)
        assert_same(got, ref.search_preassigned(xb, list_no, xq, k, table, nlist, dist))
        assert_same(got, binary_ref.search(xb, xq, k, dist))
    # a query probing only the empty list is all padding, beside queries that find rows
    table = np.zeros((nq, 2), dtype=np.int64)
    table[1::2] = (3, 5)
    D, I = search_pre(index, xq, 33, table)
    assert (I[0::2] == -1).all() and (D[0::2] == INT32_MAX).all() and (I[1::2] >= 0).all()
    assert_same((D, I), ref.search_preassigned(xb, list_no, xq, 33, table, nlist, dist))


def test_probe_tables(sized):
    index, C, xb, list_no, xq, dist = sized
    nlist, nq = len(C), len(xq)
    rng = np.random.default_rng(12)
    table = rng.integers(0, nlist, (nq, 6)).astype(np.int64)
    table[0] = -1                                   # all -1
    table[1] = (2, -1, 2, -1, 2, -1)                # the same list three times, between -1
    table[2] = (nlist, nlist + 1, 2 ** 40, -7, 4, 4)  # nlist and beyond, a negative, a list twice
    table[3] = (6, 6, 6, 6, 6, 6)
    table[4] = (nlist, -1, nlist, -1, 1 << 62, -(1 << 62))  # nothing in range
    table[16] = (0, 0, -1, nlist, 0, 0)             # the last group's first query: the empty list only
    for k in (1, 40, 200):
        got = search_pre(index, xq, k, table)
        cleaned = [row + [-1] * (6 - len(row)) for row in ref.clean_probes(table, nlist)]
        assert_same(got, ref.search_preassigned(xb, list_no, xq, k, np.array(cleaned), nlist, dist))
        assert_ordered(*got)  # no id twice in a row of I
        for i in (0, 4, 16):
            assert (got[1][i] == -1).all()


# ---------------------------------------------------------------- 5. cuts
@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_cuts(order):
    """One list of 4096 rows at d = 256, stored by distance to the first query: descending, every tile brings 64 keys
    below everything held (each tile appends, the waves cut); ascending, the first tiles fill the buffers for good."""
    d, n, cs = 256, 4096, 32
    rng = np.random.default_rng(13)
    q = rng.integers(0, 256, (1, cs), dtype=np.uint8)
    want_dist = 256 - (np.arange(n) * 256) // n  # 16 rows at every distance 256 .. 1
    flips = np.zeros((n, d), dtype=np.uint8)
    for i in range(n):
        flips[i, rng.choice(d, int(want_dist[i]), replace=False)] = 1
    xb = np.packbits(flips, axis=1, bitorder="little") ^ q
    if order == "ascending":
        xb, want_dist = xb[::-1].copy(), want_dist[::-1]
    xq = np.concatenate([q, rng.integers(0, 256, (2, cs), dtype=np.uint8)])
    dist = binary_ref.distances(xb, xq)
    assert np.array_equal(dist[0], want_dist)
    index = new_index(rng.integers(0, 256, (1, cs), dtype=np.uint8))
    index.add(xb)
    assert sizes_of(index) == [n]
    for k in (1, 32, 100):
        got = counted(index, np.zeros((3, 1), np.int64), k, lambda: index.search(xq, k))
        assert_same(got, binary_ref.search(xb, xq, k, dist))


def test_cuts_repeat_in_a_wave():
    """The same at the size at which a wave cuts more than once: a pass's grid gives a wave two entries until the lists
    hold more than 4096 tiles (two blocks per CU), and a wave's first cut comes with its second tile.  2^19 rows of 64 bits
    are 8192 tiles, four or more per wave, every one of them below everything the wave holds: the buffer of the first
    query fills and is cut again with every tile after the first.  Rows are the query with ``dist`` adjacent bits flipped
    (rotated at random), 8192 rows at every distance 64 .. 1; equal distances go by id."""
    n = 1 << 19
    rng = np.random.default_rng(22)
    q = rng.integers(0, 1 << 63, 1, dtype=np.uint64)
    want_dist = (64 - (np.arange(n, dtype=np.uint64) * np.uint64(64)) // np.uint64(n)).astype(np.uint64)
    mask = np.where(want_dist == 64, ~np.uint64(0), (np.uint64(1) << (want_dist % np.uint64(64))) - np.uint64(1))
    rot = rng.integers(0, 64, n).astype(np.uint64)
    mask = (mask << rot) | (mask >> ((np.uint64(64) - rot) % np.uint64(64)))
    xb = (q ^ mask).astype("<u8").view(np.uint8).reshape(n, 8)
    xq = np.concatenate([q.astype("<u8").view(np.uint8).reshape(1, 8), rng.integers(0, 256, (2, 8), dtype=np.uint8)])
    dist = binary_ref.distances(xb, xq)
    assert np.array_equal(dist[0], want_dist.astype(np.int32))
    index = new_index(rng.integers(0, 256, (1, 8), dtype=np.uint8))
    index.add(xb)
    for k in (32, 100):
        got = counted(index, np.zeros((3, 1), np.int64), k, lambda: index.search(xq, k))
        assert_same(got, binary_ref.search(xb, xq, k, dist))


# ---------------------------------------------------------------- 6. many lists
@pytest.mark.parametrize("nlist", [257, 1000])
def test_many_lists(nlist):
    """More lists than the offsets kernel has threads (its threads own 2 and 4 lists), three groups of queries."""
    d, nq, cs = 64, 40, 8
    n = 3 * nlist
    rng = np.random.default_rng(14 + nlist)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
    index = new_index(C)
    index.add(xb)
    sweep(index, flat_index(xb), C, xb, xq, (10, 40), (1, 5, nlist))


# ---------------------------------------------------------------- 7. large k
def test_largest_k():
    """k = ISE_MAX_K: 64 passes per group, the floor carried from each to the next."""
    d, nlist, n, cs, k = 64, 7, 5000, 8, native.MAX_K
    rng = np.random.default_rng(15)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (2, cs), dtype=np.uint8)
    index = new_index(C)
    index.add(xb)
    index.nprobe = nlist
    table = ref.probes(C, xq, nlist)
    got = counted(index, table, k, lambda: index.search(xq, k))
    assert_same(got, binary_ref.search(xb, xq, k))
    assert_same(got, ref.search(C, xb, xq, k, nlist))
    assert_same(got, flat_index(xb).search(xq, k))
    with pytest.raises(RuntimeError, match="ISE_MAX_K"):
        index.search(xq, k + 1)


# ---------------------------------------------------------------- 8. growth
@pytest.mark.parametrize("d", [64, 72, 1024])
def test_growth_and_reset(d):
    """Three adds with a search after each: old tiles move (8-byte rows at d = 64), pending rows land behind them."""
    nlist, cs = 5, d // 8
    rng = np.random.default_rng(16 + d)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (600, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (17, cs), dtype=np.uint8)
    index = new_index(C)
    D, I = counted(index, ref.probes(C, xq, 1), 5, lambda: index.search(xq, 5))  # an empty index: all padding, no pass
    assert (I == -1).all() and (D == INT32_MAX).all()
    at = 0
    for m in (250, 1, 349):
        index.add(xb[at:at + m])
        at += m
        assert index.ntotal == at and sum(sizes_of(index)) == at  # (the pending rows are counted)
        for nprobe, k in ((2, 40), (nlist, 3)):
            index.nprobe = nprobe
            got = counted(index, ref.probes(C, xq, nprobe), k, lambda: index.search(xq, k))
            assert_same(got, ref.search(C, xb[:at], xq, k, nprobe))
        check_lists(index, ref.assign(C, xb[:at]), xb[:at])
    index.add(xb[:0])
    assert index.ntotal == 600
    index.reset()
    assert index.ntotal == 0 and sizes_of(index) == [0] * nlist and index.is_trained and index.quantizer.ntotal == nlist
    D, I = index.search(xq, 4)
    assert (I == -1).all() and (D == INT32_MAX).all()
    ids, codes = index.get_list(2)
    assert ids.shape == (0,) and codes.shape == (0, cs)
    index.add(xb[100:300])  # ids start again at 0
    index.nprobe = nlist
    assert_same(index.search(xq, 7), binary_ref.search(xb[100:300], xq, 7))


# ---------------------------------------------------------------- 9. the device path
def test_device_path_and_streams():
    import torch

    d, nlist, n, cs = 136, 6, 1500, 17
    rng = np.random.default_rng(17)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (50, cs), dtype=np.uint8)
    host, dev = new_index(C), new_index(C)
    host.add(xb)
    dev.add_torch(torch.from_numpy(xb[:700]).cuda())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev.add_torch(torch.from_numpy(xb[700:]).cuda())
    assert dev.ntotal == n
    check_lists(dev, ref.assign(C, xb), xb)
    xq_dev = torch.from_numpy(xq).cuda()
    for nprobe, k in ((1, 1), (3, 40), (nlist, 70)):
        host.nprobe = dev.nprobe = nprobe
        want = host.search(xq, k)
        assert_same(want, ref.search(C, xb, xq, k, nprobe))
        D, I = dev.search_torch(xq_dev, k)
        assert D.dtype == torch.int32 and I.dtype == torch.int64 and D.is_cuda
        assert_same((D.cpu().numpy(), I.cpu().numpy()), want)
        with torch.cuda.stream(side):
            D, I = dev.search_torch(xq_dev, k)
        side.synchronize()
        assert_same((D.cpu().numpy(), I.cpu().numpy()), want)
    # two searches on one handle from two streams: the second waits for the first, both answer as one does
    other = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a = dev.search_torch(xq_dev, 70)
    with torch.cuda.stream(other):
        b = dev.search_torch(xq_dev[:33], 5)
    torch.cuda.synchronize()
    assert_same((a[0].cpu().numpy(), a[1].cpu().numpy()), want)
    assert_same((b[0].cpu().numpy(), b[1].cpu().numpy()), ref.search(C, xb, xq[:33], 5, nlist))
    D, I = dev.search_torch(xq_dev[:0], 3)
    assert D.shape == (0, 3) and I.shape == (0, 3)


# ---------------------------------------------------------------- 10. statistics
def test_stats_count_the_probed_tiles(sized):
    index, C, xb, list_no, xq, dist = sized
    nq = len(xq)  # 19: a group of 16 and one of 3
    before = index.binary_ivf_stats()
    assert set(before) == {"batches", "passes", "tiles_loaded"}
    table = np.full((nq, 2), -1, dtype=np.int64)
    table[:16, 0] = 6   # the first group: list 6 (129 rows, 3 tiles)
    table[3, 1] = 4     # ... and list 4 (65 rows, 2 tiles) through one query
    table[16:, 0] = 1   # the second group: list 1 (1 row, 1 tile)
    index.search_preassigned(xq, 70, table)  # three passes per group
    after = index.binary_ivf_stats()
    assert {key: after[key] - before[key] for key in after} == {"batches": 1, "passes": 6, "tiles_loaded": 3 * (3 + 2) + 3 * 1}
    assert ref.stats_of(table, SIZES, 70) == {"batches": 1, "passes": 6, "tiles_loaded": 18}


# ---------------------------------------------------------------- 11. training
def test_training():
    d, nlist, n, cs = 64, 7, 3000, 8
    rng = np.random.default_rng(18)
    # clustered codes: a few bits flipped around hidden centres, so that k-means has something to find
    centres = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = ref.near_centroids(rng, centres, rng.integers(0, nlist, n), flips=6)
    xq = rng.integers(0, 256, (37, cs), dtype=np.uint8)
    xq[:20] = ref.near_centroids(rng, centres, rng.integers(0, nlist, 20), flips=10)
    trained = []
    for _ in range(2):
        qz = faiss.IndexBinaryFlat(d)
        index = faiss.IndexBinaryIVF(qz, d, nlist)
        assert not index.is_trained
        with pytest.raises(RuntimeError, match="before train"):
            index.add(xb)
        with pytest.raises(RuntimeError, match="before train"):
            index.search(xq, 1)
        with pytest.raises(RuntimeError, match="training rows"):
            index.train(xb[:nlist - 1])
        assert qz.ntotal == 0 and not index.is_trained
        index.train(xb)
        assert index.is_trained and qz.ntotal == nlist
        trained.append(qz.reconstruct_n(0, nlist))
    assert np.array_equal(trained[0], trained[1])  # the same seed, the same codes
    C = trained[1]
    index.train(xb[:3])  # the quantiser holds nlist codes: a no-op
    assert np.array_equal(qz.reconstruct_n(0, nlist), C)
    index.add(xb)
    sweep(index, flat_index(xb), C, xb, xq, (1, 32, 33, 70), (1, 3, nlist))
    # a quantiser that holds neither 0 nor nlist codes
    qz = faiss.IndexBinaryFlat(d)
    qz.add(C[:3])
    index = faiss.IndexBinaryIVF(qz, d, nlist)
    assert not index.is_trained
    with pytest.raises(RuntimeError, match="neither 0 nor nlist"):
        index.train(xb)
    # a wider cp: the parameters reach Kmeans (another seed, other codes or not, but a trained index either way)
    qz = faiss.IndexBinaryFlat(d)
    index = faiss.IndexBinaryIVF(qz, d, nlist)
    index.cp.niter, index.cp.seed = 2, 99
    index.train(xb)
    assert qz.ntotal == nlist


def test_two_lists_with_one_centroid_code():
    """Two centroids that binarise to the same code: the quantiser names the earlier one, the later list stays empty."""
    d, cs = 64, 8
    rng = np.random.default_rng(19)
    C = rng.integers(0, 256, (4, cs), dtype=np.uint8)
    C[3] = C[1]
    xb = ref.near_centroids(rng, C, rng.integers(0, 4, 500))
    xq = rng.integers(0, 256, (18, cs), dtype=np.uint8)
    index = new_index(C)
    index.add(xb)
    assert index.list_size(3) == 0 and index.list_size(1) > 0
    sweep(index, flat_index(xb), C, xb, xq, (1, 40), (1, 2, 4))


# ---------------------------------------------------------------- 12. files
def test_files(tmp_path):
    d, nlist, n, cs = 72, 6, 700, 9
    rng = np.random.default_rng(20)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    C[5] = C[0]  # an empty list in the file
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (21, cs), dtype=np.uint8)
    index = new_index(C)
    index.add(xb[:400])
    index.add(xb[400:])
    index.nprobe = 3
    path = tmp_path / "binary_ivf.index"
    faiss.write_index_binary(index, path)
    buf = path.read_bytes()
    assert buf[:4] == b"IBwF"
    parts = faiss.parse_binary_ivf(buf)
    assert parts[:3] == (d, nlist, 3) and np.array_equal(parts[3], C)
    back = faiss.read_index_binary(path)
    assert isinstance(back, faiss.IndexBinaryIVF) and isinstance(back.quantizer, faiss.IndexBinaryFlat)
    assert (back.d, back.nlist, back.nprobe, back.ntotal, back.is_trained) == (d, nlist, 3, n, True)
    assert np.array_equal(back.quantizer.reconstruct_n(0, nlist), C)
    for l in range(nlist):
        (ids, codes), (wids, wcodes) = back.get_list(l), index.get_list(l)
        assert np.array_equal(ids, wids) and np.array_equal(codes, wcodes)
    assert back.list_size(5) == 0
    for k in (1, 40):
        assert_same(back.search(xq, k), index.search(xq, k))
    assert_same(back.search(xq, 40), ref.search(C, xb, xq, 40, 3))
    with pytest.raises(RuntimeError, match="truncated IndexBinaryIVF"):
        path.write_bytes(buf[:-3])
        faiss.read_index_binary(path)
    with pytest.raises(NotImplementedError):
        faiss.write_index(index, tmp_path / "float.index")
    # an untrained index goes through a file too
    empty = faiss.IndexBinaryIVF(faiss.IndexBinaryFlat(d), d, nlist)
    faiss.write_index_binary(empty, path)
    back = faiss.read_index_binary(path)
    assert isinstance(back, faiss.IndexBinaryIVF) and not back.is_trained and back.ntotal == 0 and back.quantizer.ntotal == 0
    # a flat binary file still reads as before
    flat = flat_index(xb)
    faiss.write_index_binary(flat, path)
    back = faiss.read_index_binary(path)
    assert type(back) is faiss.IndexBinaryFlat and back.ntotal == n
    assert_same(back.search(xq, 5), flat.search(xq, 5))


# ---------------------------------------------------------------- 13. what raises
def test_what_raises():
    import torch

    d, cs = 64, 8
    rng = np.random.default_rng(21)
    C = rng.integers(0, 256, (3, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (40, cs), dtype=np.uint8)
    untrained = faiss.IndexBinaryIVF(faiss.IndexBinaryFlat(d), d, 3)
    for call in (lambda: untrained.add(xb), lambda: untrained.search(xb, 1),
                 lambda: untrained.add_torch(torch.from_numpy(xb).cuda()),
                 lambda: untrained.search_torch(torch.from_numpy(xb).cuda(), 1)):
        with pytest.raises(RuntimeError, match="before train"):
            call()
    index = new_index(C)
    index.add(xb)
    with pytest.raises(AssertionError):
        index.add(xb.astype(np.float32))
    with pytest.raises(AssertionError):
        index.add(xb[:, :7])
    with pytest.raises(AssertionError):
        index.search(xb[:, :7], 1)
    with pytest.raises(AssertionError):
        index.search(xb.astype(np.int8), 1)
    with pytest.raises(AssertionError):
        index.search_torch(torch.from_numpy(xb).cuda().float(), 1)
    with pytest.raises(AssertionError):
        index.search_preassigned(xb, 1, np.zeros((3, 1), np.int64))  # one probe row per query
    with pytest.raises(AssertionError):
        faiss.IndexBinaryIVF(faiss.IndexFlatL2(d), d, 3)  # the quantiser is a binary index
    with pytest.raises(AssertionError):
        faiss.IndexBinaryIVF(faiss.IndexBinaryFlat(128), d, 3)
    with pytest.raises(RuntimeError):
        faiss.IndexBinaryIVF(faiss.IndexBinaryFlat(d), d, 0)
    with pytest.raises(NotImplementedError):
        index.range_search(xb, 3)
    with pytest.raises(NotImplementedError):
        index.remove_ids(np.arange(3))
    with pytest.raises(NotImplementedError):
        index.search(xb, 1, params=faiss.SearchParameters())
    with pytest.raises(NotImplementedError):
        index.search_torch(torch.from_numpy(xb).cuda(), 1, params=faiss.SearchParameters())
    with pytest.raises(NotImplementedError):
        faiss.IndexBinaryIDMap(faiss.IndexBinaryIVF(faiss.IndexBinaryFlat(d), d, 3))
    # list numbers outside [0, nlist) through the ABI: nothing is added
    lists = np.array([0, 3], dtype=np.int64)
    assert native.lib.ise_binary_ivf_add_host(index._h, xb.ctypes.data, lists.ctypes.data, 2) == native.E_INVALID
    assert index.ntotal == 40
    assert index.search(xb[:0], 3)[0].shape == (0, 3)
