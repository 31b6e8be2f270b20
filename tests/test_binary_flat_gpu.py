"""GPU tests of IndexBinaryFlat (include/ise_knn.h, ise_binary_index_*; csrc/ise_binary_scan.hpp) against the numpy
reference tests/binary_ref.py.  Every score is an integer, so every comparison is exact: np.array_equal on D and on I,
dtypes asserted, no tolerance anywhere.  With 600 random rows almost every query has ties at the k-th place (all of
them at code_size 1), so the tie rule -- ascending id -- is what these tests mostly check."""
import functools

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import binary_ref as ref

pytestmark = pytest.mark.gpu

# W = 1 with pad, 1, 2 with pad, 3 and 5 (odd: stored as 4 and 6 words), 8, 32, 128 (the chunked loop)
CODE_SIZES = (1, 8, 12, 24, 40, 64, 256, 1024)
N_SWEEP = 600                           # a partial last tile of 64 rows
NQ_MAX = 40
KPASS = 32                              # results per query and pass (include/ise_knn.h)


@functools.lru_cache(maxsize=None)
def sweep_data(code_size):
    """(xb, xq, dist) of the sweep, computed once and shared; never modified."""
    rng = np.random.default_rng(1000 + code_size)
    xb = rng.integers(0, 256, (N_SWEEP, code_size), dtype=np.uint8)
    xq = rng.integers(0, 256, (NQ_MAX, code_size), dtype=np.uint8)
    xq[3] = xb[17]  # a query that is a row
    dist = ref.distances(xb, xq)
    for a in (xb, xq, dist):
        a.setflags(write=False)
    return xb, xq, dist


@functools.lru_cache(maxsize=None)
def big_data():
    """70 001 codes of 8 bytes and 17 queries; rows {0, 1, 63, 64, 4095, 4096, 70 000} equal query 0: seven equal keys
    in different lanes, waves and blocks."""
    rng = np.random.default_rng(7)
    xb = rng.integers(0, 256, (70_001, 8), dtype=np.uint8)
    xq = rng.integers(0, 256, (17, 8), dtype=np.uint8)
    xb[[0, 1, 63, 64, 4095, 4096, 70_000]] = xq[0]
    dist = ref.distances(xb, xq)
    for a in (xb, xq, dist):
        a.setflags(write=False)
    return xb, xq, dist


def make_index(xb):
    index = faiss.IndexBinaryFlat(8 * xb.shape[1])
    index.add(xb)
    return index


def assert_same(got, want):
    D, I = got
    Dw, Iw = want
    assert D.dtype == np.int32 and I.dtype == np.int64
    assert D.shape == Dw.shape and I.shape == Iw.shape
    assert np.array_equal(I, Iw), f"ids differ at {np.argwhere(I != Iw)[:5].tolist()}"
    assert np.array_equal(D, Dw)


@pytest.mark.parametrize("code_size", CODE_SIZES)
def test_parity_sweep(code_size):
    xb, xq, dist = sweep_data(code_size)
    index = make_index(xb)
    assert index.ntotal == N_SWEEP and index.d == 8 * code_size and index.code_size == code_size
    for k in (1, 10, 33, 70, 605):
        want = ref.search(xb, xq, k, dist)
        for nq in (1, 16, 17, 40):
            got = index.search(xq[:nq], k)
            assert_same(got, (want[0][:nq], want[1][:nq]))
        if k == 605:
            assert (got[0][:, 600:] == ref.INT32_MAX).all() and (got[1][:, 600:] == -1).all()
            assert (got[1][:, :600] >= 0).all()


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_parity_tiny_indexes(n):
    xb, xq, _ = sweep_data(8)
    index = make_index(xb[:n])
    assert_same(index.search(xq[:17], 10), ref.search(xb[:n], xq[:17], 10))


def test_ties_across_waves_and_blocks():
    xb, xq, dist = big_data()
    index = make_index(xb)
    D, I = index.search(xq, 5)
    assert I[0].tolist() == [0, 1, 63, 64, 4095] and (D[0] == 0).all()
    assert_same((D, I), ref.search(xb, xq, 5, dist))
    assert_same(index.search(xq, 10), ref.search(xb, xq, 10, dist))
    assert index.search(xq[:1], 7)[1][0].tolist() == [0, 1, 63, 64, 4095, 4096, 70_000]


def test_query_equal_to_row_zero_survives_a_cut():
    """(distance 0, row 0) is the smallest key there is; the selection primitives need it above 0.  320 rows are five
    tiles in one block, wave 0 holds tiles 0 and 4 and cuts after the second: row 0 equals the query, row 319 -- the
    last key of that buffer -- differs in one bit, every other row in at least two."""
    rng = np.random.default_rng(21)
    q = rng.integers(0, 256, (1, 8), dtype=np.uint8)
    xb = rng.integers(0, 256, (320, 8), dtype=np.uint8)
    xb[0] = q[0]
    xb[319] = q[0]
    xb[319, 3] ^= 0x10
    near = np.flatnonzero(ref.distances(xb, q)[0] < 2)
    assert near.tolist() == [0, 319]
    index = make_index(xb)
    for k in (1, 2, 10, 33):
        assert_same(index.search(q, k), ref.search(xb, q, k))
    D, I = index.search(q, 2)
    assert I[0].tolist() == [0, 319] and D[0].tolist() == [0, 1]
    # 16 queries that all equal row 0: every lane-owned state of the wave goes through the same cut
    assert_same(index.search(np.repeat(q, 16, axis=0), 2), ref.search(xb, np.repeat(q, 16, axis=0), 2))
    assert_range_same(index.range_search(q, 2), ref.range_search(xb, q, 2))


def one_block_data(code_size):
    """(xb, xq, dist): 512 rows -- eight tiles in one block, wave 0 streams tiles 0 and 4 and cuts after the second --
    in DESCENDING distance to query 0, so that every key of its second tile passes; 16 queries."""
    rng = np.random.default_rng(3000 + code_size)
    xb = rng.integers(0, 256, (512, code_size), dtype=np.uint8)
    xq = rng.integers(0, 256, (16, code_size), dtype=np.uint8)
    xb = xb[np.argsort(-ref.distances(xb, xq[:1])[0], kind="stable")]
    dist = ref.distances(xb, xq)
    assert (np.diff(dist[0]) <= 0).all()
    return xb, xq, dist


@pytest.mark.parametrize("code_size", (8, 16, 24))  # one word, two words, the queries in LDS
def test_one_block_cut_then_short_lists(code_size):
    """k = 33: the floor-keyed second pass and the merge's floor write behind a pass that cut.  k = 513: sixteen full
    passes, then one that finds no row above its floor -- every list of the block ends short."""
    xb, xq, dist = one_block_data(code_size)
    index = make_index(xb)
    for k in (KPASS + 1, 513):
        got = index.search(xq, k)
        assert_same(got, ref.search(xb, xq, k, dist))
    assert (got[1][:, 512] == -1).all() and (got[0][:, 512] == ref.INT32_MAX).all() and (got[1][:, :512] >= 0).all()


def test_long_index_thresholds_and_worst_case_order():
    """One million rows: the grid is at its cap, so every wave streams several 64-row tiles and most keys are turned
    away by the wave's threshold (at 70 001 rows a wave sees two tiles and cuts once).  The rows are sorted by
    DESCENDING distance to query 0 -- for that query every tile beats everything before it, the worst case for the
    threshold: the buffer is cut on every second tile; the other queries see the rows in random order."""
    rng = np.random.default_rng(5)
    n = 1_000_003
    xb = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    xq = rng.integers(0, 256, (17, 8), dtype=np.uint8)
    xb = xb[np.argsort(-ref.distances(xb, xq[:1])[0], kind="stable")]
    xb[[5, 999_999, 1_000_002]] = xq[16]  # ties for the second query tile, first and last blocks
    # query 1 is row 0 itself; its runner-up (one bit off) is the last row of the second tile that wave 0 of block 0
    # streams (tile 2048 with the grid at its cap of 512 blocks), so it sits last in that wave's buffer at its first cut
    xq[1] = xb[0]
    xb[2048 * 64 + 63] = xb[0]
    xb[2048 * 64 + 63, 0] ^= 0x01
    dist = ref.distances(xb, xq)
    index = make_index(xb)
    for k in (10, 40):
        assert_same(index.search(xq, k), ref.search(xb, xq, k, dist))
    assert index.search(xq[16:], 3)[1][0].tolist() == [5, 999_999, 1_000_002]
    D, I = index.search(xq[1:2], 2)
    assert I[0].tolist() == [0, 2048 * 64 + 63] and D[0].tolist() == [0, 1]
    assert_range_same(index.range_search(xq, 17), ref.range_search(xb, xq, 17, dist))


def test_all_equal_index():
    row = np.arange(12, dtype=np.uint8)[None, :] * 19 + 5
    xb = np.repeat(row, 5000, axis=0)
    index = make_index(xb)
    xq = np.concatenate([row, row ^ np.uint8(1)])  # distance 0 and distance 12 to every row
    for k in (1, 10, 33, 100):
        D, I = index.search(xq, k)
        assert D.dtype == np.int32 and I.dtype == np.int64
        assert np.array_equal(I, np.tile(np.arange(k, dtype=np.int64), (2, 1)))
        assert (D[0] == 0).all() and (D[1] == 12).all()
    lims, D, I = index.range_search(row, 1)
    assert lims.dtype == np.uint64 and lims.tolist() == [0, 5000]
    assert D.dtype == np.int32 and I.dtype == np.int64
    assert np.array_equal(I, np.arange(5000, dtype=np.int64)) and (D == 0).all()
    lims, D, I = index.range_search(row, 0)
    assert lims.tolist() == [0, 0] and D.size == 0 and I.size == 0


def assert_range_same(got, want):
    lims, D, I = got
    lw, Dw, Iw = want
    assert lims.dtype == np.uint64 and D.dtype == np.int32 and I.dtype == np.int64
    assert np.array_equal(lims, lw)
    assert np.array_equal(I, Iw)
    assert np.array_equal(D, Dw)


@pytest.mark.parametrize("code_size", (1, 8, 256))
def test_range_search(code_size):
    xb, xq, dist = sweep_data(code_size)
    index = make_index(xb)
    for radius in (0, 1, int(np.median(dist)), 8 * code_size + 1):
        for nq in (1, 17):
            got = index.range_search(xq[:nq], radius)
            assert_range_same(got, ref.range_search(xb, xq[:nq], radius, dist[:nq]))
            if radius == 8 * code_size + 1:  # every row, for every query
                assert got[0].tolist() == [N_SWEEP * i for i in range(nq + 1)]
                assert np.array_equal(got[2], np.tile(np.arange(N_SWEEP, dtype=np.int64), nq))


def test_range_search_many_blocks():
    xb, xq, dist = big_data()
    index = make_index(xb)
    got = index.range_search(xq, 20)
    want = ref.range_search(xb, xq, 20, dist)
    counts = np.diff(want[0].astype(np.int64))
    assert counts.min() > 0 and counts[0] >= 7  # not vacuous: every query matches rows, query 0 its seven copies too
    assert np.array_equal(np.diff(got[0].astype(np.int64)), counts)
    assert_range_same(got, want)


def test_lifecycle():
    rng = np.random.default_rng(11)
    xb = rng.integers(0, 256, (7600, 12), dtype=np.uint8)
    xq = rng.integers(0, 256, (5, 12), dtype=np.uint8)
    whole = make_index(xb)
    pieces = faiss.IndexBinaryFlat(96)
    for a, b in ((0, 1), (1, 600), (600, 7600)):  # the last piece forces a regrow
        pieces.add(xb[a:b])
    assert pieces.ntotal == whole.ntotal == 7600
    want = ref.search(xb, xq, 40)
    assert_same(whole.search(xq, 40), want)
    assert_same(pieces.search(xq, 40), want)
    back = pieces.reconstruct_n(0, 7600)
    assert back.dtype == np.uint8 and np.array_equal(back, xb)
    assert np.array_equal(pieces.reconstruct_n(599, 3), xb[599:602])
    assert np.array_equal(pieces.reconstruct(7599), xb[7599])
    assert_range_same(pieces.range_search(xq, 36), ref.range_search(xb, xq, 36))

    pieces.reset()
    assert pieces.ntotal == 0
    D, I = pieces.search(xq, 3)
    assert D.dtype == np.int32 and (D == ref.INT32_MAX).all() and (I == -1).all()
    lims, Dr, Ir = pieces.range_search(xq, 97)
    assert lims.tolist() == [0] * 6 and Dr.size == 0 and Ir.size == 0
    # rows left behind by the reset are masked by row number: a short re-add sees only its own rows
    pieces.add(xb[100:170])
    assert pieces.ntotal == 70
    assert_same(pieces.search(xq, 80), ref.search(xb[100:170], xq, 80))
    assert_range_same(pieces.range_search(xq, 97), ref.range_search(xb[100:170], xq, 97))


def test_write_read_index_binary(tmp_path):
    xb, xq, dist = sweep_data(12)
    index = make_index(xb)
    path = tmp_path / "codes.index"
    faiss.write_index_binary(index, path)
    again = faiss.read_index_binary(path)
    assert isinstance(again, faiss.IndexBinaryFlat) and again.d == 96 and again.ntotal == N_SWEEP
    assert np.array_equal(again.reconstruct_n(0, N_SWEEP), xb)
    assert_same(again.search(xq, 10), index.search(xq, 10))
    assert_same(again.search(xq, 10), ref.search(xb, xq, 10, dist))


def test_device_forms():
    import torch

    xb, xq, dist = sweep_data(64)
    dev = torch.device("cuda", torch.cuda.current_device())
    index = faiss.IndexBinaryFlat(512)
    index.add_torch(torch.from_numpy(xb.copy()).to(dev))
    assert index.ntotal == N_SWEEP
    assert np.array_equal(index.reconstruct_n(0, N_SWEEP), xb)
    host = index.search(xq[:17], 33)
    assert_same(host, (ref.search(xb, xq, 33, dist)[0][:17], ref.search(xb, xq, 33, dist)[1][:17]))
    side = torch.cuda.Stream(device=dev)
    xq_dev = torch.from_numpy(xq[:17].copy()).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        D, I = index.search_torch(xq_dev, 33)
    side.synchronize()
    assert D.is_cuda and I.is_cuda and D.dtype == torch.int32 and I.dtype == torch.int64
    assert_same((D.cpu().numpy(), I.cpu().numpy()), host)


def test_counters():
    xb, xq, _ = sweep_data(8)
    index = faiss.IndexBinaryFlat(64)
    zero = {"search_batches": 0, "scan_passes": 0, "range_batches": 0}
    assert index.binary_stats() == zero
    index.search(xq[:3], 5)           # an empty index: a batch, no pass
    index.range_search(xq[:3], 10)    # ... and no range batch either
    assert index.binary_stats() == {"search_batches": 1, "scan_passes": 0, "range_batches": 0}
    index.add(xb)
    base = index.binary_stats()
    passes = lambda nq, k: -(-nq // 16) * -(-k // KPASS)
    total = 0
    for i, (nq, k) in enumerate(((1, 1), (16, 32), (17, 33), (40, 70), (5, 605))):
        index.search(xq[:nq], k)
        total += passes(nq, k)
        s = index.binary_stats()
        assert s["search_batches"] == base["search_batches"] + i + 1
        assert s["scan_passes"] == base["scan_passes"] + total
        assert s["range_batches"] == 0
    before = index.binary_stats()
    index.range_search(xq[:17], 0)
    index.range_search(xq[:17], -3)
    assert index.binary_stats() == before
    index.range_search(xq[:17], 20)
    after = index.binary_stats()
    assert after["range_batches"] == 1 and after["scan_passes"] == before["scan_passes"]
