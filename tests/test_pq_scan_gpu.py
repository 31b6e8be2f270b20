"""GPU tests of the product-quantised scan (csrc/ise_pq.hpp, pq_scan_kernel<QT>) where tests/test_pq_gpu.py does not
reach: waves that stream many tiles and cut their buffers again and again under live thresholds, rows of more than one
16-byte piece whose last piece is partly filled, the M at which QT switches (and the largest LDS footprints), more
queries than one table chunk, the encoder that reads its centroids from the codebook in place, and scores that overflow
from finite inputs.  All data are integers (tests/knn_checks.py): every comparison is bit for bit, no tolerance."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import pq_ref
from tests.knn_checks import HUGE, INT_KINDS, assert_exact_range, assert_knn_identical, int_data
from tests.sel_ref import IP, L2, pad_value

pytestmark = pytest.mark.gpu

CHUNKS = [250, 1, 349]  # the three add calls of a 600-row index
FLT_MAX = float(np.finfo(np.float32).max)


# ---- the host's grid arithmetic (csrc/ise_pq.hip, pq_grid), mirrored
def num_cu() -> int:
    import torch

    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def grid_of(M: int, n: int, cus: int) -> int:
    tiles = -(-n // 64)
    per_cu = max(1, 160 // (pq_ref.qt_of(M) * (M + 4)))  # blocks a CU holds: 160 KiB over QT * (M + 4) KiB
    return max(1, min(-(-tiles // 8), min(per_cu * cus, 1024)))


def tiles_per_wave(M: int, n: int, cus: int) -> int:
    return -(-(-(-n // 64)) // (4 * grid_of(M, n, cus)))


def passes_of(M, nq, k):
    return -(-nq // pq_ref.qt_of(M)) * -(-k // 32)


def empty_index(C, metric):
    M, _, dsub = C.shape
    index = faiss.IndexPQ(M * dsub, M, 8, metric)
    index.pq.set_centroids(C)
    assert index.is_trained and index.ntotal == 0
    return index


def added_index(M, dsub, kind, n, metric, seed, nq, chunks=None, fix=None):
    """An index of n integer rows added through ``add`` (the encoder), its codebook (after ``fix(C)``), rows, queries."""
    rng = np.random.default_rng(seed)
    C = int_data(kind, rng, M * 256, dsub).reshape(M, 256, dsub)
    if fix is not None:
        fix(C)
    xb, xq = int_data(kind, rng, n, M * dsub), int_data(kind, rng, nq, M * dsub)
    index = empty_index(C, metric)
    i0 = 0
    for c in chunks or [n]:
        index.add(xb[i0:i0 + c])
        i0 += c
        assert index.ntotal == i0
    assert i0 == n
    return index, C, xb, xq


def search_counted(index, xq, k, M):
    """search, with the counters checked: one batch, ceil(nq / QT) * ceil(k / 32) passes, ceil(nq / 64) table builds."""
    before = index.pq_stats()
    D, I = index.search(xq, k)
    after = index.pq_stats()
    assert after["search_batches"] - before["search_batches"] == 1
    assert after["scan_passes"] - before["scan_passes"] == passes_of(M, len(xq), k)
    assert after["table_builds"] - before["table_builds"] == -(-len(xq) // 64)
    return D, I


# ---------------------------------------------------------------- A. long indexes: the stream after a cut
NLONG = 400_003  # the last tile has 3 rows
LONG = [(12, 2, "signed", 17), (4, 4, "small", 17), (20, 2, "signed", 9), (64, 1, "signed", 5)]


def own_best_centroids(C, kind):
    """Centroids 255 and 254 of every sub-quantiser become vectors that are their own best match under EITHER metric:
    A = (hi, .., hi) and B = (-(hi + 1), 0, .., 0).  <A, c> <= hi * sum |c_t| <= |A|^2 and <B, c> <= (hi + 1) * hi
    < |B|^2 for every centroid c of the kind's range [lo, hi] (|lo| <= hi), with equality only at c = A; <A, B> < 0.
    A query that is decode-equal to a row of such centroids has that row (and its copies) alone at rank 0."""
    hi = INT_KINDS[kind][1]
    C[:, 255, :] = hi
    C[:, 254, :] = 0
    C[:, 254, 0] = -(hi + 1)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M,dsub,kind,nq", LONG)
def test_long_index_thresholds_repeated_cuts_and_worst_case_order(M, dsub, kind, nq, metric):
    """Every wave streams three tiles or more (seven on 256 CUs, where every one of these M gets one block per CU), so keys are
    turned away by a live threshold, appended behind the keys a cut kept, and cut again.  Query 0 sees the worst-case
    order (every tile beats or ties all before it: every key passes, a cut after every tile from the second on), the
    others a random order.  Rows: wave 0 of block 0 streams tiles 0, 4 G, 8 G, ...; the best row for query 1 is row 0
    and its runner-up the LAST row of tile 8 G, which has to get in below the threshold of the first cut."""
    cus, n = num_cu(), NLONG
    tpw, G, qt = tiles_per_wave(M, n, cus), grid_of(M, n, cus), pq_ref.qt_of(M)
    print(f"M={M} QT={qt}: {cus} CUs, grid {G}, tiles per wave {tpw}")
    assert tpw >= 3
    rng = np.random.default_rng(7000 + M)
    C = int_data(kind, rng, M * 256, dsub).reshape(M, 256, dsub)
    own_best_centroids(C, kind)
    xq = int_data(kind, rng, nq, M * dsub)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    s0 = pq_ref.adc_scores(xq[:1], C, codes, metric)[0]
    codes = codes[np.argsort(-s0 if metric == L2 else s0, kind="stable")]  # query 0: every row beats or ties its predecessors
    # query 1 = row 0 decoded; the runner-up: row 0's code with the one byte changed that costs the least
    runner = 8 * G * 64 + 63
    tie = [5, 64 * 4 * G + 1, n - 1]
    assert runner < n - 3 and tie[1] < runner
    codes[0] = 255
    xq[1] = pq_ref.decode(codes[:1], C)[0]
    T1 = pq_ref.adc_tables(xq[1:2], C, metric)[0]
    loss = T1 - T1[:, 255:] if metric == L2 else T1[:, 255:] - T1
    assert (loss >= 0).all()
    loss[loss == 0] = np.inf
    m1, j1 = np.unravel_index(np.argmin(loss), loss.shape)
    codes[runner] = codes[0]
    codes[runner, m1] = j1
    # one tie group for the last query: the first tile, a later tile of the same wave, the last (partial) tile
    codes[tie] = 254
    xq[-1] = pq_ref.decode(codes[5:6], C)[0]
    assert_exact_range(pq_ref.decode(np.unique(codes, axis=0), C), xq)

    scores = pq_ref.adc_scores(xq, C, codes, metric)
    Dw, Iw = pq_ref.adc_topk(scores, 70, metric)
    assert Iw[1, :2].tolist() == [0, runner] and Iw[-1, :3].tolist() == tie  # the data are what they were built to be
    del scores, s0

    index = empty_index(C, metric)
    index._add_codes(codes)
    assert index.ntotal == n and np.array_equal(index.codes, codes)
    for sub in sorted({1, qt + 1, nq}):
        for k in (1, 10, 33, 70):
            D, I = search_counted(index, xq[:sub], k, M)
            assert_knn_identical(D, I, Dw[:sub, :k], Iw[:sub, :k], f"nq={sub} k={k}")
            if sub > 1 and k >= 2:
                assert I[1, :2].tolist() == [0, runner], f"nq={sub} k={k}"
            if sub == nq and k >= 3:
                assert I[-1, :3].tolist() == tie, f"nq={sub} k={k}"


@pytest.mark.parametrize("metric", [L2, IP])
def test_long_index_of_equal_rows(metric):
    """Every key of every tile ties: only the ids decide, through every cut and every floor pass."""
    M, dsub, n = 12, 2, NLONG
    assert tiles_per_wave(M, n, num_cu()) >= 3
    rng = np.random.default_rng(71)
    C = int_data("signed", rng, M * 256, dsub).reshape(M, 256, dsub)
    code = rng.integers(0, 256, (1, M)).astype(np.uint8)
    codes = np.repeat(code, n, axis=0)
    row = pq_ref.decode(code, C)
    xq = np.concatenate([row, row])
    xq[1, 0] += 3.0  # the other query: the one non-zero distance 9 (inner product: another one score)
    assert_exact_range(row, xq)
    one = pq_ref.adc_scores(xq, C, code, metric).astype(np.float32)  # (2, 1)
    if metric == L2:
        assert one.tolist() == [[0.0], [9.0]]
    index = empty_index(C, metric)
    index._add_codes(codes)
    assert index.ntotal == n and np.array_equal(index.codes, codes)
    for k in (1, 32, 33, 100):
        D, I = search_counted(index, xq, k, M)
        assert_knn_identical(D, I, np.repeat(one, k, axis=1), np.tile(np.arange(k, dtype=np.int64), (2, 1)), f"k={k}")


# ---------------------------------------------------------------- B. piece boundaries and QT boundaries
def nonzero_first_centroid(C):
    C[:, 0, :] = 2  # a pad byte (zero) that is looked up all the same then changes the score


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M", [5, 6, 15, 17, 20, 35, 36, 48, 63])
def test_piece_and_qt_boundaries(M, metric):
    """M on both sides of every QT switch (5|6, 15|16, 35|36: the 144, 152 and 156 KiB launches) and rows of two to
    four pieces whose last piece is partly filled (M = 17, 20, 35, 36, 63)."""
    dsub, n = 2, 600
    index, C, xb, xq = added_index(M, dsub, "signed", n, metric, 2000 + M, 40, CHUNKS, nonzero_first_centroid)
    codes = pq_ref.encode(xb, C)
    assert np.array_equal(index.codes, codes)
    rec = index.reconstruct_n()
    assert np.array_equal(rec.view(np.uint32), pq_ref.decode(codes, C).view(np.uint32))
    assert_exact_range(rec, xq)
    qt = pq_ref.qt_of(M)
    Dw, Iw = pq_ref.adc_expected(xq, C, codes, 70, metric)
    for nq in sorted({1, qt, qt + 1, 40}):
        for k in (1, 33, 70):
            D, I = search_counted(index, xq[:nq], k, M)
            assert_knn_identical(D, I, Dw[:nq, :k], Iw[:nq, :k], f"nq={nq} k={k}")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M", [20, 35])
def test_partly_filled_piece_on_tile_edges(M, metric):
    for n in (1, 64, 65):
        index, C, xb, xq = added_index(M, 2, "signed", n, metric, 2100 + M + n, 9, None, nonzero_first_centroid)
        codes = pq_ref.encode(xb, C)
        assert np.array_equal(index.codes, codes)
        assert_exact_range(index.reconstruct_n(), xq)
        for k in (1, 33, 66):
            D, I = search_counted(index, xq, k, M)
            assert_knn_identical(D, I, *pq_ref.adc_expected(xq, C, codes, k, metric), f"n={n} k={k}")


# ---------------------------------------------------------------- C. more than one table chunk
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M", [8, 20])
def test_second_table_chunk(M, metric):
    index, C, xb, xq = added_index(M, 2, "signed", 600, metric, 3000 + M, 130, CHUNKS)
    codes = pq_ref.encode(xb, C)
    assert np.array_equal(index.codes, codes)
    assert_exact_range(index.reconstruct_n(), xq)
    Dw, Iw = pq_ref.adc_expected(xq, C, codes, 40, metric)
    for nq in (64, 65, 130):
        for k in (1, 40):
            D, I = search_counted(index, xq[:nq], k, M)  # ceil(nq / 64) table builds
            assert_knn_identical(D, I, Dw[:nq, :k], Iw[:nq, :k], f"nq={nq} k={k}")
            if nq > 64:  # the later chunks' results are those of a search of their own
                D2, I2 = index.search(xq[64:nq], k)
                assert_knn_identical(D[64:], I[64:], D2, I2, f"rows [64:] of nq={nq} k={k}")


@pytest.mark.parametrize("metric", [L2, IP])
def test_second_host_batch(metric):
    """4097 queries: two batches of the host form (4096 + 1), 64 + 1 table builds."""
    M, k = 8, 3
    index, C, xb, pool = added_index(M, 4, "small", 600, metric, 3100, 41, CHUNKS)
    codes = pq_ref.encode(xb, C)
    assert np.array_equal(index.codes, codes)
    assert_exact_range(index.reconstruct_n(), pool)
    Dw, Iw = pq_ref.adc_expected(pool, C, codes, k, metric)
    pick = np.random.default_rng(3101).integers(0, len(pool), 4097)
    before = index.pq_stats()
    D, I = index.search(pool[pick], k)
    after = index.pq_stats()
    assert_knn_identical(D, I, Dw[pick], Iw[pick], "nq=4097")
    assert after["search_batches"] - before["search_batches"] == 2
    assert after["table_builds"] - before["table_builds"] == 65
    assert after["scan_passes"] - before["scan_passes"] == passes_of(M, 4096, k) + passes_of(M, 1, k)


# ---------------------------------------------------------------- D. the encoder without LDS staging
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M,dsub", [(1, 129), (2, 192), (1, 300)])
def test_encoder_reading_the_codebook_in_place(M, dsub, metric):
    """dsub > 128: pq_encode_kernel<false>.  Two equal centroids (7 and 200): the rows on them get byte 7."""
    n, chunks = 300, [250, 1, 49]
    rng = np.random.default_rng(4000 + dsub)
    C = int_data("small", rng, M * 256, dsub).reshape(M, 256, dsub)
    C[:, 200] = C[:, 7]
    xb, xq = int_data("small", rng, n, M * dsub), int_data("small", rng, 9, M * dsub)
    xb[[3, 299]] = C[:, 7].reshape(-1)
    index = empty_index(C, metric)
    i0 = 0
    for c in chunks:
        index.add(xb[i0:i0 + c])
        i0 += c
    assert index.ntotal == n
    codes = pq_ref.encode(xb, C)
    assert (codes[[3, 299]] == 7).all()
    got = index.codes
    assert np.array_equal(got, codes) and (got[[3, 299]] == 7).all()
    assert np.array_equal(index.sa_encode(xb), codes)
    rec = index.reconstruct_n()
    assert np.array_equal(rec.view(np.uint32), pq_ref.decode(codes, C).view(np.uint32))
    assert_exact_range(rec, xq)
    for m in range(M):  # the encoder's own distances are exact too
        assert_exact_range(np.ascontiguousarray(xb[:, m * dsub:(m + 1) * dsub]), np.ascontiguousarray(C[m]))
    for k in (1, 33):
        D, I = search_counted(index, xq, k, M)
        assert_knn_identical(D, I, *pq_ref.adc_expected(xq, C, codes, k, metric), f"k={k}")
    block = xb[:130].copy()
    block[77, M * dsub - 1] = np.nan
    with pytest.raises(ValueError):
        index.add(block)
    assert index.ntotal == n
    with pytest.raises(ValueError):
        index.sa_encode(block)
    assert np.array_equal(index.codes, codes)


# ---------------------------------------------------------------- E. scores that overflow from finite inputs
SQ = (4095.0, 90.0, 9.0, 3.0)  # 4095^2 + 90^2 + 9^2 + 3^2 = 2^24 - 1: times 2^104 that is FLT_MAX, every partial sum exact
M_HUGE, J_HUGE, M_EDGE, J_EDGE = 3, 100, 5, 101
N_PLAIN = 4  # plain queries behind the special ones


def overflow_case(metric):
    """M = 8, dsub = 4, 600 rows of chosen codes.  Sub-quantiser 3: entry 1 of every centroid is 0 but HUGE = 2^64 at
    centroid 100.  Sub-quantiser 5: every centroid is 0 but centroid 101 = SQ * 2^52, of squared norm FLT_MAX exactly.
    Every query is the decoding of a code without these two centroids, so its entries facing them are 0: each table
    entry is a small integer, +-2^128 (float32: +-inf) or +-FLT_MAX, whatever the order it is summed in.  Inner product:
    query 0 gets HUGE, query 1 -HUGE in that column; query 2 is -centroid 101 in sub-quantiser 5 and 0 elsewhere."""
    M, dsub, n = 8, 4, 600
    rng = np.random.default_rng(5000)
    C = int_data("small", rng, M * 256, dsub).reshape(M, 256, dsub)
    C[M_HUGE, :, 1] = 0
    C[M_HUGE, J_HUGE, 1] = HUGE
    C[M_EDGE] = 0
    C[M_EDGE, J_EDGE] = np.asarray(SQ, np.float32) * np.float32(2.0 ** 52)
    assert (C[M_EDGE, J_EDGE].astype(np.float64) ** 2).sum() == FLT_MAX
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    special = 3 if metric == IP else 0
    qcodes = rng.integers(0, 256, (special + N_PLAIN, M)).astype(np.uint8)
    qcodes[:, M_HUGE], qcodes[:, M_EDGE] = 5, 6
    xq = pq_ref.decode(qcodes, C)
    # decode-copies of the plain queries, then made to overflow: a row that leaks shows at rank 0 (L2)
    huge_rows, edge_rows = [0, 63, 64, 300], [1, 65, 301, 599]
    for rows, (m, j) in ((huge_rows, (M_HUGE, J_HUGE)), (edge_rows, (M_EDGE, J_EDGE))):
        for i, r in enumerate(rows):
            codes[r] = qcodes[special + i % N_PLAIN]
            codes[r, m] = j
    if metric == IP:
        xq[0, M_HUGE * dsub + 1] = HUGE
        xq[1, M_HUGE * dsub + 1] = -HUGE
        xq[2] = 0
        xq[2, M_EDGE * dsub:(M_EDGE + 1) * dsub] = -C[M_EDGE, J_EDGE]
    # the precondition on the float64 tables
    T = pq_ref.adc_tables(xq, C, metric)
    big = np.abs(T) >= 2.0 ** 24
    assert np.isin(np.abs(T[big]), (2.0 ** 128, FLT_MAX)).all() and np.array_equal(T[~big], np.rint(T[~big]))
    assert np.abs(np.where(big, 0.0, T)).max(axis=2).sum(axis=1).max() < 2.0 ** 24
    for q in range(len(xq)):  # no query has large entries of both signs: no sum is inf - inf
        assert not ((T[q] >= 2.0 ** 24).any() and (T[q] <= -2.0 ** 24).any())
    index = empty_index(C, metric)
    index._add_codes(codes)
    assert index.ntotal == n and np.array_equal(index.codes, codes)
    planted_edge = edge_rows
    huge_rows = np.flatnonzero(codes[:, M_HUGE] == J_HUGE)  # the planted ones and those the random codes hold
    edge_rows = np.flatnonzero(codes[:, M_EDGE] == J_EDGE)
    assert len(huge_rows) >= 4 and len(edge_rows) >= 4
    return index, C, codes, xq, T, huge_rows, edge_rows, planted_edge


def test_overflowing_l2_scores_never_enter():
    """A distance that is inf in float32 (2^128), and one that is FLT_MAX exactly: neither is < FLT_MAX."""
    index, C, codes, xq, T, huge_rows, edge_rows, planted_edge = overflow_case(L2)
    n = len(codes)
    assert (T[:, M_HUGE, J_HUGE] == 2.0 ** 128).all() and (T[:, M_EDGE, J_EDGE] == FLT_MAX).all()
    scores = pq_ref.adc_scores(xq, C, codes, L2)
    out = np.union1d(huge_rows, edge_rows)
    assert (scores[:, out] >= FLT_MAX).all()
    assert all(scores[i % N_PLAIN, r] == FLT_MAX for i, r in enumerate(planted_edge))  # the copies: FLT_MAX exactly
    for k in (1, 33, n):
        D, I = search_counted(index, xq, k, 8)
        assert_knn_identical(D, I, *pq_ref.adc_topk(scores, k, L2), f"k={k}")
        assert not np.isin(I, out).any()
    assert (I[:, n - len(out):] == -1).all() and (D[:, n - len(out):] == pad_value(L2)).all()
    assert (I[:, :n - len(out)] >= 0).all()


def test_overflowing_inner_products():
    """+inf enters first (D = +inf, ascending ids); -inf and -FLT_MAX exactly never enter."""
    index, C, codes, xq, T, huge_rows, edge_rows, _ = overflow_case(IP)
    n, nh, ne = len(codes), len(huge_rows), len(edge_rows)
    assert T[0, M_HUGE, J_HUGE] == 2.0 ** 128 and T[1, M_HUGE, J_HUGE] == -2.0 ** 128 and T[2, M_EDGE, J_EDGE] == -FLT_MAX
    scores = pq_ref.adc_scores(xq, C, codes, IP)
    assert (scores[2, edge_rows] == -FLT_MAX).all()
    for k in (1, 33, n):
        D, I = search_counted(index, xq, k, 8)
        assert_knn_identical(D, I, *pq_ref.adc_topk(scores, k, IP), f"k={k}")
    assert I[0, :nh].tolist() == huge_rows.tolist() and np.isposinf(D[0, :nh]).all() and np.isfinite(D[0, nh:]).all()
    assert not np.isin(I[1], huge_rows).any() and (I[1, n - nh:] == -1).all() and (D[1, n - nh:] == pad_value(IP)).all()
    assert not np.isin(I[2], edge_rows).any() and (I[2, n - ne:] == -1).all() and (D[2, n - ne:] == pad_value(IP)).all()
    assert (I[2, :n - ne] >= 0).all() and (I[3:] >= 0).all()


# ---------------------------------------------------------------- F. one block: a cut, then lists that end short
@pytest.mark.parametrize("M", [4, 12, 20, 64])  # QT = 16, 8, 4, 2
def test_one_block_cut_then_short_lists(M):
    """512 rows are eight tiles in one block: wave 0 streams tiles 0 and 4 and cuts after the second, every wave folds.
    The rows lie in descending distance to query 0 (every key of the second tile passes), k = 33 runs the floor-keyed
    second pass and the merge's floor write.  Sub-quantiser 0 has two HUGE centroids: a row coded with one of them is at
    distance inf from every ordinary query and never enters.  The last three queries are far from all other rows:
    query 13 sits on centroid 255 (20 rows are finite: a first pass that ends short, a finished second pass), query 15
    on centroid 254 (exactly 32 rows: a full first pass, then nothing above the floor), query 14 on neither (no row)."""
    dsub, n, nq, k = 2, 512, 16, 33
    qt = pq_ref.qt_of(M)
    assert grid_of(M, n, 256) == 1 and qt == {4: 16, 12: 8, 20: 4, 64: 2}[M]
    rng = np.random.default_rng(9000 + M)
    C = int_data("small", rng, M * 256, dsub).reshape(M, 256, dsub)
    C[0, 255], C[0, 254] = (HUGE, 0), (-HUGE, 0)
    codes = rng.integers(0, 254, (n, M)).astype(np.uint8)
    xq = pq_ref.decode(rng.integers(0, 254, (nq, M)).astype(np.uint8), C)
    assert_exact_range(pq_ref.decode(np.unique(codes, axis=0), C), xq)
    codes = codes[np.argsort(-pq_ref.adc_scores(xq[:1], C, codes, L2)[0], kind="stable")]
    on255, on254 = np.arange(7, n, 26)[:20], np.arange(2, n, 16)  # spread over the eight tiles
    assert len(on255) == 20 and len(on254) == 32 and not np.intersect1d(on255, on254).size
    codes[on255, 0], codes[on254, 0] = 255, 254
    xq[13, :2], xq[14, :2], xq[15, :2] = (HUGE, 0), (0, HUGE), (-HUGE, 0)
    scores = pq_ref.adc_scores(xq, C, codes, L2)
    fin = scores < FLT_MAX
    assert (fin[:13].sum(1) == n - 52).all() and fin[13:].sum(1).tolist() == [20, 0, 32]
    assert (scores[~fin] >= 2.0 ** 127).all() and scores[fin].max() < 2.0 ** 24  # inf in any order | exact in any order
    plain = np.setdiff1d(np.arange(n), np.union1d(on255, on254))
    assert (np.diff(scores[0, plain]) <= 0).all()  # query 0: every row beats or ties its predecessors
    Dw, Iw = pq_ref.adc_topk(scores, k, L2)
    assert (Iw[13, 20:] == -1).all() and (Iw[14] == -1).all() and Iw[15, 32] == -1 and (Iw[[13, 15], :20] >= 0).all()
    index = empty_index(C, L2)
    index._add_codes(codes)
    assert index.ntotal == n and np.array_equal(index.codes, codes)
    D, I = search_counted(index, xq, k, M)
    assert_knn_identical(D, I, Dw, Iw, f"M={M} QT={qt}")
    assert (D[I < 0] == pad_value(L2)).all()
