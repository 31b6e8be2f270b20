"""GPU tests of the large-batch (GEMM-shaped) passes at the edges of their shapes: a ragged last row tile, rows
padded from d to dp, chunk and stage tails, k at the gate, packed keys with an id base, removal and a far shift
(csrc/ise_gemm_scan.hpp, csrc/ise_gemm_bf16.hpp, search_large_chunk in csrc/ise_knn.hip).

All data but the last test's are the integers 0..15 (tests/knn_checks.py; the inner-product queries of the cases at
d = 100 carry random signs, see ``_base``): every score is exact in float32 and in bf16, so D and I must equal the
oracle's bit for bit, ties by ascending id -- ``assert_knn_identical``, no tolerance.
Every case asserts its route (``gemm_chunks`` against tests/gemm_ref.py) and, for the flavours without a re-rank
(float32 inner product, bf16 rows), how many queries the pass lost to the streaming passes behind it
(``gemm_lost_queries``): none, unless the case is built to overflow.

Every index is the smallest the gate admits, 131 072 rows plus a tail.  The tail rows are built from the queries
(a copy for L2, the double for inner product), so that a tail the pass does not scan shows at rank 0; the
all-zero (L2) and all-minus-one (inner product) queries would rank a zero pad row first if one entered.

The reference of the cases at d = 100 is the oracle's top k over the first 131 072 rows, computed once per metric,
merged by (score, id) with the float64 scores of the rows behind them: the same set as the oracle over all rows.

Measured on an MI355X, and asserted below: the overflow construction of the keys test sends all 256 queries of the
float32 L2 flavour to the exact scan (exact_scan = 256) and loses all 256 queries of each plain flavour
(gemm_lost_queries = 256); every other case loses none; the uniform case sends no query to the exact scan
(exact_scan = 0).  Not asserted: after the far shift all 256 queries take the exact scan (the bound is as wide as
the distances there), with identical results."""
import functools
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests import gemm_ref as gr
from tests import keycodec
from tests.knn_checks import ATOL_UNIFORM, assert_exact_range, assert_knn_identical, assert_knn_matches, int_data

pytestmark = pytest.mark.gpu

L2, IP = ko.METRIC_L2, ko.METRIC_INNER_PRODUCT
assert (L2, IP) == (gr.L2, gr.IP)
FLAVOURS = [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")]
BASE = gr.GEMM_MIN_ROWS   # 131 072 rows: the shortest index the path takes; a multiple of either slab
D0, NQ0, K0 = 100, 256, 10  # d < dp = 128 for either storage; one full chunk stage set; the usual k
KREF = 33                 # ranks of the shared reference: the largest k below
ID_BASE = 3_000_000_000   # above 2^31; ID_BASE + n below 2^32

# ---- the case tables (tests/test_gemm_shapes.py checks them against tests/gemm_ref.py without a GPU)
# (a) n - 131 072 after each add: around a lane's four rows, a 16-row tile, (bf16) a wave's two tiles, a slab
WALK = {"f32": (1, 3, 4, 5, 15, 16, 17, 127, 128, 129),
        "bf16": (1, 3, 4, 15, 16, 17, 31, 32, 33, 255, 256, 257)}
# (b) d on either side of the gate, n = 131 073
DIMS_ON = {"f32": (65, 101, 127, 250, 330, 500), "bf16": (97, 101, 127, 250, 330, 500)}
DIMS_OFF = {"f32": (129, 257), "bf16": (96,)}
# (c) batch sizes: the smallest, uneven stage splits of the threshold sample, a second chunk of one query
NQ_EDGES = {"f32": (257, 287, 1025), "bf16": (128, 129, 191, 1025)}
NQ_EDGE_CASES = [(m, s, nq) for m, s in FLAVOURS for nq in NQ_EDGES[s] if nq <= 287 or m == L2]  # oracle cost: L2 only
# (d) the largest k of the path and the first beyond it
K_GATE = [(L2, "f32", 28, 29), (IP, "f32", 32, 33), (L2, "bf16", 32, 33), (IP, "bf16", 32, 33)]
DIM_CASES = sorted((d, m, s, on) for m, s in FLAVOURS for on, table in ((True, DIMS_ON), (False, DIMS_OFF))
                   for d in table[s])  # by (d, metric): the two storages share a reference


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _index(faiss, xb, metric, storage):
    index = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    index.add(xb)
    return index


def _free(*indexes):
    import torch

    for index in indexes:
        index.__del__()
    torch.cuda.empty_cache()


def _stats(index):
    return {**index.exact_stats(), **index.gemm_stats()}


def _plain(metric, storage):
    """The flavours without a re-rank: a lost query shows only in gemm_lost_queries."""
    return not (metric == L2 and storage == "f32")


def _routed(index, run, metric, storage, nq, k, lost=0):
    """run() with the route asserted against gemm_ref.expects_gemm and the lost queries against ``lost`` (None: the
    caller asserts them).  -> (run's result, the counters' deltas)."""
    before = _stats(index)
    out = run()
    now = _stats(index)
    dt = {key: now[key] - before[key] for key in now}
    print(f"n={index.ntotal} d={index.d} {storage} metric={metric} nq={nq} k={k}: {dt}")
    on = gr.expects_gemm(index.ntotal, index.d, storage, metric, nq, k)
    assert dt["gemm_chunks"] == (gr.chunks(nq) if on else 0), (dt, on)
    if lost is not None:
        assert dt["gemm_lost_queries"] == lost, dt
    if not _plain(metric, storage):
        assert dt["gemm_lost_queries"] == 0, "float32 L2 loses queries to the exact scan, not to this counter"
    return out, dt


def _tail_row(x, metric):
    """The row that must be rank 0 of query x: a copy (L2: distance 0), or the double (inner product)."""
    return x.copy() if metric == L2 else 2.0 * x


@functools.lru_cache(maxsize=None)
def _base(metric):
    """131 072 x 100 rows, 1025 queries (inner product: with random signs) and the oracle's KREF best of the queries
    the cases of this metric use.
    Query 255 is the one a zero pad row would win: all zero (L2), all minus one (inner product: every row sums to
    a positive number, so every real score is negative)."""
    rng = _rng("base")
    xb0, xq = int_data("small", rng, BASE, D0), int_data("small", rng, 1025, D0)
    if metric == IP:
        # Random signs on the queries.  Between all-positive queries the double of one beats every row of the
        # threshold sample for every other query too: a tail of 9 or more such rows puts over 2048 candidates (rows x
        # 256 queries) into the buffer of the one wave that holds their tile, which overflows, and the streaming
        # passes rewrite the chunk (measured: 256 lost queries at n = 131 087) -- the pass's own answer for the tail
        # would never be seen.  With signs q'.q is centred on zero and a double is a candidate of few other queries.
        # Every query is signed as a whole so that its entries sum to a positive number: the rows built from it then
        # score negative against the all-minus-one query, like the rows of the index.
        xq *= rng.choice([-1.0, 1.0], xq.shape).astype(np.float32)
        xq[xq.sum(1) < 0] *= -1.0
        xq[xq.sum(1) == 0, 0] = np.abs(xq[xq.sum(1) == 0, 0]) + 1.0
        assert xq.sum(1).min() > 0
    xq[255] = 0.0 if metric == L2 else -1.0
    assert xb0.sum(1).min() > 0
    assert_exact_range(np.concatenate([xb0, 2.0 * xq]), xq)  # with the doubled queries of the tails
    nref = 1025 if metric == L2 else 287  # (the inner-product oracle is four times slower; its cases stop at 287)
    D, I = ko.knn_exact(xb0, xq[:nref], KREF, metric)
    for a in (xb0, xq, D, I):
        a.setflags(write=False)
    return xb0, xq, D, I


def _merged_ref(metric, qsel, tail, k):
    """The reference over the base rows followed by ``tail``: the base's KREF best merged with the float64 scores
    of the tail rows, by (score, id)."""
    _, xq, D0_, I0_ = _base(metric)
    assert k <= KREF and qsel.max() < D0_.shape[0]
    S = ko.pairwise_f64(xq[qsel], tail, metric)
    D = np.empty((len(qsel), k), np.float32)
    I = np.empty((len(qsel), k), np.int64)
    tail_ids = BASE + np.arange(len(tail), dtype=np.int64)
    for j, q in enumerate(qsel):
        sc = np.concatenate([D0_[q].astype(np.float64), S[j]])
        ids = np.concatenate([I0_[q], tail_ids])
        order = np.lexsort((ids, sc if metric == L2 else -sc))[:k]
        D[j], I[j] = sc[order].astype(np.float32), ids[order]
    return D, I


def _one_tail_case(faiss, metric, storage, nq, k, plant_q):
    """A fresh index of 131 073 rows at d = 100 whose last row is the best of query ``plant_q``; -> index, queries,
    reference."""
    xb0, xq_all, _, _ = _base(metric)
    xq = np.ascontiguousarray(xq_all[:nq])
    tail = _tail_row(xq[plant_q], metric)[None, :]
    D_ref, I_ref = _merged_ref(metric, np.arange(nq), tail, k)
    assert I_ref[plant_q, 0] == BASE, "the premise: the last row is rank 0 of its query"
    index = _index(faiss, np.concatenate([xb0, tail]), metric, storage)
    return index, xq, D_ref, I_ref


# ------------------------------------------------------------------------------------------ (a) the growing tail
@pytest.mark.parametrize("metric,storage", FLAVOURS)
def test_growing_tail(faiss, metric, storage):
    """One index grown past 131 072 rows through WALK, searched after every add: a last lane quad, tile and slab of
    every fill, a slab of one row, and (float32 L2) rows added after a search."""
    xb0, xq_all, _, _ = _base(metric)
    xq = np.ascontiguousarray(xq_all[:NQ0])
    steps = WALK[storage]
    nsrc = NQ0 - 1  # the tail rows are built from the queries before the fixed one, in turn
    tail = np.stack([_tail_row(xq[i % nsrc], metric) for i in range(steps[-1])])
    index = _index(faiss, xb0, metric, storage)
    have = 0
    for r in (0,) + steps:
        if r:
            index.add(tail[have:r])
        n = BASE + r
        assert index.ntotal == n
        D_ref, I_ref = _merged_ref(metric, np.arange(NQ0), tail[:r], K0)
        for i in range(have, r):  # the rows of this step: rank 0 of their query, or rank 1 behind its earlier copy
            q, rank = i % nsrc, i // nsrc
            assert I_ref[q, rank] == BASE + i and D_ref[q, rank] == D_ref[q, 0], "the premise: the tail rows win"
        assert (D_ref[255] > 0).all() if metric == L2 else (D_ref[255] < 0).all(), "the premise: a zero row would win"
        (D, I), _ = _routed(index, lambda: index.search(xq, K0), metric, storage, NQ0, K0)
        assert (I < n).all() and (I >= 0).all(), "a row past the end entered"
        assert_knn_identical(D, I, D_ref, I_ref, f"n = 131072 + {r}")
        have = r
    # the merged reference against the oracle over all rows, once
    D_all, I_all = ko.knn_exact(np.concatenate([xb0, tail]), xq, K0, metric)
    assert_knn_identical(D_ref, I_ref, D_all, I_all, "merged reference")
    _free(index)


# ------------------------------------------------------------------------------------- (b) d against dp, the gate
@functools.lru_cache(maxsize=1)
def _dim_case(d, metric):
    rng = _rng("dims", d)
    n = BASE + 1
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, NQ0, d)
    xb[n - 1] = _tail_row(xq[0], metric)
    assert_exact_range(xb, xq)
    D_ref, I_ref = ko.knn_exact(xb, xq, K0, metric)
    assert I_ref[0, 0] == n - 1, "the premise: the last row is rank 0 of query 0"
    return xb, xq, D_ref, I_ref


@pytest.mark.parametrize("d,metric,storage,on", DIM_CASES)
def test_row_padding_and_the_dimension_gate(faiss, d, metric, storage, on):
    """A fresh index of 131 073 rows: d below dp on the path (the zero fill of the query prep, the odd-d half pair
    of the bf16 prep, the shift's padding), and the d whose dp is no multiple of 128 off it."""
    xb, xq, D_ref, I_ref = _dim_case(d, metric)
    assert gr.expects_gemm(len(xb), d, storage, metric, NQ0, K0) == on
    index = _index(faiss, xb, metric, storage)
    (D, I), dt = _routed(index, lambda: index.search(xq, K0), metric, storage, NQ0, K0)
    assert dt["gemm_chunks"] == (1 if on else 0)
    assert_knn_identical(D, I, D_ref, I_ref, f"d = {d}")
    _free(index)


# ------------------------------------------------------------------------------------ (c) chunk and stage edges
@pytest.mark.parametrize("metric,storage,nq", NQ_EDGE_CASES)
def test_chunk_and_stage_edges(faiss, metric, storage, nq):
    """Batches at the gate, with stages that split unevenly over the threshold sample's blocks, and with a second
    chunk of one query (one stage, one part, a fallback plan shaped for one query)."""
    index, xq, D_ref, I_ref = _one_tail_case(faiss, metric, storage, nq, K0, nq - 1)
    (D, I), dt = _routed(index, lambda: index.search(xq, K0), metric, storage, nq, K0)
    assert dt["gemm_chunks"] == -(-nq // 1024)
    assert_knn_identical(D, I, D_ref, I_ref, f"nq = {nq}")
    _free(index)


# ----------------------------------------------------------------------------------------- (d) k at the gate
@pytest.mark.parametrize("metric,storage,k_on,k_off", K_GATE)
def test_k_at_the_gate(faiss, metric, storage, k_on, k_off):
    index, xq, D_ref, I_ref = _one_tail_case(faiss, metric, storage, NQ0, KREF, 0)
    for k, chunks in ((k_on, 1), (k_off, 0)):
        (D, I), dt = _routed(index, lambda: index.search(xq, k), metric, storage, NQ0, k)
        assert dt["gemm_chunks"] == chunks, (k, dt)
        assert_knn_identical(D, I, D_ref[:, :k], I_ref[:, :k], f"k = {k}")
    _free(index)


# --------------------------------------------------------------------------------------- (e) keys and id_base
def _keys(index, xq, k, metric):
    import torch

    keys = index.search_keys_torch(torch.tensor(xq).cuda(), k, id_base=ID_BASE)
    torch.cuda.synchronize()
    return keycodec.decode(keys.cpu().numpy().view(np.uint64), metric)


@pytest.mark.parametrize("metric,storage", FLAVOURS)
def test_keys_with_an_id_base(faiss, metric, storage):
    """search_keys_torch on the path: packed keys, ids shifted by a base above 2^31."""
    index, xq, D_ref, I_ref = _one_tail_case(faiss, metric, storage, NQ0, K0, 0)
    assert ID_BASE > 1 << 31 and ID_BASE + index.ntotal < 1 << 32
    (D, I), _ = _routed(index, lambda: _keys(index, xq, K0, metric), metric, storage, NQ0, K0)
    assert_knn_identical(D, I, D_ref, I_ref + ID_BASE, "keys")
    _free(index)


@pytest.mark.parametrize("metric,storage", FLAVOURS)
def test_keys_with_an_id_base_through_the_overflow(faiss, metric, storage):
    """Binary values on 3 of the columns, the 8 distinct rows repeated in turn: every sampled slab holds 16 copies
    of each, so a query's admit threshold is the score of its best distinct row and all its 16 384 copies are
    admitted, more than the query's candidate slots.  Float32 L2 hands every query to the exact scan; the others
    lose queries and the streaming passes queued behind the chunk rewrite it.  Either way the keys carry the id
    base."""
    n, nq = BASE + 1, NQ0
    rng = _rng("overflow", metric, storage)
    xb, xq = np.zeros((n, D0), np.float32), np.zeros((nq, D0), np.float32)
    pattern = np.arange(n) % 8
    xb[:, :3] = (pattern[:, None] >> np.arange(3)) & 1
    xq[:, :3] = int_data("binary", rng, nq, 3)
    assert np.bincount(pattern).min() >= 16_384 > gr.GEMM_CAPQ and K0 + gr.EXACT_EXTRA <= 16
    assert_exact_range(xb, xq)
    D_ref, I_ref = ko.knn_exact(xb, xq, K0, metric)
    index = _index(faiss, xb, metric, storage)
    (D, I), dt = _routed(index, lambda: _keys(index, xq, K0, metric), metric, storage, nq, K0, lost=None)
    if _plain(metric, storage):
        assert dt["gemm_lost_queries"] == nq, "every query's best row has more copies than the query has slots"
    else:
        assert dt["exact_scan"] == nq, "an overflowed candidate array must send its query to the exact scan"
    assert_knn_identical(D, I, D_ref, I_ref + ID_BASE, "keys through the overflow")
    _free(index)


# ------------------------------------------------------------------------------------------------- (f) removal
@pytest.mark.parametrize("metric,storage", FLAVOURS)
def test_removal_leaves_a_ragged_tail_and_then_the_path(faiss, metric, storage):
    """131 072 + 40 rows, the last 40 the best rows of queries 0..39; 35 scattered rows removed (five of them in
    the tail, three in the last tile): n = 5 mod 16, and copies of queries lie as stale rows right behind the end.
    Identical to a fresh index of the rows that are left.  Six more removed: the index falls below the gate."""
    xb0, xq_all, _, _ = _base(metric)
    xq = np.ascontiguousarray(xq_all[:NQ0])
    xb = np.concatenate([xb0, np.stack([_tail_row(xq[i], metric) for i in range(40)])])
    rng = _rng("remove")
    gone = np.concatenate([rng.choice(BASE, 30, replace=False), BASE + np.array([2, 17, 33, 36, 39])])
    more = np.concatenate([rng.choice(BASE - 64, 4, replace=False), [BASE - 40, BASE - 1]])  # ids after the first removal
    index = _index(faiss, xb, metric, storage)
    keep = np.ones(len(xb), bool)
    for ids, left in ((gone, BASE + 5), (more, BASE - 1)):
        assert index.remove_ids(ids.astype(np.int64)) == len(ids)
        keep[np.flatnonzero(keep)[ids]] = False
        assert index.ntotal == left == keep.sum()
        fresh = _index(faiss, xb[keep], metric, storage)
        (Dw, Iw), _ = _routed(fresh, lambda: fresh.search(xq, K0), metric, storage, NQ0, K0)
        (D, I), dt = _routed(index, lambda: index.search(xq, K0), metric, storage, NQ0, K0)
        assert dt["gemm_chunks"] == (1 if left >= BASE else 0)
        assert (I < left).all()
        assert_knn_identical(D, I, Dw, Iw, f"after removal, n = {left}")
        _free(fresh)
    _free(index)


# ---------------------------------------------------------------------------------------------- (g) a far shift
def test_far_shift_keeps_the_padding_zero(faiss):
    """Float32 L2 at d = 101 after set_shift with a far shift: the shift's entries between d and dp must stay zero
    (a non-zero one would move every padded row and query apart).  Results do not depend on the shift."""
    d = 101
    xb, xq, D_ref, I_ref = _dim_case(d, L2)
    index = _index(faiss, xb, L2, "f32")
    index.set_shift(np.full(d, 1e3, np.float32))
    (D, I), dt = _routed(index, lambda: index.search(xq, K0), L2, "f32", NQ0, K0)
    assert dt["gemm_chunks"] == 1
    assert_knn_identical(D, I, D_ref, I_ref, "far shift")
    _free(index)


# --------------------------------------------------------------------------------------------- (h) uniform data
def test_uniform_rows_below_the_padded_dimension(faiss):
    """Float32 L2 on uniform [0, 1) data at n = 131 073, d = 100: no query may need the exact scan (the bound's
    width depends on dp, not on d), and distances stay within the absolute bound."""
    rng = np.random.default_rng(100)
    n = BASE + 1
    xb, xq = rng.random((n, D0), dtype=np.float32), rng.random((NQ0, D0), dtype=np.float32)
    xq[3] = xb[n - 1]
    index = _index(faiss, xb, L2, "f32")
    (D, I), dt = _routed(index, lambda: index.search(xq, K0), L2, "f32", NQ0, K0)
    assert dt["gemm_chunks"] == 1
    assert dt["exact_scan"] == 0, "certificate failed on uniform data"
    D_ref, I_ref = ko.knn_exact(xb, xq, K0, L2)
    assert_knn_matches(D, I, D_ref, I_ref, xb, xq, L2, atol=ATOL_UNIFORM)
    assert I[3, 0] == n - 1 and D[3, 0] == 0.0
    _free(index)
