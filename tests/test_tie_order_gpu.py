"""GPU tests of tie order and exact distances on every kNN path, on integer data (tests/knn_checks.py).

On small integers every product and partial sum is an integer below 2^24: float32 arithmetic is exact in any
order and bf16 holds the values exactly.  So every kernel's D must equal the oracle's D bit for bit, and the only
correct I is the (score, id) order, ties by ascending id (DESIGN.md sections 2 and 3).  Every
case asserts the route counter that shows which path answered, and compares with ``assert_knn_identical``:
no tolerance, no near-tie escape."""
import contextlib
import threading
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.knn_checks import (assert_exact_range, assert_knn_identical, assert_knn_matches, int_data, level_rows,
                              plant_ties)
from tests.test_exact_l2_gpu import force_direct, forced_exact, no_direct, no_short

pytestmark = pytest.mark.gpu

L2, IP = ko.METRIC_L2, ko.METRIC_INNER_PRODUCT
STORAGES = [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")]
KIND_D = {"binary": 16, "small": 64, "signed": 64}


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _index(faiss, xb, metric, storage="f32"):
    import torch

    if storage == "bf16":  # the index rounds rows and queries to bf16: a no-op on these integers
        assert np.array_equal(torch.from_numpy(xb).to(torch.bfloat16).to(torch.float32).numpy(), xb)
    index = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    index.add(xb)
    return index


def _ref(xb, xq, k, metric, id_offset=0):
    assert_exact_range(xb, xq)
    return ko.knn_exact(xb, xq, k, metric, id_offset)


def _routes(index):
    return {**index.exact_stats(), **index.host_stats(), **index.short_stats(), **index.gemm_stats()}


def _delta(index, before):
    now = _routes(index)
    return {key: now[key] - before[key] for key in now}


def _kmax(metric, storage):
    """Largest k of one pass (the short kernel's limit): candidates kc <= KPASS_MAX = 36, where float32 L2
    keeps kc = k + 4 (4 spare candidates for the exact re-rank) and the others kc = k."""
    return 32 if (metric == L2 and storage == "f32") else 36


# ------------------------------------------------------------------------------- short-index kernel
@pytest.mark.parametrize("kind", ["binary", "small", "signed"])
@pytest.mark.parametrize("n", [1000, 4097, 100_000])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_short_kernel_tie_order(faiss, metric, storage, n, kind):
    """Batches of 1 to 64 queries, k = 1, 10 and the largest one-pass k, through the short-index kernel and
    (no_short) the streaming kernel: both identical to the oracle.  A planted group of four copies at ids 3,
    n/2, n/2 + 1 and n - 1, with query 0 on it."""
    d = KIND_D[kind]
    rng = _rng("short", metric, storage, n, kind)
    xb, xq_all = int_data(kind, rng, n, d), int_data(kind, rng, 64, d)
    plant_ties(xb, 3, [n // 2, n // 2 + 1, n - 1])
    xq_all[0] = xb[3]
    index = _index(faiss, xb, metric, storage)
    kmax = _kmax(metric, storage)
    for nq in (1, 16, 33, 64):
        if nq == 1 and metric == L2 and storage == "f32":
            continue  # the one-query direct scan: test_direct_scan_tie_order
        xq = xq_all[:nq]
        D_ref, I_ref = _ref(xb, xq, kmax, metric)
        for k in (1, 10, kmax):
            before = _routes(index)
            D, I = index.search(xq, k)
            assert _delta(index, before)["short_batches"] == 1, (nq, k)
            assert_knn_identical(D, I, D_ref[:, :k], I_ref[:, :k], f"short kernel nq={nq} k={k}")
            with no_short():
                Ds, Is = index.search(xq, k)
            assert _delta(index, before)["short_batches"] == 1
            assert_knn_identical(Ds, Is, D_ref[:, :k], I_ref[:, :k], f"streaming kernel nq={nq} k={k}")


@pytest.mark.parametrize("layout", ["all_equal", "runs"])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_short_kernel_general_selection(faiss, metric, storage, layout):
    """More than 64 rows of one wave at or below its threshold: the short kernel's general selection
    (wave_select) instead of ranking up to 64 survivors.  An index of one repeated row, and binary rows with
    runs of identical all-one rows -- the best row for every query of either metric (L2 queries on the all-one
    row, inner-product queries binary) -- one run of 600 rows, longer than a block's 32 row tiles at most, so it
    straddles a block boundary.  For float32 inner product and bf16 the block lists reach the result directly.
    For float32 L2 the certificate fails on such ties and the exact scan answers: the branch is only
    indirectly observable there (its lists feed the re-rank), and the exact_scan count is asserted."""
    n, d = (20_000, 16) if layout == "all_equal" else (100_000, 16)
    rng = _rng("general", metric, storage, layout)
    if layout == "all_equal":
        xb = np.repeat(int_data("binary", rng, 1, d), n, axis=0)
    else:
        xb = int_data("binary", rng, n, d)
        xb[xb.sum(1) == d] = 0  # the runs are the only all-one rows
        for lo, length in ((100, 120), (4000, 600), (50_001, 150), (n - 130, 130)):
            xb[lo:lo + length] = 1.0
    index = _index(faiss, xb, metric, storage)
    for nq, k in ((16, 10), (64, _kmax(metric, storage)), (33, 1)):
        xq = int_data("binary", rng, nq, d)
        if metric == L2:
            xq[: nq // 2] = 1.0 if layout == "runs" else xb[0]
        before = _routes(index)
        D, I = index.search(xq, k)
        dt = _delta(index, before)
        assert dt["short_batches"] == 1
        if metric == L2 and storage == "f32":
            assert dt["reranked"] == nq and dt["exact_scan"] >= nq // 2
        D_ref, I_ref = _ref(xb, xq, k, metric)
        assert_knn_identical(D, I, D_ref, I_ref, f"nq={nq} k={k}")
        if layout == "all_equal":
            assert (I == np.arange(k)[None, :]).all()


# --------------------------------------------------------------------------------- streaming kernel
@pytest.mark.parametrize("case", ["nq48_binary", "nq48_small", "nq65", "d2048"])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_streaming_kernel_tie_order(faiss, metric, storage, case):
    """Batches the short kernel does not take: 48 queries against 300k x 96 rows (three query tiles per pass,
    thresholds exchanged between blocks, whose bound must keep every id at the exchanged score), 65 queries
    (three passes), and the reference's descriptor width (2048 floats, 8 KB rows) at 3000 rows."""
    n, d, nq, kind = {"nq48_binary": (300_000, 96, 48, "binary"), "nq48_small": (300_000, 96, 48, "small"),
                      "nq65": (50_000, 64, 65, "small"), "d2048": (3000, 2048, 16, "small")}[case]
    rng = _rng("stream", metric, storage, case)
    xb, xq = int_data(kind, rng, n, d), int_data(kind, rng, nq, d)
    plant_ties(xb, 7, [n // 3, n // 3 + 1, n - 1])
    xq[0] = xb[7]
    index = _index(faiss, xb, metric, storage)
    D_ref, I_ref = _ref(xb, xq, 20, metric)
    for k in (1, 10, 20):
        before = _routes(index)
        D, I = index.search(xq, k)
        dt = _delta(index, before)
        assert dt["short_batches"] == 0 and dt["gemm_chunks"] == 0 and dt["direct_queries"] == 0
        if metric == L2 and storage == "f32":
            assert dt["reranked"] == nq
            if kind == "binary":
                assert dt["exact_scan"] > 0
        assert_knn_identical(D, I, D_ref[:, :k], I_ref[:, :k], f"{case} k={k}")


# ------------------------------------------------------------------------------ one-query direct scan
@pytest.mark.parametrize("n", [1000, 100_000])
@pytest.mark.parametrize("kind", ["binary", "small", "signed"])
def test_direct_scan_tie_order(faiss, kind, n):
    """One float32 L2 query, k = 1, 10, 32: the direct-difference scan and its final quickselect over the list
    keys (by default up to 128 row tiles; at 100k rows under force_direct).  The same bits from the filtered
    path (no_direct)."""
    d = KIND_D[kind]
    rng = _rng("direct", kind, n)
    xb, xq = int_data(kind, rng, n, d), int_data(kind, rng, 4, d)
    plant_ties(xb, 9, [10, n // 2, n - 1])
    xq[0] = xb[9]
    index = _index(faiss, xb, L2)
    D_ref, I_ref = _ref(xb, xq, 32, L2)
    ctx = force_direct if n > 2048 else contextlib.nullcontext
    for k in (1, 10, 32):
        for j in range(4):
            with ctx():
                before = _routes(index)
                D, I = index.search(xq[j:j + 1], k)
                assert _delta(index, before)["direct_queries"] == 1
            assert_knn_identical(D, I, D_ref[j:j + 1, :k], I_ref[j:j + 1, :k], f"direct q={j} k={k}")
            with no_direct():
                before = _routes(index)
                Df, If = index.search(xq[j:j + 1], k)
                assert _delta(index, before)["direct_queries"] == 0
            assert_knn_identical(Df, If, D_ref[j:j + 1, :k], I_ref[j:j + 1, :k], f"filtered q={j} k={k}")


# ---------------------------------------------------------------------------------------- exact scan
@pytest.mark.parametrize("short", [True, False])
def test_exact_scan_tie_order(faiss, short):
    """Binary rows: ties at the k-th distance make certificates fail on their own, and the exact scan answers;
    forced_exact fails every certificate.  Both identical to the oracle."""
    rng = _rng("exact", short)
    n, d, nq, k = 24_000, 16, 16, 10
    xb, xq = int_data("binary", rng, n, d), int_data("binary", rng, nq, d)
    index = _index(faiss, xb, L2)
    D_ref, I_ref = _ref(xb, xq, k, L2)
    ctx = contextlib.nullcontext if short else no_short
    with ctx():
        before = _routes(index)
        D, I = index.search(xq, k)
        dt = _delta(index, before)
    assert dt["exact_scan"] > 0 and dt["reranked"] == nq and dt["short_batches"] == (1 if short else 0)
    assert_knn_identical(D, I, D_ref, I_ref, "natural certificate failures")
    with ctx(), forced_exact():
        before = _routes(index)
        Df, If = index.search(xq, k)
        dt = _delta(index, before)
    assert dt["exact_scan"] == nq and dt["short_batches"] == (1 if short else 0)
    assert_knn_identical(Df, If, D_ref, I_ref, "forced exact")


# ----------------------------------------------------------------------------------- multi-pass k
def _pass_groups(k):
    """Tie-group sizes whose groups straddle every multiple of KPASS_MAX = 36 ranks (a pass boundary of the
    floor-keyed passes) up to k + 40, with one group ending exactly at k."""
    cuts = sorted({k} | {18 + 36 * m for m in range((k + 40) // 36 + 1)})
    return [b - a for a, b in zip([0] + cuts, cuts)]


@pytest.mark.parametrize("k", [33, 100, 500])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_multipass_k_with_ties_across_pass_boundaries(faiss, metric, storage, k):
    """k beyond one pass (float32 L2: k + 4 candidates): each pass admits only keys above the previous pass's
    last key.  Query 0 sees tie groups of identical rows across ranks 36/37, 72/73, ...; queries 1-3 are
    binary (dense natural ties)."""
    n, d = 50_000, 64
    rng = _rng("multipass", metric, storage, k)
    sizes = _pass_groups(k)
    xb = level_rows(rng, sizes, d, len(sizes) + 2, n)
    xq = int_data("binary", rng, 4, d)
    xq[0] = 0.0 if metric == L2 else -1.0
    D_ref, I_ref = _ref(xb, xq, k, metric)
    for b in range(36, k - 1, 36):  # the premise: query 0 has a tie across every pass boundary below k
        assert D_ref[0, b - 1] == D_ref[0, b], b
    index = _index(faiss, xb, metric, storage)
    before = _routes(index)
    D, I = index.search(xq, k)
    dt = _delta(index, before)
    kc = k + 4 if (metric == L2 and storage == "f32") else k
    # candidates of one pass (kc <= KPASS_MAX) are the short kernel's; more take the streaming passes
    assert dt["short_batches"] == (1 if kc <= 36 else 0) and dt["gemm_chunks"] == 0 and dt["direct_queries"] == 0
    if metric == L2 and storage == "f32":
        assert dt["reranked"] == 4
    assert_knn_identical(D, I, D_ref, I_ref, f"k={k}")


# ------------------------------------------------------------------------------------- GEMM paths
GEMM_CAPQ = 4096  # candidate slots per query of the GEMM-shaped pass (csrc/ise_knn.hip)


@pytest.mark.parametrize("kind", ["small", "overflow"])
@pytest.mark.parametrize("metric,storage,nq", [(L2, "f32", 256), (L2, "f32", 300), (IP, "f32", 256),
                                               (IP, "f32", 300), (L2, "bf16", 128), (IP, "bf16", 300)])
def test_gemm_path_tie_order(faiss, metric, storage, nq, kind):
    """Large batches against 140k x 128 rows: the GEMM-shaped pass.  0..15 data: sparse ties, the ordinary run.
    "overflow": binary values on 3 of the 128 columns, the 8 distinct rows repeated in turn, so every 128-row
    slab of the threshold sample holds 16 copies of each -- at least kc (14 at most here) -- and a query's
    admit threshold (the kc-th best sample score) is the score of its best distinct row: all 17 500 copies of
    that row are admitted, more than a query's candidate slots.  The buffers overflow, and the float32 L2 pass
    hands every query to the exact scan, the others re-run the batch through the streaming passes.  Identical to
    the oracle and to the same queries in batches the streaming passes take."""
    n, d, k = 140_000, 128, 10
    rng = _rng("gemm", metric, storage, nq, kind)
    if kind == "small":
        xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
        plant_ties(xb, 11, [12, n // 2, n - 1])
        xq[0] = xb[11]
    else:
        xb, xq = np.zeros((n, d), np.float32), np.zeros((nq, d), np.float32)
        pattern = np.arange(n) % 8
        xb[:, :3] = (pattern[:, None] >> np.arange(3)) & 1
        xq[:, :3] = int_data("binary", rng, nq, 3)
        # the premise: period 8 (16 copies of every distinct row in any 128 rows), each row > GEMM_CAPQ times
        assert np.array_equal(xb[:, :3] @ np.array([1, 2, 4], np.float32), pattern)
        assert np.bincount(pattern).min() > GEMM_CAPQ and k + 4 <= 16
    index = _index(faiss, xb, metric, storage)
    before = _routes(index)
    D, I = index.search(xq, k)
    dt = _delta(index, before)
    assert dt["gemm_chunks"] == 1
    if kind == "overflow" and metric == L2 and storage == "f32":
        assert dt["exact_scan"] == nq, "an overflowed candidate array must send its query to the exact scan"
    if not (metric == L2 and storage == "f32"):  # the flavours without a re-rank count the queries they lose
        assert dt["gemm_lost_queries"] >= 1 if kind == "overflow" else dt["gemm_lost_queries"] == 0, dt
    D_ref, I_ref = _ref(xb, xq, k, metric)
    assert_knn_identical(D, I, D_ref, I_ref, "GEMM path")
    step = 64 if storage == "bf16" else 128
    before = _routes(index)
    parts = [index.search(xq[i:i + step], k) for i in range(0, nq, step)]
    assert _delta(index, before)["gemm_chunks"] == 0, "these batches take the streaming passes"
    assert_knn_identical(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), D_ref, I_ref,
                         "streaming batches")


# ---------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("metric,storage", [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")])
def test_shard_keys_merge_with_ties_across_shards(faiss, metric, storage):
    """Three unequal shards (one smaller than k) searched with global ids (id_base) and merged: tie groups on
    both sides of every shard boundary; merged == unsharded == oracle."""
    import torch

    rng = _rng("shards", metric, storage)
    n, d, nq, k = 30_000, 16, 16, 20
    xb, xq = int_data("binary", rng, n, d), int_data("binary", rng, nq, d)
    plant_ties(xb, 5, [12, 13, 17_999, 18_000, 29_999])
    xq[0] = xb[5]
    bounds = [0, 13, 18_000, n]
    D_ref, I_ref = _ref(xb, xq, k, metric)
    whole = _index(faiss, xb, metric, storage)
    D0, I0 = whole.search(xq, k)
    assert whole.short_stats()["short_batches"] == 1
    assert_knn_identical(D0, I0, D_ref, I_ref, "unsharded")
    tq = torch.from_numpy(xq).cuda()
    keys = []
    for lo, hi in zip(bounds, bounds[1:]):
        sh = _index(faiss, xb[lo:hi], metric, storage)
        keys.append(sh.search_keys_torch(tq, k, id_base=lo))
        torch.cuda.synchronize()
        assert sh.short_stats()["short_batches"] == 1
    D1, I1 = faiss.merge_keys_torch(torch.stack(keys), metric)
    assert_knn_identical(D1.cpu().numpy(), I1.cpu().numpy(), D_ref, I_ref, "merged shards")


# ---------------------------------------------------------------------------------- assignment kernel
@pytest.mark.parametrize("kind", ["small", "binary"])
@pytest.mark.parametrize("metric", [IP, L2])
def test_assignment_kernel_tie_order(faiss, metric, kind):
    """k = 1 assignment kernel: integer centroids with copies at non-adjacent ids (7, 40, 100, 200 and 13, 90,
    250), rows on those centroids, and (binary) rows equidistant from several centroids.  D and I identical to
    the oracle, and to the general scan path.

    For L2 the kernel scores x.c - |c|^2 / 2 around the index's shift vector (the column mean, no integer):
    rounding then splits exact ties between DISTINCT centroids at the same distance (seen on 0..15 data: 6 rows
    of 4096), and D = |x|^2 - 2 score is not exact.  So the exact comparison runs with the shift pinned to zero,
    where the kernel's arithmetic is exact on these integers; with the default shift the copies of one
    centroid still resolve to the lowest id and every answer is a true near-tie (assert_knn_matches, with the
    expanded form's error at this magnitude)."""
    import torch

    rng = _rng("assign", metric, kind)
    K, d, n = 256, (64 if kind == "small" else 32), 4096
    cent, X = int_data(kind, rng, K, d), int_data(kind, rng, n, d)
    plant_ties(cent, 7, [40, 100, 200])
    plant_ties(cent, 13, [90, 250])
    X[:64], X[64:128] = cent[7], cent[13]
    index = _index(faiss, cent, metric)
    assert index._assign_applies(n, 1)
    if metric == L2:
        D_ref, I_ref = _ref(cent, X, 1, metric)
        D, I = index.search(X, 1)
        assert (I[:64] == 7).all() and (I[64:128] == 13).all()
        # (the expanded form around the shift: absolute error ~1e-3 at |x - mu|^2 ~ 4e3, also for D = 0)
        assert_knn_matches(D, I, D_ref, I_ref, cent, X, metric, rtol=2e-3)
        index.set_shift(np.zeros(d, np.float32))
    D_ref, I_ref = _ref(cent, X, 1, metric)
    if metric == L2:
        assert (I_ref[:64] == 7).all() and (I_ref[64:128] == 13).all()
    D, I = index.search(X, 1)
    assert_knn_identical(D, I, D_ref, I_ref, "assignment kernel")
    Dt, It = index.assign_torch(torch.from_numpy(X).cuda())
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D_ref, I_ref, "assign_torch")
    before = _routes(index)
    Ds, Is = index.search(X[:64], 1)  # below ASSIGN_MIN_NQ: the general scan path (short kernel)
    assert _delta(index, before)["short_batches"] == 1
    assert_knn_identical(Ds, Is, D_ref[:64], I_ref[:64], "scan path")


# --------------------------------------------------------------------------------- concurrent callers
@pytest.mark.parametrize("metric", [L2, IP])
def test_concurrent_one_query_callers_on_tie_data(faiss, metric):
    """8 host threads making one-query searches at once on binary rows (dense ties): calls are combined into
    shared batches, and every caller's result is identical to the oracle."""
    rng = _rng("threads", metric)
    n, d, k, nthreads, per = 100_000, 16, 10, 8, 24
    xb, xq = int_data("binary", rng, n, d), int_data("binary", rng, nthreads * per, d)
    plant_ties(xb, 1, [2, n // 2, n - 1])
    xq[::per] = xb[1]
    D_ref, I_ref = _ref(xb, xq, k, metric)
    index = _index(faiss, xb, metric)
    before = _routes(index)
    errors = []
    start = threading.Barrier(nthreads)

    def work(i):
        try:
            start.wait()
            for j in range(i * per, (i + 1) * per):
                D, I = index.search(xq[j:j + 1], k)
                assert_knn_identical(D, I, D_ref[j:j + 1], I_ref[j:j + 1], f"query {j}")
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(nthreads)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors[:3]
    dt = _delta(index, before)
    assert dt["combined_calls"] == nthreads * per
    assert dt["combined_batches"] < dt["combined_calls"], "no calls shared a batch"
