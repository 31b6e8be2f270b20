"""GPU tests of NaN, inf and overflowing rows and queries on every kNN path (tests/knn_checks.py).

Every kernel carries its own copy of Faiss's strict gate: an L2 score enters only below FLT_MAX, an inner product
only above -FLT_MAX (+inf enters).  The rows here are integers, so every finite score is exact in any order, and
every case is compared bit for bit with the oracle (``assert_knn_identical``) and asserts the route counter that
shows which path answered.  Poisoned rows are copies of the queries: a gate that leaks shows as a wrong id at
rank 0.  Each clean query has 14 planted rows at distinct L2 distances and every other row is far, so the
float32 L2 certificate holds on its own: a poisoned row must not send any query to the exact scan."""
import contextlib
import threading
import zlib

import numpy as np
import pytest

from oracle import flat_oracle as fo
from oracle import knn_oracle as ko
from tests.knn_checks import (HUGE, assert_knn_identical, assert_nonfinite_range, decoy_ids, int_data, plant_decoys,
                              poison)
from tests.test_exact_l2_gpu import force_direct, forced_exact, no_short
from tests.test_tie_order_gpu import _delta, _routes

pytestmark = pytest.mark.gpu

L2, IP = ko.METRIC_L2, ko.METRIC_INNER_PRODUCT
STORAGES = [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")]
KINDS = ["nan", "inf", "-inf", "all_nan"]
NEAR = 14  # planted rows per query (separated)


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def separated(rng, n, d, nq, extra=()):
    """Rows of 0..15 and queries of 20..35 (>= 1600 from every such row), plus for every query NEAR rows at ids off
    the decoy places: the query with its first m + 1 entries raised by 3 (L2 distance 9 (m + 1)).  The gaps of 9
    between them exceed the float32 L2 lower bound's slack at these norms, so the certificate holds.  Returns xb,
    xq and the decoy ids (decoy_ids(n, extra))."""
    xb, xq = int_data("small", rng, n, d), 20 + int_data("small", rng, nq, d)
    xb[:, 0] *= rng.choice([-1.0, 1.0], n).astype(np.float32)  # column 0: negative, zero and positive entries
    ids = decoy_ids(n, extra)
    free = np.setdiff1d(np.arange(n), ids)
    near = rng.choice(free, (nq, NEAR), replace=False)
    for q in range(nq):
        for m in range(NEAR):
            xb[near[q, m]] = xq[q]
            xb[near[q, m], : m + 1] += 3
    return xb, xq, ids


def _index(faiss, xb, metric, storage="f32"):
    index = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    index.add(xb)
    return index


def _ref(xb, xq, k, metric, storage="f32", id_offset=0):
    """The oracle on the stored values (bf16 storage: rows and queries rounded to nearest even by torch)."""
    import torch

    if storage == "bf16":
        xb = torch.from_numpy(xb).to(torch.bfloat16).to(torch.float32).numpy()
        xq = torch.from_numpy(xq).to(torch.bfloat16).to(torch.float32).numpy()
    assert_nonfinite_range(xb, xq, metric)
    return ko.knn_exact(xb, xq, k, metric, id_offset)


def _poison_queries(xq):
    """Query 1: a NaN coordinate; query 2: +inf at column 0 (for inner product that meets negative, zero and
    positive row entries: -inf, NaN and +inf scores)."""
    poison(xq, [1], "nan", col=5)
    poison(xq, [2], "inf", col=0)
    return xq


def _search(index, xq, k, expect, ctx=contextlib.nullcontext):
    with ctx():
        before = _routes(index)
        D, I = index.search(xq, k)
        dt = _delta(index, before)
    for key, want in expect.items():
        assert dt[key] == want, (key, dt)
    return D, I


# ------------------------------------------------------------ short kernel, streaming kernel, direct and exact scans
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1000, 100_000])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_poisoned_rows_and_queries_on_scan_paths(faiss, metric, storage, n, kind):
    """Poisoned copies of the queries at ids 0, n - 1 and on 16-row tile edges; a batch of 16 queries, two of them
    poisoned.  The short kernel, the streaming kernel (no_short), and for float32 L2 the one-query direct scan
    and the exact scan (forced_exact): all identical to the oracle and to each other; the clean queries also
    identical to a batch of clean queries alone."""
    d, nq, k = 64, 16, 10
    rng = _rng("scan", metric, storage, n, kind)
    xb, xq, ids = separated(rng, n, d, nq)
    plant_decoys(xb, xq, ids, kind, col=rng.integers(0, d))
    _poison_queries(xq)
    index = _index(faiss, xb, metric, storage)
    D_ref, I_ref = _ref(xb, xq, k, metric, storage)
    f32l2 = metric == L2 and storage == "f32"
    no_exact = {"exact_scan": 0} if f32l2 else {}
    D, I = _search(index, xq, k, {"short_batches": 1, "gemm_chunks": 0, **no_exact})
    assert_knn_identical(D, I, D_ref, I_ref, "short kernel")
    Ds, Is = _search(index, xq, k, {"short_batches": 0, "gemm_chunks": 0, **no_exact}, no_short)
    assert_knn_identical(Ds, Is, D_ref, I_ref, "streaming kernel")
    clean = [0] + list(range(3, nq))
    Dc, Ic = _search(index, xq[clean], k, {"short_batches": 1})
    assert_knn_identical(Dc, Ic, D_ref[clean], I_ref[clean], "clean queries alone")
    if metric == L2:
        assert (I[1:3] == -1).all()
    if f32l2:
        for j in (0, 1, 2):
            ctx = force_direct if n > 2048 else contextlib.nullcontext
            D1, I1 = _search(index, xq[j:j + 1], k, {"direct_queries": 1, "exact_scan": 0}, ctx)
            assert_knn_identical(D1, I1, D_ref[j:j + 1], I_ref[j:j + 1], f"direct scan q={j}")
        Df, If = _search(index, xq, k, {"exact_scan": nq, "short_batches": 1}, forced_exact)
        assert_knn_identical(Df, If, D_ref, I_ref, "exact scan")


@pytest.mark.parametrize("nq", [48, 65])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_poisoned_rows_on_streaming_batches(faiss, metric, storage, nq):
    """Batches of 48 (three query tiles sharing thresholds) and 65 queries (three passes) on the streaming kernel,
    every fourth query poisoned, against rows with every kind of poison."""
    n, d, k = 50_000, 64, 10
    rng = _rng("stream", metric, storage, nq)
    xb, xq, ids = separated(rng, n, d, nq, extra=[n // 4])
    for j, kind in enumerate(KINDS):
        plant_decoys(xb, xq, ids[j::4], kind, col=j)
    for j in range(1, nq, 4):
        poison(xq, [j], KINDS[(j // 4) % 4], col=j % d)
    index = _index(faiss, xb, metric, storage)
    D_ref, I_ref = _ref(xb, xq, k, metric, storage)
    no_exact = {"exact_scan": 0} if (metric == L2 and storage == "f32") else {}
    D, I = _search(index, xq, k, {"short_batches": 0, "gemm_chunks": 0, "direct_queries": 0, **no_exact}, no_short)
    assert_knn_identical(D, I, D_ref, I_ref, f"streaming nq={nq}")


@pytest.mark.parametrize("k", [33, 100])
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_poisoned_rows_on_multipass_k(faiss, metric, storage, k):
    """k beyond one pass (float32 L2: k + 4 candidates > 36): poisoned rows at the decoy ids and two poisoned
    queries; each pass admits only keys above the previous pass's last."""
    n, d, nq = 50_000, 64, 8
    rng = _rng("multipass", metric, storage, k)
    xb, xq, ids = separated(rng, n, d, nq)
    for j, kind in enumerate(KINDS):
        plant_decoys(xb, xq, ids[j::4], kind, col=3)
    _poison_queries(xq)
    index = _index(faiss, xb, metric, storage)
    kc = k + 4 if (metric == L2 and storage == "f32") else k
    D, I = _search(index, xq, k, {"short_batches": 1 if kc <= 36 else 0, "gemm_chunks": 0})
    D_ref, I_ref = _ref(xb, xq, k, metric, storage)
    assert_knn_identical(D, I, D_ref, I_ref, f"k={k}")


# ------------------------------------------------------------------------------------------------ GEMM paths
@pytest.mark.parametrize("metric,storage,nq", [(L2, "f32", 256), (L2, "f32", 300), (IP, "f32", 256),
                                               (IP, "f32", 300), (L2, "bf16", 128), (IP, "bf16", 300)])
def test_poisoned_rows_and_queries_on_gemm_path(faiss, metric, storage, nq):
    """Large batches against 140k x 128 rows: the GEMM-shaped pass, with poisoned copies of the queries on tile
    edges and two poisoned queries.  Identical to the oracle and to the same queries in batches the streaming
    passes take; float32 L2 without one exact scan."""
    n, d, k = 140_000, 128, 10
    rng = _rng("gemm", metric, storage, nq)
    xb, xq, ids = separated(rng, n, d, nq, extra=[n // 3])
    for j, kind in enumerate(KINDS):
        plant_decoys(xb, xq, ids[j::4], kind, col=j)
    _poison_queries(xq)
    index = _index(faiss, xb, metric, storage)
    # (the GEMM pass's certificate also covers the rows its threshold cut: a query with no candidate at all --
    # the two poisoned ones -- cannot prove it and takes the exact scan; no clean query may)
    no_exact = {"exact_scan": 2} if (metric == L2 and storage == "f32") else {}
    # (the flavours without a re-rank count the queries whose candidates the pass left incomplete.  Inner product: the
    # +inf query scores +inf on every row with a positive first entry, about 65 000 rows tied at the top, more than a
    # query's candidate slots whatever the threshold: that one query is lost and the streaming passes rewrite the chunk)
    if not (metric == L2 and storage == "f32"):
        no_exact = {"gemm_lost_queries": 1 if metric == IP else 0}
    D, I = _search(index, xq, k, {"gemm_chunks": 1, **no_exact})
    D_ref, I_ref = _ref(xb, xq, k, metric, storage)
    assert_knn_identical(D, I, D_ref, I_ref, "GEMM path")
    step = 64 if storage == "bf16" else 128
    before = _routes(index)
    parts = [index.search(xq[i:i + step], k) for i in range(0, nq, step)]
    assert _delta(index, before)["gemm_chunks"] == 0
    assert_knn_identical(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), D_ref, I_ref,
                         "streaming batches")


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_bf16_rows_above_bf16_max(faiss, kind):
    """bf16 storage rounds rows to nearest even: finite values above the bf16 maximum become +-inf (query copies
    with one such entry), NaN stays NaN.  Inner product only: finite overflow on bf16 L2 is approximate by
    design.  Short kernel and GEMM pass against the oracle on the torch-rounded rows."""
    import torch

    big = np.float32(3.4e38)  # finite in float32, above bf16's largest finite value
    assert torch.isinf(torch.tensor([big]).to(torch.bfloat16)).all()
    for n, nq, route in ((1000, 16, "short_batches"), (140_000, 300, "gemm_chunks")):
        rng = _rng("bf16max", kind, n)
        xb, xq, ids = separated(rng, n, 128, nq)
        xb[ids] = xq[np.arange(len(ids)) % nq]
        xb[ids[::2], 0] = big if kind == "inf" else np.nan
        xb[ids[1::2], 1] = -big
        index = _index(faiss, xb, IP, "bf16")
        D, I = _search(index, xq, 10, {route: 1, "gemm_lost_queries": 0})
        D_ref, I_ref = _ref(xb, xq, 10, IP, "bf16")
        assert np.isin(I_ref[:, 0], ids[::2]).all() if kind == "inf" else not np.isin(I_ref, ids).any()
        assert_knn_identical(D, I, D_ref, I_ref, f"bf16 rows above the bf16 maximum n={n}")


# ------------------------------------------------------------------------------- overflowing float32 L2 norms
def test_overflowing_norms_on_every_float32_l2_path(faiss):
    """Row 100 holds HUGE (2^64) in 8 columns and row n - 1 -HUGE there: their |y - mu|^2 overflow float32.  Query
    0 is row 100 plus 1 in column 3: its |x - mu|^2 overflows too, its answer is row 100 at distance 1, and every
    other row is >= 2^131 away.  Its lower bounds are all lost, so it must go to the exact scan (and only it); the
    other queries must not lose a row and must not be sent there.  Short kernel, streaming kernel, one-query
    direct scan and GEMM pass."""
    for n, nq, route, ctx in ((1000, 16, "short_batches", contextlib.nullcontext), (100_000, 16, "short_batches",
                              contextlib.nullcontext), (100_000, 16, "short_batches", no_short),
                              (140_000, 256, "gemm_chunks", contextlib.nullcontext)):
        d = 128 if route == "gemm_chunks" else 64
        rng = _rng("overflow", n, nq, route, ctx.__name__)
        xb, xq, _ = separated(rng, n, d, nq)
        xb[100, 8:16] = HUGE
        xb[n - 1, 8:16] = -HUGE
        xq[0] = xb[100]
        xq[0, 3] += 1
        index = _index(faiss, xb, L2)
        mu = index.get_shift()
        with np.errstate(over="ignore"):
            norm = lambda v: np.float32(((v - mu) ** 2).sum(dtype=np.float32))  # noqa: E731
            assert np.isinf(norm(xb[100])) and np.isinf(norm(xb[n - 1])) and np.isinf(norm(xq[0]))
            assert all(np.isfinite(norm(x)) for x in xq[1:]), "the premise: only query 0 overflows"
        D_ref, I_ref = _ref(xb, xq, 10, L2)
        assert I_ref[0, 0] == 100 and D_ref[0, 0] == 1.0 and (I_ref[0, 1:] == -1).all()
        want = {"exact_scan": 1, "short_batches": 0 if ctx is no_short else int(route == "short_batches")}
        if route == "gemm_chunks":
            want["gemm_chunks"] = 1
        D, I = _search(index, xq, 10, want, ctx)
        assert_knn_identical(D, I, D_ref, I_ref, f"n={n} {route} {ctx.__name__}")
        if route == "short_batches" and n > 2048:
            D1, I1 = _search(index, xq[:1], 10, {"direct_queries": 1}, force_direct)
            assert_knn_identical(D1, I1, D_ref[:1], I_ref[:1], "direct scan")


# -------------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("metric,storage", STORAGES)
def test_poisoned_rows_across_shards(faiss, metric, storage):
    """Three unequal shards searched with global ids and merged, poisoned rows on both sides of every shard
    boundary and two poisoned queries: merged == unsharded == oracle."""
    import torch

    n, d, nq, k = 30_000, 64, 16, 20
    bounds = [0, 13, 18_000, n]
    rng = _rng("shards", metric, storage)
    xb, xq, ids = separated(rng, n, d, nq, extra=bounds[1:-1])
    for j, kind in enumerate(KINDS):
        plant_decoys(xb, xq, ids[j::4], kind, col=j)
    _poison_queries(xq)
    D_ref, I_ref = _ref(xb, xq, k, metric, storage)
    D0, I0 = _search(_index(faiss, xb, metric, storage), xq, k, {"short_batches": 1})
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


# --------------------------------------------------------------------------------------------- assignment kernel
@pytest.mark.parametrize("metric", [IP, L2])
def test_assignment_kernel_with_poisoned_centroids_and_rows(faiss, metric):
    """k = 1 assignment: a NaN centroid and an inf-entry centroid that are copies of input rows 0 and 1, an
    all-NaN centroid, and input rows with a NaN and an inf entry.  L2 with the shift pinned to zero (the default
    shift rounds exact ties, tests/test_tie_order_gpu.py).  Identical to the oracle and to the scan path."""
    import torch

    rng = _rng("assign", metric)
    K, d, n = 256, 32, 4096
    cent, X = int_data("small", rng, K, d), int_data("small", rng, n, d)
    cent[:, 0] *= rng.choice([-1.0, 1.0], K).astype(np.float32)
    X[:, 0] = rng.choice([-1.0, 0.0, 1.0], n)
    cent[[7, 8, 200]] = X[[0, 1, 2]]
    poison(cent, [7], "nan", col=4)
    poison(cent, [8, 9], "inf", col=0)
    poison(cent, [200], "all_nan")
    poison(X, [3, 64], "nan", col=2)
    poison(X, [4, 65], "inf", col=0)
    index = _index(faiss, cent, metric)
    assert index._assign_applies(n, 1)
    if metric == L2:
        index.set_shift(np.zeros(d, np.float32))
    D_ref, I_ref = _ref(cent, X, 1, metric)
    D, I = index.search(X, 1)
    assert_knn_identical(D, I, D_ref, I_ref, "assignment kernel")
    Dt, It = index.assign_torch(torch.from_numpy(X).cuda())
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D_ref, I_ref, "assign_torch")
    Ds, Is = _search(index, X[:64], 1, {"short_batches": 1})  # below ASSIGN_MIN_NQ: the scan path
    assert_knn_identical(Ds, Is, D_ref[:64], I_ref[:64], "scan path")


# -------------------------------------------------------------------------------------------- concurrent callers
@pytest.mark.parametrize("metric", [L2, IP])
def test_concurrent_one_query_callers_with_one_nan_caller(faiss, metric):
    """8 host threads making one-query searches at once, combined into shared batches; one caller's queries are
    NaN, and no other caller's result may change."""
    n, d, k, nthreads, per = 100_000, 64, 10, 8, 12
    rng = _rng("threads", metric)
    xb, xq, ids = separated(rng, n, d, nthreads * per)
    plant_decoys(xb, xq, ids, "nan", col=1)
    poison(xq, np.arange(3 * per, 4 * per), "nan", col=7)
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
    if metric == L2:
        assert dt["exact_scan"] == 0


# --------------------------------------------------------------------------------------------- normalize_L2
def _edge_rows(d):
    return np.stack([np.zeros(d), np.full(d, 1e-30), np.full(d, 1e20), np.r_[np.nan, np.arange(1, d)],
                     np.r_[np.inf, np.arange(1, d)], np.r_[np.arange(1, d), -np.inf]]).astype(np.float32)


@pytest.mark.parametrize("d", [8, 512, 2048, 3, 2049, 4100])
def test_normalize_L2_edge_rows(faiss, d):
    """The vector path (d % 4 == 0, d <= 2048) and the scalar one (d = 3, 2049, 4100; and a tensor whose data
    pointer is 4 bytes off 16-byte alignment): zero, tiny (float32 |x|^2 = 0), huge (|x|^2 overflows), NaN-entry
    and inf-entry rows bit for bit with fvec_renorm_L2's C restatement; ordinary rows within 2e-6."""
    import torch

    rng = _rng("normalize", d)
    x = np.concatenate([_edge_rows(d), rng.standard_normal((37, d)).astype(np.float32)])
    e = len(_edge_rows(d))
    want = x.copy()
    fo.renorm_L2(want)
    host = x.copy()
    faiss.normalize_L2(host)
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(x.shape)  # a contiguous view at a storage offset of one float
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    t.copy_(torch.from_numpy(x))
    faiss.normalize_L2(t)
    torch.cuda.synchronize()
    dev = t.cpu().numpy()
    for got, what in ((host, "host"), (dev, "unaligned tensor")):
        # NaN positions equal, every other entry's bits (a NaN made by inf * 0 has no portable sign bit)
        nan = np.isnan(want[:e])
        assert np.array_equal(np.isnan(got[:e]), nan), what
        assert np.array_equal(got[:e][~nan].view(np.uint32), want[:e][~nan].view(np.uint32)), (what, got[:e, :3])
        np.testing.assert_allclose(got[e:], want[e:], rtol=2e-6, atol=1e-7, err_msg=what)
    assert np.array_equal(want[1].view(np.uint32), x[1].view(np.uint32)) and (want[2] == 0).all()
