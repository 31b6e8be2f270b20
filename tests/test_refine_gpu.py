"""GPU tests of subset scoring on the flat index (include/ise_knn.h, ise_index_search_subset_* /
ise_index_distance_subset_*; csrc/ise_subset.hpp) and of IndexRefine / IndexRefineFlat on top of it.  On integer data
every comparison is bit for bit against tests/refine_ref.py; on real data against the selector-filtered search and the
unfiltered search of the same index, which the header promises the same bits as."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data, plant_ties, poison
from tests.refine_ref import refine_ref
from tests.sel_ref import IP, L2, pad_value

pytestmark = pytest.mark.gpu

INVALID = np.array([-1, -1, -7, -(1 << 40), 1 << 40], dtype=np.int64)  # with n and n + 5, added per table


def candidate_table(rng, n, nq, kc):
    """Random ids with duplicates, -1, ids >= n, negative ids and (nq > 1) one all-invalid row."""
    cand = rng.integers(0, n, (nq, kc)).astype(np.int64)
    bad = np.concatenate((INVALID, [n, n + 5]))
    hit = rng.random((nq, kc)) < 0.15
    cand[hit] = rng.choice(bad, int(hit.sum()))
    if kc > 1:
        cand[:, kc - 1] = cand[:, 0]  # a duplicate in every row, far apart in the table
    if nq > 1:
        cand[nq // 2] = rng.choice(bad, kc)
    return cand


def flat_index(xb, metric, storage="f32"):
    index = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    index.add(xb)
    return index


# (n, d, nq, kc, k): k > kc; kc not a multiple of 16; a row past the 256-float segment of exact_l2_rows; the largest
# sort; the reference's descriptor length
SHAPES = [(300, 20, 1, 1, 1), (300, 20, 17, 37, 10), (300, 20, 3, 5, 10), (3000, 260, 5, 100, 100),
          (2500, 512, 16, 2048, 32), (64, 2048, 1, 64, 20)]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("n,d,nq,kc,k", SHAPES)
def test_subset_exact(n, d, nq, kc, k, metric):
    rng = np.random.default_rng(n + d + kc)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    cand = candidate_table(rng, n, nq, kc)
    index = flat_index(xb, metric)
    D, I = index.search_subset(xq, k, cand)
    assert_knn_identical(D, I, *refine_ref(xb, xq, cand, k, metric), f"n={n} d={d} nq={nq} kc={kc} k={k}")
    # the scores on their own, in candidate order
    dist = index.compute_distance_subset(xq, cand)
    assert dist.dtype == np.float32 and dist.shape == cand.shape
    ok = (cand >= 0) & (cand < n)
    b, x = xb.astype(np.float64), xq.astype(np.float64)
    for q in range(nq):
        rows = b[cand[q][ok[q]]]
        want = ((rows - x[q]) ** 2).sum(1) if metric == L2 else (rows * x[q]).sum(1)
        assert np.array_equal(dist[q][ok[q]], want.astype(np.float32)), f"query {q}"
        assert (dist[q][~ok[q]] == pad_value(metric)).all()


def gaussian(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [100, 512])
@pytest.mark.parametrize("nq", [1, 16])
def test_subset_has_the_bits_of_search(d, nq, metric):
    n, k, kc = 2000, 10, 70
    xb, xq = gaussian(n, d, 3), gaussian(nq, d, 4)
    rng = np.random.default_rng(5)
    cand = rng.integers(0, n, (nq, kc)).astype(np.int64)
    cand[:, 7] = -1
    cand[:, kc - 1] = cand[:, 0]
    index = flat_index(xb, metric)
    D, I = index.search_subset(xq, k, cand)
    for q in range(nq):
        sel = faiss.IDSelectorBatch(cand[q][cand[q] >= 0])
        Ds, Is = index.search(xq[q:q + 1], k, params=faiss.SearchParameters(sel=sel))
        assert np.array_equal(I[q], Is[0]), f"query {q}"
        assert np.array_equal(D[q].view(np.uint32), Ds[0].view(np.uint32)), f"query {q}"
    Df, If = index.search(xq, n)  # every row, with the D the unfiltered search reports
    assert (If >= 0).all()
    by_id = np.empty((nq, n), dtype=np.float32)
    np.put_along_axis(by_id, If, Df, axis=1)
    dist = index.compute_distance_subset(xq, cand)
    ok = cand >= 0
    want = np.take_along_axis(by_id, np.where(ok, cand, 0), axis=1)
    assert np.array_equal(dist[ok].view(np.uint32), want[ok].view(np.uint32))
    assert (dist[~ok] == pad_value(metric)).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_ties_go_by_ascending_id(metric):
    rng = np.random.default_rng(8)
    n, d, nq, k = 400, 24, 3, 12
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    group = [399, 17, 16, 200, 3]
    plant_ties(xb, 150, group)
    xq[0] = xb[150]  # L2: the whole group at distance 0 of query 0
    cand = np.tile(np.arange(n - 1, n - 1 - 300, -1, dtype=np.int64), (nq, 1))  # descending ids 399 .. 100
    cand[:, :4] = [[3, 17, 16, 399]] * nq  # ... with the low members of the group in front, out of order
    index = flat_index(xb, metric)
    D, I = index.search_subset(xq, k, cand)
    assert_knn_identical(D, I, *refine_ref(xb, xq, cand, k, metric))
    for q in range(nq):
        pos = [int(np.flatnonzero(I[q] == g)[0]) for g in sorted(group + [150]) if g in I[q]]
        assert pos == sorted(pos) and (np.diff(pos) == 1).all(), f"query {q}: the tie group is not in id order"
    if metric == L2:
        assert I[0, :6].tolist() == [3, 16, 17, 150, 200, 399] and (D[0, :6] == 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_non_finite_rows_and_queries(metric):
    """Faiss's gate (tests/knn_checks.py): an L2 score enters only below FLT_MAX, an inner product only above -FLT_MAX,
    NaN never.  An inner product of +inf does enter, so the inner-product cases give the query the sign that makes the
    poisoned rows' scores -inf."""
    rng = np.random.default_rng(9)
    n, d, nq, k, kc = 300, 20, 4, 8, 40
    xb0, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d) + 1
    cand = rng.integers(0, n, (nq, kc)).astype(np.int64)
    bad_rows = cand[:, 3].copy()
    for kind in ("nan", "inf", "-inf", "all_nan"):
        xb = poison(xb0.copy(), bad_rows, kind)
        x = xq.copy()
        if metric == IP and kind == "inf":
            x[:, 0] = -x[:, 0]
        index = flat_index(xb, metric)
        D, I = index.search_subset(x, k, cand)
        assert not np.isin(I, bad_rows).any(), kind
        assert_knn_identical(D, I, *refine_ref(xb, x, cand, k, metric), kind)
        for q in range(nq):
            sel = faiss.IDSelectorBatch(cand[q])
            Ds, Is = index.search(x[q:q + 1], k, params=faiss.SearchParameters(sel=sel))
            assert_knn_identical(D[q:q + 1], I[q:q + 1], Ds, Is, f"{kind} query {q}")
        dist = index.compute_distance_subset(x, cand)
        assert not np.isfinite(dist[:, 3]).any() and np.isfinite(dist[~np.isin(cand, bad_rows)]).all(), kind
        # a NaN query: nothing enters
        x[1, 5] = np.nan
        D, I = index.search_subset(x, k, cand)
        assert (I[1] == -1).all() and (D[1] == pad_value(metric)).all() and (I[[0, 2, 3], 0] >= 0).all()
        assert np.isnan(index.compute_distance_subset(x, cand)[1]).all()


def test_errors_stats_and_the_empty_index():
    rng = np.random.default_rng(10)
    n, d, nq = 200, 16, 5
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    index = flat_index(xb, L2)
    good = rng.integers(0, n, (nq, 6)).astype(np.int64)
    for kc in (0, 2049):
        with pytest.raises(RuntimeError, match="kc"):
            index.search_subset(xq, 3, np.zeros((nq, kc), np.int64))
        with pytest.raises(RuntimeError, match="kc"):
            index.compute_distance_subset(xq, np.zeros((nq, kc), np.int64))
    for k in (0, -1, 2049):
        with pytest.raises((RuntimeError, ValueError)):
            index.search_subset(xq, k, good)
    half = flat_index(xb, L2, storage="bf16")
    with pytest.raises(RuntimeError, match="bf16"):
        half.search_subset(xq, 3, good)
    with pytest.raises(RuntimeError, match="bf16"):
        half.compute_distance_subset(xq, good)
    assert index.subset_stats() == {"subset_batches": 0, "score_launches": 0, "rows_scored": 0}  # refused calls count nothing
    cand = candidate_table(rng, n, nq, 37)
    valid = int(((cand >= 0) & (cand < n)).sum())
    index.search_subset(xq, 4, cand)
    assert index.subset_stats() == {"subset_batches": 1, "score_launches": 1, "rows_scored": valid}
    index.compute_distance_subset(xq, cand)
    assert index.subset_stats() == {"subset_batches": 2, "score_launches": 2, "rows_scored": 2 * valid}
    D, I = index.search_subset(xq[:0], 4, cand[:0])
    assert D.shape == (0, 4) and I.shape == (0, 4) and index.subset_stats()["subset_batches"] == 2
    for metric in (L2, IP):
        empty = faiss.IndexFlat(d, metric)
        D, I = empty.search_subset(xq, 4, cand)
        assert (I == -1).all() and (D == pad_value(metric)).all()
        assert (empty.compute_distance_subset(xq, cand) == pad_value(metric)).all()
        assert empty.subset_stats() == {"subset_batches": 2, "score_launches": 0, "rows_scored": 0}


@pytest.mark.parametrize("metric", [L2, IP])
def test_one_handle_from_two_streams(metric):
    """Subset scoring keeps ONE key workspace per handle: a call on another stream than the previous call's waits for
    it through an event, and a workspace that has to grow (here from 3 x 8 to 17 x 64 keys) is replaced behind a drain.
    Four calls on two streams with nothing waited for in between; every result has the bits of the host form."""
    import torch

    rng = np.random.default_rng(300)
    n, d = 300, 20
    xb = int_data("small", rng, n, d)
    index = flat_index(xb, metric)
    dev = torch.device("cuda", index.device)
    shapes = {"small": (3, 5, 5), "large": (17, 37, 10)}
    host, cuda = {}, {}
    for name, (nq, kc, _) in shapes.items():
        host[name] = (int_data("small", rng, nq, d), candidate_table(rng, n, nq, kc))
        assert_exact_range(xb, host[name][0])
        cuda[name] = tuple(torch.from_numpy(a).to(dev) for a in host[name])
    torch.cuda.synchronize(dev)  # the inputs are there: from here on no stream waits for another through torch
    side = torch.cuda.Stream(device=dev)
    first = index.search_subset_torch(cuda["small"][0], shapes["small"][2], cuda["small"][1])
    with torch.cuda.stream(side):
        grown = index.search_subset_torch(cuda["large"][0], shapes["large"][2], cuda["large"][1])
        dist = index.compute_distance_subset_torch(*cuda["large"])
    again = index.search_subset_torch(cuda["small"][0], shapes["small"][2], cuda["small"][1])
    torch.cuda.synchronize(dev)
    assert index.subset_stats()["subset_batches"] == 4
    want_small = index.search_subset(host["small"][0], shapes["small"][2], host["small"][1])
    want_large = index.search_subset(host["large"][0], shapes["large"][2], host["large"][1])
    for got, want, what in ((first, want_small, "default stream"), (grown, want_large, "side stream"),
                            (again, want_small, "default stream again")):
        assert_knn_identical(got[0].cpu().numpy(), got[1].cpu().numpy(), *want, what)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), index.compute_distance_subset(*host["large"]).view(np.uint32))


# ------------------------------------------------------------------ IndexRefineFlat
def refine_over_pq(n, metric, seed, nq=9):
    rng = np.random.default_rng(seed)
    M, dsub = 4, 4
    d = M * dsub
    C = int_data("small", rng, M * 256, dsub).reshape(M, 256, dsub)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    index = faiss.IndexRefineFlat(faiss.IndexPQ(d, M, 8, metric))
    assert not index.is_trained and index.ntotal == 0 and index.k_factor == 1.0
    assert (index.d, index.metric_type) == (d, metric) and isinstance(index.refine_index, faiss.IndexFlat)
    index.base_index.pq.set_centroids(C)
    assert index.is_trained
    index.add(xb[:n // 3])
    index.add(xb[n // 3:])
    assert index.ntotal == n and index.base_index.ntotal == n and index.refine_index.ntotal == n
    return index, xb, xq


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("n", [500, 3000])
def test_refine_over_pq(n, metric):
    index, xb, xq = refine_over_pq(n, metric, 20 + n)
    assert_exact_range(xb, xq)
    k = 10
    for k_factor in (1, 3.5, 50):
        index.k_factor = k_factor
        k_base = int(k * k_factor)
        labels = index.base_index.search(xq, k_base)[1]
        D, I = index.search(xq, k)
        assert_knn_identical(D, I, *refine_ref(xb, xq, labels, k, metric), f"k_factor={k_factor}")
        if k_factor == 1:  # the base's id set, in exact order
            assert np.array_equal(np.sort(I, axis=1), np.sort(labels, axis=1))
        if k_base >= n:  # every row is a candidate: the flat index's own answer
            assert_knn_identical(D, I, *index.refine_index.search(xq, k), "k * k_factor >= ntotal")
    assert (k * 50 >= n) == (n == 500)
    index.k_factor = 1
    Dp, Ip = index.search(xq, k, params=faiss.IndexRefineSearchParameters(k_factor=3.5))
    index.k_factor = 3.5
    assert_knn_identical(Dp, Ip, *index.search(xq, k), "params override the attribute")
    assert np.array_equal(index.reconstruct_n(3, 4), xb[3:7]) and np.array_equal(index.reconstruct(n - 1), xb[n - 1])
    index.k_factor = 21
    with pytest.raises(ValueError, match="2048"):
        index.search(xq, 100)
    with pytest.raises(ValueError, match="2048"):
        index.search(xq, 10, params=faiss.IndexRefineSearchParameters(k_factor=205))
    with pytest.raises(TypeError):
        index.search(xq, 10, params=faiss.SearchParameters())
    index.refine_index.add(xb[:1])  # the two sides out of step
    with pytest.raises(RuntimeError, match="rows"):
        index.search(xq, 10)
    index.reset()
    assert index.ntotal == 0 and index.base_index.ntotal == 0 and index.is_trained


@pytest.mark.parametrize("metric", [L2, IP])
def test_refine_over_ivf_ignores_the_padding(metric):
    rng = np.random.default_rng(30)
    n, d, nq, k = 300, 20, 6, 5
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    quantizer = faiss.IndexFlatL2(d)  # an L2 coarse quantiser for both metrics: lists of similar length
    quantizer.add(xb[:8])
    index = faiss.IndexRefineFlat(faiss.IndexIVFFlat(quantizer, d, 8, metric))
    assert index.is_trained
    index.train(xb)  # a no-op: the quantiser holds its centroids
    index.add(xb)
    index.base_index.nprobe = 1
    index.k_factor = 24
    labels = index.base_index.search(xq, k * 24)[1]
    assert (labels == -1).any(), "a probed list as long as k_base: the case is not exercised"
    assert_knn_identical(*index.search(xq, k), *refine_ref(xb, xq, labels, k, metric))


@pytest.mark.parametrize("metric", [L2, IP])
def test_refine_over_bf16_rows(metric):
    rng = np.random.default_rng(31)
    n, d, nq, k = 700, 40, 5, 10
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    index = faiss.IndexRefineFlat(faiss.IndexFlat(d, metric, storage="bf16"))
    index.add(xb)
    index.k_factor = 4
    D, I = index.search(xq, k)
    labels = index.base_index.search(xq, 4 * k)[1]
    assert_knn_identical(D, I, *refine_ref(xb, xq, labels, k, metric))
    flat = flat_index(xb, metric)
    by_id = flat.compute_distance_subset(xq, I)  # the float32 index's bits for the returned ids
    assert np.array_equal(D.view(np.uint32), by_id.view(np.uint32))


@pytest.mark.parametrize("metric", [L2, IP])
def test_torch_forms(metric):
    import torch

    index, xb, xq = refine_over_pq(500, metric, 40)
    index.k_factor = 6
    k = 10
    D, I = index.search(xq, k)
    dev = torch.device("cuda", index.device)
    xt = torch.from_numpy(xq).to(dev)
    Dt, It = index.search_torch(xt, k)
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D, I, "default stream")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        Ds, Is = index.search_torch(xt, k, params=faiss.IndexRefineSearchParameters(k_factor=6))
    side.synchronize()
    assert_knn_identical(Ds.cpu().numpy(), Is.cpu().numpy(), D, I, "side stream")
    cand = index.base_index.search_torch(xt, 60)[1]
    flat = index.refine_index
    dist = flat.compute_distance_subset_torch(xt, cand).cpu().numpy()
    assert np.array_equal(dist.view(np.uint32), flat.compute_distance_subset(xq, cand.cpu().numpy()).view(np.uint32))
    # add_torch builds the same index; a refused add leaves both sides alone
    twin = faiss.IndexRefineFlat(faiss.IndexPQ(index.d, 4, 8, metric))
    twin.base_index.pq.set_centroids(index.base_index.pq.centroids)
    twin.k_factor = 6
    twin.add_torch(torch.from_numpy(xb[:123]).to(dev))
    twin.add_torch(torch.from_numpy(xb[123:]).to(dev))
    assert twin.ntotal == 500 and np.array_equal(twin.base_index.codes, index.base_index.codes)
    assert_knn_identical(*twin.search(xq, k), D, I, "add_torch")
    bad = xb[:20].copy()
    bad[7, 3] = np.nan
    with pytest.raises(ValueError):
        index.add(bad)
    assert index.ntotal == 500 and index.base_index.ntotal == 500 and index.refine_index.ntotal == 500
    with pytest.raises(ValueError):
        twin.add_torch(torch.from_numpy(bad).to(dev))
    assert twin.base_index.ntotal == 500 and twin.refine_index.ntotal == 500


@pytest.mark.parametrize("metric", [L2, IP])
def test_write_and_read_index(metric, tmp_path):
    path = str(tmp_path / "refine.index")
    index, xb, xq = refine_over_pq(500, metric, 50)
    index.k_factor = 7.5
    flat_based = faiss.IndexRefineFlat(faiss.IndexFlat(index.d, metric))
    flat_based.add(xb)
    flat_based.k_factor = 2
    for src, base_type in ((index, faiss.IndexPQ), (flat_based, faiss.IndexFlat)):
        faiss.write_index(src, path)
        back = faiss.read_index(path)
        assert isinstance(back, faiss.IndexRefineFlat) and isinstance(back.base_index, base_type)
        assert back.k_factor == src.k_factor and back.ntotal == 500 and back.base_index.ntotal == 500
        assert (back.d, back.metric_type, back.is_trained) == (src.d, metric, True)
        for k in (1, 20):
            assert_knn_identical(*back.search(xq, k), *src.search(xq, k), f"k={k}")
    empty = faiss.IndexRefineFlat(faiss.IndexFlat(8, metric))
    faiss.write_index(empty, path)
    back = faiss.read_index(path)
    assert isinstance(back, faiss.IndexRefineFlat) and back.ntotal == 0 and back.k_factor == 1.0
    quantizer = faiss.IndexFlat(8, metric)
    for base in (faiss.IndexIVFFlat(quantizer, 8, 4, metric), faiss.IndexFlat(8, metric, storage="bf16")):
        with pytest.raises(NotImplementedError):
            faiss.write_index(faiss.IndexRefineFlat(base), path)


def test_wrappers_and_what_stays_unprovided():
    from image_search_engine_amd.utils import create_search_index

    x = gaussian(600, 32, 8)
    index = create_search_index(x, "pq-refine")
    assert isinstance(index, faiss.IndexRefineFlat) and isinstance(index.base_index, faiss.IndexPQ)
    assert index.is_trained and index.ntotal == 600 and index.k_factor == 16
    assert (index.base_index.M, index.metric_type) == (16, L2)
    D, I = index.search(x[:5], 20)  # the reference's k: 320 candidates
    assert (I[:, 0] == np.arange(5)).all() and (D[:, 0] == 0).all()
    with pytest.raises(NotImplementedError):
        faiss.IndexIDMap(faiss.IndexRefineFlat(faiss.IndexFlat(8)))
    with pytest.raises(NotImplementedError):
        index.range_search(x[:1], 1.0)
    with pytest.raises(NotImplementedError):
        index.remove_ids(np.arange(3))
    # IndexRefine with the caller's refine index: the pairing is checked
    with pytest.raises(AssertionError):
        faiss.IndexRefine(faiss.IndexFlat(8), faiss.IndexFlat(9))
    with pytest.raises(AssertionError):
        faiss.IndexRefine(faiss.IndexFlat(8), faiss.IndexFlat(8, IP))
    with pytest.raises(AssertionError):
        faiss.IndexRefine(faiss.IndexFlat(8), faiss.IndexFlat(8, storage="bf16"))
    full = faiss.IndexFlat(8)
    full.add(np.zeros((2, 8), np.float32))
    with pytest.raises(AssertionError):
        faiss.IndexRefine(full, faiss.IndexFlat(8))
    with pytest.raises(AssertionError):
        faiss.IndexRefine(faiss.IndexFlat(8), full)
    pair = faiss.IndexRefine(faiss.IndexFlat(8, storage="bf16"), faiss.IndexFlat(8))
    assert pair.refine_index.storage == "f32" and pair.k_factor == 1.0
