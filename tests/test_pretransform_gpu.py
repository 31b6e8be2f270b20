"""GPU tests of IndexPreTransform and the transform kinds over every sub-index kind: a transform chain
in front of an index answers exactly what the index answers for the transformed rows."""
import numpy as np
import pytest
import torch

from image_search_engine_amd import faiss_compat as faiss
from image_search_engine_amd.utils import create_search_index
from tests import transform_ref as ref

pytestmark = pytest.mark.gpu

N, D_IN, D, NQ, K = 2000, 64, 16, 5, 7
L2, IP = faiss.METRIC_L2, faiss.METRIC_INNER_PRODUCT
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.asarray(a).dtype)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(0)
    xb = (rng.standard_normal((N, D_IN)) * np.linspace(3, 0.3, D_IN)).astype(np.float32)
    xq = (rng.standard_normal((NQ, D_IN)) * np.linspace(3, 0.3, D_IN)).astype(np.float32)
    return xb, xq


def transform():
    rng = np.random.default_rng(1)
    lt = faiss.LinearTransform(D_IN, D, True)
    lt.A = rng.standard_normal((D, D_IN)) / 8
    lt.b = rng.standard_normal(D)
    return lt


def centroids(rng, metric):
    q = faiss.IndexFlat(D, metric)
    q.add((rng.standard_normal((8, D)) * 2).astype(np.float32))
    return q


def sq_trained():
    return np.concatenate((np.full(D, -9, dtype=np.float32), np.full(D, 18, dtype=np.float32)))


def sub_index(kind, metric):
    """A sub-index of dimension D with a given codec: nothing to train, so a twin made the same way is the same."""
    rng = np.random.default_rng(2)
    if kind == "flat":
        return faiss.IndexFlat(D, metric)
    if kind == "bf16":
        return faiss.IndexFlat(D, metric, storage="bf16")
    if kind in ("pq", "refine"):
        index = faiss.IndexPQ(D, 4, 8, metric)
        index.pq.set_centroids((rng.standard_normal((4, 256, 4)) * 2).astype(np.float32))
        if kind == "refine":
            index = faiss.IndexRefineFlat(index)
            index.k_factor = 4
        return index
    if kind == "sq":
        index = faiss.IndexScalarQuantizer(D, faiss.ScalarQuantizer.QT_8bit, metric)
        index.sq.set_trained(sq_trained())
        return index
    if kind == "ivfflat":
        index = faiss.IndexIVFFlat(centroids(rng, metric), D, 8, metric)
        index.nprobe = 3
        return index
    if kind == "ivfsq":
        index = faiss.IndexIVFScalarQuantizer(centroids(rng, metric), D, 8, faiss.ScalarQuantizer.QT_8bit, metric,
                                              by_residual=False)
        index.sq.set_trained(sq_trained())
        index.nprobe = 3
        return index
    assert kind == "idmap"
    return faiss.IndexIDMap(faiss.IndexFlat(D, metric))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", ["flat", "bf16", "pq", "sq", "ivfflat", "ivfsq", "refine", "idmap"])
def test_search_equals_the_twin_fed_transformed_rows(kind, metric, data):
    xb, xq = data
    lt = transform()
    pre, twin = faiss.IndexPreTransform(lt, sub_index(kind, metric)), sub_index(kind, metric)
    assert pre.is_trained and pre.d == D_IN and pre.metric_type == metric and pre.chain == [lt] and pre.ntotal == 0
    yb, yq = lt.apply(xb), lt.apply(xq)
    assert np.array_equal(bits(pre.apply_chain(xb)), bits(yb))
    if kind == "idmap":
        ids = np.arange(N, dtype=np.int64) * 3 + 11
        pre.add_with_ids(xb, ids)
        twin.add_with_ids(yb, ids)
    else:
        pre.add(xb[:700])
        pre.add_torch(torch.from_numpy(xb[700:]).cuda())
        twin.add(yb)
        assert pre.device == twin.device
    assert pre.ntotal == N
    D_want, I_want = twin.search(yq, K)
    D_got, I_got = pre.search(xq, K)
    assert np.array_equal(I_got, I_want) and np.array_equal(bits(D_got), bits(D_want))
    assert (I_got >= 0).all()
    if kind != "idmap":  # the id map has no device-resident form
        Dt, It = pre.search_torch(torch.from_numpy(xq).cuda(), K)
        assert np.array_equal(It.cpu().numpy(), I_want) and np.array_equal(bits(Dt.cpu().numpy()), bits(D_want))
    pre.reset()
    assert pre.ntotal == 0 and pre.is_trained


def test_a_stored_row_is_at_distance_zero():
    """4099 rows added in one ``add_torch`` through a PCA 64 -> 16, then 17 of them sent as queries, one per call and in
    one batch: a row's transform has the same bits either way, so the flat index finds it at distance exactly 0."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((4099, D_IN)) * np.linspace(4, 0.5, D_IN) + 3).astype(np.float32)
    pca = faiss.PCAMatrix(D_IN, D)
    pre = faiss.IndexPreTransform(pca, faiss.IndexFlatL2(D))
    assert not pre.is_trained
    pre.train(x)
    assert pre.is_trained
    x_dev = torch.from_numpy(x).cuda()
    pre.add_torch(x_dev)
    st = pca.linear_stats()
    assert st["tiled_launches"] >= 1
    rows = np.array([0, 1, 15, 16, 17, 63, 64, 65, 100, 1000, 2048, 3000, 4000, 4095, 4096, 4097, 4098])
    Db, Ib = pre.search_torch(x_dev[torch.from_numpy(rows).cuda()], 3)
    Db, Ib = Db.cpu().numpy(), Ib.cpu().numpy()
    assert np.array_equal(Ib[:, 0], rows) and (Db[:, 0] == 0.0).all() and (Db[:, 1] > 0).all()
    for r, i in enumerate(rows):
        D1, I1 = pre.search_torch(x_dev[i:i + 1], 3)
        assert int(I1[0, 0]) == i and float(D1[0, 0]) == 0.0
        assert np.array_equal(bits(D1.cpu().numpy()[0]), bits(Db[r])) and np.array_equal(I1.cpu().numpy()[0], Ib[r])
        D1, I1 = pre.search(x[i:i + 1], 3)
        assert I1[0, 0] == i and D1[0, 0] == 0.0
    assert pca.linear_stats()["few_row_launches"] >= 2 * len(rows)


def test_chains(data):
    xb, xq = data
    pca = faiss.PCAMatrix(D_IN, D)
    pre = faiss.IndexPreTransform(pca, faiss.IndexPQ(D, 4, 8))
    pre.index.cp.niter = 2
    with pytest.raises(RuntimeError, match="before train"):
        pre.add(xb)
    with pytest.raises(RuntimeError, match="before train"):
        pre.search(xq, K)
    with pytest.raises(RuntimeError, match="before train"):
        pre.apply_chain(torch.from_numpy(xq).cuda())
    assert not pca.is_trained and not pre.index.is_trained
    pre.train(xb)
    assert pca.is_trained and pre.index.is_trained and pre.is_trained
    pre.add(xb)
    assert (pre.search(xq, K)[1] >= 0).all()
    # PCA, then NormalizationTransform
    norm = faiss.IndexPreTransform(faiss.NormalizationTransform(D), faiss.IndexFlatIP(D))
    norm.prepend_transform(pca)
    want = pca.apply(xb)
    assert np.array_equal(bits(want), bits(pca.apply_torch(torch.from_numpy(xb).cuda()).cpu().numpy()))
    faiss.normalize_L2(want)
    assert np.array_equal(bits(norm.apply_chain(xb)), bits(want))
    assert np.array_equal(bits(norm.apply_chain(torch.from_numpy(xb).cuda()).cpu().numpy()), bits(want))
    assert (np.abs(np.linalg.norm(want.astype(np.float64), axis=1) - 1) < 1e-6).all()
    # CenteringTransform: x - mean, one rounding
    cnt = faiss.CenteringTransform(D_IN)
    cnt.train(xb)
    assert np.array_equal(bits(cnt.apply(xb)), bits(xb - cnt.mean[None, :]))
    assert np.array_equal(bits(cnt.apply_torch(torch.from_numpy(xq).cuda()).cpu().numpy()), bits(xq - cnt.mean[None, :]))
    # dimensions that do not meet
    with pytest.raises(AssertionError, match="mismatch"):
        faiss.IndexPreTransform(faiss.PCAMatrix(D_IN, D + 1), faiss.IndexFlatL2(D))
    with pytest.raises(AssertionError, match="mismatch"):
        norm.prepend_transform(faiss.PCAMatrix(D_IN, D))
    with pytest.raises(AssertionError, match="mismatch"):
        norm.search(xq[:, :5], K)
    with pytest.raises(AssertionError):
        pca.apply_torch(torch.zeros((2, D_IN + 1), device="cuda"))


def test_forwarding(data):
    xb, xq = data
    lt = transform()
    pre, twin = faiss.IndexPreTransform(lt, faiss.IndexFlatL2(D)), faiss.IndexFlatL2(D)
    pre.add(xb)
    twin.add(lt.apply(xb))
    yq = lt.apply(xq)
    radius = float(np.sort(twin.search(yq, 40)[0][:, -1])[2])
    for got, want in zip(pre.range_search(xq, radius), twin.range_search(yq, radius)):
        assert np.array_equal(got, want)
    sel = faiss.SearchParameters(sel=faiss.IDSelectorRange(100, 300))
    want = twin.search(yq, K, params=sel)
    for params in (sel, faiss.SearchParametersPreTransform(index_params=sel)):
        got = pre.search(xq, K, params=params)
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
        got = pre.search_torch(torch.from_numpy(xq).cuda(), K, params=params)
        assert np.array_equal(got[1].cpu().numpy(), want[1])
        for a, b in zip(pre.range_search(xq, radius, params=params), twin.range_search(yq, radius, params=sel)):
            assert np.array_equal(a, b)
    assert ((want[1] >= 100) & (want[1] < 300)).all()
    assert pre.remove_ids(faiss.IDSelectorRange(0, 50)) == twin.remove_ids(faiss.IDSelectorRange(0, 50)) == 50
    assert pre.ntotal == N - 50
    got, want = pre.search(xq, K), twin.search(yq, K)
    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
    coded = faiss.IndexPreTransform(transform(), sub_index("pq", L2))
    coded.add(xb[:300])
    with pytest.raises(NotImplementedError):
        coded.range_search(xq, 1.0)
    with pytest.raises(NotImplementedError):
        coded.remove_ids(faiss.IDSelectorRange(0, 5))
    with pytest.raises(NotImplementedError):
        coded.search(xq, K, params=sel)
    with pytest.raises(NotImplementedError):
        coded.search(xq, K, params=faiss.SearchParametersPreTransform(index_params=sel))


def test_reconstruct():
    rng = np.random.default_rng(4)
    # a permutation: integer rows survive it, and come back exactly
    perm = faiss.LinearTransform(D, D)
    perm.A = np.eye(D, dtype=np.float32)[rng.permutation(D)]
    perm.set_is_orthonormal()
    pre = faiss.IndexPreTransform(perm, faiss.IndexFlatL2(D))
    x = rng.integers(-50, 51, (300, D)).astype(np.float32)
    pre.add(x)
    assert np.array_equal(pre.reconstruct_n(0, 300), x) and np.array_equal(pre.reconstruct(17), x[17])
    assert np.array_equal(pre.reconstruct_n(290), x[290:])
    # a random rotation 64 -> 64.  A = Q + E, Q orthogonal, |E| <= u |Q|, so |E|_2 <= |E|_F <= u sqrt(d).  The kernel's y
    # = A x + dy with |dy_j| <= gamma_m sum_k |A_jk x_k|, so |dy|_2 <= gamma_m | |A| |_2 |x|_2 <= gamma_m sqrt(d) (1 + u)
    # |x|_2; reverse_transform is A^T y in float64, narrowed once (u |x^|).  x^ - x = (A^T A - I) x + A^T dy + narrowing:
    # |x^ - x|_2 <= [(2 u sqrt(d) + u^2 d) + gamma_m sqrt(d) (1 + u sqrt(d))^2 + 2 u] |x|_2, m = 256 + 1 + 1
    d = D_IN
    rot = faiss.RandomRotationMatrix(d, d)
    rot.init(9)
    pre = faiss.IndexPreTransform(rot, faiss.IndexFlatL2(d))
    x = rng.standard_normal((300, d)).astype(np.float32)
    pre.add(x)
    m = ref.LIN_KSEG + 1 + 1
    gamma = m * U / (1 - m * U)
    rel = (2 * U * np.sqrt(d) + U * U * d) + gamma * np.sqrt(d) * (1 + U * np.sqrt(d)) ** 2 + 2 * U
    err = np.linalg.norm(pre.reconstruct_n(0, 300).astype(np.float64) - x, axis=1)
    worst = float((err / (rel * np.linalg.norm(x.astype(np.float64), axis=1))).max())
    print(f"reconstruct through a random rotation: worst |x^ - x| / bound = {worst:.4f}")
    assert worst <= 1.0
    # whitening has no reverse
    white = faiss.PCAMatrix(d, D, eigen_power=-0.5)
    pre = faiss.IndexPreTransform(white, faiss.IndexFlatL2(D))
    pre.train(x)
    pre.add(x)
    with pytest.raises(RuntimeError, match="orthonormal"):
        pre.reconstruct(0)


@pytest.mark.parametrize("kind", ["flat", "pq", "sq", "ivfsq", "refine", "idmap"])
def test_write_and_read_index(kind, data, tmp_path):
    xb, xq = data
    pca = faiss.PCAMatrix(D_IN, D, 0, True)
    pca.train(xb)
    pre = faiss.IndexPreTransform(faiss.NormalizationTransform(D), sub_index(kind, L2))
    pre.prepend_transform(pca)
    if kind == "idmap":
        pre.add_with_ids(xb, np.arange(N) + 5)
    else:
        pre.add(xb)
    path = tmp_path / "pre.index"
    faiss.write_index(pre, path)
    back = faiss.read_index(path)
    assert type(back) is faiss.IndexPreTransform and type(back.index) is type(pre.index)
    assert [type(t) for t in back.chain] == [faiss.PCAMatrix, faiss.NormalizationTransform]
    assert (back.d, back.ntotal, back.metric_type, back.is_trained) == (D_IN, N, L2, True)
    want, got = pre.search(xq, K), back.search(xq, K)
    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
    with open(path, "rb") as f:
        d, metric, chain, fourcc, _ = faiss.parse_pretransform(f.read())
    assert (d, metric, len(chain)) == (D_IN, L2, 2) and np.array_equal(chain[0].A, pca.A)


def test_an_inverted_flat_sub_index_keeps_refusing(data, tmp_path):
    pre = faiss.IndexPreTransform(transform(), sub_index("ivfflat", L2))
    path = tmp_path / "pre.index"
    path.write_bytes(b"as it was")
    with pytest.raises(NotImplementedError):
        faiss.write_index(pre, path)
    assert path.read_bytes() == b"as it was"
    refine = faiss.IndexRefineFlat(faiss.IndexPreTransform(transform(), sub_index("pq", L2)))
    with pytest.raises(NotImplementedError):
        faiss.write_index(refine, path)
    assert path.read_bytes() == b"as it was"


@pytest.fixture(scope="module")
def uneven():
    """8192 rows of 32 entries: the first 8 coordinates have variance 100, the rest 0.01."""
    x = np.random.default_rng(5).standard_normal((8192, 32))
    x[:, :8] *= 10
    x[:, 8:] *= 0.1
    return x.astype(np.float32)


def test_opq_balances_the_sub_quantisers(uneven):
    """Plain IndexPQ(32, 4) spends one 256-word codebook on all eight heavy coordinates; a balancing rotation spends
    four.  The condition (not a measurement): the mean squared reconstruction error behind the trained OPQMatrix is at
    most half of plain PQ's."""
    x = uneven
    plain = faiss.IndexPQ(32, 4, 8)
    plain.train(x)
    mse_plain = float(((plain.sa_decode(plain.sa_encode(x)).astype(np.float64) - x) ** 2).sum(1).mean())
    opq = faiss.OPQMatrix(32, 4)
    opq.niter = 10
    pre = faiss.IndexPreTransform(opq, faiss.IndexPQ(32, 4, 8))
    pre.train(x)
    assert opq.is_trained and pre.index.is_trained and opq.is_orthonormal
    A = opq.A.astype(np.float64)
    assert np.abs(A @ A.T - np.eye(32)).max() <= 4 * U
    pre.add(x)
    mse_opq = float(((pre.reconstruct_n(0, x.shape[0]).astype(np.float64) - x) ** 2).sum(1).mean())
    print(f"IndexPQ(32, 4) mse {mse_plain:.3f}, behind OPQMatrix {mse_opq:.3f}: ratio {mse_plain / mse_opq:.2f}")
    assert mse_opq <= 0.5 * mse_plain


def test_refine_over_opq_pq_with_every_row_a_candidate(uneven):
    x = uneven[:300]
    opq = faiss.OPQMatrix(32, 4)
    opq.niter = 2
    index = faiss.IndexRefineFlat(faiss.IndexPreTransform(opq, faiss.IndexPQ(32, 4, 8)))
    index.base_index.index.cp.niter = 2
    index.train(x)
    assert index.is_trained
    index.add(x)
    flat = faiss.IndexFlatL2(32)
    flat.add(x)
    xq = uneven[5000:5005]
    want = flat.search(xq, K)
    params = faiss.IndexRefineSearchParameters(k_factor=300 / K + 1)
    for got in (index.search(xq, K, params=params),
                tuple(t.cpu().numpy() for t in index.search_torch(torch.from_numpy(xq).cuda(), K, params=params))):
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))


@pytest.mark.parametrize("index_type", ["pca256-l2", "opq-pq"])
def test_create_search_index(index_type, monkeypatch):
    rng = np.random.default_rng(6)
    d = 320 if index_type == "pca256-l2" else 32
    x = (rng.standard_normal((1500, d)) * np.linspace(2, 0.2, d)).astype(np.float32)
    monkeypatch.setattr(faiss.OPQMatrix, "niter", 2)  # Faiss's 50 rounds of 16 k-means each take longer than a test may
    index = create_search_index(x, index_type)
    assert type(index) is faiss.IndexPreTransform and index.ntotal == 1500 and index.d == d and index.is_trained
    if index_type == "pca256-l2":
        assert type(index.chain[0]) is faiss.PCAMatrix and index.chain[0].d_out == 256 and type(index.index) is faiss.IndexFlatL2
        D1, I1 = index.search(x[:9], 3)
        assert np.array_equal(I1[:, 0], np.arange(9)) and (D1[:, 0] == 0).all()
    else:
        assert type(index.chain[0]) is faiss.OPQMatrix and type(index.index) is faiss.IndexPQ and index.index.M == 16
        D1, I1 = index.search(x[:9], 3)
        assert (I1 >= 0).all() and (np.diff(D1, axis=1) >= 0).all()
