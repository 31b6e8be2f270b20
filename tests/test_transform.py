"""CPU tests of the vector transforms (faiss_compat.VectorTransform and its kinds, IndexPreTransform's file format):
the exact-fmaf emulation of tests/transform_ref.py, PCA training against numpy, the "IxPT" file functions, the public
surface and the stand-alone packing check.  Nothing here touches a GPU: ``train``, ``A``, ``b`` and the file functions
need none.

    python -m tests.test_transform > tests/golden/faiss_compat_surface_transform.json     writes the surface fixture
"""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import transform_ref as ref
from tests.test_compat_surface import _KEPT_DUNDERS, _problems, describe_surface

U = 2.0 ** -24  # the unit roundoff of float32
F64_SLACK = 1e-10  # relative room for two float64 routes to the same quantity (summation order, LAPACK): far below U

_TRANSFORM = ("VectorTransform", "LinearTransform", "RandomRotationMatrix", "PCAMatrix", "OPQMatrix",
              "NormalizationTransform", "CenteringTransform", "IndexPreTransform", "SearchParametersPreTransform",
              "serialize_pretransform", "parse_pretransform")


# ---------------------------------------------------------------- the fmaf emulation
def f32(v):
    return np.float32(v)


# (a, b, c, fma(a, b, c)): a float64 multiply-add narrowed to float32 rounds twice and misses each of these
DOUBLE_ROUNDING = [
    # a b = 2^-24 + 2^-60 (2^36 + 1 = (2^12 + 1)(2^24 - 2^12 + 1)): just above the tie between 1 and 1 + 2^-23; float64
    # drops the 2^-60, lands on the tie and goes to even, 1
    (f32(2 ** 12 + 1), f32((2 ** 24 - 2 ** 12 + 1) * 2.0 ** -60), f32(1), f32(1 + 2.0 ** -23)),
    # a b = 2^-24 - 2^-60 (2^36 - 1 = (2^18 - 1)(2^18 + 1)): just below the tie between 1 + 2^-23 and 1 + 2^-22
    (f32(2 ** 18 - 1), f32((2 ** 18 + 1) * 2.0 ** -60), f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23)),
    # a b = 2^36 - 2^-10 under c = 2^60 (1 + 2^-23): just below the tie, float64 rounds onto it
    (f32(2 ** 18 + 2.0 ** -5), f32(2 ** 18 - 2.0 ** -5), f32(2.0 ** 60 * (1 + 2.0 ** -23)), f32(2.0 ** 60 * (1 + 2.0 ** -23))),
]


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("case", range(len(DOUBLE_ROUNDING)))
def test_fmaf_on_double_rounding_cases(case, sign):
    a, b, c, want = DOUBLE_ROUNDING[case]
    a, c, want = f32(sign * a), f32(sign * c), f32(sign * want)
    for v in (a, b, c):
        assert float(f32(v)) == float(v)  # the operands are float32 numbers as written
    twice = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert twice != want, "not a double-rounding case"
    assert ref.fmaf_rational(a, b, c) == want
    assert ref.fmaf(a, b, c) == want


def test_fmaf_against_rational_arithmetic():
    rng = np.random.default_rng(0)
    for scale in (0, 0, 30, -30, -60):  # the last: results in the subnormal range
        a, b, c = (rng.standard_normal((3, 400)) * 2.0 ** scale).astype(np.float32)
        if scale == -60:
            c = (c * 2.0 ** -70).astype(np.float32)
        got = ref.fmaf(a, b, c)
        for i in range(a.size):
            assert got[i] == ref.fmaf_rational(a[i], b[i], c[i]), (a[i], b[i], c[i])
    # cancellation: a b + c with c = -round(a b) is the product's own rounding error, exactly
    a, b = rng.standard_normal((2, 400)).astype(np.float32)
    c = -(a * b)
    err = ref.fmaf(a, b, c)
    assert np.array_equal(err.astype(np.float64), a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))
    # IEEE specials
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    assert ref.fmaf(inf, f32(2), f32(1)) == inf and np.isnan(ref.fmaf(inf, f32(0), f32(1)))
    assert np.isnan(ref.fmaf(inf, f32(1), -inf)) and np.isnan(ref.fmaf(nan, f32(1), f32(1)))
    assert ref.fmaf(f32(3e38), f32(3e38), f32(0)) == inf
    z = ref.fmaf(f32(0), f32(-1), f32(0))
    assert z == 0 and not np.signbit(z)  # a chain from +0 never holds -0: zero padding is exact


def test_linear_apply_is_the_segmented_chain():
    """Integer data: the contract's value is the integer product.  And a case where the segment cut shows."""
    rng = np.random.default_rng(1)
    A = rng.integers(-3, 4, (5, 600)).astype(np.float32)
    x = rng.integers(-8, 9, (4, 600)).astype(np.float32)
    b = rng.integers(-9, 10, 5).astype(np.float32)
    assert np.array_equal(ref.linear_apply(A, b, x), (x.astype(np.float64) @ A.T.astype(np.float64) + b).astype(np.float32))
    # k = 0: 2^24, k = 256: 1, k = 257: 1.  One chain would lose both ones (2^24 + 1 -> 2^24 twice); the contract adds
    # the second segment's 2 in one step
    A = np.zeros((1, 258), dtype=np.float32)
    A[0, [0, 256, 257]] = [2.0 ** 24, 1, 1]
    assert ref.linear_apply(A, None, np.ones((1, 258), dtype=np.float32))[0, 0] == np.float32(2.0 ** 24 + 2)


# ---------------------------------------------------------------- linear transforms on the host
def test_linear_transform_host_side():
    lt = faiss.LinearTransform(6, 4)
    assert not lt.is_trained and not lt.have_bias
    with pytest.raises(RuntimeError, match="before train"):
        lt.apply(np.zeros((1, 6), dtype=np.float32))
    with pytest.raises(AssertionError):
        lt.A = np.zeros((6, 4), dtype=np.float32)
    perm = np.eye(6, dtype=np.float32)[[4, 0, 5, 2]]
    lt.A = perm
    assert lt.is_trained and not lt.is_orthonormal
    with pytest.raises(RuntimeError, match="orthonormal"):
        lt.reverse_transform(np.zeros((1, 4), dtype=np.float32))
    lt.set_is_orthonormal()
    assert lt.is_orthonormal
    lt.b = np.arange(4)
    assert lt.have_bias
    y = np.arange(8, dtype=np.float32).reshape(2, 4)
    assert np.array_equal(lt.reverse_transform(y), (y - lt.b) @ perm)
    lt.A = 1.0001 * perm
    lt.set_is_orthonormal()
    assert not lt.is_orthonormal
    assert lt.linear_stats() == {"calls": 0, "few_row_launches": 0, "tiled_launches": 0}
    for d_in, d_out in ((64, 64), (64, 16), (16, 64), (2048, 256)):
        r = faiss.RandomRotationMatrix(d_in, d_out)
        r.init(7)
        A = r.A.astype(np.float64)
        gram = A @ A.T if d_out <= d_in else A.T @ A
        assert np.abs(gram - np.eye(min(d_in, d_out))).max() <= 4 * U  # 2 u + u^2 from float32 storage, and as much again
        assert r.is_orthonormal == (d_out <= d_in) and r.is_trained
    with pytest.raises(NotImplementedError):
        faiss.NormalizationTransform(8, 1.0)
    c = faiss.CenteringTransform(3)
    assert not c.is_trained
    c.train(np.array([[1, 2, 3], [3, 4, 5]], dtype=np.float32))
    assert c.is_trained and np.array_equal(c.mean, [2, 3, 4])
    assert np.array_equal(c.reverse_transform(np.zeros((1, 3), dtype=np.float32)), [[2, 3, 4]])
    with pytest.raises(AssertionError):
        faiss.IndexPreTransform(faiss.NormalizationTransform(5), _Sub(4))
    pre = faiss.IndexPreTransform(_Sub(4))
    pre.prepend_transform(faiss.RandomRotationMatrix(9, 4))
    pre.prepend_transform(faiss.NormalizationTransform(9))
    assert pre.d == 9 and [type(t).__name__ for t in pre.chain] == ["NormalizationTransform", "RandomRotationMatrix"]
    assert not pre.is_trained


class _Sub:
    """What IndexPreTransform asks of a sub-index before anything runs."""
    metric_type, ntotal, is_trained, device = faiss.METRIC_L2, 0, True, 0

    def __init__(self, d):
        self.d = d

    def add(self, x):
        raise AssertionError

    search = add


# ---------------------------------------------------------------- PCA
D_IN, D_OUT, N = 24, 8, 4000
PLANTED = np.array([20, 18, 16, 14, 12, 11, 10, 9, 4.5, 4, 3.5, 3, 2.5, 2, 1.8, 1.6, 1.4, 1.2, 1, .8, .6, .4, .2, .1])


@pytest.fixture(scope="module")
def planted():
    """Rows with a planted spectrum (a 2x eigenvalue gap behind D_OUT, so the leading subspace is well conditioned) and
    numpy's float64 answer: the mean, the covariance / n, its eigenvalues descending and eigenvectors as rows."""
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.standard_normal((D_IN, D_IN)))
    x = ((rng.standard_normal((N, D_IN)) * np.sqrt(PLANTED)) @ q.T + rng.standard_normal(D_IN) * 5).astype(np.float32)
    x64 = x.astype(np.float64)
    cov = np.cov(x64.T, bias=True)
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1], vec[:, ::-1].T
    assert lam[D_OUT - 1] / lam[D_OUT] > 1.7, "the planted gap did not survive sampling"
    return x, x64, cov, lam, vec


def test_pca_against_numpy(planted):
    x, x64, cov, lam, vec = planted
    pca = faiss.PCAMatrix(D_IN, D_OUT)
    assert not pca.is_trained
    pca.train(x)
    assert pca.is_trained and pca.is_orthonormal and pca.have_bias
    assert pca.A.dtype == np.float32 and pca.A.shape == (D_OUT, D_IN) and pca.b.shape == (D_OUT,)
    assert pca.PCAMat.shape == (D_IN, D_IN) and pca.mean.shape == (D_IN,)
    # a float32 copy of a float64 eigenvalue: relative u
    assert (np.abs(pca.eigenvalues.astype(np.float64) - lam) <= U * lam + F64_SLACK * lam[0]).all()
    assert (np.abs(pca.mean.astype(np.float64) - x64.mean(0)) <= U * np.abs(x64.mean(0)) + F64_SLACK).all()
    # A = V + E with |E| <= u |V| entrywise, V's rows orthonormal: (A A^T - I)_ij = sum_k (V E^T + E V^T + E E^T)_ij is at
    # most (2 u + u^2) sum_k |V_ik V_jk| <= 2 u + u^2 (Cauchy-Schwarz)
    A = pca.A.astype(np.float64)
    assert np.abs(A @ A.T - np.eye(D_OUT)).max() <= (2 * U + U * U) * (1 + F64_SLACK)
    # the projector, for the same reason: (A^T A - V^T V)_ik <= (2 u + u^2) sum_j |V_ji V_jk| <= 2 u + u^2; the float64
    # subspaces themselves agree to eps64 |C| / gap, far below
    proj = vec[:D_OUT].T @ vec[:D_OUT]
    assert np.abs(A.T @ A - proj).max() <= (2 * U + U * U) + F64_SLACK
    # b = -A mean, one rounding of the float64 product
    b64 = -(A @ x64.mean(0))
    assert (np.abs(pca.b - b64) <= U * np.abs(b64) + 4 * U * np.abs(A) @ np.abs(x64.mean(0))).all()


def test_pca_whitening(planted):
    x, x64, cov, lam, vec = planted
    pca = faiss.PCAMatrix(D_IN, D_OUT, eigen_power=-0.5)
    pca.train(x)
    assert not pca.is_orthonormal
    with pytest.raises(RuntimeError, match="orthonormal"):
        pca.reverse_transform(np.zeros((1, D_OUT), dtype=np.float32))
    A = pca.A.astype(np.float64)
    y = x64 @ A.T + pca.b.astype(np.float64)
    got = np.cov(y.T, bias=True)
    # A = W + E, W = L^-1/2 V (W C W^T = I exactly) and |E| <= u |W|: (A C A^T - I)_ij = (E C W^T + W C E^T)_ij + O(u^2), and
    # (C W^T)_kj = sqrt(l_j) V_jk, W_ik = V_ik / sqrt(l_i), so |(E C W^T)_ij| <= u sqrt(l_j / l_i) sum_k |V_ik V_jk| <= u
    # sqrt(l_j / l_i); b only shifts y.  The mean of y is -A mean + b: zero up to b's rounding.
    r = np.sqrt(lam[:D_OUT][None, :] / lam[:D_OUT][:, None])
    assert (np.abs(got - np.eye(D_OUT)) <= U * (r + r.T) * (1 + 2.0 ** -10) + F64_SLACK).all()
    assert np.abs(y.mean(0)).max() <= 4 * U * (np.abs(A) @ np.abs(x64.mean(0))).max()


def test_pca_random_rotation_keeps_the_subspace(planted):
    x, x64, cov, lam, vec = planted
    pca = faiss.PCAMatrix(D_IN, D_OUT, 0, True)
    pca.train(x)
    A = pca.A.astype(np.float64)
    assert pca.is_orthonormal
    assert np.abs(A.T @ A - vec[:D_OUT].T @ vec[:D_OUT]).max() <= (2 * U + U * U) + F64_SLACK
    assert np.abs(A - pca.PCAMat[:D_OUT]).max() > 0.01  # and it did rotate


def test_pca_gram_path_against_the_covariance_path():
    """n < d_in: the (n, n) Gram matrix has the covariance's non-zero eigenvalues, and X^T u / sqrt(n l) its
    eigenvectors."""
    rng = np.random.default_rng(4)
    n, d, d_out = 10, 24, 4
    x = (rng.standard_normal((n, d)) * np.sqrt(PLANTED)).astype(np.float32)
    gram, cov = faiss.PCAMatrix(d, d_out), faiss.PCAMatrix(d, d_out)
    cov._gram = False
    gram.train(x)   # n < d_in: the Gram path by default
    cov.train(x)
    assert gram.PCAMat.shape == (n - 1, d) and cov.PCAMat.shape == (d, d)  # centring takes one direction
    lg, lc = gram.eigenvalues.astype(np.float64), cov.eigenvalues.astype(np.float64)
    assert (lg[n - 1:] == 0).all() and (lc[n - 1:] <= 1e-12 * lc[0]).all()
    # two float32 copies of one float64 quantity: u each
    assert (np.abs(lg - lc)[:n - 1] <= 2 * U * lc[:n - 1] + F64_SLACK * lc[0]).all()
    Ag, Ac = gram.A.astype(np.float64), cov.A.astype(np.float64)
    assert np.abs(Ag.T @ Ag - Ac.T @ Ac).max() <= 2 * (2 * U + U * U) + 1e-9  # two stored projectors; gaps are O(1)
    assert np.abs(np.abs(gram.b) - np.abs(cov.b)).max() <= 1e-5  # eigenvector signs are unpinned
    with pytest.raises(RuntimeError, match="principal directions"):
        faiss.PCAMatrix(d, 12).train(x)


# ---------------------------------------------------------------- "IxPT" files
def every_kind():
    """A chain 6 -> 6 -> 6 -> 4 -> 4 -> 4 -> 4 with every transform kind in it."""
    rng = np.random.default_rng(5)
    cnt = faiss.CenteringTransform(6)
    cnt.mean = rng.standard_normal(6)
    rrot = faiss.RandomRotationMatrix(6, 6)
    rrot.init(3)
    pca = faiss.PCAMatrix(6, 4, -0.5, True)
    pca.train((rng.standard_normal((50, 6)) * np.arange(1, 7)).astype(np.float32))
    lt = faiss.LinearTransform(4, 4, True)
    lt.A = rng.standard_normal((4, 4))
    lt.b = rng.standard_normal(4)
    opq = faiss.OPQMatrix(4, 2)
    opq.A = np.eye(4, dtype=np.float32)[[1, 0, 3, 2]]
    lt.set_is_orthonormal()   # a file does not hold the flag: the reader takes it from A, as Faiss's does
    opq.set_is_orthonormal()
    return [cnt, rrot, pca, lt, opq, faiss.NormalizationTransform(4)]


def sub_images():
    """Every sub-index image the writers here write, for d = 4."""
    rng = np.random.default_rng(6)
    xb = rng.standard_normal((3, 4)).astype(np.float32)
    cent = rng.standard_normal((2, 256, 2)).astype(np.float32)
    codes = rng.integers(0, 256, (3, 2)).astype(np.uint8)
    trained = np.concatenate((xb.min(0), np.ptp(xb, axis=0))).astype(np.float32)
    bytes8 = rng.integers(0, 256, (3, 4)).astype(np.uint8)
    lists = [(np.array([2], dtype=np.int64), bytes8[:1]), (np.array([0, 1], dtype=np.int64), bytes8[1:])]
    flat = faiss.serialize_flat(4, faiss.METRIC_L2, xb)
    pq = faiss.serialize_pq(4, faiss.METRIC_L2, cent, codes)
    return {"IxF2": flat, "IxFI": faiss.serialize_flat(4, faiss.METRIC_INNER_PRODUCT, xb),
            "IxMp": faiss.serialize_idmap(4, faiss.METRIC_L2, xb, [7, 8, 9]), "IxPq": pq,
            "IxSQ": faiss.serialize_sq(4, faiss.METRIC_L2, 0, trained, bytes8),
            "IwSq": faiss.serialize_ivfsq(4, faiss.METRIC_L2, 2, 1, faiss.METRIC_L2, xb[:2], 0, trained, lists),
            "IxRF": faiss.serialize_refine(flat, 4, faiss.METRIC_L2, xb, 2.0),
            "IxRF/pq": faiss.serialize_refine(pq, 4, faiss.METRIC_L2, xb, 2.0)}


def same_transform(a, b):
    assert (a.d_in, a.d_out, a.is_trained) == (b.d_in, b.d_out, b.is_trained)
    if isinstance(a, faiss.LinearTransform):
        assert isinstance(b, faiss.LinearTransform) and a.have_bias == b.have_bias
        assert np.array_equal(a.A, b.A) and np.array_equal(a.b, b.b)
        assert a.is_orthonormal == b.is_orthonormal
    if isinstance(a, faiss.PCAMatrix):
        assert type(b) is faiss.PCAMatrix and (a.eigen_power, a.random_rotation) == (b.eigen_power, b.random_rotation)
        assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("mean", "eigenvalues", "PCAMat"))
    if isinstance(a, faiss.CenteringTransform):
        assert type(b) is faiss.CenteringTransform and np.array_equal(a.mean, b.mean)
    if isinstance(a, faiss.NormalizationTransform):
        assert type(b) is faiss.NormalizationTransform and a.norm == b.norm


@pytest.mark.parametrize("sub", sorted(sub_images()))
def test_ixpt_round_trip(sub):
    chain, image = every_kind(), sub_images()[sub]
    buf = faiss.serialize_pretransform(chain, image, 6, faiss.METRIC_L2, 3)
    assert buf[:4] == b"IxPT" and buf.endswith(image)
    d, metric, chain2, fourcc, parts = faiss.parse_pretransform(buf)
    assert (d, metric, fourcc) == (6, faiss.METRIC_L2, image[:4]) and len(chain2) == len(chain)
    for a, b in zip(chain, chain2):
        same_transform(a, b)
    # OPQMatrix is written as a plain LinearTransform; every other kind comes back as itself
    assert [type(t).__name__ for t in chain2] == ["CenteringTransform", "RandomRotationMatrix", "PCAMatrix",
                                                  "LinearTransform", "LinearTransform", "NormalizationTransform"]
    assert faiss.serialize_pretransform(chain2, image, 6, faiss.METRIC_L2, 3) == buf
    assert parts[0] == 4  # the sub-index's own parser read it: d first


def test_ixpt_untrained_and_empty_chains():
    chain = [faiss.CenteringTransform(5), faiss.PCAMatrix(5, 4), faiss.OPQMatrix(4, 2)]
    image = faiss.serialize_flat(4, faiss.METRIC_L2, np.zeros((0, 4), dtype=np.float32))
    buf = faiss.serialize_pretransform(chain, image, 5, faiss.METRIC_L2, 0, False)
    chain2 = faiss.parse_pretransform(buf)[2]
    assert [t.is_trained for t in chain2] == [False, False, False]
    for a, b in zip(chain, chain2):
        same_transform(a, b)
    assert faiss.parse_pretransform(faiss.serialize_pretransform([], image, 4, faiss.METRIC_L2, 0))[2] == []


def test_ixpt_truncation_foreign_and_inconsistent_files():
    chain = every_kind()
    image = sub_images()["IxF2"]
    buf = faiss.serialize_pretransform(chain, image, 6, faiss.METRIC_L2, 3)
    for cut in range(len(buf)):
        with pytest.raises(RuntimeError):
            faiss.parse_pretransform(buf[:cut])
    with pytest.raises(RuntimeError, match="bytes behind"):
        faiss.parse_pretransform(buf + b"\0")
    with pytest.raises(RuntimeError, match="not an IndexPreTransform"):
        faiss.parse_pretransform(image)
    first = faiss._HDR.size + 4
    assert buf[first:first + 4] == b"VCnt"
    with pytest.raises(RuntimeError, match="unsupported vector transform b'ITQm'"):
        faiss.parse_pretransform(buf[:first] + b"ITQm" + buf[first + 4:])
    with pytest.raises(RuntimeError, match="unsupported index type"):
        faiss.parse_pretransform(buf[:-len(image)] + b"IxZZ" + image[4:])
    with pytest.raises(RuntimeError, match="IxPT"):
        faiss.parse_pretransform(buf[:-len(image)] + buf)
    # sizes that do not agree: a header of another d, a chain that does not chain, a matrix of another size
    with pytest.raises(RuntimeError, match="do not match the header"):
        faiss.parse_pretransform(faiss.serialize_pretransform(chain, image, 7, faiss.METRIC_L2, 3))
    with pytest.raises(RuntimeError, match="do not match the header"):
        faiss.parse_pretransform(faiss.serialize_pretransform(chain[:2], image, 6, faiss.METRIC_L2, 3))
    with pytest.raises(RuntimeError, match="do not chain"):
        faiss.parse_pretransform(faiss.serialize_pretransform(chain[:2] + chain[3:], image, 6, faiss.METRIC_L2, 3))
    rec = chain[3]._record()
    bad = rec[:-faiss._VT_TAIL.size] + faiss._VT_TAIL.pack(4, 5, 1)
    with pytest.raises(RuntimeError, match="sizes do not agree"):
        faiss.parse_pretransform(buf.replace(rec, bad))
    with pytest.raises(RuntimeError, match="header"):
        faiss.parse_pretransform(buf[:faiss._HDR.size] + struct.pack("<i", -1) + buf[first:])


# ---------------------------------------------------------------- the public surface
def describe_transform_surface() -> dict:
    out = {name: desc for name, desc in describe_surface().items() if name in _TRANSFORM}
    for desc in out.values():
        if desc["kind"] == "class":
            desc["attrs"] = {a: v for a, v in desc["attrs"].items() if not a.startswith("_") or a in _KEPT_DUNDERS}
    return out


def test_nothing_recorded_of_the_transforms_has_gone_or_changed(golden_dir):
    with open(os.path.join(golden_dir, "faiss_compat_surface_transform.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(_TRANSFORM)
    problems = _problems(recorded, describe_transform_surface())
    assert not problems, "\n".join(problems)
    opq = faiss.OPQMatrix(32, 4)
    assert (opq.niter, opq.niter_pq, opq.niter_pq_0, opq.max_train_points) == (50, 4, 40, 256 * 256)
    assert (opq.d_in, opq.d_out, faiss.OPQMatrix(32, 4, 16).d_out) == (32, 32, 16)


# ---------------------------------------------------------------- the packing of the matrix
def test_panel_packing_under_the_sanitizers(tmp_path):
    """csrc/ise_linear_plan.hpp is host-only: tests/native/linear_plan_check.cpp is built with the host compiler under
    AddressSanitizer and UBSan and run on its own (nothing sanitized is loaded into Python)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone check (it is a tool of the build, not hardware)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "linear_plan_check.cpp")
    exe = str(tmp_path / "linear_plan_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized build failed (no unsanitized fallback):\n" + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


if __name__ == "__main__":
    print(json.dumps(describe_transform_surface(), indent=1, sort_keys=True))
