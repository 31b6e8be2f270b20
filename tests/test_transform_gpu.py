"""GPU tests of the linear-transform kernels (include/ise_knn.h, ise_linear_*): ``apply_torch`` and
``apply`` against tests/transform_ref.py bit for bit, in both launch shapes, ragged against every tile and segment."""
import numpy as np
import pytest
import torch

from image_search_engine_amd import _native
from image_search_engine_amd import faiss_compat as faiss
from tests import transform_ref as ref

pytestmark = pytest.mark.gpu

FEW = _native.LINEAR_FEW_ROWS  # the exported switch point: n <= FEW takes the few-row launch shape
NS = (1, 15, 16, 17, FEW, FEW + 1, 4099)
# every d_in of {1, 3, 4, 255, 256, 257, 513, 2048} at two d_out, every d_out of {1, 15, 16, 17, 100, 256} at two d_in
SHAPES = [(1, 1), (1, 17), (3, 15), (3, 256), (4, 16), (4, 100), (255, 1), (255, 17), (256, 16), (256, 100), (257, 15),
          (257, 256), (513, 17), (513, 100), (2048, 16), (2048, 256)]
NMAX = max(NS)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(d_in, d_out, A, b):
    lt = faiss.LinearTransform(d_in, d_out, b is not None)
    lt.A = A
    if b is not None:
        lt.b = b
    return lt


def run_all_n(lt, x):
    """-> {n: (apply_torch(x[:n]), apply(x[:n]))} as numpy, and the launch counters."""
    x_dev = torch.from_numpy(x).cuda()
    out = {}
    for n in NS:
        out[n] = (lt.apply_torch(x_dev[:n]).cpu().numpy(), lt.apply(x[:n]))
    return out, lt.linear_stats()


def check_stats(st):
    few = sum(1 for n in NS if n <= FEW)
    assert st["few_row_launches"] == 2 * few and st["tiled_launches"] == 2 * (len(NS) - few), st
    assert st["calls"] == 2 * len(NS)


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_integer_data_every_row(d_in, d_out):
    """Entries in [-3, 3] x [-8, 8] and an integer bias: every partial sum is an integer below 2^24, so the contract's
    value is the integer product itself -- every row of every batch is checked."""
    rng = np.random.default_rng(d_in * 1000 + d_out)
    A = rng.integers(-3, 4, (d_out, d_in))
    b = rng.integers(-100, 101, d_out)
    x = rng.integers(-8, 9, (NMAX, d_in))
    x64, A64 = x.astype(np.float64), A.astype(np.float64)  # integers: the float64 product is exact
    want = (x64 @ A64.T + b[None, :]).astype(np.float32)
    assert (np.abs(x64) @ np.abs(A64).T).max() + 100 < 2 ** 24
    out, st = run_all_n(make(d_in, d_out, A.astype(np.float32), b.astype(np.float32)), x.astype(np.float32))
    for n, (yt, yh) in out.items():
        assert np.array_equal(bits(yt), bits(want[:n])), (n, "apply_torch")
        assert np.array_equal(bits(yh), bits(want[:n])), (n, "apply")
    check_stats(st)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_gaussian_data_bit_for_bit(d_in, d_out, bias):
    """N(0, 1) data against the exact-fmaf reference.  The reference is computed once for a set of rows (3 at the long
    d_in, where it is slow) that every batch size reaches into; by the contract a row's bits do not depend on the
    batch, so the same reference rows serve every n."""
    rng = np.random.default_rng(d_in * 1000 + d_out + 7)
    A = rng.standard_normal((d_out, d_in)).astype(np.float32)
    b = rng.standard_normal(d_out).astype(np.float32) if bias else None
    x = rng.standard_normal((NMAX, d_in)).astype(np.float32)
    rows = np.array([0, 16, 4098] if d_in > 600 else [0, 1, 14, 15, 16, 17, 31, 63, 64, 65, 127, 4032, 4095, 4096, 4098])
    want = ref.linear_apply(A, b, x[rows])
    out, st = run_all_n(make(d_in, d_out, A, b), x)
    for n, (yt, yh) in out.items():
        sel = rows < n
        assert np.array_equal(bits(yt[rows[sel]]), bits(want[sel])), (n, "apply_torch")
        assert np.array_equal(bits(yh), bits(yt)), (n, "apply against apply_torch")
    check_stats(st)


@pytest.mark.parametrize("d_in,d_out,n", [(2048, 256, 4099), (513, 100, 4099), (2048, 256, FEW)])
def test_float64_bound_at_the_larger_shapes(d_in, d_out, n):
    """|err_j| <= gamma_m (|b_j| + sum_k |A_jk x_k|), m = LIN_KSEG + segments + 1 (tests/transform_ref.linear_bound)."""
    rng = np.random.default_rng(5)
    A = rng.standard_normal((d_out, d_in)).astype(np.float32)
    b = rng.standard_normal(d_out).astype(np.float32)
    x = rng.standard_normal((n, d_in)).astype(np.float32)
    y = make(d_in, d_out, A, b).apply_torch(torch.from_numpy(x).cuda()).cpu().numpy()
    y64, bound = ref.linear_bound(A, b, x)
    worst = float((np.abs(y.astype(np.float64) - y64) / bound).max())
    print(f"{d_in}->{d_out}, n={n}: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("d_in,d_out", [(257, 100), (2048, 256)])
def test_a_row_has_the_same_bits_wherever_it_stands(d_in, d_out):
    """Alone, at positions 0, 7 and 4098 of a batch of 4099, from a slice that is only 4-byte aligned, and on two
    streams at once."""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((d_out, d_in)).astype(np.float32)
    b = rng.standard_normal(d_out).astype(np.float32)
    lt = make(d_in, d_out, A, b)
    row = rng.standard_normal(d_in).astype(np.float32)
    x = rng.standard_normal((4099, d_in)).astype(np.float32)
    for pos in (0, 7, 4098):
        x[pos] = row
    x_dev = torch.from_numpy(x).cuda()
    alone = lt.apply_torch(x_dev[:1]).cpu().numpy()[0]
    assert np.array_equal(bits(alone), bits(ref.linear_apply(A, b, row[None])[0]))
    batch = lt.apply_torch(x_dev).cpu().numpy()
    for pos in (0, 7, 4098):
        assert np.array_equal(bits(batch[pos]), bits(alone)), pos
    # one float into a flat buffer: rows that are 4-byte aligned and no more, for a few rows and for many
    flat = torch.empty(4099 * d_in + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(4099, d_in)
    off.copy_(x_dev)
    assert off.data_ptr() % 16 == 4
    assert np.array_equal(bits(lt.apply_torch(off).cpu().numpy()), bits(batch))
    assert np.array_equal(bits(lt.apply_torch(off[7:8]).cpu().numpy()[0]), bits(alone))
    # a slice of rows of odd length
    if d_in % 2:
        assert x_dev[1:].data_ptr() % 16 != 0
        assert np.array_equal(bits(lt.apply_torch(x_dev[1:]).cpu().numpy()), bits(batch[1:]))
    # two streams at once, one handle
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(4):
        for s, xs in ((s1, x_dev), (s2, x_dev[:17])):
            with torch.cuda.stream(s):
                outs.append(lt.apply_torch(xs))
    torch.cuda.synchronize()
    for o in outs:
        assert np.array_equal(bits(o.cpu().numpy()), bits(batch[:o.shape[0]]))


@pytest.mark.parametrize("n", [20, 70])
def test_nan_and_inf_stay_in_their_row(n):
    d_in, d_out = 300, 40
    rng = np.random.default_rng(n)
    A = rng.standard_normal((d_out, d_in)).astype(np.float32)
    x = rng.standard_normal((n, d_in)).astype(np.float32)
    x[3, 299] = np.nan
    x[5, 0] = np.inf
    x[17, 256] = -np.inf
    y = make(d_in, d_out, A, None).apply_torch(torch.from_numpy(x).cuda()).cpu().numpy()
    bad = np.array([3, 5, 17])
    assert not np.isfinite(y[bad]).any()
    assert np.isnan(y[3]).all()
    good = np.setdiff1d(np.arange(n), bad)
    assert np.array_equal(bits(y[good]), bits(ref.linear_apply(A, None, x[good])))


@pytest.mark.parametrize("n", [3, 70])
def test_subnormals_are_kept(n):
    """Subnormal entries, products and sums come through as IEEE has them."""
    d_in, d_out = 5, 3
    rng = np.random.default_rng(1)
    A = rng.integers(1, 4, (d_out, d_in)).astype(np.float32)
    x = (rng.integers(1, 8, (n, d_in)) * 2.0 ** -140).astype(np.float32)
    b = np.full(d_out, 2.0 ** -149, dtype=np.float32)
    y = make(d_in, d_out, A, b).apply_torch(torch.from_numpy(x).cuda()).cpu().numpy()
    want = ref.linear_apply(A, b, x)
    assert (want != 0).all() and (np.abs(want) < np.finfo(np.float32).tiny).all()
    assert np.array_equal(bits(y), bits(want))


def test_argument_errors():
    lt = make(4, 4, np.eye(4, dtype=np.float32), None)
    x = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    lt.apply_torch(x)
    h = lt._lh._h
    st = torch.cuda.current_stream().cuda_stream
    lib = _native.lib
    assert lib.ise_linear_apply_device(h, x.data_ptr(), 3, x.data_ptr(), st) == _native.E_INVALID  # in place
    assert lib.ise_linear_apply_device(h, x.data_ptr(), 3, x.data_ptr() + 16, st) == _native.E_INVALID  # overlapping
    assert lib.ise_linear_apply_device(h, x.data_ptr(), 0, x.data_ptr(), st) == _native.E_INVALID
    assert lib.ise_linear_apply_device(h, None, 3, x.data_ptr(), st) == _native.E_INVALID
    assert lib.ise_linear_apply_host(h, None, 3, None) == _native.E_INVALID
    big = faiss.LinearTransform(_native.LINEAR_MAX_D + 1, 1)
    big.A = np.zeros((1, _native.LINEAR_MAX_D + 1), dtype=np.float32)
    with pytest.raises(RuntimeError, match="ISE_LINEAR_MAX_D"):
        big.apply(np.zeros((1, _native.LINEAR_MAX_D + 1), dtype=np.float32))
    assert lt.apply(np.zeros((0, 4), dtype=np.float32)).shape == (0, 4)
    # the widest matrix the few-row shape takes: 16 segments, one wave each
    wide = make(_native.LINEAR_MAX_D, 2, np.ones((2, _native.LINEAR_MAX_D), dtype=np.float32), None)
    assert np.array_equal(wide.apply(np.ones((2, _native.LINEAR_MAX_D), dtype=np.float32)),
                          np.full((2, 2), _native.LINEAR_MAX_D, dtype=np.float32))
