"""Query staging of the shadow-row filters (csrc/ise_stage.hpp) on the GPU, on its own and end to end.

A staging error that loosens the bound is invisible in search results (the exact scan repairs them), so the staging
is read back through ise_index_stage_query_debug, which runs the scan kernel's own device functions on one query in a
one-block kernel: the limbs and sh must equal the numpy restatements (tests/byte_filter_ref.py, tests/half_filter_ref.py,
imported), e_q must cover the true residual, and |v|^2 must sit within the rounding budget of its summation
(P / 32 fmaf steps per staging thread and a 5-step butterfly).  Aligned and 4-byte-offset query pointers
run the vector path and the scalar fallback.  End to end, D and I are bit-identical to the float32 filter with the
route counters asserted."""
import zlib

import numpy as np
import pytest

from tests import byte_filter_ref as br
from tests import half_filter_ref as hr
from tests.test_exact_l2_gpu import env_knob, no_direct

pytestmark = pytest.mark.gpu
N = 262_144 + 256  # past the shadows' threshold
U = 2.0 ** -24
DIMS = [64, 500, 509, 512, 1000, 1024]


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def faiss(torch_mod):
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _build(faiss, torch, d, scale=1.0, offset=0.0, seed=0):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + d + seed)
    index = faiss.IndexFlatL2(d)
    step = 65_536
    for i0 in range(0, N, step):
        xb = torch.rand((min(step, N - i0), d), device="cuda", generator=g)
        if scale != 1.0 or offset != 0.0:
            xb = xb * scale + offset
        index.add_torch(xb)
    return index


@pytest.fixture(scope="module")
def indexes(faiss, torch_mod):
    return {d: _build(faiss, torch_mod, d) for d in DIMS}


def _on_device(torch, x, misalign):
    """x as a device vector whose pointer is 16-byte aligned, or 4 bytes past such an address."""
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = 1 if misalign else 0
    buf[off:off + x.size] = torch.from_numpy(x).cuda()
    q = buf[off:off + x.size]
    assert q.data_ptr() % 16 == (4 if misalign else 0)
    return q


def _vec_expected(d, P, misalign):
    return d % 4 == 0 and not misalign and P % 128 == 0 and P <= 1024


def _check(index, torch, x, misalign, route):
    d = index.d
    out = index.stage_query_debug(_on_device(torch, x, misalign), route)
    mu = index.get_shift()
    P = br.dpb_for(d) if route == "byte" else hr.dph_for(d)
    assert out["hi"].shape == (P,) and out["vec"] == _vec_expected(d, P, misalign), (d, P, misalign, out["vec"])
    if route == "byte":
        hi, lo, sh, vt, nv, eq = br.staged_query(x, mu)
    else:
        vt, nv, eq = hr.staged_query(x, mu)
    if vt is None:  # non-finite or overflowing: no limbs, |v|^2 = NaN or +inf, the row is keyed without a bound
        assert not out["hi"].any() and not out["lo"].any()
        assert (np.isnan(out["vn2"]) and np.isnan(nv)) or (out["vn2"] == np.inf and nv == np.inf), (out["vn2"], nv)
        return out
    if route == "byte":
        assert out["sh"] == sh
        assert np.array_equal(out["hi"][:d], hi) and np.array_equal(out["lo"][:d], lo)
        steps = P // 32 + 5
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            amax = float(np.abs((x - mu).astype(np.float32)).max(initial=0.0))
        assert out["sh"] == hr._scale_exp(amax)
        got = np.ldexp(out["hi"][:d].astype(np.float64) + out["lo"][:d].astype(np.float64), -out["sh"])
        assert np.array_equal(got, vt)
        steps = P // 32 + 5 + 2  # hi + lo is rounded to float32 before it is squared
    assert not out["hi"][d:].any() and not out["lo"][d:].any(), "padding columns must be zero"
    print(f"d={d} P={P} {route} misalign={misalign} vec={out['vec']}: e_q {out['eq']:.6e} >= {eq:.6e}; "
          f"|v|^2 rel err {abs(out['vn2'] - nv) / max(nv, 1e-300):.3e} budget {steps * U * 1.001:.3e}")
    assert out["eq"] >= eq, (out["eq"], eq)
    if nv * (1.0 - steps * U * 1.001) > br.FMAX:  # |v|^2 itself overflows float32: +inf, keyed without a bound
        assert out["vn2"] == np.inf, (out["vn2"], nv)
    else:
        assert abs(out["vn2"] - nv) <= steps * U * 1.001 * nv + 2.0 ** -149, (out["vn2"], nv)
    return out


@pytest.mark.parametrize("route", ["byte", "half"])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("d", DIMS)
def test_staged_limbs_equal_the_restatement(indexes, torch_mod, d, misalign, route):
    index = indexes[d]
    rng = _rng("stg", d, misalign, route)
    for x in (rng.random(d, dtype=np.float32), (0.5 + 0.01 * rng.standard_normal(d)).astype(np.float32),
              (3.0 * rng.standard_normal(d)).astype(np.float32)):
        _check(index, torch_mod, x, misalign, route)


@pytest.mark.parametrize("route", ["byte", "half"])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("d", [512, 1000, 509])
def test_special_queries(indexes, torch_mod, d, misalign, route):
    index = indexes[d]
    rng = _rng("spc", d)
    index.stage_query_debug(_on_device(torch_mod, np.zeros(d, np.float32), False), route)  # the shift is in place
    mu = index.get_shift()
    base = rng.random(d, dtype=np.float32)
    nan1, inf1, sub = base.copy(), base.copy(), base.copy()
    nan1[d // 3] = np.nan
    inf1[d - 1] = -np.inf
    sub[::3] = np.float32(1e-40)
    sub[1::7] = np.float32(-1e-42)
    for x in (np.zeros(d, np.float32), mu.copy(), nan1, inf1, sub):
        out = _check(index, torch_mod, x, misalign, route)
    out = _check(index, torch_mod, mu.copy(), misalign, route)
    assert out["sh"] == 0 and out["vn2"] == 0.0 and out["eq"] == 0.0 and not out["hi"].any() and not out["lo"].any()


@pytest.mark.parametrize("route", ["byte", "half"])
@pytest.mark.parametrize("misalign", [False, True])
def test_overflowing_difference(faiss, torch_mod, misalign, route):
    d = 128
    index = _build(faiss, torch_mod, d, seed=7)
    index.set_shift(np.full(d, 3e38, np.float32))  # a fixed shift far from the rows
    index.stage_query_debug(_on_device(torch_mod, np.zeros(d, np.float32), False), route)
    mu = index.get_shift()
    x = np.full(d, 1e38, np.float32)
    x[5] = np.float32(-3e38)
    with np.errstate(over="ignore"):
        assert np.isinf(x[5] - mu[5]), ("the test's own construction: x - mu must overflow", mu[5])
    out = _check(index, torch_mod, x, misalign, route)
    assert out["vn2"] == np.inf and not out["hi"].any() and not out["lo"].any()
    big = (mu * np.float32(0.999)).astype(np.float32)  # huge but finite: |x - mu| ~ 3e35, limbs and e_q are finite,
    big[::2] = mu[::2]                                   # |v|^2 overflows float32 (+inf: keyed without a bound)
    out = _check(index, torch_mod, big, misalign, route)
    assert np.isfinite(out["eq"]) and out["vn2"] == np.inf and out["hi"].any()


def test_debug_call_needs_the_shadow(faiss, torch_mod):
    index = faiss.IndexFlatL2(64)
    index.add_torch(torch_mod.rand((1000, 64), device="cuda"))
    with pytest.raises(Exception):
        index.stage_query_debug(torch_mod.zeros(64, device="cuda"), "byte")
    with pytest.raises(Exception):
        index.stage_query_debug(torch_mod.zeros(64, device="cuda"), "half")


def _counts(index):
    return index.byte_stats()["byte_batches"], index.half_stats()["half_batches"], index.exact_stats()["exact_scan"]


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("d", [512, 1000])
def test_end_to_end_bit_identical_to_the_float32_filter(indexes, torch_mod, d, misalign):
    torch = torch_mod
    index = indexes[d]
    cases = [(nq, k, "byte") for nq in (2, 7, 15, 16) for k in (1, 10)]
    cases += [(nq, 10, "half") for nq in (17, 32, 48)] + [(nq, k, "half") for nq in (7, 16, 32) for k in (11, 12)]
    g = torch.Generator(device="cuda")
    g.manual_seed(99 + d)
    for nq, k, route in cases:
        buf = torch.zeros(nq * d + 8, dtype=torch.float32, device="cuda")
        off = 1 if misalign else 0
        buf[off:off + nq * d] = torch.rand(nq * d, device="cuda", generator=g)
        xq = buf[off:off + nq * d].view(nq, d)
        assert xq.data_ptr() % 16 == (4 if misalign else 0)
        with no_direct():
            b0, h0, e0 = _counts(index)
            D, I = index.search_torch(xq, k)
            torch.cuda.synchronize()
            b1, h1, e1 = _counts(index)
            with env_knob("ISE_NO_HALF_FILTER"):
                Df, If = index.search_torch(xq, k)
                torch.cuda.synchronize()
            b2, h2, e2 = _counts(index)
        assert (b1 - b0, h1 - h0) == ((1, 1) if route == "byte" else (0, 1)), (nq, k, route, b1 - b0, h1 - h0)
        assert (b2 - b1, h2 - h1) == (0, 0), "ISE_NO_HALF_FILTER=1 still read shadow rows"
        # zero exact scans is asserted where the recorded hard-data probe covers the class (uniform rows, d <= 512)
        print(f"d={d} nq={nq} k={k} {route}: queries sent to the exact scan {e1 - e0} (shadow), {e2 - e1} (float32)")
        if d <= 512:
            assert e1 - e0 == 0 and e2 - e1 == 0, ("queries sent to the exact scan", nq, k, route, e1 - e0, e2 - e1)
        assert torch.equal(I, If), (nq, k, route)
        assert torch.equal(D.view(torch.int32), Df.view(torch.int32)), (nq, k, route)
