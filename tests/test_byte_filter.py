"""CPU checks of the byte shadow-row filter (tests/byte_filter_ref.py restates csrc/ise_rows.hpp byte_rows_kernel,
the BYTE staging of csrc/ise_scan.hpp and csrc/ise_common.hpp byte_lower_bound)."""
import numpy as np
import pytest

from tests import byte_filter_ref as br
from tests import half_filter_ref as hr
from tests.test_half_filter import _d64, _family


@pytest.mark.parametrize("d", [8, 100, 512, 1024])
@pytest.mark.parametrize("kind", ["uniform", "clustered", "offset", "subnormal", "huge", "mixed_scale"])
def test_bound_below_direct_distance(kind, d):
    rng = np.random.default_rng([len(kind), d, sum(map(ord, kind)), 8])
    n, nq = 300, 10
    xb = _family(kind, rng, n, d)
    xq = np.concatenate([_family(kind, rng, nq - 4, d), xb[:4] + np.float32(0)])  # some queries on the rows
    mu = xb.astype(np.float64).mean(0).astype(np.float32)
    lo = br.lower_bounds(xb, xq, mu)
    d64 = _d64(xb, xq)
    ok = np.isnan(lo) | (lo <= d64)
    assert ok.all(), (kind, d, np.argwhere(~ok)[:3], lo[~ok][:3], d64[~ok][:3])
    assert not np.isnan(lo).any()  # finite inputs: always a bound (or -FLT_MAX)


@pytest.mark.parametrize("kind", ["uniform", "clustered", "offset", "subnormal", "huge", "mixed_scale"])
def test_quantiser(kind):
    rng = np.random.default_rng([sum(map(ord, kind)), 81])
    xb = _family(kind, rng, 200, 96)
    mu = xb.astype(np.float64).mean(0).astype(np.float32)
    q, cr, er, e = br.byte_rows(xb, mu)
    a = xb.astype(np.float64) - mu.astype(np.float64)
    assert q.dtype == np.int8 and np.abs(q.astype(int)).max() <= 127
    assert (cr * 127 >= np.abs(a).max(1)).all()  # c_r rounded up: no entry clips
    # c_r is a bf16 value, e_r / c_r an fp16 one, and their product stays exact in float32
    assert (np.float32(cr).view(np.uint32) & 0xFFFF == 0).all()
    ratio = er / np.where(cr > 0, cr, 1.0)
    assert (ratio.astype(np.float16).astype(np.float64) == ratio).all()
    assert (np.float32(er).astype(np.float64) == er).all()
    # e_r bounds the quantisation error (stored rounded up) and is within an fp16 step of it
    res = np.linalg.norm(a - cr[:, None] * q, axis=1)
    assert (er >= res).all() and (er <= res * (1 + 2.0 ** -9) + 1e-300).all()
    # per entry the error is at most half a step
    assert (np.abs(a - cr[:, None] * q) <= cr[:, None] / 2 * (1 + 1e-12) + 1e-300).all()


def test_nonfinite_rows_and_queries():
    rng = np.random.default_rng(4)
    xb = rng.random((50, 16), dtype=np.float32)
    xq = rng.random((3, 16), dtype=np.float32)
    xb[5, 3] = np.nan
    xb[6, 0] = np.inf
    xq[1, 2] = -np.inf
    q, cr, er, _ = br.byte_rows(xb, np.zeros(16, np.float32))
    assert not q[5].any() and not q[6].any() and cr[5] == cr[6] == 0 and er[5] == er[6] == 0
    lo = br.lower_bounds(xb, xq, np.zeros(16, np.float32))
    assert np.isnan(lo[:, 5]).all() and np.isnan(lo[:, 6]).all() and np.isnan(lo[1]).all()
    assert not np.isnan(np.delete(np.delete(lo, 1, 0), [5, 6], 1)).any()


@pytest.mark.parametrize("kind", ["uniform", "offset", "subnormal", "huge", "mixed_scale"])
def test_query_limbs(kind):
    """The two int8 limbs of V = 2^sh v: max |V| in [2^13, 2^14), hi within +-65, lo within int8, and e_q is the
    residual of 2^sh v against 256 hi + lo (at most half a unit per entry)."""
    rng = np.random.default_rng([sum(map(ord, kind)), 7])
    xb = _family(kind, rng, 64, 200)
    mu = xb.astype(np.float64).mean(0).astype(np.float32)
    for x in _family(kind, rng, 6, 200):
        hi, lo, sh, vt, nv, eq = br.staged_query(x, mu)
        V = np.ldexp((x - mu).astype(np.float32).astype(np.float64), sh)
        assert 2.0 ** 13 <= np.abs(V).max() < 2.0 ** 14
        assert np.abs(hi.astype(int)).max() <= 65
        v = x.astype(np.float64) - mu.astype(np.float64)
        assert np.isclose(np.linalg.norm(v - vt), eq, rtol=1e-12, atol=0)
        assert (np.abs(np.ldexp(v, sh) - (256.0 * hi + lo)) <= 0.5 + 2.0 ** -20).all()
        assert eq <= 0.5 * np.sqrt(v.size) * 2.0 ** -sh * (1 + 1e-9)


def test_bound_with_pinned_far_shift():
    rng = np.random.default_rng(3)
    xb = rng.random((300, 64), dtype=np.float32)
    xq = rng.random((8, 64), dtype=np.float32)
    for mu in (np.zeros(64, np.float32), np.full(64, 1e3, np.float32), np.full(64, -7.5e7, np.float32)):
        lo = br.lower_bounds(xb, xq, mu)
        assert (lo <= _d64(xb, xq)).all()


def test_certificate_at_kc32_on_a_smaller_index():
    """60k x 512 uniform rows (the benchmark distribution), 64 queries, k = 10: the byte filter's expanded bound
    certifies every query with 32 candidates, and at the smaller kc where it fails the triangle form certifies no
    further query (so the kernel keys by the expanded form alone); the fp16 bound certifies at k + 4."""
    rng = np.random.default_rng(1234)
    n, d, nq, k = 60_000, 512, 64, 10
    xb = rng.random((n, d), dtype=np.float32)
    xq = rng.random((nq, d), dtype=np.float32)
    mu = xb.astype(np.float64).mean(0).astype(np.float32)
    a, b = xb.astype(np.float64), xq.astype(np.float64)
    dist = (a * a).sum(1)[None, :] + (b * b).sum(1)[:, None] - 2.0 * b @ a.T
    lo_b = br.lower_bounds(xb, xq, mu)
    assert (lo_b <= dist + 1e-9 * dist).all()
    lo_t = br.triangle_bounds(xb, xq, mu)
    assert hr.certificate_failures(lo_b, dist, k, 22) == 0
    # where the expanded form fails (kc = 14 .. 28), adding the triangle form certifies no further query
    for spare in (4, 10, 14, 18):
        assert hr.certificate_failures(np.maximum(lo_b, lo_t), dist, k, spare) == \
            hr.certificate_failures(lo_b, dist, k, spare), spare
    assert hr.certificate_failures(hr.lower_bounds(xb, xq, mu), dist, k, 4) == 0
