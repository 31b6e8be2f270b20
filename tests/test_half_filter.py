"""CPU checks of the fp16 shadow-row filter (tests/half_filter_ref.py restates csrc/ise_rows.hpp shadow_rows_kernel,
the HALF staging of csrc/ise_scan.hpp and csrc/ise_common.hpp half_lower_bound)."""
import numpy as np
import pytest

from tests import half_filter_ref as hr


def _d64(xb, xq):
    a, b = xb.astype(np.float64), xq.astype(np.float64)
    return ((b[:, None, :] - a[None, :, :]) ** 2).sum(-1)


def _family(kind, rng, n, d):
    if kind == "uniform":
        return rng.random((n, d), dtype=np.float32)
    if kind == "clustered":
        c = (rng.standard_normal((6, d)) * 20).astype(np.float32)
        return (c[rng.integers(0, 6, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    if kind == "offset":       # |mu| >> spread
        return (1e4 + rng.random((n, d))).astype(np.float32)
    if kind == "subnormal":
        return (rng.random((n, d)) * 1e-40).astype(np.float32)
    if kind == "huge":         # finite, norms far beyond fp16 (and float32 squares overflow)
        return (rng.standard_normal((n, d)) * 1e30).astype(np.float32)
    if kind == "mixed_scale":  # rows scaled by 10^[-20, 20]
        return (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-20, 20, (n, 1))).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("d", [8, 100, 512])
@pytest.mark.parametrize("kind", ["uniform", "clustered", "offset", "subnormal", "huge", "mixed_scale"])
def test_bound_below_direct_distance(kind, d):
    rng = np.random.default_rng([len(kind), d, sum(map(ord, kind))])
    n, nq = 400, 12
    xb = _family(kind, rng, n, d)
    xq = np.concatenate([_family(kind, rng, nq - 4, d), xb[:4] + np.float32(0)])  # some queries on the rows
    mu = xb.astype(np.float64).mean(0).astype(np.float32)
    lo = hr.lower_bounds(xb, xq, mu)
    d64 = _d64(xb, xq)
    ok = np.isnan(lo) | (lo <= d64)
    assert ok.all(), (kind, d, np.argwhere(~ok)[:3], lo[~ok][:3], d64[~ok][:3])
    assert not np.isnan(lo).any()  # finite inputs: always a bound (or -FLT_MAX)
    # the shadow's own facts: e_r bounds the quantisation, |u~| within it of |a|
    u, s, nu, e = hr.shadow_rows(xb, mu)
    a = xb.astype(np.float64) - mu.astype(np.float64)
    assert (np.abs(np.sqrt(nu) - np.linalg.norm(a, axis=1)) <= e * (1 + 1e-9) + 1e-300).all()
    assert (np.abs(np.ldexp(u, s[:, None])) < 32768.0 + 1).all()


def test_bound_with_pinned_far_shift():
    rng = np.random.default_rng(3)
    xb = rng.random((300, 64), dtype=np.float32)
    xq = rng.random((8, 64), dtype=np.float32)
    for mu in (np.zeros(64, np.float32), np.full(64, 1e3, np.float32), np.full(64, -7.5e7, np.float32)):
        lo = hr.lower_bounds(xb, xq, mu)
        assert (lo <= _d64(xb, xq)).all()


def test_nonfinite_rows_and_queries():
    rng = np.random.default_rng(4)
    xb = rng.random((50, 16), dtype=np.float32)
    xq = rng.random((3, 16), dtype=np.float32)
    xb[5, 3] = np.nan
    xb[6, 0] = np.inf
    xq[1, 2] = -np.inf
    lo = hr.lower_bounds(xb, xq, np.zeros(16, np.float32))
    assert np.isnan(lo[:, 5]).all() and np.isnan(lo[:, 6]).all() and np.isnan(lo[1]).all()
    assert not np.isnan(np.delete(np.delete(lo, 1, 0), [5, 6], 1)).any()


def test_certificate_table_on_a_smaller_index():
    """The issue's table restated at 60k x 512 uniform rows (the benchmark distribution), 64 queries: with k = 10
    and 4 spare candidates the fp16 shadow certifies every query, as the float32 filter does, while bf16-rounded
    rows and queries (the 2-byte alternative) fail on many."""
    rng = np.random.default_rng(1234)
    n, d, nq, k = 60_000, 512, 64, 10
    xb = rng.random((n, d), dtype=np.float32)
    xq = rng.random((nq, d), dtype=np.float32)
    mu = xb.astype(np.float64).mean(0).astype(np.float32)
    a, b = xb.astype(np.float64), xq.astype(np.float64)
    dist = (a * a).sum(1)[None, :] + (b * b).sum(1)[:, None] - 2.0 * b @ a.T  # float64 is ample for ranking here
    lo_h = hr.lower_bounds(xb, xq, mu)
    assert (lo_h <= dist + 1e-9 * dist).all()
    lo_f = hr.float32_filter_bounds(xb, xq, mu)
    # bf16 alternative: rows and queries rounded to bf16 (around mu), e = |a - a~| exact
    def bf16(x):
        u = np.asarray(x, np.float32).view(np.uint32)
        return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).view(np.float32).astype(np.float64)
    ab, vb = bf16((a - mu).astype(np.float32)), bf16((b - mu).astype(np.float32))
    er, eq = np.linalg.norm((a - mu) - ab, axis=1), np.linalg.norm((b - mu) - vb, axis=1)
    db = np.maximum((ab * ab).sum(1)[None, :] + (vb * vb).sum(1)[:, None] - 2.0 * vb @ ab.T, 0.0)
    lo_b = np.maximum(np.sqrt(db) - er[None, :] - eq[:, None], 0.0) ** 2
    fails = {name: [hr.certificate_failures(lo, dist, k, sp) for sp in (2, 4, 6)]
             for name, lo in (("fp16", lo_h), ("fp32", lo_f), ("bf16", lo_b))}
    assert fails["fp16"][1] == 0 and fails["fp16"][2] == 0, fails
    assert fails["fp32"][1] == 0, fails
    assert fails["bf16"][1] > 8 * max(1, fails["fp16"][0]), fails
