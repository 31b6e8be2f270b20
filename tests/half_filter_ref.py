"""numpy restatement of the fp16 shadow-row filter of long float32 L2 indexes (csrc/ise_rows.hpp
shadow_rows_kernel, csrc/ise_scan.hpp HALF, csrc/ise_common.hpp half_lower_bound).

Rows:    a = y - mu (float64, exact for float32 y and mu), s_r = 14 - ilogb(max |a|), u~ = 2^-s_r fp16(2^s_r a),
         |u~|^2 and e_r = |a - u~|.
Queries: v = x - mu split exactly into float32 v_hi + v_lo, scaled by 2^sh (max |v| in [2^14, 2^15)), then fp16
         hi + lo halves; v~ = 2^-sh (hi + lo), e_q = |v - v~|.
Key:     lo = (max(0, sqrt(max(0, d~ - beta tt)) - e_r - e_q))^2 * shrink, d~ = tt - 2 u~.v~, tt = |u~|^2 + |v~|^2.
"""
import numpy as np

U = 2.0 ** -24


def dph_for(d: int) -> int:
    """Shadow row length: whole 64-byte k-steps of 32 halves, more than 4 steps rounded to a multiple of 4."""
    steps = (d + 31) // 32
    return (((steps + 3) // 4 * 4) if steps > 4 else steps) * 32


def dp_for(d: int) -> int:
    """The float32 rows' padded length (16 floats per k-step)."""
    steps = (d + 15) // 16
    return (((steps + 3) // 4 * 4) if steps > 4 else steps) * 16


def half_beta(dph: int) -> float:
    return (5.0 * dph + 128.0) * U * 1.02


def half_lo_shrink(dp: int) -> float:
    return 1.0 - (dp / 16.0 + 96.0) * U


def _scale_exp(amax: float) -> int:
    return 14 - (int(np.frexp(amax)[1]) - 1) if amax > 0 else 0


def shadow_row(y: np.ndarray, mu: np.ndarray):
    """(u~ as float64, s_r, |u~|^2 as float64, e_r as float64) of one float32 row; None for a non-finite row."""
    y = np.asarray(y, np.float32)
    if not np.isfinite(y).all():
        return None
    a = y.astype(np.float64) - np.asarray(mu, np.float32).astype(np.float64)
    s = _scale_exp(float(np.abs(a).max(initial=0.0)))
    u = np.ldexp(np.ldexp(a, s).astype(np.float32).astype(np.float16).astype(np.float64), -s)
    return u, s, float(u @ u), float(np.sqrt(((a - u) ** 2).sum()))


def shadow_meta(y, mu):
    """What ise_index_shadow_row reports: (|u~|^2, e_r, s_r) -- e_r before the device's outward rounding."""
    r = shadow_row(y, mu)
    if r is None:
        return np.nan, 0.0, 0
    u, s, nu, e = r
    return nu, e, s


def staged_query(x: np.ndarray, mu: np.ndarray):
    """(v~ as float64, |v~|^2, e_q) of one float32 query, the float32 steps of the kernel's staging restated."""
    x = np.asarray(x, np.float32)
    m = np.asarray(mu, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        vh = (x - m).astype(np.float32)
        bb = (vh - x).astype(np.float32)
        vl = ((x - (vh - bb)) + (-m - bb)).astype(np.float32)
    amax = float(np.abs(vh).max(initial=0.0))
    if not np.isfinite(x).all():
        return None, np.nan, 0.0
    if not np.isfinite(amax):
        return None, np.inf, 0.0
    sh = _scale_exp(amax)
    V, VL = np.ldexp(vh.astype(np.float64), sh), np.ldexp(vl.astype(np.float64), sh)
    h1 = V.astype(np.float32).astype(np.float16).astype(np.float64)
    h2 = ((V - h1) + VL).astype(np.float32).astype(np.float16).astype(np.float64)
    vt = np.ldexp(h1 + h2, -sh)
    v = vh.astype(np.float64) + vl.astype(np.float64)
    return vt, float(vt @ vt), float(np.sqrt(((v - vt) ** 2).sum()))


def shadow_rows(xb: np.ndarray, mu: np.ndarray):
    """Vectorised shadow_row over the rows of xb: (u~ [n][d] float64, s_r [n], |u~|^2 [n], e_r [n]); rows with a
    non-finite entry get |u~|^2 = NaN and a zero shadow."""
    xb = np.asarray(xb, np.float32)
    bad = ~np.isfinite(xb).all(1)
    a = np.where(bad[:, None], 0.0, xb.astype(np.float64)) - np.asarray(mu, np.float32).astype(np.float64)
    a[bad] = 0.0
    amax = np.abs(a).max(1, initial=0.0)
    s = np.where(amax > 0, 14 - (np.frexp(amax)[1] - 1), 0)
    with np.errstate(over="ignore"):
        u = np.ldexp(np.ldexp(a, s[:, None]).astype(np.float32).astype(np.float16).astype(np.float64), -s[:, None])
    nu = np.einsum("ij,ij->i", u, u)
    nu[bad] = np.nan
    e = np.sqrt(((a - u) ** 2).sum(1))
    return u, s, nu, e


def lower_bounds(xb: np.ndarray, xq: np.ndarray, mu: np.ndarray) -> np.ndarray:
    """[nq][n] float64 keys of the shadow filter (exact arithmetic apart from the quantisation; the MFMA's and the
    epilogue's roundings are what beta and the margins cover).  NaN where a row or query has a non-finite entry,
    -FLT_MAX where the bound overflowed."""
    d = xb.shape[1]
    beta, shrink = half_beta(dph_for(d)), half_lo_shrink(dp_for(d))
    u, _, nu, er = shadow_rows(xb, mu)
    fmax = float(np.finfo(np.float32).max)
    out = np.empty((xq.shape[0], xb.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for qi, x in enumerate(xq):
            vt, nv, eq = staged_query(x, mu)
            if vt is None:
                out[qi] = np.nan if nv != nv else -fmax
                continue
            nu32 = nu.astype(np.float32).astype(np.float64)  # |u~|^2 as the device stores it
            tt = nu32 + nv
            dd = tt - 2.0 * (u @ vt) - beta * tt
            rr = np.sqrt(np.maximum(dd, 0.0)) - (er + eq)
            lo = np.where(rr > 0, rr * rr * shrink, 0.0)
            lo = np.where(lo <= fmax, lo, -fmax)
            lo = np.where(tt <= fmax, lo, -fmax)
            out[qi] = np.where(np.isnan(tt), np.nan, lo)
    return out


def float32_filter_bounds(xb: np.ndarray, xq: np.ndarray, mu: np.ndarray) -> np.ndarray:
    """The float32 filter's key for comparison (ise_common.hpp l2_lower_bound, beta of ise_flat.hpp exact_beta), in
    float64: |x-mu|^2 + |y-mu|^2 - 2 (x-mu).(y-mu) - beta (|x-mu|^2 + |y-mu|^2)."""
    beta = (0.5625 * dp_for(xb.shape[1]) + 256.0) * U * 1.02
    a = xb.astype(np.float64) - np.asarray(mu, np.float32).astype(np.float64)
    v = xq.astype(np.float64) - np.asarray(mu, np.float32).astype(np.float64)
    na, nv = np.einsum("ij,ij->i", a, a), np.einsum("ij,ij->i", v, v)
    tt = na[None, :] + nv[:, None]
    return tt - 2.0 * (v @ a.T) - beta * tt


def certificate_failures(lo: np.ndarray, d: np.ndarray, k: int, spare: int) -> int:
    """Queries whose certificate lo_(kc) > d_(k) fails when the kc = k + spare rows of smallest lo are re-ranked
    exactly by d (ise_exact.hpp)."""
    fails = 0
    kc = k + spare
    for q in range(lo.shape[0]):
        order = np.lexsort((np.arange(lo.shape[1]), lo[q]))
        cand = order[:kc]
        dk = np.sort(d[q, cand])[k - 1]
        fails += not (lo[q, order[kc]] > dk)
    return fails
