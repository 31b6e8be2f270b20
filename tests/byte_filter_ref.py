"""numpy restatement of the byte shadow-row filter of long float32 L2 indexes (csrc/ise_rows.hpp byte_rows_kernel,
csrc/ise_scan.hpp BYTE, csrc/ise_common.hpp byte_lower_bound).

Rows:    a = y - mu (float64, exact for float32 y and mu), c_r = max |a| / 127 rounded up to bf16,
         q = rint(a / c_r) in [-127, 127], u~ = c_r q, e_r = |a - u~| (stored as c_r times an fp16 ratio, rounded up).
Queries: V = 2^sh fl(x - mu) with max |V| in [2^13, 2^14), int8 limbs hi = rint(V / 256), lo = rint(V - 256 hi +
         2^sh v_lo) (v_lo the TwoSum remainder), v~ = 2^-sh (256 hi + lo), e_q = |v - v~|.
Key:     lo = |v|^2 + |a|^2 - 2 v~.u~ - 2 (|v| e_r + |a| e_q + e_r e_q) - beta tt, times shrink when positive.
"""
import numpy as np

from tests.half_filter_ref import U, dp_for, half_lo_shrink

FMAX = float(np.finfo(np.float32).max)


def dpb_for(d: int) -> int:
    """Byte row length: whole 64-byte k-steps, more than 4 steps rounded to a multiple of 4."""
    steps = (d + 63) // 64
    return (((steps + 3) // 4 * 4) if steps > 4 else steps) * 64


def byte_beta(dp: int) -> float:
    return (dp / 8.0 + 64.0) * U * 1.02


def _f32_up(x: float) -> np.float32:
    f = np.float32(x)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < x else f


def _bf16_up(f: np.float32) -> float:
    b = int(np.float32(f).view(np.uint32))
    if b & 0xFFFF:
        b = (b + 0x10000) & 0xFFFF0000
    return float(np.uint32(b).view(np.float32))


def _f16_up(x: float) -> float:
    ef = _f32_up(x)
    h = np.float16(ef)
    if np.float32(h) < ef:
        h = np.nextafter(h, np.float16(np.inf))
    return float(h)


def byte_rows(xb: np.ndarray, mu: np.ndarray):
    """(q [n][d] int8, c_r [n], e_r [n] as stored, e_r [n] exact) of the rows of xb; rows with a non-finite entry get
    a zero shadow and c_r = e_r = 0."""
    xb = np.asarray(xb, np.float32)
    bad = ~np.isfinite(xb).all(1)
    a = np.where(bad[:, None], 0.0, xb.astype(np.float64)) - np.asarray(mu, np.float32).astype(np.float64)
    a[bad] = 0.0
    amax = np.abs(a).max(1, initial=0.0)
    cr = np.array([_bf16_up(_f32_up(m / 127.0)) if m > 0 else 0.0 for m in amax])
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(cr[:, None] > 0, np.clip(np.rint(a / cr[:, None]), -127, 127), 0.0)
    res = a - cr[:, None] * q
    e = np.sqrt((res * res).sum(1))
    nu = np.sqrt((a * a).sum(1))
    e_dev = e * (1.0 + 2.0 ** -40) + nu * 2.0 ** -49
    stored = np.array([c * _f16_up(ed / c * (1.0 + 2.0 ** -40)) if c > 0 else 0.0 for c, ed in zip(cr, e_dev)])
    return q.astype(np.int8), cr, stored, e


def byte_meta(y, mu):
    """What ise_index_byte_row reports: (c_r, e_r)."""
    _, cr, er, _ = byte_rows(np.asarray(y, np.float32)[None, :], mu)
    return float(cr[0]), float(er[0])


def staged_query(x: np.ndarray, mu: np.ndarray):
    """(hi, lo, sh, v~ as float64, |v|^2 as float64, e_q) of one float32 query, the kernel's float32 staging restated;
    (None, .., |v|^2 = NaN or inf) for a non-finite or overflowing query."""
    x = np.asarray(x, np.float32)
    m = np.asarray(mu, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        vh = (x - m).astype(np.float32)
        bb = (vh - x).astype(np.float32)
        vl = ((x - (vh - bb)) + (-m - bb)).astype(np.float32)
    if not np.isfinite(x).all():
        return None, None, 0, None, np.nan, 0.0
    amax = float(np.abs(vh).max(initial=0.0))
    if not np.isfinite(amax):
        return None, None, 0, None, np.inf, 0.0
    sh = 13 - (int(np.frexp(amax)[1]) - 1) if amax > 0 else 0
    V, VL = np.ldexp(vh.astype(np.float64), sh), np.ldexp(vl.astype(np.float64), sh)
    hi = np.rint(V / 256.0)
    r1 = V - 256.0 * hi
    lo = np.rint(r1 + VL)
    wrap = lo > 127
    hi, lo = np.where(wrap, hi + 1, hi), np.where(wrap, lo - 256, lo)
    assert np.abs(hi).max(initial=0) <= 127 and lo.min(initial=0) >= -128 and lo.max(initial=0) <= 127
    vt = np.ldexp(256.0 * hi + lo, -sh)
    v = vh.astype(np.float64) + vl.astype(np.float64)
    vv = vh.astype(np.float64)
    return hi.astype(np.int8), lo.astype(np.int8), sh, vt, float(vv @ vv), float(np.sqrt(((v - vt) ** 2).sum()))


def lower_bounds(xb: np.ndarray, xq: np.ndarray, mu: np.ndarray) -> np.ndarray:
    """[nq][n] float64 keys of the byte filter (exact arithmetic apart from the quantisation; the epilogue's float32
    roundings are what beta and the margins cover).  NaN where a row or query has a non-finite entry, -FLT_MAX where
    the bound overflowed.  |y - mu|^2 is the float32 norm the index stores, restated in float64 here."""
    xb = np.asarray(xb, np.float32)
    d = xb.shape[1]
    beta, shrink = byte_beta(dp_for(d)), half_lo_shrink(dp_for(d))
    q, cr, er, _ = byte_rows(xb, mu)
    bad = ~np.isfinite(xb).all(1)
    a = np.where(bad[:, None], 0.0, xb.astype(np.float64)) - np.asarray(mu, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        na = np.where(bad, np.nan, (a * a).sum(1).astype(np.float32).astype(np.float64))
    u = cr[:, None] * q.astype(np.float64)
    out = np.empty((xq.shape[0], xb.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for qi, x in enumerate(xq):
            hi, lo_, sh, vt, nv, eq = staged_query(x, mu)
            if vt is None:
                out[qi] = np.nan if nv != nv else -FMAX
                continue
            nv32 = float(np.float32(nv))
            tt = na + nv32
            E = np.sqrt(nv32) * er + np.sqrt(na) * eq + er * eq
            dd = tt - 2.0 * (u @ vt) - 2.0 * E - beta * tt
            lo = np.where(dd > 0, dd * shrink, dd)
            lo = np.where(np.abs(lo) <= FMAX, lo, -FMAX)
            lo = np.where(tt <= FMAX, lo, -FMAX)
            out[qi] = np.where(np.isnan(tt), np.nan, lo)
    return out


def triangle_bounds(xb: np.ndarray, xq: np.ndarray, mu: np.ndarray) -> np.ndarray:
    """The triangle form (|u~ - v~| - e_r - e_q)^2 on the same byte rows, for comparison (exact arithmetic)."""
    q, cr, er, _ = byte_rows(xb, mu)
    u = cr[:, None] * q.astype(np.float64)
    out = np.empty((xq.shape[0], xb.shape[0]))
    for qi, x in enumerate(xq):
        _, _, _, vt, _, eq = staged_query(x, mu)
        r = np.sqrt(((u - vt[None, :]) ** 2).sum(1)) - er - eq
        out[qi] = np.where(r > 0, r * r, 0.0)
    return out
