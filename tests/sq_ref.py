"""numpy reference of the scalar-quantised index (tests only): the step, encode, decode and min/max training as
include/ise_knn.h states them, the expected kNN (a float64 brute force over the DECODED rows), the kernel's pass rule,
block size and grid, the integer construction on which every score is exact, an emulation of the scan's arithmetic
(``emulate_scores``) and the worst-case bound of its error derived in DESIGN.md 4.15 (``score_bound``)."""
import functools

import numpy as np

from tests.knn_checks import HUGE, assert_exact_range, brute_knn, int_data
from tests.sel_ref import L2

QT_8BIT, QT_8BIT_UNIFORM = 0, 2
MAX_D = 2048
LDS_LIMIT = 160 * 1024
BLOCK_ROWS = 2 * 4 * 64  # rows per block a short index's grid is sized for: 2 tiles of 64 rows for each of 4 waves
TILE_ROWS = 64
MERGE_LISTS_MAX = 1024  # most blocks of a pass: the merge's list count
U = 2.0 ** -24  # float32's unit roundoff: |rnd(v) - v| <= U |v|


def qt_of(d: int) -> int:
    """Queries per scan pass (csrc/ise_sq.hpp, sq_qt): 16 while two limb images of 2 dpad + 16 bytes, 4 KiB of selection
    buffers and 16 bytes per query fit 160 KiB, else 8."""
    dpad = -(-d // 64) * 64
    return 16 if 16 * (2 * (2 * dpad + 16) + 4 * 128 * 8 + 16) <= LDS_LIMIT else 8


def passes_of(d: int, nq: int, k: int) -> int:
    return -(-nq // qt_of(d)) * -(-k // 32)


def lds_bytes(d: int) -> int:
    """Dynamic LDS of a scan block (csrc/ise_sq.hpp, sq_lds_bytes)."""
    dpad = -(-d // 64) * 64
    return qt_of(d) * (2 * (2 * dpad + 16) + 4 * 128 * 8 + 16)


def grid_of(n: int, d: int, cus: int) -> int:
    """Blocks of a pass over n rows (csrc/ise_sq.hip, sq_grid): two tiles per wave of four on a short index, at most
    the blocks the CUs' LDS holds at once, at most the merge's list count."""
    tiles = -(-n // TILE_ROWS)
    per_cu = max(1, LDS_LIMIT // lds_bytes(d))
    return max(1, min(-(-tiles // 8), per_cu * cus, MERGE_LISTS_MAX))


def expand(trained, d: int, qtype: int):
    """-> (vmin, vdiff) float32 (d,) of a trained vector in Faiss's layout."""
    t = np.asarray(trained, dtype=np.float32).reshape(-1)
    if qtype == QT_8BIT_UNIFORM:
        assert t.size == 2
        return np.full(d, t[0], np.float32), np.full(d, t[1], np.float32)
    assert t.size == 2 * d
    return t[:d].copy(), t[d:].copy()


def step_of(vdiff) -> np.ndarray:
    """s = vdiff / 255.0f: one float32 division."""
    return (np.asarray(vdiff, np.float32) / np.float32(255.0)).astype(np.float32)


def train_minmax(x, qtype: int) -> np.ndarray:
    x = np.asarray(x, np.float32)
    if qtype == QT_8BIT_UNIFORM:
        return np.array([x.min(), x.max() - x.min()], dtype=np.float32)
    return np.concatenate([x.min(0), x.max(0) - x.min(0)]).astype(np.float32)


def encode(x, vmin, vdiff, dtype=np.float32) -> np.ndarray:
    """uint8 codes; ``dtype=np.float64`` gives the float64 reference of the real-data checks."""
    s = step_of(vdiff).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.floor((np.asarray(x, np.float32).astype(dtype) - np.asarray(vmin, np.float32).astype(dtype)) / s)
    t = np.where(s == 0, 0, np.clip(np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0), 0, 255))
    return t.astype(np.uint8)


def encode_t64(x, vmin, vdiff) -> np.ndarray:
    """The float64 quotient (x - vmin) / s before the floor (s the float32 step)."""
    s = step_of(vdiff).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(x, np.float64) - np.asarray(vmin, np.float64)) / s


def decode(codes, vmin, vdiff) -> np.ndarray:
    """fmaf(c + 0.5, s, vmin) as float32.  (c + 0.5) * s is exact in float64 (9 x 24 bits), so the float64 sum is the
    exact value rounded once to 53 bits; the second rounding to float32 differs from the fused one only if that sum is
    inexact AND lands on a float32 midpoint."""
    s = step_of(vdiff).astype(np.float64)
    y = (np.asarray(codes, np.float64) + 0.5) * s + np.asarray(vmin, np.float64)
    return y.astype(np.float32)


def expected(xq, dec, k: int, metric: int):
    """The kNN over the decoded rows; a zero score is +0."""
    D, I = brute_knn(dec, xq, k, metric)
    return D + np.float32(0.0), I


# ---- the integer construction: (vmin_j, vdiff_j) is (m_j - 0.5, 255) [s = 1] or (m_j - 1, 510) [s = 2] with integer
# m_j in [-2, 2]; a row m_j + s_j * base_j encodes to base_j and decodes to itself
def integer_trained(rng, d: int, qtype: int):
    """-> (trained vector, m (d,), s (d,))"""
    cnt = 1 if qtype == QT_8BIT_UNIFORM else d
    m = rng.integers(-2, 3, cnt).astype(np.float32)
    s = rng.integers(1, 3, cnt).astype(np.float32)
    vmin = m - np.float32(0.5) * s
    vdiff = np.float32(255.0) * s
    t = np.concatenate([vmin, vdiff]).astype(np.float32)
    return t, np.broadcast_to(m, (d,)).copy(), np.broadcast_to(s, (d,)).copy()


def integer_rows(rng, n: int, d: int, m, s, kind: str = "small"):
    """-> (rows float32 (n, d), their codes uint8 (n, d))"""
    base = int_data(kind, rng, n, d)
    return (m[None, :] + s[None, :] * base).astype(np.float32), base.astype(np.uint8)


# ---- exact top-k on integer data
def top_of_scores(s, ids, k: int, metric: int):
    """The k best of the float64 scores ``s`` of rows ``ids`` (exact integers), ties by ascending id."""
    key = s if metric == L2 else -s
    if len(ids) > k:
        cand = np.flatnonzero(key <= np.partition(key, k - 1)[k - 1])
    else:
        cand = np.arange(len(ids))
    order = cand[np.lexsort((ids[cand], key[cand]))][:k]
    return s[order].astype(np.float32) + np.float32(0.0), ids[order]


def exact_top(xb64, norms, x, ids, k: int, metric: int):
    """The k best of rows ``ids`` for one query on integer data (float64 is exact), ties by ascending id."""
    dots = xb64[ids] @ x if len(ids) < len(xb64) else xb64 @ x
    s = (norms[ids] + x @ x - 2.0 * dots) if metric == L2 else dots
    return top_of_scores(s, ids, k, metric)


def scores_from_codes(codes, m, s, xq, metric: int, chunk: int = 32768) -> np.ndarray:
    """(n, nq) float64 scores of the integer construction's rows m + s * codes against integer queries: one float64
    BLAS product per chunk of rows.  Every entry is an integer below 2^24 (the caller asserts the range), so the
    products and sums are exact in any order."""
    m64, s64, x64 = np.asarray(m, np.float64), np.asarray(s, np.float64), np.asarray(xq, np.float64)
    out = np.empty((len(codes), len(x64)), np.float64)
    for i0 in range(0, len(codes), chunk):
        y = m64[None, :] + s64[None, :] * codes[i0:i0 + chunk].astype(np.float64)
        dots = y @ x64.T
        out[i0:i0 + chunk] = ((y * y).sum(1)[:, None] + (x64 * x64).sum(1)[None, :] - 2.0 * dots) if metric == L2 else dots
    return out


# ---- the scan's arithmetic (csrc/ise_sq.hpp: sq_stage_kernel, sq_scan_body)
def offset_of(vmin, vdiff) -> np.ndarray:
    """o = fmaf(0.5, s, vmin) as float32 (0.5 s is exact; the float64 sum is rounded once more, as in ``decode``)."""
    return (0.5 * step_of(vdiff).astype(np.float64) + np.asarray(vmin, np.float64)).astype(np.float32)


def staged_weights(xq, vmin, vdiff, metric: int):
    """-> (base, w, sh): base = x - o (L2) or x (inner product) and w = s * base as the float32 values the staging
    kernel forms, and the query's shift sh = 14 - ilogb(max |w|) (0 for an all-zero w)."""
    xq = np.asarray(xq, np.float32)
    base = (xq - offset_of(vmin, vdiff)[None, :]).astype(np.float32) if metric == L2 else xq
    w = (step_of(vdiff)[None, :] * base).astype(np.float32)
    amax = np.abs(w).max(1)
    sh = np.where(amax > 0, 15 - np.frexp(amax)[1], 0).astype(np.int64)  # frexp: amax = f 2^e, f in [0.5, 1)
    return base, w, sh


def emulate_scores(xq, codes, vmin, vdiff, metric: int) -> np.ndarray:
    """(nq, n) float32: the scan's score of every (finite query, row) pair, modelled in numpy -- the float32 weights,
    their fp16 hi + lo limbs at the query's power of two, one float32 rounding of each accumulator chain per MFMA (32
    entries: of step S the bytes [64 S + 16 g, + 8) of the four lane groups g, then the other eight of each), the
    float64 bracket, row term and assembly, one final rounding, the clamp and the +0.  What the model leaves out -- the
    order of the adds inside an MFMA and of the float64 chains -- cannot show where every term is an exact integer:
    there the result is the exact score.  On real data it is a lower estimate of the device's error."""
    codes = np.asarray(codes, np.uint8)
    n, d = codes.shape
    dpad = -(-d // 64) * 64
    s64, o64 = step_of(vdiff).astype(np.float64), offset_of(vmin, vdiff).astype(np.float64)
    base, w, sh = staged_weights(xq, vmin, vdiff, metric)
    cc = np.full((n, dpad), -128.0)  # centred codes; the stride's pad bytes are zero
    cc[:, :d] += codes
    rterm = ((s64[None, :] * codes) ** 2).sum(1)
    first = (np.arange(64) % 16) < 8
    out = np.empty((len(w), n), np.float32)
    for q in range(len(w)):
        V = np.ldexp(w[q], int(sh[q])).astype(np.float32)
        h1 = V.astype(np.float16)
        h2 = (V - h1.astype(np.float32)).astype(np.float16)  # the difference is exact
        hi, lo = np.zeros(dpad), np.zeros(dpad)
        hi[:d], lo[:d] = h1, h2
        acc0, acc1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for S in range(dpad // 64):
            for half in (first, ~first):
                idx = 64 * S + np.flatnonzero(half)
                acc0 = (acc0.astype(np.float64) + cc[:, idx] @ hi[idx]).astype(np.float32)
                acc1 = (acc1.astype(np.float64) + cc[:, idx] @ lo[idx]).astype(np.float32)
        dot = np.ldexp(acc0.astype(np.float64) + acc1.astype(np.float64), -int(sh[q]))
        wsum = np.ldexp((hi + lo).sum(), -int(sh[q]))
        b64 = base[q].astype(np.float64)
        if metric == L2:
            sc = (((b64 * b64).sum() - 256.0 * wsum + rterm) - 2.0 * dot).astype(np.float32)
            sc = np.maximum(sc, np.float32(0.0))
        else:
            sc = ((b64 * o64).sum() + 128.0 * wsum + dot).astype(np.float32)
        out[q] = sc + np.float32(0.0)
    return out


def score_bound(xq, codes, vmin, vdiff, metric: int):
    """-> (E (nq,), parts): the worst case of |score the scan assembles - float64 score over the decoded rows| BEFORE
    the final rounding to float32, over every row, per query (DESIGN.md 4.15 derives each term).  The reported D then
    lies within ``E (1 + U) + U |D64|`` of the float64 value D64.  With w the staged float32 weights, A = 128 sum |w_j|
    and nsteps = dpad / 64:
      dot      (2^-22 + 2 nsteps 2^-24) A   the limbs drop what lies under 22 bits of a weight; the hi chain rounds
                                            2 nsteps partial sums of at most A to 24 bits
      lo       2 nsteps 2^-24 2^-9 A        what the line above leaves out: the hi limbs exceed the weights by up to
                                            2^-11 of them, the lo chain holds up to 2^-11 (1 + 2^-11) of them and is
                                            rounded as often, and a rounded partial sum exceeds A by up to 2 nsteps U A
                                            (2^-11 + 2^-11 + 2^-22 + 2^-18 < 2^-9)
      bracket  2^-22 A                      128 sum (w~_j - w_j): the bracket is taken of the limbs
      under    256 d 2^-25 2^-sh            a limb below fp16's normal range is rounded to a multiple of 2^-24
      weights  2 r A                        w_j against s_j (x_j - o_j) [r = 2 U + 4 U^2: two roundings] or s_j x_j
                                            [r = U + 2 U^2: one], through the bracket and the dot
      base     (2 U + 4 U^2) sum b_j^2      L2: the bracket squares the float32 x_j - o_j
      decode   max over rows of             the reference row is fmaf(c + 0.5, s, vmin) rounded to float32, the scan's
               sum_j e_ij (2 |x_j - y_ij| + e_ij) [L2], sum_j |x_j| e_ij [IP], e_ij = U (|y_ij| + |o_j|)
                                            o_j + s_j c_j with o_j rounded to float32
      f64      2^-40 (sum of the magnitudes the float64 chains add)
    L2: E = 2 (dot + lo + bracket + under + weights) + base + decode + f64; IP: E = the five + decode + f64."""
    xq = np.asarray(xq, np.float32)
    codes = np.asarray(codes, np.uint8)
    d = codes.shape[1]
    nsteps = -(-d // 64)
    base, w, sh = staged_weights(xq, vmin, vdiff, metric)
    A = 128.0 * np.abs(w.astype(np.float64)).sum(1)
    parts = {"dot": (2.0 ** -22 + 2 * nsteps * U) * A, "lo": 2 * nsteps * U * 2.0 ** -9 * A, "bracket": 2.0 ** -22 * A,
             "under": 256.0 * d * 2.0 ** -25 * np.ldexp(1.0, -sh),
             "weights": 2.0 * ((2 * U + 4 * U * U) if metric == L2 else (U + 2 * U * U)) * A}
    y = decode(codes, vmin, vdiff).astype(np.float64)
    o64, s64, x64 = offset_of(vmin, vdiff).astype(np.float64), step_of(vdiff).astype(np.float64), xq.astype(np.float64)
    e = U * (np.abs(y) + np.abs(o64)[None, :])
    rmax = float(((s64[None, :] * codes) ** 2).sum(1).max(initial=0.0))
    b2 = (base.astype(np.float64) ** 2).sum(1)
    if metric == L2:
        parts["base"] = (2 * U + 4 * U * U) * b2
        parts["decode"] = np.array([(e * (2.0 * np.abs(x[None, :] - y) + e)).sum(1).max(initial=0.0) for x in x64])
        parts["f64"] = 2.0 ** -40 * (b2 + rmax + 4.0 * A)
        E = 2.0 * (parts["dot"] + parts["lo"] + parts["bracket"] + parts["under"] + parts["weights"])
        E = E + parts["base"] + parts["decode"] + parts["f64"]
    else:
        parts["decode"] = np.array([(np.abs(x)[None, :] * e).sum(1).max(initial=0.0) for x in x64])
        parts["f64"] = 2.0 ** -40 * ((np.abs(x64) * np.abs(o64)[None, :]).sum(1) + 2.0 * A)
        E = parts["dot"] + parts["lo"] + parts["bracket"] + parts["under"] + parts["weights"] + parts["decode"] + parts["f64"]
    return E, parts


# ---- the data of the error-bound cases
def stretched_case(family, d, qtype, seed=0, n=600, nq=8):
    """-> (training rows, rows, queries) of the error-bound cases: N(c, 1) with one all-zero training row that stretches
    the trained range (family = c), a tight range at a large offset (family "offset": N(1e5, 1), no outlier), sparse
    ReLU-like rows with one entry of 60 (family "relu")."""
    rng = np.random.default_rng([seed, d, qtype])
    if family == "relu":
        xb = np.maximum(rng.standard_normal((n, d)), 0.0).astype(np.float32)
        xb[n // 2, d // 3] = 60.0
        return xb, xb, np.maximum(rng.standard_normal((nq, d)), 0.0).astype(np.float32)
    c = 1e5 if family == "offset" else float(family)
    xb = (c + rng.standard_normal((n, d))).astype(np.float32)
    xq = (c + rng.standard_normal((nq, d))).astype(np.float32)
    train = xb if family == "offset" else np.concatenate([xb, np.zeros((1, d), np.float32)])
    return train, xb, xq


# ---- one block that cuts, then lists that end short (tests/test_sq_scan_gpu.py, tests/test_ivfsq_gpu.py)
@functools.lru_cache(maxsize=None)
def one_block_case(d: int, qtype: int = QT_8BIT):
    """-> (trained, rows, codes, plain queries, queries, D, I): 512 rows of the integer construction -- eight tiles in one
    block, wave 0 streams tiles 0 and 4 and cuts after the second -- in DESCENDING L2 distance to query 0 (every key of
    its second tile passes); 16 queries of which the last three get an entry of 2^64 (finite weights, every distance
    rounds to inf: their lists end without a key); the expected k = 33 results (a floor-keyed second pass).  Computed
    once, shared, read-only."""
    n, nq, k, far = 512, 16, 33, [13, 14, 15]
    rng = np.random.default_rng(9100 + d)
    t, m, s = integer_trained(rng, d, qtype)
    xb, base = integer_rows(rng, n, d, m, s, "binary")
    plain = int_data("binary", rng, nq, d)
    assert_exact_range(xb, plain)
    d0 = ((xb.astype(np.float64) - plain[0].astype(np.float64)) ** 2).sum(1)
    order = np.argsort(-d0, kind="stable")  # query 0: every row beats or ties its predecessors
    xb, base = np.ascontiguousarray(xb[order]), np.ascontiguousarray(base[order])
    xq = plain.copy()
    xq[far, [0, d // 2, d - 1]] = HUGE
    Dw, Iw = expected(xq, xb, k, L2)
    assert (Iw[far] == -1).all() and (Iw[:13] >= 0).all() and (np.diff(Dw[0]) >= 0).all()
    out = (t, xb, base, plain, xq, Dw, Iw)
    for a in out:
        a.setflags(write=False)
    return out
