"""The arithmetic contract of the linear transform (include/ise_knn.h, ise_linear_*) in numpy, for
tests/test_transform*.py.

    y_j = ((b_j + s_0) + s_1) + ...        float32 adds, ascending segments; b_j = +0 without a bias
    s_i = the k-ascending float32 fmaf chain over k in [256 i, min(256 i + 256, d_in)), started from +0:
          s = fmaf(A[j][k], x[k], s)

Python 3.10 has no ``math.fma`` and a float64 multiply-add narrowed to float32 rounds twice, so ``fmaf`` below is an
exact emulation: the product of two float32 is exact in float64 (48 bits), TwoSum gives the exact error of adding the
third operand, and the float64 sum is turned into its round-to-odd value before it is narrowed -- a 53-bit round-to-odd
intermediate (>= 2 * 24 + 2 bits) narrows to the correctly rounded float32 (Boldo and Melquiond, "Emulation of FMA and
correctly rounded sums", 2008).  ``fmaf_rational`` is the same function in rational arithmetic, one triple at a time:
the check of the emulation.
"""
from fractions import Fraction

import numpy as np

LIN_KSEG = 256


def fmaf(a, b, c) -> np.ndarray:
    """float32 fma(a, b, c) with one rounding, elementwise over broadcastable float32 arrays."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = a * b                                # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)            # TwoSum: p + c == s + e exactly
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        # round to odd: of the two float64 around the exact sum, the one with the odd significand
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def round_fraction_f32(v: Fraction) -> np.float32:
    """The float32 nearest to a non-zero rational below the overflow threshold, ties to even."""
    assert v != 0
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)
    m = v / q
    f = m.numerator // m.denominator
    r = m - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return np.float32(sign * float(f * q))  # f * q has at most 25 significant bits: exact in float64, and in float32


def fmaf_rational(a, b, c) -> np.float32:
    """fma(a, b, c) of three finite float32 with a non-zero exact result, by rational arithmetic."""
    v = Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c)))
    return round_fraction_f32(v)


def linear_apply(A, b, x) -> np.ndarray:
    """A float32 (d_out, d_in), b float32 (d_out,) or None, x float32 (n, d_in) -> y float32 (n, d_out) with the
    contract's bits."""
    A = np.asarray(A, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    d_out, d_in = A.shape
    n = x.shape[0]
    assert x.shape[1] == d_in
    out = np.zeros((n, d_out), dtype=np.float32)
    if b is not None:
        out += np.asarray(b, dtype=np.float32)[None, :]
    with np.errstate(all="ignore"):
        for k0 in range(0, d_in, LIN_KSEG):
            s = np.zeros((n, d_out), dtype=np.float32)
            for k in range(k0, min(k0 + LIN_KSEG, d_in)):
                s = fmaf(A[None, :, k], x[:, k, None], s)
            out = out + s
    return out


def linear_bound(A, b, x) -> tuple:
    """(y in float64, the bound on |y_float32 - y|): gamma_m (|b_j| + sum_k |A_jk x_k|) with m = LIN_KSEG + segments
    + 1, gamma_m = m u / (1 - m u), u = 2^-24 -- every product is rounded into a sum of at most LIN_KSEG terms, then
    passes through at most `segments` adds more (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)."""
    A64, x64 = np.asarray(A, dtype=np.float64), np.asarray(x, dtype=np.float64)
    y = x64 @ A64.T
    mag = np.abs(x64) @ np.abs(A64).T
    if b is not None:
        y = y + np.asarray(b, dtype=np.float64)[None, :]
        mag = mag + np.abs(np.asarray(b, dtype=np.float64))[None, :]
    segments = -(-A64.shape[1] // LIN_KSEG)
    m = LIN_KSEG + segments + 1
    u = 2.0 ** -24
    return y, m * u / (1 - m * u) * mag
