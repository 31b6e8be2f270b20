"""Summation order of the shadow filters' query staging (csrc/ise_stage.hpp), restated in numpy float32.

|v|^2 and e_q's sum of squares are taken by 32 threads per query row: a thread's own elements as one chain, then a
5-step xor butterfly.  The vector path gives thread t the 4 adjacent elements of the 16-byte slots t, t + 32, ...
(rows over 512 elements: the upper half of the row first), the scalar path the elements t, t + 32, ...  Either way a
thread runs P / 32 steps.  Here every product and every sum is rounded to float32 on its own, which is no tighter than
the kernel's fmaf chain, and the result is held against the float64 sum of the same float32 terms:
  |v|^2   within the share DESIGN.md 4.1 gives it in beta_8, (dpb / 32 + 8) u, and in beta_h, (dph + 8) u;
  e_q     the float32 sum times the (1 + 2^-9) margin of the kernel covers the float64 sum.
The limbs themselves are checked on the GPU against the same restatements (tests/test_shadow_staging_gpu.py)."""
import zlib

import numpy as np
import pytest

from tests import byte_filter_ref as br
from tests import half_filter_ref as hr

U = 2.0 ** -24
TPR = 32
QV = 4  # 16-byte slots per staging thread and half row


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def owned_elements(P: int, d: int, aligned: bool = True):
    """Per staging thread, the padded row's element indexes in the order its chain adds them."""
    if d % 4 == 0 and aligned and P % (4 * TPR) == 0 and P <= 8 * TPR * QV:
        halves = [1, 0] if P // 4 > TPR * QV else [0]
        out = []
        for t in range(TPR):
            idx = []
            for h in halves:
                for i in range(QV):
                    j4 = h * TPR * QV + t + i * TPR
                    if j4 < P // 4:
                        idx += [4 * j4 + e for e in range(4)]
            out.append(idx)
        return out
    return [list(range(t, P, TPR)) for t in range(TPR)]


def staged_sum_of_squares(v: np.ndarray, P: int, d: int, aligned: bool = True) -> np.float32:
    """sum v_j^2 over the padded row in the staging's order, products and sums rounded to float32."""
    w = np.zeros(P, np.float32)
    w[: v.size] = v
    part = np.zeros(TPR, np.float32)
    for t, idx in enumerate(owned_elements(P, d, aligned)):
        s = np.float32(0.0)
        for j in idx:
            s = np.float32(s + np.float32(w[j] * w[j]))
        part[t] = s
    o = TPR // 2
    while o:
        part = (part + part[np.arange(TPR) ^ o]).astype(np.float32)
        o >>= 1
    return part[0]


def _queries(kind, rng, d):
    if kind == "uniform":
        return rng.random(d, dtype=np.float32), np.full(d, 0.5, np.float32)
    if kind == "offset":  # |mu| >> spread
        mu = np.full(d, 300.0, np.float32)
        return (mu + 0.05 * rng.standard_normal(d)).astype(np.float32), mu
    if kind == "subnormal":
        return (rng.standard_normal(d) * 1e-40).astype(np.float32), np.zeros(d, np.float32)
    if kind == "huge":
        return (rng.standard_normal(d) * 1e37).astype(np.float32), (rng.standard_normal(d) * 1e36).astype(np.float32)
    raise ValueError(kind)


def test_every_element_is_owned_once_and_no_thread_exceeds_its_steps():
    for d in (4, 60, 64, 100, 128, 500, 509, 512, 516, 1000, 1024):
        for P in (br.dpb_for(d), hr.dph_for(d)):
            for aligned in (True, False):
                own = owned_elements(P, d, aligned)
                assert sorted(j for idx in own for j in idx) == list(range(P))
                assert max(len(idx) for idx in own) <= -(-P // TPR), (d, P, aligned)


@pytest.mark.parametrize("kind", ["uniform", "offset", "subnormal", "huge"])
@pytest.mark.parametrize("d", [64, 512, 1000, 1024])
def test_byte_sums_within_their_share(kind, d):
    x, mu = _queries(kind, _rng("b", kind, d), d)
    hi, lo, sh, vt, nv, eq = br.staged_query(x, mu)
    P = br.dpb_for(d)
    vh = (x - mu).astype(np.float32)
    V = np.ldexp(vh, sh).astype(np.float32)  # exact: max |V| in [2^13, 2^14)
    assert np.array_equal(V.astype(np.float64), np.ldexp(vh.astype(np.float64), sh))
    for aligned in (True, False):
        sn = float(staged_sum_of_squares(V, P, d, aligned))
        ref = float(V.astype(np.float64) @ V.astype(np.float64))
        assert abs(sn - ref) <= (P / 32 + 8) * U * ref, (kind, d, aligned, sn, ref)
        assert abs(sn - ref) <= (P / 32 + 5) * U * 1.001 * ref  # what the GPU test allows the kernel
        # the residuals of the limbs, in scaled units
        v = vh.astype(np.float64) + _two_sum_low(x, mu).astype(np.float64)
        res = np.ldexp(v - vt, sh).astype(np.float32)
        e2 = float(staged_sum_of_squares(res, P, d, aligned))
        ref2 = float(res.astype(np.float64) @ res.astype(np.float64))
        assert e2 * (1.0 + 2.0 ** -9) >= ref2, (kind, d, aligned, e2, ref2)


@pytest.mark.parametrize("kind", ["uniform", "offset", "subnormal", "huge"])
@pytest.mark.parametrize("d", [64, 512, 1000, 1024])
def test_half_sums_within_their_share(kind, d):
    x, mu = _queries(kind, _rng("h", kind, d), d)
    vt, nv, eq = hr.staged_query(x, mu)
    P = hr.dph_for(d)
    vh = (x - mu).astype(np.float32)
    sh = hr._scale_exp(float(np.abs(vh).max(initial=0.0)))
    wv64 = np.ldexp(vt, sh)  # hi + lo, exact in float64
    wv = wv64.astype(np.float32)  # the kernel squares float32(hi + lo)
    for aligned in (True, False):
        sn = float(staged_sum_of_squares(wv, P, d, aligned))
        ref = float(wv64 @ wv64)
        assert abs(sn - ref) <= (P + 8) * U * ref, (kind, d, aligned, sn, ref)
        assert abs(sn - ref) <= (P / 32 + 5 + 2) * U * 1.001 * ref  # what the GPU test allows the kernel
        v = vh.astype(np.float64) + _two_sum_low(x, mu).astype(np.float64)
        res = np.ldexp(v - vt, sh).astype(np.float32)
        e2 = float(staged_sum_of_squares(res, P, d, aligned))
        ref2 = float(res.astype(np.float64) @ res.astype(np.float64))
        assert e2 * (1.0 + 2.0 ** -9) >= ref2, (kind, d, aligned, e2, ref2)


def _two_sum_low(x, mu):
    """The TwoSum remainder of fl(x - mu) (x - mu = vh + vl exactly)."""
    x64, m64 = x.astype(np.float64), mu.astype(np.float64)
    vh = (x - mu).astype(np.float32)
    return ((x64 - m64) - vh.astype(np.float64)).astype(np.float32)
