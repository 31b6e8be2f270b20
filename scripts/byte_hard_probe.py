"""Which data the byte shadow's bound certifies (CPU, the float64 restatements of tests/byte_filter_ref.py and
tests/half_filter_ref.py; no GPU).  For each kind: queries whose certificate lo_(kc) > d_(k) fails through the byte
filter at kc = 32, the fp16 shadow at kc = k + 4 and the float32 filter at kc = k + 4, and the index statistic the
library routes by (mean e_r / |y - mu| over the finite rows, ise_knn.hip byte_rel_err).  One JSON line per kind.

    python scripts/byte_hard_probe.py [--n 60000] [--d 512] [--nq 64] [--k 10] [--kinds uniform,gaussian,...]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import byte_filter_ref as br  # noqa: E402
from tests import half_filter_ref as hr  # noqa: E402


def make(kind, rng, n, d, scale):
    if kind == "uniform":
        return rng.random((n, d), dtype=np.float32)
    if kind == "gaussian":
        return rng.standard_normal((n, d)).astype(np.float32)
    if kind == "relu":         # CNN-like: max(N(0,1), 0) times a per-column scale
        return (np.maximum(rng.standard_normal((n, d)), 0) * scale).astype(np.float32)
    if kind == "sparse_relu":  # sparser activations: max(N(0,1) - 1, 0) times the same scale
        return (np.maximum(rng.standard_normal((n, d)) - 1, 0) * scale).astype(np.float32)
    if kind == "clustered":
        c = rng.standard_normal((64, d)).astype(np.float32)
        return (c[rng.integers(0, 64, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    if kind == "clustered_uniform":  # bounded centres and noise: light tails, tight neighbourhoods
        c = rng.random((64, d), dtype=np.float32)
        return (c[rng.integers(0, 64, n)] + 0.1 * rng.random((n, d))).astype(np.float32)
    raise ValueError(kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60_000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,gaussian,clustered,clustered_uniform,relu,sparse_relu")
    a = ap.parse_args()
    for kind in a.kinds.split(","):
        rng = np.random.default_rng([sum(map(ord, kind)), a.n, a.d])
        scale = rng.gamma(2.0, 0.5, a.d)
        xb = make(kind, rng, a.n, a.d, scale)
        xq = make(kind, rng, a.nq, a.d, scale)
        mu = xb.astype(np.float64).mean(0).astype(np.float32)
        x, y = xb.astype(np.float64), xq.astype(np.float64)
        dist = (x * x).sum(1)[None, :] + (y * y).sum(1)[:, None] - 2.0 * y @ x.T
        _, _, er, _ = br.byte_rows(xb, mu)
        spread = np.linalg.norm(x - mu.astype(np.float64), axis=1)
        rel = float(np.mean(er / np.where(spread > 0, spread, 1.0)))
        lo_b = br.lower_bounds(xb, xq, mu)
        lo_h = hr.lower_bounds(xb, xq, mu)
        lo_f = hr.float32_filter_bounds(xb, xq, mu)
        rec = {"kind": kind, "n": a.n, "d": a.d, "nq": a.nq, "k": a.k, "byte_rel_err": round(rel, 6),
               "fails_byte_kc32": hr.certificate_failures(lo_b, dist, a.k, 32 - a.k),
               "fails_fp16_kc14": hr.certificate_failures(lo_h, dist, a.k, 4),
               "fails_f32_kc14": hr.certificate_failures(lo_f, dist, a.k, 4)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
