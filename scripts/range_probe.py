"""Range search against search(k=10) on the same data: wall time per host call (median of --reps after a
warm-up), for the issue's two goals -- 1M x 512 float32 L2, nq = 16, a selective radius (tens to hundreds of
rows per query), and 1000 x 2048 with one query per call.  One JSON record per case on stdout and in
profiles/range/range_probe.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_search_engine_amd.faiss_compat as faiss  # noqa: E402


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range", "range_probe.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    recs = []
    for n, d, nq, metric, storage in [(1 << 20, 512, 16, faiss.METRIC_L2, "f32"),
                                      (1 << 20, 512, 16, faiss.METRIC_INNER_PRODUCT, "f32"),
                                      (100_000, 512, 16, faiss.METRIC_INNER_PRODUCT, "bf16"),
                                      (1000, 2048, 1, faiss.METRIC_L2, "f32"),
                                      (1000, 2048, 1, faiss.METRIC_INNER_PRODUCT, "f32")]:
        xb = rng.standard_normal((n, d)).astype(np.float32)
        xq = rng.standard_normal((nq, d)).astype(np.float32)
        if storage == "bf16":
            faiss.normalize_L2(xb)
            faiss.normalize_L2(xq)
        idx = faiss.IndexFlat(d, metric, storage=storage)
        idx.add(xb)
        D0, _ = idx.search(xq, 100)
        r = float(np.median(D0[:, 60])) if n > 1000 else float(np.median(D0[:, 20]))
        lims, _, _ = idx.range_search(xq, r)
        rec = {"n": n, "d": d, "nq": nq, "metric": "L2" if metric == faiss.METRIC_L2 else "IP", "storage": storage,
               "radius": r, "mean_rows_per_query": float(lims[-1]) / nq,
               "range_us": wall(lambda: idx.range_search(xq, r), a.reps),
               "search_k10_us": wall(lambda: idx.search(xq, 10), a.reps),
               "overflow_batches": idx.range_stats()["range_overflow_batches"]}
        rec["ratio"] = rec["range_us"] / rec["search_k10_us"]
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del idx
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
