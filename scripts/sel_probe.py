"""Selector-filtered search against what there was before it, in the same run:

  filtered search with a reused DeviceSelector, and with a selector built inside the call, against
  (a) the unfiltered search(k), (b) the oversampled search(k') + host filter with the smallest k' that fills k for
  this data (None where k' would pass the library's largest k), (c) a fresh sub-index's build + first search.

Shapes: 1M x 512 float32 L2, nq = 16, k = 10 (contiguous 10 %, random 10 %, random 0.1 %, all but one id);
100k x 512 bf16 inner product, nq = 16; 1000 x 2048 float32 L2, one query per call.  Wall time per host call, median of
--reps runs after a warm-up.  Every shape runs in a child process under its own time limit, and the first one that
fails ends the probe.  One JSON record per case on stdout and in profiles/sel/sel_probe.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (n, d, nq, metric, storage, time limit of the child in seconds)
    "1Mx512_f32_L2": (1 << 20, 512, 16, "L2", "f32", 420),
    "100kx512_bf16_IP": (100_000, 512, 16, "IP", "bf16", 180),
    "1000x2048_f32_L2": (1000, 2048, 1, "L2", "f32", 120),
}
K = 10
MAX_K = 2048


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def child(name, reps):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    n, d, nq, metric, storage, _ = SHAPES[name]
    met = faiss.METRIC_L2 if metric == "L2" else faiss.METRIC_INNER_PRODUCT
    rng = np.random.default_rng(0)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    if storage == "bf16":
        faiss.normalize_L2(xb)
        faiss.normalize_L2(xq)
    xb_dev = torch.from_numpy(xb).cuda()
    idx = faiss.IndexFlat(d, met, storage=storage)
    idx.add_torch(xb_dev)
    idx.search(xq, K)
    a = n // 2 - n // 20
    one = int(idx.search(xq[:1], 1)[1][0, 0])
    sels = [("contiguous 10 %", faiss.IDSelectorRange(a, a + n // 10)),
            ("random 10 %", faiss.IDSelectorBatch(rng.choice(n, n // 10, replace=False))),
            ("random 0.1 %", faiss.IDSelectorBatch(rng.choice(n, max(n // 1000, 1), replace=False))),
            ("all but 1 id", faiss.IDSelectorNot(faiss.IDSelectorBatch([one])))]
    unfiltered = wall(lambda: idx.search(xq, K), reps)
    for case, sel in sels:
        P = faiss.SearchParameters
        m = sel.members(np.arange(n))
        ds = idx.make_selector(sel)
        info = ds.info()
        want = idx.search(xq, K, params=P(sel=ds))
        rec = {"shape": name, "n": n, "d": d, "nq": nq, "k": K, "metric": metric, "storage": storage, "case": case,
               "reps": reps, "selected": info["selected"], "window_rows": info["window"][1] - info["window"][0],
               "nonempty_tiles": info["tiles"], "unfiltered_us": unfiltered,
               "reused_selector_us": wall(lambda: idx.search(xq, K, params=P(sel=ds)), reps),
               "per_call_selector_us": wall(lambda: idx.search(xq, K, params=P(sel=sel)), reps)}
        # (b) the smallest k' whose host-filtered result fills k for every query
        kk, found = K, None
        while kk <= MAX_K:
            _, I = idx.search(xq, kk)
            if (m[np.maximum(I, 0)] & (I >= 0)).sum(1).min() >= min(K, info["selected"]):
                found = kk
                break
            kk = min(kk * 2, MAX_K) if kk < MAX_K else MAX_K + 1
        if found is not None:  # bisect down to the smallest
            lo, hi = max(K, found // 2), found
            while lo < hi:
                mid = (lo + hi) // 2
                _, I = idx.search(xq, mid)
                if (m[np.maximum(I, 0)] & (I >= 0)).sum(1).min() >= min(K, info["selected"]):
                    hi = mid
                else:
                    lo = mid + 1
            found = hi

            def oversampled():
                D, I = idx.search(xq, found)
                keep = m[np.maximum(I, 0)] & (I >= 0)
                return [(D[q][keep[q]][:K], I[q][keep[q]][:K]) for q in range(nq)]

            got = oversampled()
            assert all(np.array_equal(g[1], w[w >= 0]) for g, w in zip(got, want[1]))
            rec["oversample_k"] = found
            rec["oversample_us"] = wall(oversampled, reps)
        else:
            rec["oversample_k"] = None
            rec["oversample_us"] = None
        # (c) a fresh sub-index: build + first search
        rows = torch.from_numpy(np.flatnonzero(m)).cuda()

        def rebuild():
            sub = faiss.IndexFlat(d, met, storage=storage)
            sub.add_torch(xb_dev[rows])
            return sub.search(xq, K)

        rec["subindex_build_search_us"] = wall(rebuild, reps)
        print(json.dumps(rec), flush=True)
        ds.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", default=None, help="run one shape in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sel", "sel_probe.jsonl"))
    a = ap.parse_args()
    if a.shape:
        child(a.shape, max(a.reps, 10))
        return
    lines = []
    for name, shape in SHAPES.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=shape[5])
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.exit(f"{name}: exit status {r.returncode}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
                lines.append(ln)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
