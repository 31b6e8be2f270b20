"""Host-call cost of the float index's features beside the plain search, for comparing two builds of the library
(``$ISE_KNN_LIB`` names the build; ``--lib`` labels the records): range search plain and masked, the staged and the
combined host search, the filtered search with a reused selector, subset scoring in its host and its torch form.
100k x 512 float32 L2, wall time per call, median of --reps after a warm-up.  One JSON line per case on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_search_engine_amd.faiss_compat as faiss  # noqa: E402
import torch  # noqa: E402


def wall(fn, reps):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--lib", default="?")
a = ap.parse_args()
rng = np.random.default_rng(0)
n, d = 100_000, 512
xb = rng.standard_normal((n, d)).astype(np.float32)
xq = rng.standard_normal((20, d)).astype(np.float32)
idx = faiss.IndexFlatL2(d)
idx.add(xb)
D0, I0 = idx.search(xq, 100)
r = float(np.median(D0[:, 20]))
ds = idx.make_selector(faiss.IDSelectorRange(1000, 11000))
P = faiss.SearchParameters
cand = np.ascontiguousarray(I0[:16])
xt, ct = torch.from_numpy(xq[:16]).cuda(), torch.from_numpy(cand).cuda()


def subset_torch():
    idx.search_subset_torch(xt, 10, ct)
    torch.cuda.synchronize()


cases = {
    "range_search nq=16": lambda: idx.range_search(xq[:16], r),
    "search host nq=20 k=10 (staged)": lambda: idx.search(xq, 10),
    "search host nq=1 k=10 (combined)": lambda: idx.search(xq[:1], 10),
    "filtered search nq=16 k=10 (reused selector)": lambda: idx.search(xq[:16], 10, params=P(sel=ds)),
    "filtered range_search nq=16": lambda: idx.range_search(xq[:16], r, params=P(sel=ds)),
    "search_subset host nq=16 kc=100 k=10": lambda: idx.search_subset(xq[:16], 10, cand),
    "search_subset_torch nq=16 kc=100 k=10 + sync": subset_torch,
}
for name, fn in cases.items():
    print(json.dumps({"probe": "flat_host", "lib": a.lib, "case": name, "reps": a.reps, "us": wall(fn, a.reps)}), flush=True)
