"""Wall time of one call through the Python wrapper of the coded and inverted-list kinds, for comparing two trees of
the package over one build of the library (``$ISE_KNN_LIB`` names the build; ``--side`` labels the records): ``search``
(numpy in and out) and ``search_torch`` followed by a stream synchronise, nq = 1, k = 10 on n = 4096, d = 64 indexes --
IndexPQ (M = 8), IndexScalarQuantizer, IndexIVFFlat and IndexIVFScalarQuantizer (nlist = 16, nprobe = 4) and
IndexRefineFlat over IndexPQ -- where the device has the least to do and Python's share of a call is largest.  Median
of --reps calls after --warmup calls.  One JSON line per case on stdout."""
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


def wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--side", default="?")
a = ap.parse_args()
rng = np.random.default_rng(0)
n, d, k = 4096, 64, 10
xb = rng.standard_normal((n, d)).astype(np.float32)
xq = rng.standard_normal((1, d)).astype(np.float32)
SQ = faiss.ScalarQuantizer
kinds = {
    "IndexPQ": faiss.IndexPQ(d, 8),
    "IndexScalarQuantizer": faiss.IndexScalarQuantizer(d, SQ.QT_8bit),
    "IndexIVFFlat": faiss.IndexIVFFlat(faiss.IndexFlatL2(d), d, 16),
    "IndexIVFScalarQuantizer": faiss.IndexIVFScalarQuantizer(faiss.IndexFlatL2(d), d, 16, SQ.QT_8bit, by_residual=False),
    "IndexRefineFlat(IndexPQ)": faiss.IndexRefineFlat(faiss.IndexPQ(d, 8)),
}
for name, index in kinds.items():
    index.train(xb)
    index.add(xb)
    if hasattr(index, "nprobe"):
        index.nprobe = 4
    xt = torch.from_numpy(xq).to(torch.device("cuda", index.device))
    stream = torch.cuda.current_stream(xt.device)

    def host():
        index.search(xq, k)

    def device():
        index.search_torch(xt, k)
        stream.synchronize()

    for form, fn in (("search", host), ("search_torch + synchronize", device)):
        print(json.dumps({"probe": "wrapper_call", "side": a.side, "kind": name, "form": form, "nq": 1, "k": k, "n": n,
                          "d": d, "reps": a.reps, "us": wall(fn, a.warmup, a.reps)}), flush=True)
