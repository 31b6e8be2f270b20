"""IndexIVFPQ (by_residual=False) against the indexes it is made of and checked against: 1M x 512
float32 L2 rows, nlist = 1024 trained on a 100k sample, M = 16 and 64 code bytes a row, k = 10.

  search   device time per call between HIP events on the stream of ``search_torch`` -- the quantiser's search, the
           table build, the mask and work-list kernels, the passes and their merges together -- for nq in {1, 16, 1024}
           and nprobe in {1, 8, 32}; in the same process and interleaved with it call by call, ``IndexPQ`` (the same
           codebook), ``IndexIVFScalarQuantizer`` (the same quantiser object, so the same centroids and probes) and
           ``IndexFlatL2`` on the same rows (median of --reps after a warm-up; a quarter of them for 1024 queries); the
           quantiser's own search alone; the 64-row tiles the passes visited (ise_ivfpq_stats) beside the tiles in all;
           and recall@10 against the flat result, beside ``IndexPQ``'s own
  build    wall time of ``train`` (k-means, then the codebook with ``pq.cp.niter`` = --pq-niter), of ``add_torch`` of all
           rows and of the first search after it (the rebuild)

Two data sets, as scripts/ivfsq_probe.py has them, each with each M in a child process of its own under a time limit:
  gaussian  i.i.d. N(0, 1) rows and queries: no cluster structure, a few hub lists and many nearly empty ones
  mixture   4096 Gaussian clusters (centres N(0, 1), spread 0.3), queries drawn like rows
One JSON record per case on stdout, appended to profiles/ivfpq/ivfpq_probe.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, NLIST, NTRAIN, K = 1 << 20, 512, 1024, 100_000, 10
MS = (16, 64)
CHILD_LIMIT = 420
DATA = ("gaussian", "mixture")


def make(data, n, g, dev):
    import torch

    x = torch.randn((n, D), generator=g, device=dev, dtype=torch.float32)
    if data == "mixture":
        centres = torch.randn((4096, D), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        x = centres[torch.randint(0, 4096, (n,), generator=g, device=dev)] + 0.3 * x
    return x.contiguous()


def child(reps, run, data, M, pq_niter):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xb = make(data, N, g, dev)
    xq_all = make(data, 1024, g, dev)
    flat = faiss.IndexFlatL2(D)
    flat.add_torch(xb)
    qz = faiss.IndexFlatL2(D)  # one quantiser for both inverted-list indexes
    ivfpq = faiss.IndexIVFPQ(qz, D, NLIST, M, 8, faiss.METRIC_L2, by_residual=False)
    ivfpq.pq.cp.niter = pq_niter
    t = time.perf_counter()
    ivfpq.train(xb[:NTRAIN].cpu().numpy())
    train_s = time.perf_counter() - t
    t = time.perf_counter()
    ivfpq.add_torch(xb)
    torch.cuda.synchronize()
    add_s = time.perf_counter() - t
    t = time.perf_counter()
    ivfpq.search_torch(xq_all[:1], K)
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t
    pq = faiss.IndexPQ(D, M, 8)
    pq.pq.set_centroids(ivfpq.pq.centroids)
    pq.add_torch(xb)
    ivfsq = faiss.IndexIVFScalarQuantizer(qz, D, NLIST, faiss.ScalarQuantizer.QT_8bit, faiss.METRIC_L2, by_residual=False)
    ivfsq.sq.train(xb[:NTRAIN].cpu().numpy())
    ivfsq.add_torch(xb)
    sizes = np.array([ivfpq.list_size(l) for l in range(NLIST)])
    tiles_total = int(((sizes + 63) // 64).sum())
    print(json.dumps({"run": run, "data": data, "case": "build", "n": N, "d": D, "M": M, "nlist": NLIST, "train_rows": NTRAIN,
                      "pq_niter": pq_niter, "train_wall_s": train_s, "add_wall_s": add_s, "first_search_wall_s": first_s,
                      "list_size_min": int(sizes.min()), "list_size_median": float(np.median(sizes)),
                      "list_size_max": int(sizes.max()), "tiles_total": tiles_total, "tiles_of_a_flat_array": (N + 63) // 64}),
          flush=True)

    def timed(fns, reps):
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        evs = [[] for _ in fns]
        for _ in range(reps):  # interleaved: all see the same clocks and the same cache state
            for fn, ev in zip(fns, evs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev.append((a, b))
        torch.cuda.synchronize()
        return [float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3 for ev in evs]

    def recall_of(I, I_flat):
        return float(np.mean([len(set(I[q]) & set(I_flat[q])) / K for q in range(len(I))]))

    for nq in (1, 16, 1024):
        xq = xq_all[:nq].contiguous()
        r = reps if nq < 1024 else max(3, reps // 4)
        I_flat = flat.search_torch(xq, K)[1].cpu().numpy()
        I_pq = pq.search_torch(xq, K)[1].cpu().numpy()
        for nprobe in (1, 8, 32):
            ivfpq.nprobe = ivfsq.nprobe = nprobe
            s0 = ivfpq.ivfpq_stats()
            Ig = ivfpq.search_torch(xq, K)[1].cpu().numpy()
            s1 = ivfpq.ivfpq_stats()
            ivfpq_us, pq_us, ivfsq_us, flat_us, qz_us = timed(
                [lambda: ivfpq.search_torch(xq, K), lambda: pq.search_torch(xq, K), lambda: ivfsq.search_torch(xq, K),
                 lambda: flat.search_torch(xq, K), lambda: qz.search_torch(xq, nprobe)], r)
            print(json.dumps({"run": run, "data": data, "case": "search", "M": M, "nq": nq, "nprobe": nprobe, "k": K, "reps": r,
                              "ivfpq_device_us": ivfpq_us, "pq_device_us": pq_us, "ivfsq_device_us": ivfsq_us,
                              "flat_device_us": flat_us, "quantizer_device_us": qz_us, "quantizer_share": qz_us / ivfpq_us,
                              "ivfpq_over_pq": ivfpq_us / pq_us, "ivfpq_over_ivfsq": ivfpq_us / ivfsq_us,
                              "ivfpq_over_flat": ivfpq_us / flat_us, "recall_at_10": recall_of(Ig, I_flat),
                              "pq_recall_at_10": recall_of(I_pq, I_flat),
                              "tiles_loaded": s1["tiles_loaded"] - s0["tiles_loaded"], "tiles_total": tiles_total,
                              "passes": s1["passes"] - s0["passes"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run", type=int, default=1, help="label of this run in the records")
    ap.add_argument("--pq-niter", type=int, default=25, help="k-means iterations per sub-quantiser (pq.cp.niter)")
    ap.add_argument("--child", choices=DATA, default=None, help="measure this data set in this process (the driver's children)")
    ap.add_argument("--M", type=int, default=0, help="the child's code bytes a row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq", "ivfpq_probe.jsonl"))
    a = ap.parse_args()
    if a.child:
        child(max(a.reps, 5), a.run, a.child, a.M, a.pq_niter)
        return
    lines = []
    for data in DATA:
        for M in MS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", data, "--M", str(M), "--reps", str(a.reps),
                                "--run", str(a.run), "--pq-niter", str(a.pq_niter)], capture_output=True, text=True,
                               timeout=CHILD_LIMIT)
            sys.stderr.write(r.stderr[-2000:])
            for ln in r.stdout.splitlines():
                if ln.startswith("{"):
                    print(ln, flush=True)
                    lines.append(ln)
            if r.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.exit(f"{data} M={M}: exit status {r.returncode}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
