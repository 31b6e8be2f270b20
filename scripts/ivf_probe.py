"""IndexIVFFlat against the flat index it is checked against: 1M x 512 float32 L2 rows, nlist = 1024
trained on a 100k sample, k = 10.

  search   device time per call between HIP events on the stream of ``search_torch`` -- the quantiser's search, the mask
           kernel, the pass and the merge together -- for nq in {1, 16} and nprobe in {1, 8, 32, 1024}; in the same
           process and interleaved with it call by call, ``IndexFlatL2.search_torch`` on the same rows (median of --reps
           after a warm-up); and recall@10 against the flat result
  add      wall time of ``add_torch`` of all rows, and of the first search after it (the rebuild: one stable scatter of
           the whole index, the shift vector and the norms)

Two data sets, each in a child process of its own under a time limit:
  gaussian  i.i.d. N(0, 1) rows and queries: no cluster structure.  k-means on such rows gives a few hub lists and many
            nearly empty ones, so a probe reads far more than nprobe / nlist of the rows and the recall is a floor
  mixture   4096 Gaussian clusters (centres N(0, 1), spread 0.3), queries drawn like rows: what descriptors look like
            more.  The lists are uneven here too (recorded: 1 ... 25 562 rows, median 275, after ten Lloyd iterations
            from random rows), but a query's neighbours sit in the lists it probes
tiles_loaded is the pass's own count of 16-row tiles read (ise_ivf_stats).  One JSON record per case on stdout, appended
to profiles/ivf/ivf_probe.jsonl."""
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
CHILD_LIMIT = 240


DATA = ("gaussian", "mixture")


def make(data, n, g, dev):
    import torch

    x = torch.randn((n, D), generator=g, device=dev, dtype=torch.float32)
    if data == "mixture":
        centres = torch.randn((4096, D), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        x = centres[torch.randint(0, 4096, (n,), generator=g, device=dev)] + 0.3 * x
    return x.contiguous()


def child(reps, run, data):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xb = make(data, N, g, dev)
    xq_all = make(data, 16, g, dev)
    flat = faiss.IndexFlatL2(D)
    flat.add_torch(xb)
    qz = faiss.IndexFlatL2(D)
    ivf = faiss.IndexIVFFlat(qz, D, NLIST)
    t = time.perf_counter()
    ivf.train(xb[:NTRAIN].cpu().numpy())
    train_s = time.perf_counter() - t
    t = time.perf_counter()
    ivf.add_torch(xb)
    torch.cuda.synchronize()
    add_s = time.perf_counter() - t
    t = time.perf_counter()
    ivf.search_torch(xq_all[:1], K)
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t
    sizes = np.array([ivf.list_size(l) for l in range(NLIST)])
    print(json.dumps({"run": run, "data": data, "case": "build", "n": N, "d": D, "nlist": NLIST, "train_rows": NTRAIN, "train_wall_s": train_s,
                      "add_wall_s": add_s, "first_search_wall_s": first_s, "list_size_min": int(sizes.min()),
                      "list_size_median": float(np.median(sizes)), "list_size_max": int(sizes.max())}), flush=True)

    def timed(fn_a, fn_b):
        fn_a(), fn_b()
        torch.cuda.synchronize()
        ea, eb = [], []
        for _ in range(reps):  # interleaved: both see the same clocks and the same cache state
            for fn, ev in ((fn_a, ea), (fn_b, eb)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev.append((a, b))
        torch.cuda.synchronize()
        return [float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3 for ev in (ea, eb)]

    for nq in (1, 16):
        xq = xq_all[:nq].contiguous()
        I_flat = flat.search_torch(xq, K)[1].cpu().numpy()
        for nprobe in (1, 8, 32, 1024):
            ivf.nprobe = nprobe
            s0 = ivf.ivf_stats()
            I = ivf.search_torch(xq, K)[1].cpu().numpy()
            s1 = ivf.ivf_stats()
            recall = float(np.mean([len(set(I[q]) & set(I_flat[q])) / K for q in range(nq)]))
            if nprobe == NLIST:
                assert np.array_equal(I, I_flat), "every list probed: the flat result"
            ivf_us, flat_us = timed(lambda: ivf.search_torch(xq, K), lambda: flat.search_torch(xq, K))
            qz_us, _ = timed(lambda: qz.search_torch(xq, nprobe), lambda: None)
            print(json.dumps({"run": run, "data": data, "case": "search", "nq": nq, "nprobe": nprobe, "k": K, "reps": reps,
                              "ivf_device_us": ivf_us, "flat_device_us": flat_us, "ivf_over_flat": ivf_us / flat_us,
                              "quantizer_device_us": qz_us, "recall_at_10": recall,
                              "tiles_loaded": s1["tiles_loaded"] - s0["tiles_loaded"], "tiles_total": int(((sizes + 15) // 16).sum()),
                              "passes": s1["passes"] - s0["passes"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run", type=int, default=1, help="label of this run in the records")
    ap.add_argument("--child", choices=DATA, default=None, help="measure this data set in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf", "ivf_probe.jsonl"))
    a = ap.parse_args()
    if a.child:
        child(max(a.reps, 5), a.run, a.child)
        return
    lines = []
    for data in DATA:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", data, "--reps", str(a.reps), "--run", str(a.run)],
                           capture_output=True, text=True, timeout=CHILD_LIMIT)
        sys.stderr.write(r.stderr[-2000:])
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
                lines.append(ln)
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.exit(f"{data}: exit status {r.returncode}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
