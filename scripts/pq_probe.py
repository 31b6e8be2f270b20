"""IndexPQ against the flat index: 1M x 512 float32 L2 rows, k = 10, M = 16 and M = 64 code bytes per
row, the codebook trained on the first 65 536 rows with the default ``cp``.

  search   device time per call between HIP events on the stream of ``search_torch`` -- the table build, the passes and
           their merges together -- for nq in {1, 16, 1024}; in the same process and interleaved with it call by call,
           ``IndexFlatL2.search_torch`` on the same rows (median of --reps after a warm-up; a quarter of them for 1024
           queries); and recall@10 against the flat result
  check    for the 16-query batch, the largest relative difference between the D returned and the 10 smallest
           table sums worked out with torch over all 1M codes (asserted below 1e-4: the scan at a size no test has)
  build    wall time of ``train`` and of ``add_torch`` of all rows, and the bytes of code storage on the device

Two data sets, as scripts/ivf_probe.py has them:
  gaussian  i.i.d. N(0, 1) rows and queries: no structure at all, the worst case for a product quantiser (the ten nearest
            of a million such rows differ by less than the quantisation error), so its recall is a floor
  mixture   4096 Gaussian clusters (centres N(0, 1), spread 0.3), queries drawn like rows
Each (data set, M) runs in a child process of its own under a time limit.  One JSON record per case on stdout, appended to
profiles/pq/pq_probe.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, NTRAIN, K = 1 << 20, 512, 1 << 16, 10
MS = (16, 64)
DATA = ("gaussian", "mixture")
CHILD_LIMIT = 200


def make(data, n, g, dev):
    import torch

    x = torch.randn((n, D), generator=g, device=dev, dtype=torch.float32)
    if data == "mixture":
        centres = torch.randn((4096, D), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        x = centres[torch.randint(0, 4096, (n,), generator=g, device=dev)] + 0.3 * x
    return x.contiguous()


def adc_check(pq, xq, D_got):
    """The k smallest table sums of every query over all codes, with torch; -> largest relative difference to D_got."""
    import torch

    M, dsub = pq.M, pq.d // pq.M
    C = torch.from_numpy(pq.pq.centroids).to(xq.device)
    codes = torch.from_numpy(pq.codes).to(xq.device).long()
    T = ((xq.view(-1, M, 1, dsub) - C[None]) ** 2).sum(-1)  # (nq, M, 256)
    score = torch.zeros((xq.shape[0], codes.shape[0]), device=xq.device)
    for m in range(M):
        score += T[:, m][:, codes[:, m]]
    want = score.topk(K, largest=False).values
    return float(((D_got - want).abs() / want.abs().clamp(min=1)).max())


def child(reps, run, data, M):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xb = make(data, N, g, dev)
    xq_all = make(data, 1024, g, dev)
    flat = faiss.IndexFlatL2(D)
    flat.add_torch(xb)
    pq = faiss.IndexPQ(D, M, 8)
    t = time.perf_counter()
    pq.train(xb[:NTRAIN].cpu().numpy())
    train_s = time.perf_counter() - t
    t = time.perf_counter()
    pq.add_torch(xb)
    torch.cuda.synchronize()
    add_s = time.perf_counter() - t
    print(json.dumps({"run": run, "data": data, "case": "build", "n": N, "d": D, "M": M, "train_rows": NTRAIN, "niter": pq.cp.niter,
                      "train_wall_s": train_s, "add_wall_s": add_s, "code_bytes": pq.pq_stats()["code_bytes"],
                      "row_bytes": N * D * 4}), flush=True)

    def timed(fn_a, fn_b, reps):
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

    for nq in (1, 16, 1024):
        xq = xq_all[:nq].contiguous()
        I_flat = flat.search_torch(xq, K)[1].cpu().numpy()
        s0 = pq.pq_stats()
        D_pq, I_pq = pq.search_torch(xq, K)
        I = I_pq.cpu().numpy()
        s1 = pq.pq_stats()
        extra = {}
        if nq == 16:
            extra["adc_max_rel_err"] = adc_check(pq, xq, D_pq)
            assert extra["adc_max_rel_err"] < 1e-4, extra
        recall = float(np.mean([len(set(I[q]) & set(I_flat[q])) / K for q in range(nq)]))
        r = reps if nq < 1024 else max(3, reps // 4)
        pq_us, flat_us = timed(lambda: pq.search_torch(xq, K), lambda: flat.search_torch(xq, K), r)
        print(json.dumps({"run": run, "data": data, "case": "search", "M": M, "nq": nq, "k": K, "reps": r, "pq_device_us": pq_us,
                          "flat_device_us": flat_us, "pq_over_flat": pq_us / flat_us, "recall_at_10": recall,
                          "passes": s1["scan_passes"] - s0["scan_passes"],
                          "table_builds": s1["table_builds"] - s0["table_builds"], **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run", type=int, default=1, help="label of this run in the records")
    ap.add_argument("--child", default=None, help="DATA:M -- measure this case in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq", "pq_probe.jsonl"))
    a = ap.parse_args()
    if a.child:
        data, M = a.child.split(":")
        assert data in DATA and int(M) in MS
        child(max(a.reps, 5), a.run, data, int(M))
        return
    lines = []
    for data, M in ((data, M) for data in DATA for M in MS):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{data}:{M}", "--reps", str(a.reps),
                            "--run", str(a.run)], capture_output=True, text=True, timeout=CHILD_LIMIT)
        sys.stderr.write(r.stderr[-2000:])
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
                lines.append(ln)
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.exit(f"{data}, M = {M}: exit status {r.returncode}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
