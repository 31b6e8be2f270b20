"""IndexScalarQuantizer (QT_8bit) against the flat index: float32 L2 rows, k = 10, on two shapes,
1M x 512 and 250k x 2048 (the reference's ResNet-50 descriptor width), trained on all rows.

  search   device time per call between HIP events on the stream of ``search_torch`` -- the passes and their merges
           together -- for nq in {1, 16, 1024}; in the same process and interleaved with it call by call,
           ``IndexFlatL2.search_torch`` on the same rows (median of --reps after a warm-up; a quarter of them for 1024
           queries); recall@10 against the flat result; and the time one read of the code bytes takes at 8 TB/s per pass,
           with the measured time as a multiple of it
  check    for the 16-query batch, the largest relative difference between the D returned and the 10 smallest squared
           distances to the decoded rows worked out with torch in float64 (asserted below 1e-4: the scan at a size no
           test has)
  build    wall time of ``train`` (host min / max) and of ``add_torch`` of all rows, and the bytes of code storage on the
           device

Two data sets, as scripts/pq_probe.py has them:
  gaussian  i.i.d. N(0, 1) rows and queries
  mixture   4096 Gaussian clusters (centres N(0, 1), spread 0.3), queries drawn like rows
Each (data set, shape) runs in a child process of its own under a time limit.  One JSON record per case on stdout,
appended to profiles/sq/sq_probe.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 10
SHAPES = ((1 << 20, 512), (250_000, 2048))
DATA = ("gaussian", "mixture")
CHILD_LIMIT = 240
HBM_BYTES_PER_US = 8e6  # 8 TB/s


def make(data, n, d, g, dev):
    import torch

    x = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    if data == "mixture":
        centres = torch.randn((4096, d), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        x = centres[torch.randint(0, 4096, (n,), generator=g, device=dev)] + 0.3 * x
    return x.contiguous()


def decoded_check(sq, xq, D_got):
    """The k smallest squared distances of every query to the decoded rows, float64 with torch in slabs; -> largest
    relative difference to D_got."""
    import torch

    t = torch.from_numpy(sq.sq.trained).to(xq.device)
    vmin, step = t[:sq.d].double(), (t[sq.d:] / 255.0).double()
    codes = torch.from_numpy(sq.codes).to(xq.device)
    best = None
    for i0 in range(0, codes.shape[0], 1 << 16):
        y = (codes[i0:i0 + (1 << 16)].double() + 0.5) * step + vmin
        dist = torch.cdist(xq.double(), y) ** 2
        part = dist.topk(K, largest=False).values
        best = part if best is None else torch.cat([best, part], 1).topk(K, largest=False).values
    return float(((D_got.double() - best).abs() / best.abs().clamp(min=1)).max())


def child(reps, run, data, n, d):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xb = make(data, n, d, g, dev)
    xq_all = make(data, 1024, d, g, dev)
    flat = faiss.IndexFlatL2(d)
    flat.add_torch(xb)
    sq = faiss.IndexScalarQuantizer(d, faiss.ScalarQuantizer.QT_8bit)
    t = time.perf_counter()
    sq.train(xb.cpu().numpy())
    train_s = time.perf_counter() - t
    t = time.perf_counter()
    sq.add_torch(xb)
    torch.cuda.synchronize()
    add_s = time.perf_counter() - t
    code_bytes = sq.sq_stats()["code_bytes"]
    print(json.dumps({"run": run, "data": data, "case": "build", "n": n, "d": d, "train_wall_s": train_s, "add_wall_s": add_s,
                      "code_bytes": code_bytes, "row_bytes": n * d * 4}), flush=True)

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
        s0 = sq.sq_stats()
        D_sq, I_sq = sq.search_torch(xq, K)
        I = I_sq.cpu().numpy()
        passes = sq.sq_stats()["scan_passes"] - s0["scan_passes"]
        extra = {}
        if nq == 16:
            extra["decoded_max_rel_err"] = decoded_check(sq, xq, D_sq)
            assert extra["decoded_max_rel_err"] < 1e-4, extra
        recall = float(np.mean([len(set(I[q]) & set(I_flat[q])) / K for q in range(nq)]))
        r = reps if nq < 1024 else max(3, reps // 4)
        sq_us, flat_us = timed(lambda: sq.search_torch(xq, K), lambda: flat.search_torch(xq, K), r)
        floor_us = passes * n * d / HBM_BYTES_PER_US
        print(json.dumps({"run": run, "data": data, "case": "search", "n": n, "d": d, "nq": nq, "k": K, "reps": r,
                          "sq_device_us": sq_us, "flat_device_us": flat_us, "sq_over_flat": sq_us / flat_us,
                          "recall_at_10": recall, "passes": passes, "code_read_us_at_8TBs": floor_us,
                          "sq_over_code_read": sq_us / floor_us, **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run", type=int, default=1, help="label of this run in the records")
    ap.add_argument("--child", default=None, help="DATA:N:D -- measure this case in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq", "sq_probe.jsonl"))
    a = ap.parse_args()
    if a.child:
        data, n, d = a.child.split(":")
        assert data in DATA and (int(n), int(d)) in SHAPES
        child(max(a.reps, 5), a.run, data, int(n), int(d))
        return
    lines = []
    for data, (n, d) in ((data, shape) for data in DATA for shape in SHAPES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{data}:{n}:{d}", "--reps", str(a.reps),
                            "--run", str(a.run)], capture_output=True, text=True, timeout=CHILD_LIMIT)
        sys.stderr.write(r.stderr[-2000:])
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
                lines.append(ln)
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.exit(f"{data}, {n} x {d}: exit status {r.returncode}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
