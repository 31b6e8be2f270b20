"""The linear transform and IndexPreTransform, three cases, each in a child process of its own under a
time limit; one JSON record per line on stdout, appended to profiles/pretransform/pretransform_probe.jsonl.

  apply    device time of ``LinearTransform.apply_torch`` between HIP events at 2048 -> 256, 512 -> 128 and 512 -> 512
           for n in {1, 16, 1024, 1M}, interleaved call by call with ``torch.addmm`` on the same tensors (median of
           --reps after a warm-up; a quarter of them at 1M rows), the rate in TFLOP/s, and the largest difference of the
           two results relative to sum_k |A_jk x_k|
  search   ``search_torch`` through ``IndexPreTransform(PCAMatrix(2048, 256), IndexFlatL2(256))`` (the factory's
           "pca256-l2", trained on 65536 of the rows) against ``IndexFlatL2(2048)`` on the same 1M clustered rows, k = 10,
           for 1 / 16 / 1024 queries: device time of each, recall@10 against the full-width result, and the share of the
           time the transform takes (its own device time over the whole call's)
  opq      ``IndexPQ(128, 16)`` with and without ``OPQMatrix(128, 16)`` in front on 100k rows with a decaying spectrum
           (standard deviation 1 / sqrt(1 + j) in a random basis): recall@10 against the flat index for 1024 queries and
           the wall time of ``train``
"""
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
SHAPES = ((2048, 256), (512, 128), (512, 512))
NS = (1, 16, 1024, 1 << 20)
CHILD_LIMIT = 400


def timed(fn_a, fn_b, reps):
    import torch

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


def recall(I, I_ref):
    return float(np.mean([len(set(I[q]) & set(I_ref[q])) / K for q in range(I.shape[0])]))


def child_apply(reps, run):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for d_in, d_out in SHAPES:
        A = torch.randn((d_out, d_in), generator=g, device=dev) / d_in ** 0.5
        b = torch.randn(d_out, generator=g, device=dev)
        lt = faiss.LinearTransform(d_in, d_out, True)
        lt.A, lt.b = A.cpu().numpy(), b.cpu().numpy()
        At = A.t().contiguous()
        x_all = torch.randn((max(NS), d_in), generator=g, device=dev)
        for n in NS:
            x = x_all[:n]
            y, y_ref = lt.apply_torch(x), torch.addmm(b, x, At)
            mag = x[:4096].abs() @ At.abs() + b.abs()
            diff = float(((y[:4096] - y_ref[:4096]).abs() / mag).max())
            r = reps if n < (1 << 20) else max(3, reps // 4)
            ours_us, torch_us = timed(lambda: lt.apply_torch(x), lambda: torch.addmm(b, x, At), r)
            print(json.dumps({"run": run, "case": "apply", "d_in": d_in, "d_out": d_out, "n": n, "reps": r,
                              "apply_device_us": ours_us, "addmm_device_us": torch_us, "apply_over_addmm": ours_us / torch_us,
                              "apply_tflops": 2.0 * n * d_in * d_out / ours_us * 1e-6,
                              "addmm_tflops": 2.0 * n * d_in * d_out / torch_us * 1e-6,
                              "max_diff_over_magnitude": diff}), flush=True)


def child_search(reps, run):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    n, d, d_out = 1 << 20, 2048, 256
    centres = torch.randn((4096, d), generator=g, device=dev)

    def draw(m):
        return (centres[torch.randint(0, 4096, (m,), generator=g, device=dev)] + 0.3 * torch.randn((m, d), generator=g, device=dev)).contiguous()

    xb, xq_all = draw(n), draw(1024)
    flat = faiss.IndexFlatL2(d)
    flat.add_torch(xb)
    pca = faiss.PCAMatrix(d, d_out)
    pre = faiss.IndexPreTransform(pca, faiss.IndexFlatL2(d_out))
    t = time.perf_counter()
    pre.train(xb[:: n // 65536].cpu().numpy())
    train_s = time.perf_counter() - t
    t = time.perf_counter()
    pre.add_torch(xb)
    torch.cuda.synchronize()
    add_s = time.perf_counter() - t
    print(json.dumps({"run": run, "case": "search_build", "n": n, "d": d, "d_out": d_out, "train_rows": 65536,
                      "train_wall_s": train_s, "add_wall_s": add_s}), flush=True)
    for nq in (1, 16, 1024):
        xq = xq_all[:nq].contiguous()
        I_flat = flat.search_torch(xq, K)[1].cpu().numpy()
        I_pre = pre.search_torch(xq, K)[1].cpu().numpy()
        r = reps if nq < 1024 else max(3, reps // 4)
        pre_us, flat_us = timed(lambda: pre.search_torch(xq, K), lambda: flat.search_torch(xq, K), r)
        apply_us, _ = timed(lambda: pca.apply_torch(xq), lambda: None, r)
        print(json.dumps({"run": run, "case": "search", "n": n, "d": d, "d_out": d_out, "nq": nq, "k": K, "reps": r,
                          "pretransform_device_us": pre_us, "flat2048_device_us": flat_us, "pre_over_flat": pre_us / flat_us,
                          "transform_device_us": apply_us, "transform_share": apply_us / pre_us,
                          "recall_at_10": recall(I_pre, I_flat)}), flush=True)


def child_opq(reps, run):
    import torch

    import image_search_engine_amd.faiss_compat as faiss

    rng = np.random.default_rng(0)
    n, d, M = 100_000, 128, 16
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    scale = 1.0 / np.sqrt(1.0 + np.arange(d))
    xb = ((rng.standard_normal((n, d)) * scale) @ q.T).astype(np.float32)
    xq = ((rng.standard_normal((1024, d)) * scale) @ q.T).astype(np.float32)
    flat = faiss.IndexFlatL2(d)
    flat.add(xb)
    I_flat = flat.search(xq, K)[1]
    for name, index in (("pq", faiss.IndexPQ(d, M, 8)),
                        ("opq-pq", faiss.IndexPreTransform(faiss.OPQMatrix(d, M), faiss.IndexPQ(d, M, 8)))):
        t = time.perf_counter()
        index.train(xb)
        train_s = time.perf_counter() - t
        index.add(xb)
        rec = index.reconstruct_n(0, 20000).astype(np.float64)
        print(json.dumps({"run": run, "case": "opq", "index": name, "n": n, "d": d, "M": M, "train_wall_s": train_s,
                          "recall_at_10": recall(index.search(xq, K)[1], I_flat),
                          "mse": float(((rec - xb[:20000]) ** 2).sum(1).mean())}), flush=True)


CHILDREN = {"apply": child_apply, "search": child_search, "opq": child_opq}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run", type=int, default=1, help="label of this run in the records")
    ap.add_argument("--cases", default="apply,search,opq")
    ap.add_argument("--child", default=None, help="measure this case in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretransform", "pretransform_probe.jsonl"))
    args = ap.parse_args()
    if args.child:
        CHILDREN[args.child](args.reps, args.run)
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for case in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(args.reps), "--run", str(args.run)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {CHILD_LIMIT} s; stopping", file=sys.stderr)
            return 1
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        with open(args.out, "a") as f:
            f.write(r.stdout)
        if r.returncode != 0:  # nothing more is started on the device behind a child that failed
            sys.stderr.write(r.stderr[-2000:])
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
