"""remove_ids at 1M x 512 float32 L2 with both shadows present, against the two yardsticks of DESIGN.md 4.8, neither
of which is the code under test:

  (1) wall time of remove_ids + the first search(k=10, nq=16) after it, against the only alternative there was
      before: reset() + add_torch(kept rows) + the first search (which retakes mu, the norms and both shadows);
  (2) the bytes the slab launches moved over their time by HIP events (ise_index_remove_last_timing), against a
      plain device-to-device copy of the same number of bytes on the same stream kind.

Three removals: 1 row at position 0, 1000 scattered rows, a random 10 %.  Median of --reps runs, each on a freshly
built index.  One JSON record per case on stdout and in profiles/remove/remove_probe.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_search_engine_amd.faiss_compat as faiss  # noqa: E402


def build(xb_dev, xq):
    idx = faiss.IndexFlatL2(xb_dev.shape[1])
    idx.add_torch(xb_dev)
    idx.search(xq, 10)  # mu, norms, both shadows
    idx.shadow_row(0), idx.byte_row(0)
    return idx


def memcpy_rate(nbytes, reps=5):
    """GB/s of a device-to-device copy of nbytes (torch's copy_ of a contiguous byte tensor is hipMemcpyAsync)."""
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b.copy_(a)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return nbytes / (float(np.median(ts)) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove", "remove_probe.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n, d = a.n, a.d
    xb = rng.random((n, d), dtype=np.float32)
    xq = rng.random((16, d), dtype=np.float32)
    xb_dev = torch.from_numpy(xb).cuda()
    cases = [("1 row at 0", np.array([0])), ("1000 scattered", np.sort(rng.choice(n, 1000, replace=False))),
             ("random 10 %", np.sort(rng.choice(n, n // 10, replace=False)))]
    recs = []
    for name, gone in cases:
        keep = np.ones(n, dtype=bool)
        keep[gone] = False
        kept_dev = xb_dev[torch.from_numpy(keep).cuda()].contiguous()
        t_rm, t_rb, rates, ref = [], [], [], None
        for _ in range(a.reps):
            idx = build(xb_dev, xq)
            torch.cuda.synchronize()
            t = time.perf_counter()
            assert idx.remove_ids(gone) == len(gone)
            D, I = idx.search(xq, 10)
            t_rm.append(time.perf_counter() - t)
            ms, nbytes = idx.remove_last_timing()
            rates.append(nbytes / (ms * 1e-3) / 1e9)
            del idx
            idx = build(xb_dev, xq)
            torch.cuda.synchronize()
            t = time.perf_counter()
            idx.reset()
            idx.add_torch(kept_dev)
            D2, I2 = idx.search(xq, 10)
            t_rb.append(time.perf_counter() - t)
            assert np.array_equal(I, I2) and np.array_equal(D, D2)  # the same index either way
            del idx
        rec = {"n": n, "d": d, "case": name, "removed": int(len(gone)), "reps": a.reps,
               "remove_plus_search_ms": float(np.median(t_rm)) * 1e3,
               "reset_add_search_ms": float(np.median(t_rb)) * 1e3,
               "moved_bytes": int(nbytes), "slab_launches_ms": float(ms),
               "moved_GBps": float(np.median(rates)), "memcpy_GBps": memcpy_rate(int(nbytes))}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
