"""Selector-filtered search and remove_ids of IndexBinaryFlat at the near-duplicate workload's size:
1M x 64-bit and 1M x 2048-bit codes, k = 10, nq = 1 and 16.

  filtered search   device time per call between HIP events on the stream of ``search_torch`` with a REUSED device
                    selector (median of --reps after a warm-up) for four selections -- every row, a random 10 %, a random
                    1 %, a contiguous 1 % window -- next to the unfiltered ``search_torch`` of the same run; and the wall
                    time of the blocking ``search`` with a per-call selector (selector build + destroy included)
  removal           wall time of ``remove_ids`` + the first ``search`` after it for 1 row / 1000 scattered rows / a random
                    10 %, against ``reset()`` + ``add_torch(kept)`` + the first search on the same build; the bytes the
                    compaction moved (rows behind the first removed one, one read and one write each way through the
                    bounce buffer counted once) over the wall time of ``remove_ids`` alone, against a device-to-device
                    copy of the same number of bytes

Every result is checked against the numpy reference (tests/binary_ref.py, tests/binary_sel_ref.py) before it is timed.
Every shape runs in a child process under its own time limit, and the first one that fails ends the probe.  One JSON
record per case on stdout and in profiles/binary/binary_sel_probe.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (n, d_bits, time limit of the child in seconds)
    "1Mx64": (1 << 20, 64, 300),
    "1Mx2048": (1 << 20, 2048, 400),
}
K = 10


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def device_us(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def memcpy_rate(nbytes, reps=5):
    """GB/s of a device-to-device copy of nbytes."""
    import torch

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


def child(name, reps):
    import torch

    import image_search_engine_amd.faiss_compat as faiss
    from tests import binary_ref as ref
    from tests import binary_sel_ref as sref

    class Mask(faiss.IDSelector):
        def __init__(self, mask):
            self.mask = mask

        def is_member(self, i):
            return bool(self.mask[int(i)])

        def members(self, ids):
            return self.mask[np.asarray(ids, dtype=np.int64)]

    n, d, _ = SHAPES[name]
    cs = d // 8
    rng = np.random.default_rng(0)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq_all = rng.integers(0, 256, (16, cs), dtype=np.uint8)
    xb_dev = torch.from_numpy(xb).cuda()
    index = faiss.IndexBinaryFlat(d)
    index.add_torch(xb_dev)
    dist = ref.distances(xb, xq_all)
    selections = [("100 %", faiss.IDSelectorRange(0, n)), ("10 % random", Mask(rng.random(n) < 0.10)),
                  ("1 % random", Mask(rng.random(n) < 0.01)),
                  ("1 % window", faiss.IDSelectorRange(n // 2, n // 2 + n // 100))]
    for nq in (1, 16):
        xq = xq_all[:nq]
        xq_dev = torch.from_numpy(xq.copy()).cuda()
        D, I = index.search(xq, K)
        Dw, Iw = ref.search(xb, xq, K, dist[:nq])
        assert np.array_equal(D, Dw) and np.array_equal(I, Iw), "search differs from the reference"
        plain_us = device_us(lambda: index.search_torch(xq_dev, K), reps)
        for sname, sel in selections:
            members = sref.members_of(sel, n)
            ds = index.make_selector(sel)
            info = ds.info()
            assert info == sref.census(members), "selector census differs from the reference"
            p = faiss.SearchParameters(sel=ds)
            D, I = index.search(xq, K, params=p)
            Dw, Iw = sref.search(xb, xq, K, members, dist[:nq])
            assert np.array_equal(D, Dw) and np.array_equal(I, Iw), "filtered search differs from the reference"
            Dt, It = index.search_torch(xq_dev, K, params=p)
            assert np.array_equal(Dt.cpu().numpy(), Dw) and np.array_equal(It.cpu().numpy(), Iw)
            sel_us = device_us(lambda: index.search_torch(xq_dev, K, params=p), reps)
            per_call = faiss.SearchParameters(sel=sel)
            rec = {"what": "filtered search", "shape": name, "n": n, "d_bits": d, "nq": nq, "k": K, "reps": reps,
                   "selection": sname, "selected": info["selected"], "window": info["window"],
                   "nonempty_tiles": info["tiles"], "tiles": (n + 63) // 64,
                   "unfiltered_device_us": plain_us, "filtered_device_us": sel_us,
                   "per_call_selector_host_wall_us": wall(lambda: index.search(xq, K, params=per_call), max(reps // 3, 3)),
                   "unfiltered_host_wall_us": wall(lambda: index.search(xq, K), max(reps // 3, 3))}
            print(json.dumps(rec), flush=True)
            ds.close()
    # ---- removal
    xq = xq_all
    rb = 8 if cs <= 8 else (cs + 15) // 16 * 16  # stored bytes per row
    cases = [("1 row at 0", np.array([0])), ("1000 scattered", np.sort(rng.choice(n, 1000, replace=False))),
             ("random 10 %", np.sort(rng.choice(n, n // 10, replace=False)))]
    rreps = max(reps // 6, 3)
    for cname, gone in cases:
        keep = np.ones(n, dtype=bool)
        keep[gone] = False
        kept_dev = xb_dev[torch.from_numpy(keep).cuda()].contiguous()
        want = ref.search(xb[keep], xq, K, dist[:, keep])
        t_rm, t_only, t_rb = [], [], []
        for _ in range(rreps):
            idx = faiss.IndexBinaryFlat(d)
            idx.add_torch(xb_dev)
            idx.search(xq, K)
            torch.cuda.synchronize()
            t = time.perf_counter()
            assert idx.remove_ids(gone) == len(gone)
            t_only.append(time.perf_counter() - t)
            D, I = idx.search(xq, K)
            t_rm.append(time.perf_counter() - t)
            assert np.array_equal(D, want[0]) and np.array_equal(I, want[1]), "after remove_ids: differs"
            moved = idx.remove_stats()["rows_moved"]
            del idx
            idx = faiss.IndexBinaryFlat(d)
            idx.add_torch(xb_dev)
            idx.search(xq, K)
            torch.cuda.synchronize()
            t = time.perf_counter()
            idx.reset()
            idx.add_torch(kept_dev)
            D2, I2 = idx.search(xq, K)
            t_rb.append(time.perf_counter() - t)
            assert np.array_equal(D2, want[0]) and np.array_equal(I2, want[1])
            del idx
        nbytes = int(moved) * rb
        rec = {"what": "removal", "shape": name, "n": n, "d_bits": d, "case": cname, "removed": int(len(gone)),
               "reps": rreps, "remove_plus_search_ms": float(np.median(t_rm)) * 1e3,
               "remove_only_ms": float(np.median(t_only)) * 1e3, "reset_add_search_ms": float(np.median(t_rb)) * 1e3,
               "moved_bytes": nbytes, "moved_GBps_of_remove_wall": nbytes / float(np.median(t_only)) / 1e9,
               "memcpy_GBps": memcpy_rate(max(nbytes, 1 << 20))}
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", default=None, help="run one shape in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binary", "binary_sel_probe.jsonl"))
    a = ap.parse_args()
    if a.shape:
        child(a.shape, max(a.reps, 5))
        return
    # Each shape's checked records are appended to <out>.partial as that shape completes and the file replaces <out>
    # only after the last one: a failure or a time limit keeps what was measured and leaves an earlier <out> alone.
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    partial = a.out + ".partial"
    open(partial, "w").close()
    for name, shape in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", name, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=shape[2])
            out, err, status = r.stdout, r.stderr, r.returncode
        except subprocess.TimeoutExpired as e:
            out, err, status = e.stdout or "", e.stderr or "", f"none within {shape[2]} s"
        out, err = (x.decode(errors="replace") if isinstance(x, bytes) else x for x in (out, err))
        sys.stderr.write(err[-2000:])
        with open(partial, "a") as f:  # a record is printed only after its check, also by a child that fails later
            for ln in out.splitlines():
                if ln.startswith("{"):
                    print(ln, flush=True)
                    f.write(ln + "\n")
        if status != 0:  # nothing more is started on the GPU after a failure or a time limit
            sys.exit(f"{name}: exit status {status}; the records so far are in {partial}")
    os.replace(partial, a.out)


if __name__ == "__main__":
    main()
