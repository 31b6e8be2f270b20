"""IndexBinaryFlat at the near-duplicate workload's size: search(k = 10) and range_search over
1M x 64-bit and 1M x 2048-bit codes, for nq = 1 and 16.

  search        device time per call between HIP events on the stream of ``search_torch`` (median of --reps after a
                warm-up), and the wall time of the blocking host ``search``
  range_search  wall time of the host call (it has one synchronisation inside), at a radius that keeps about one row
                in 10 000

Algorithmic bytes = the codes read once per pass (twice for range search: a count pass and a fill pass); the fraction
is of the 8 TB/s HBM peak.  1M x 64-bit codes are 8 MB and stay in the Infinity Cache, so that shape is expected to be
bound by launches and selection, not by HBM.  Every result is checked against the numpy reference (tests/binary_ref.py)
before it is timed.  Every shape runs in a child process under its own time limit, and the first one that fails ends the
probe.  One JSON record per case on stdout and in profiles/binary/binary_probe.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (n, d_bits, range radius, time limit of the child in seconds)
    "1Mx64": (1 << 20, 64, 18, 240),
    "1Mx2048": (1 << 20, 2048, 940, 300),
}
K = 10
HBM_PEAK = 8e12


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
    from tests import binary_ref as ref

    n, d, radius, _ = SHAPES[name]
    cs = d // 8
    rng = np.random.default_rng(0)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq_all = rng.integers(0, 256, (16, cs), dtype=np.uint8)
    index = faiss.IndexBinaryFlat(d)
    index.add(xb)
    dist = ref.distances(xb, xq_all)
    for nq in (1, 16):
        xq = xq_all[:nq]
        D, I = index.search(xq, K)
        Dw, Iw = ref.search(xb, xq, K, dist[:nq])
        assert np.array_equal(D, Dw) and np.array_equal(I, Iw), "search differs from the reference"
        lims, Dr, Ir = index.range_search(xq, radius)
        lw, Drw, Irw = ref.range_search(xb, xq, radius, dist[:nq])
        assert np.array_equal(lims, lw) and np.array_equal(Dr, Drw) and np.array_equal(Ir, Irw), "range differs"
        xq_dev = torch.from_numpy(xq.copy()).cuda()
        index.search_torch(xq_dev, K)
        torch.cuda.synchronize()
        ev = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            index.search_torch(xq_dev, K)
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        dev_us = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
        nbytes = n * cs
        range_us = wall(lambda: index.range_search(xq, radius), reps)
        rec = {"shape": name, "n": n, "d_bits": d, "nq": nq, "k": K, "reps": reps,
               "search_device_us": dev_us, "search_host_wall_us": wall(lambda: index.search(xq, K), reps),
               "search_bytes": nbytes, "search_frac_of_8TBps": nbytes / (dev_us * 1e-6) / HBM_PEAK,
               "range_radius": radius, "range_rows_per_query": float(lims[-1]) / nq, "range_host_wall_us": range_us,
               "range_bytes": 2 * nbytes, "range_frac_of_8TBps": 2 * nbytes / (range_us * 1e-6) / HBM_PEAK}
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", default=None, help="run one shape in this process (the driver's children)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binary", "binary_probe.jsonl"))
    a = ap.parse_args()
    if a.shape:
        child(a.shape, max(a.reps, 5))
        return
    lines = []
    for name, shape in SHAPES.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=shape[3])
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
