"""IndexBinaryIVF against IndexBinaryFlat on the same rows: n = 2^20 codes of d = 256 bits, clustered
(a centre of 1024 with every bit flipped with probability 0.1), nlist = 1024 trained on a 40960 sample, nq = 256, k = 10.

  search   device time per call between HIP events on the stream of ``search_torch`` -- the quantiser's search, the
           query padding, the mask and work-list kernels, the passes and their merges together -- at nprobe 1 / 8 /
           nlist, and of ``IndexBinaryFlat.search_torch``; mean of --reps calls after a warm-up, the kinds one after the
           other in each of --rounds rounds; the two halves of the call on their own (the quantiser's search for the
           probes, ise_binary_ivf_search_device with the probes given); the 64-row tiles the passes visited per call
           (ise_binary_ivf_stats, the timed calls of ``search_torch`` only) beside the flat pass's; recall@10 against
           the flat result, and at nprobe = nlist whether the results are equal
  build    wall time of ``train``, ``add`` of all rows into both indexes, and the list sizes

One JSON line per round on stdout, appended to --out when given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clustered(rng, centres, n, d, p):
    flip = np.packbits(rng.random((n, d), dtype=np.float32) < p, axis=1, bitorder="little")
    return centres[rng.integers(0, len(centres), n)] ^ flip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from image_search_engine_amd import _native as native
    from image_search_engine_amd import faiss_compat as faiss

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    rng = np.random.default_rng(1)
    centres = rng.integers(0, 256, (a.nlist, a.d // 8), dtype=np.uint8)
    xb = clustered(rng, centres, a.n, a.d, 0.1)
    xq = clustered(rng, centres, a.nq, a.d, 0.1)

    qz = faiss.IndexBinaryFlat(a.d)
    index = faiss.IndexBinaryIVF(qz, a.d, a.nlist)
    index.cp.niter = 5
    t0 = time.time()
    index.train(xb[:40 * a.nlist])
    t1 = time.time()
    index.add(xb)
    t2 = time.time()
    flat = faiss.IndexBinaryFlat(a.d)
    flat.add(xb)
    sizes = np.array([index.list_size(l) for l in range(a.nlist)])
    emit({"n": a.n, "d": a.d, "nlist": a.nlist, "nq": a.nq, "k": a.k, "train_s": round(t1 - t0, 2), "add_s": round(t2 - t1, 2),
          "list_rows_min": int(sizes.min()), "list_rows_max": int(sizes.max()), "empty_lists": int((sizes == 0).sum()),
          "tiles": int(((sizes + 63) // 64).sum()), "flat_tiles": (a.n + 63) // 64})
    xq_dev = torch.from_numpy(xq).cuda()

    def timed(fn):
        for _ in range(a.warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3  # us per call

    Df, If = flat.search_torch(xq_dev, a.k)
    groups = (a.nq + 15) // 16
    for rnd in range(a.rounds):
        row = {"round": rnd, "flat_us": round(timed(lambda: flat.search_torch(xq_dev, a.k)), 1),
               "flat_tiles_per_call": groups * ((a.n + 63) // 64)}
        for nprobe in (1, 8, a.nlist):
            index.nprobe = nprobe
            before = index.binary_ivf_stats()
            row[f"ivf_nprobe{nprobe}_us"] = round(timed(lambda: index.search_torch(xq_dev, a.k)), 1)
            after = index.binary_ivf_stats()
            row[f"ivf_nprobe{nprobe}_tiles_per_call"] = (after["tiles_loaded"] - before["tiles_loaded"]) // (a.warm + a.reps)
            # the two halves of that call on their own: the quantiser's search for the probes, the lists' passes
            row[f"quantizer_nprobe{nprobe}_us"] = round(timed(lambda: qz.search_torch(xq_dev, nprobe)), 1)
            probes = qz.search_torch(xq_dev, nprobe)[1].contiguous()
            D1, I1 = torch.empty_like(Df), torch.empty_like(If)
            st = torch.cuda.current_stream().cuda_stream
            row[f"lists_nprobe{nprobe}_us"] = round(timed(lambda: native.check(native.lib.ise_binary_ivf_search_device(
                index._h, xq_dev.data_ptr(), a.nq, a.k, probes.data_ptr(), nprobe, D1.data_ptr(), I1.data_ptr(), st))), 1)
            D1, I1 = index.search_torch(xq_dev, a.k)
            if nprobe == a.nlist:
                row["nprobe_nlist_equals_flat"] = bool(torch.equal(D1, Df) and torch.equal(I1, If))
            else:
                row[f"recall_nprobe{nprobe}"] = round(float((I1[:, :, None] == If[:, None, :]).any(2).float().mean()), 4)
        emit(row)


if __name__ == "__main__":
    main()
