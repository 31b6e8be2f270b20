"""Exact-scan rate of the fp16 shadow filter against the float32 filter on hard distributions at 1M rows
(DESIGN.md 5.0a): per kind, 64 queries near random rows in batches of 16, the queries each filter sent to the exact
scan, the per-batch time of each, and whether both return the same bits.  One JSON line per kind."""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_search_engine_amd.faiss_compat as faiss
from image_search_engine_amd import _native

N, nq, k = int(os.environ.get("N", "1000000")), 64, 10
dev = torch.device("cuda")


def rows(kind, g):
    if kind == "cluster_sorted":        # rows sorted by class: the mean drifts all the way through the index
        d = 128
        c = torch.sort(torch.randint(0, 8, (N,), generator=g, device=dev)).values
        x = (torch.randn((8, d), generator=g, device=dev) * 20.0)[c] + 0.1 * torch.randn((N, d), generator=g, device=dev)
    elif kind == "two_far_clusters":    # 1e3 apart, spread 1e-1
        d = 128
        x = 0.1 * torch.randn((N, d), generator=g, device=dev)
        x[N // 2:, 0] += 1000.0
    elif kind == "near_duplicates":     # 50k groups of ~20 rows 1e-3 apart around uniform centres
        d = 512
        c = torch.rand((N // 20, d), generator=g, device=dev)
        x = c[torch.randint(0, N // 20, (N,), generator=g, device=dev)] + 1e-3 * torch.randn((N, d), generator=g, device=dev)
    elif kind == "cnn_like":            # non-negative ReLU features with a large common component (config 2's shape)
        d = 2048
        base = torch.rand((d,), generator=g, device=dev) * 2.0
        x = torch.relu(base + 0.5 * torch.randn((N, d), generator=g, device=dev))
    elif kind == "uniform":
        d = 512
        x = torch.rand((N, d), generator=g, device=dev)
    else:
        raise ValueError(kind)
    return x.contiguous()


def knob(v):
    if v:
        os.environ["ISE_NO_HALF_FILTER"] = "1"
    else:
        os.environ.pop("ISE_NO_HALF_FILTER", None)
    _native.lib.ise_refresh_env_knobs()


for kind in sys.argv[1:] or ["uniform", "cluster_sorted", "two_far_clusters", "near_duplicates", "cnn_like"]:
    g = torch.Generator(device=dev).manual_seed(11)
    x = rows(kind, g)
    d = x.shape[1]
    index = faiss.IndexFlatL2(d)
    index.add_torch(x)
    q = (x[torch.randint(0, N, (nq,), generator=g, device=dev)] + 0.03 * torch.randn((nq, d), generator=g, device=dev)).contiguous()
    del x
    out = {"kind": kind, "n": N, "d": d, "nq": nq, "k": k}
    res = {}
    for name, off in (("shadow", False), ("float32", True)):
        knob(off)
        index.search_torch(q[:16], k)  # builds the shadow / warms up
        torch.cuda.synchronize()
        e0 = index.exact_stats()["exact_scan"]
        t0 = time.time()
        D, I = [], []
        for q0 in range(0, nq, 16):
            Dq, Iq = index.search_torch(q[q0:q0 + 16], k)
            D.append(Dq); I.append(Iq)
        torch.cuda.synchronize()
        out[name] = {"exact_scan": index.exact_stats()["exact_scan"] - e0 - 0,
                     "ms_per_batch": (time.time() - t0) * 1e3 / (nq // 16)}
        res[name] = (torch.cat(D).cpu().numpy(), torch.cat(I).cpu().numpy())
    knob(False)
    out["half_batches"] = index.half_stats()["half_batches"]
    out["same_bits"] = bool(np.array_equal(res["shadow"][1], res["float32"][1]) and
                            np.array_equal(res["shadow"][0].view(np.uint32), res["float32"][0].view(np.uint32)))
    print(json.dumps(out), flush=True)
    del index
    torch.cuda.empty_cache()
