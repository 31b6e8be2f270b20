"""The workload behind profiles/pq/kernel_stats.txt: 20 device searches (k = 10) with 16 queries
against 1M x 512 Gaussian rows coded with M = 16 and with M = 64 (random centroids: the scan's work does not depend on
them), to be run under a kernel tracer in a process of its own, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python scripts/pq_trace_workload.py``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import image_search_engine_amd.faiss_compat as faiss

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(0)
xb = torch.randn((1 << 20, 512), generator=g, device=dev)
xq = torch.randn((16, 512), generator=g, device=dev)
for M in (16, 64):
    index = faiss.IndexPQ(512, M, 8)
    index.pq.set_centroids(torch.randn((M, 256, 512 // M), generator=g, device=dev).cpu().numpy())
    index.add_torch(xb)
    for _ in range(20):
        index.search_torch(xq, 10)
    torch.cuda.synchronize()
print("done")
