"""The workload behind profiles/binary/kernel_stats_nq*.txt: 20 device searches (k = 10) and 10 range
searches with NQ queries against 1M x 64-bit and 1M x 2048-bit codes, to be run under a kernel tracer in a process of
its own, e.g. ``rocprofv3 --kernel-trace --stats -d OUT -- python scripts/binary_trace_workload.py NQ``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import image_search_engine_amd.faiss_compat as faiss

nq = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rng = np.random.default_rng(0)
for d, radius in ((64, 18), (2048, 940)):
    xb = rng.integers(0, 256, (1 << 20, d // 8), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, d // 8), dtype=np.uint8)
    index = faiss.IndexBinaryFlat(d)
    index.add(xb)
    xq_dev = torch.from_numpy(xq).cuda()
    for _ in range(20):
        index.search_torch(xq_dev, 10)
    torch.cuda.synchronize()
    for _ in range(10):
        index.range_search(xq, radius)
print("done")
