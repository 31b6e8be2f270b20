"""Host time of one search_into call (dev aid): 64 calls issued round-robin on 16 streams behind a synchronise,
timed before anything waits; median and p10/p90 per call over 40 such bursts.  $ISE_SCAN_DEPTH / $ISE_KNN_LIB select
the plan rule and the build."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_search_engine_amd.faiss_compat as faiss
d, k, nq, n = 512, 10, 16, 1_000_000
xb = torch.rand((n, d), device="cuda"); xq = torch.rand((nq, d), device="cuda")
index = faiss.IndexFlatL2(d); index.add_torch(xb)
streams = [torch.cuda.Stream() for _ in range(16)]
outs = [(torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda")) for _ in streams]
index.reserve(nq, k)
per = []
for burst in range(45):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(64):
        index.search_into(xq, k, outs[i % 16][0], outs[i % 16][1], streams[i % 16].cuda_stream)
    per.append((time.perf_counter() - t) / 64 * 1e6)
torch.cuda.synchronize()
per = np.array(per[5:])
st = index.depth_stats() if hasattr(index, "depth_stats") else {}
print(f"search_into host time per call: median {np.median(per):.2f} us (p10 {np.percentile(per, 10):.2f}, p90 {np.percentile(per, 90):.2f}); depth stats {st}")
