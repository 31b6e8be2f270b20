"""dev build: phase stamps inside merge_kernel<true> (merge + exact re-rank) behind a 1M x 512 scan, ALONE and LOADED -- while a
second index of the same size is searched on 15 other streams, so that the stamps show what a trip to memory costs
under the benchmark's load (scripts/merge_stamp_probe.py is the alone half).
run: ISE_KNN_LIB=.../libise_knn_ablate.so ISE_DEBUG_STAMPS=1 python scripts/merge_stamp_loaded_probe.py"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_search_engine_amd.faiss_compat as faiss
n, d, nq, k = 1_000_000, 512, 16, 10
g = torch.Generator(device="cuda").manual_seed(1)
xb = torch.rand((n, d), generator=g, device="cuda"); xq = torch.rand((nq, d), generator=g, device="cuda")
a = faiss.IndexFlatL2(d); a.add_torch(xb)
b = faiss.IndexFlatL2(d); b.add_torch(xb)
D = torch.empty((nq, k), device="cuda"); I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
outs = [(torch.empty((nq, k), device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda")) for _ in range(15)]
sa = torch.cuda.Stream(); sb = [torch.cuda.Stream() for _ in range(15)]
for _ in range(20):
    a.search_into(xq, k, D, I, sa.cuda_stream)
torch.cuda.synchronize()
print("== alone", flush=True)
for _ in range(6):
    for _ in range(20):
        a.search_into(xq, k, D, I, sa.cuda_stream)
    torch.cuda.synchronize()
    a.exact_stats()
print("== loaded: 15 streams of a second index keep scans running", flush=True)
for _ in range(6):
    for i in range(120):
        b.search_into(xq, k, outs[i % 15][0], outs[i % 15][1], sb[i % 15].cuda_stream)
        if i % 8 == 7 and i < 64:
            a.search_into(xq, k, D, I, sa.cuda_stream)
    torch.cuda.synchronize()
    a.exact_stats()
