"""In-kernel phase stamps of the scan kernel (dev aid; ablate build + ISE_STAMPS).
usage: ISE_KNN_LIB=.../libise_knn_ablate.so python scripts/stamp_probe.py [n:nq ...]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_search_engine_amd.faiss_compat as faiss
d, k = 512, 10
shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(125_000, 16), (1_000_000, 16), (1_000_000, 32), (1_000_000, 48)]
for n, nq in shapes:
    xb = torch.rand((n, d), device="cuda"); xq = torch.rand((nq, d), device="cuda")
    index = faiss.IndexFlatL2(d); index.add_torch(xb)
    for _ in range(5): index.search_torch(xq, k)
    st = torch.zeros((1024 * 8 * 16,), dtype=torch.int64, device="cuda")
    b0, h0 = index.byte_stats()["byte_batches"], index.half_stats()["half_batches"]
    os.environ["ISE_STAMPS"] = str(st.data_ptr())
    index.search_torch(xq, k); torch.cuda.synchronize()
    os.environ.pop("ISE_STAMPS")
    b1, h1 = index.byte_stats()["byte_batches"], index.half_stats()["half_batches"]
    route = "byte shadow" if b1 > b0 else ("fp16 shadow" if h1 > h0 else "own rows")  # half_batches counts both shadows
    s = st.cpu().numpy().reshape(1024, 8, 16).astype(np.float64)
    used = s[:, :, 0].max(axis=1) > 0
    s = s[used]                      # [blocks][waves][stamps]
    t0 = s[:, :, 0].min()
    us = (s - t0) / 100.0            # 100 MHz -> us
    names = ["entry", "staged", "boot in", "boot out", "loop end", "final barrier", "exit"]
    clk = (s[:, :, 9] - s[:, :, 8]) / np.maximum(s[:, :, 4] - s[:, :, 1], 1) * 100.0  # MHz
    print(f"n={n} nq={nq}: route of the stamped search: {route};  blocks={s.shape[0]}  in-kernel clock over the main loop: median {np.median(clk):.0f} MHz (min {clk.min():.0f}, max {clk.max():.0f})")
    for i, nm in enumerate(names):
        v = us[:, :, i]
        print(f"  {nm:14s} min {v.min():8.2f}  median {np.median(v):8.2f}  max {v.max():8.2f} us")
    print(f"  per-wave final phase (exit - final barrier): median {np.median(us[:,:,6]-us[:,:,5]):.2f} max {(us[:,:,6]-us[:,:,5]).max():.2f}")
    print(f"  per-wave boot (out - in): median {np.median(us[:,:,3]-us[:,:,2]):.2f} max {(us[:,:,3]-us[:,:,2]).max():.2f}")
    print(f"  boot: wait for block (barrier1 - in): median {np.median(us[:,:,7]-us[:,:,2]):.2f} max {(us[:,:,7]-us[:,:,2]).max():.2f};"
          f" select+barrier2 (out - barrier1): median {np.median(us[:,:,3]-us[:,:,7]):.2f} max {(us[:,:,3]-us[:,:,7]).max():.2f}")
    # boot, finer (stamps 10-13; zero where the path does not set them).  Seeded boot (byte shadow, one query tile):
    # 2 first tile scored, 7 minimum folded / published, 10 second tile scored, 11 past the barrier, 12 exchange read
    # + selection of the wave's first query done, 13 that query seeded, 3 boot out.  Boot with the cut: 12 / 13 are the
    # start and end of exchange() (both queries of the wave).
    def diff(a, b):
        ok = (s[:, :, a] > 0) & (s[:, :, b] > 0)
        v = (s[:, :, a] - s[:, :, b])[ok] / 100.0
        return f"median {np.median(v):.2f} max {v.max():.2f} ({ok.sum()} waves)" if ok.any() else "not stamped"
    if (s[:, :, 10] > 0).any():  # the seeded boot ran (stamp 10 is its alone)
        print(f"  seeded boot: fold + publish (7 - 2): {diff(7, 2)}; second tile (10 - 7): {diff(10, 7)}; barrier wait (11 - 10): {diff(11, 10)}")
        print(f"  seeded boot: exchange of one query (12 - 11): {diff(12, 11)}; seeding it (13 - 12): {diff(13, 12)}; second query + barrier (3 - 13): {diff(3, 13)}")
    else:
        print(f"  boot with the cut: exchange() of two queries (13 - 12): {diff(13, 12)}; boot out to exchange start (12 - 3): {diff(12, 3)}")
    print(f"  barrier wait (final barrier - loop end): median {np.median(us[:,:,5]-us[:,:,4]):.2f} max {(us[:,:,5]-us[:,:,4]).max():.2f}")
    del index, xb
