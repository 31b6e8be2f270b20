// ise_binary_ivf.hpp -- kernels of IndexBinaryIVF: inverted lists over the bit codes of ise_binary_scan.hpp and the
// Hamming pass that scans only the probed ones (include/ise_knn.h, ise_binary_ivf_*).  Host side:
// ise_binary_ivf.hip.  The launch below (binary_ivf_scan_launch) has a second user: tests/native/binary_ivf_harness.hip
// hands it crafted work lists (tests/test_binary_ivf_lists_gpu.py).
//
// Layout.  All lists live in ONE array: codes [slots][ws] 64-bit words (ws as in ise_binary_scan.hpp: 1, or
// ceil(code_size / 8) rounded up to an even count; the bytes past code_size zero) and ids [slots] uint32 (the row's
// insertion number).  List l owns the 64-row tiles [list_tile0[l], list_tile0[l + 1]) -- a wave's unit in the Hamming
// scan; inside a list the slots are in ascending id order, the slots behind list_size[l] rows are zero codes with id
// 0xFFFFFFFF, masked by position.  A code row carries no row term: a rebuild (ivf_rebuild_launch, ise_ivf_tiles.hpp)
// moves words and ids only, in 8-byte units -- a row of ws == 1 is half a 16-byte unit, and a slot may be odd.
//
// A pass serves one group of BIN_QT = 16 queries and BIN_KPASS = 32 results:
//   masks, work list   the lists' own kernels (ivf_mask_kernel, ivf_offsets_kernel, ivf_work_kernel through
//                      ivf_work_list_launch, ise_ivf_tiles.hpp) with qshift = 4: per group the entries (tile, valid
//                      rows, query mask) of the tiles of the lists that a query of the group probes, in slot order.
//   scan               binary_ivf_scan_kernel: wave w of block b takes entries b BIN_WAVES + w + j gridDim.x BIN_WAVES,
//                      lane l owns slot tile * 64 + l (valid while l < valid rows), hamming16 gives its 16 distances, the
//                      key is bin_key(distance, ids[slot]) -- the id, not the slot, so ties go by ascending id whatever
//                      list a row sits in -- and a query whose bit of the entry's mask is clear is skipped before its
//                      ballot.  Behind that candidate test everything is the flat pass's (binary_scan_body): the LDS
//                      buffers of BIN_CAP keys trimmed by wave_cut, the waves' counts, the block's wave_select,
//                      pass_merge_kernel<int> and the floor-keyed repeat for k > 32.
// The body is this file's own: binary_scan_body and its instantiations are not touched (DESIGN.md 4.18 has their resource
// figures, before and after).
//
// Determinism.  Keys are unique (ids are), a pass's result is the kp smallest keys >= lo over the probed rows, and every
// stage -- a wave's cut (keeps the smallest), the block's wave_select, the merge -- is exact on the key SET it is given:
// what a launch changes is which wave meets which key, never which keys survive.
#pragma once
#include "ise_binary_scan.hpp"
#include "ise_ivf_tiles.hpp"

#define BIN_IVF_TILE 64 /* rows of a list tile: a wave's unit, and the work list's */
#define BIN_IVF_CHUNK 64 /* queries whose work lists are built per launch: BIN_IVF_CHUNK / BIN_QT groups */
static_assert(BIN_IVF_TILE == IVF_WORK_TILE, "ivf_work_kernel counts a tile's valid rows in units of IVF_WORK_TILE");
static_assert(BIN_IVF_CHUNK % BIN_QT == 0 && (1 << 4) == BIN_QT, "groups of 16 queries: qshift = 4");

struct BinIvfScanParams {
    const u64* codes;       // [tiles * 64][ws]
    const uint32_t* ids;    // [tiles * 64]
    int ws;
    const u64* qpad;        // the group's queries, [16][ws] readable
    int nqt, kp;            // queries of the group (<= 16), results of this pass (<= BIN_KPASS)
    const u64* lo;          // [nqt] smallest key admitted (KEY_PAD: the query is finished); null in the first pass: 0
    u64* lists;             // [grid][16][BIN_KPASS]: one sorted list per block and query, KEY_PAD behind the last
    const u32x4* work;      // the group's entries: (tile, valid rows, query mask, 0)
    const uint32_t* count;  // [1] entries of the group
    unsigned long long* tiles_loaded;  // += the entries this pass visits
};

// All 64 lanes are active at every readlane / ballot: what is skipped (a block without an entry, a query that does not
// probe the entry's list) is skipped by whole blocks or whole waves.
template <int WT>
__global__ __launch_bounds__(BIN_WAVES * 64) void binary_ivf_scan_kernel(const BinIvfScanParams p) {
    extern __shared__ __align__(16) unsigned char smem_bin[];
    u64* buf = reinterpret_cast<u64*>(smem_bin);  // [BIN_WAVES][16][BIN_CAP]
    int* cnts = reinterpret_cast<int*>(buf + BIN_WAVES * BIN_QT * BIN_CAP);  // [BIN_WAVES][16] keys held at the end
    u64* qs = buf + BIN_WAVES * BIN_QT * BIN_CAP + BIN_CNT_BYTES / 8;  // WT == 0: [16][ws]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long nent = (long long)__builtin_amdgcn_readfirstlane((int)*p.count);
    if (blockIdx.x == 0 && threadIdx.x == 0 && nent) atomicAdd(p.tiles_loaded, (unsigned long long)nent);
    if ((long long)blockIdx.x * BIN_WAVES >= nent) {  // no entry for this block: its lists are padding
        for (int i = threadIdx.x; i < p.nqt * BIN_KPASS; i += BIN_WAVES * 64)
            p.lists[(size_t)blockIdx.x * BIN_QT * BIN_KPASS + i] = KEY_PAD;
        return;
    }
    BinQueries<WT> qr;
    qr.init(qs, p.qpad, p.ws, p.nqt);
    u64* mybuf = buf + w * BIN_QT * BIN_CAP;
    const int kp = p.kp;
    // per-query state of the wave, query q in lane q: keys held, threshold (a new key must be below it), floor
    int cnt_v = 0;
    u64 thr_v = KEY_PAD;
    const u64 lo_v = lane < p.nqt ? (p.lo ? p.lo[lane] : 0ull) : KEY_PAD;
    const u64 lt_mask = (1ull << lane) - 1ull;

    // query q's buffer is nearly full (more than BIN_CAP - 64 >= BIN_CUT_MAX keys): keep between kp and kmax of them,
    // unsorted; everything kept is <= the cut key, which becomes the threshold
    const int kmax = kp + kp / 2 + 4 < BIN_CUT_MAX ? kp + kp / 2 + 4 : BIN_CUT_MAX;
    auto cut = [&](int q) {
        const int cnt = __builtin_amdgcn_readlane(cnt_v, q);
        u64 kk[2];
#pragma unroll
        for (int e = 0; e < 2; e++) kk[e] = lane + 64 * e < cnt ? mybuf[q * BIN_CAP + lane + 64 * e] : KEY_PAD;
        u64 ckey = KEY_PAD;
        const int nw = wave_cut<2>(kk, BIN_CAP, kp, kmax, mybuf + q * BIN_CAP, &ckey);
        wave_lds_fence();
        if (lane == q) {
            cnt_v = nw;
            thr_v = ckey;
        }
    };

    for (long long e = (long long)blockIdx.x * BIN_WAVES + w; e < nent; e += (long long)gridDim.x * BIN_WAVES) {
        const u32x4 ent = p.work[e];  // e is wave-uniform
        const long long tile = (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)ent[0]);
        const int nvalid = __builtin_amdgcn_readfirstlane((int)ent[1]);
        const uint32_t qm = (uint32_t)__builtin_amdgcn_readfirstlane((int)ent[2]);
        const long long slot = tile * BIN_IVF_TILE + lane;
        const bool valid = lane < nvalid;
        const uint32_t id = p.ids[slot];  // the slots are whole tiles: a pad slot reads ~0 and is masked by position
        int acc[BIN_QT];
        hamming16<WT>(p.codes, p.ws, slot, valid, qr, acc);
#pragma unroll
        for (int q = 0; q < BIN_QT; q++) {
            if (q < p.nqt && ((qm >> q) & 1u)) {  // wave-uniform: a query that does not probe this list casts no ballot
                const u64 key = bin_key(acc[q], (long long)id);
                const bool c = valid && key >= readlane_u64(lo_v, q) && key < readlane_u64(thr_v, q);
                const u64 m = __ballot(c);
                if (m) {
                    const int cnt = __builtin_amdgcn_readlane(cnt_v, q);
                    if (c) mybuf[q * BIN_CAP + cnt + __popcll(m & lt_mask)] = key;
                    if (lane == q) cnt_v += __popcll(m);
                }
            }
        }
        wave_lds_fence();
        u64 need = __ballot(cnt_v > BIN_CAP - 64);  // the next tile may not fit
        while (need) {
            const int q = __ffsll((long long)need) - 1;
            need &= need - 1;
            cut(q);
        }
    }
    if (lane < BIN_QT) cnts[w * BIN_QT + lane] = cnt_v;
    __syncthreads();
    // the waves' buffers -> the block's sorted list
    for (int q = w; q < p.nqt; q += BIN_WAVES) {
        u64 kk[2 * BIN_WAVES];
#pragma unroll
        for (int e = 0; e < 2 * BIN_WAVES; e++) {
            const int sw = e >> 1, i = lane + 64 * (e & 1);
            kk[e] = i < cnts[sw * BIN_QT + q] ? buf[(sw * BIN_QT + q) * BIN_CAP + i] : KEY_PAD;
        }
        u64* dst = p.lists + ((size_t)blockIdx.x * BIN_QT + q) * BIN_KPASS;
        u64 kth_unused = 0;
        const int nw = wave_select<2 * BIN_WAVES>(kk, BIN_WAVES * BIN_CAP, kp, dst, &kth_unused);
        for (int i = nw + lane; i < kp; i += 64) dst[i] = KEY_PAD;
    }
}

// One pass's scan on st: grid blocks of the kernel for wt = 1, 2 (ws words a row) or 0 (any longer row, the queries in
// LDS: [16][ws] words behind the buffers and the counts).  The caller takes hipGetLastError()
inline void binary_ivf_scan_launch(int wt, unsigned grid, int ws, hipStream_t st, const BinIvfScanParams& sp) {
    static LdsAttrOnce attr[3];
    const size_t lds = BIN_BUF_BYTES + BIN_CNT_BYTES + (wt == 0 ? (size_t)BIN_QT * ws * 8 : 0);
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), BIN_LDS_MAX);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(BIN_WAVES * 64), lds, st, sp);
    };
    if (wt == 1) go(binary_ivf_scan_kernel<1>, attr[0]);
    else if (wt == 2) go(binary_ivf_scan_kernel<2>, attr[1]);
    else go(binary_ivf_scan_kernel<0>, attr[2]);
}
