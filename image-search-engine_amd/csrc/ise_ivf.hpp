// ise_ivf.hpp -- IndexIVFFlat: inverted lists of float32 rows and the pass that scans only the probed ones
// (Faiss's IndexIVFFlat::search_preassigned).
//
// Layout.  All lists live in ONE row array xb [16 tiles][dp], list l owning the 16-row tiles
// [list_tile0[l], list_tile0[l + 1]): every list starts on a tile boundary, so the tile functions of ise_range.hpp
// run on it unchanged.  Slot s of the array carries ids[s], the row's insertion number (its id), and norms[s] =
// |y - mu|^2 (L2); inside a list the slots are in ascending id order, and the slots behind list_size[l] rows are zero
// padding that every kernel masks by position.  tile_list[t] names the list of tile t.
//
// ivf_scan_kernel makes one pass per group of 16 queries (grid.y).  It is sel_scan_kernel's loop (ise_sel_scan.hpp)
// with the selector's half-word replaced by two tests -- "position < list size" and "this query's bit in the list's
// mask" -- and with these differences:
//   masks        ivf_mask_kernel (ise_ivf_tiles.hpp; groups of 16: qshift 4) turns the probe table [nq][nprobe] into
//                one 16-bit query mask per (group, list); -1 and out-of-range entries set nothing, a duplicate sets
//                its bit twice.
//   work split   the tiles are dealt ROUND-ROBIN: round r gives block b the 8 consecutive tiles from (r blocks + b) 8,
//                wave w the w-th of them, so the tiles of a probed list spread over all blocks however few lists are
//                probed.  (sel_scan_kernel's contiguous slabs would leave one probed list to one or two blocks; they
//                exist for its tie rule, which this kernel does not use -- see pruning.)
//   tile skip    a wave looks up 64 of its tiles at a time, lane i the list (tile_list) and that list's mask of its
//                i-th tile, and visits only the tiles whose mask is not empty: a tile nobody probes is NOT LOADED.
//                The tiles it does load are counted, one atomic add per block (ise_ivf_stats, out3[2]).
//   keys         ord(score) << 32 | ids[slot]: the ORIGINAL id, so results carry ids and ties go by ascending id.
//   pruning      a wave does not meet its rows in ascending id order (a later list may hold a smaller id), so a
//                float32 L2 row is proved out only by lo > tau's distance (d >= lo > tau_d); at lo == tau_d it is
//                re-evaluated and its full key (d, id) decides on insertion.  Inner product compares full keys too.
// Scoring, the wave lists, the block fold, merge_kernel and the floor-keyed repeat for k > 32 are sel_scan_kernel's.
#pragma once
#include "ise_merge.hpp"
#include "ise_sel_scan.hpp"

struct IvfScanParams {
    const float* xb;            // [tiles * 16][dp] rows, list after list
    const float* norms;         // [tiles * 16] |y - mu|^2 (L2)
    const float* mu;            // [dp] shift vector (L2), zero padded
    const float* q;             // [nq][dp] float32 queries, zero padded to dp
    const uint32_t* ids;        // [tiles * 16] insertion number of the row in a slot
    const uint32_t* list_tile0; // [nlist + 1]
    const uint32_t* list_size;  // [nlist] rows
    const uint32_t* tile_list;  // [tiles] the list a tile belongs to
    const uint32_t* masks;      // [groups][nlist] bit c: query 16 group + c probes the list
    int nlist;
    int d, dp, qs_stride, row_slots, nq, metric;
    int tpr, vec_q;             // query staging (RangeStage)
    float beta;
    int tiles_total;
    int kpass;                  // <= SEL_KPASS_MAX
    const u64* floor_keys;      // [nq] or null: only keys above it enter (k > 32)
    u64* part;                  // [groups][gridDim.x][16][kpass] sorted keys per block
    unsigned long long* tiles_loaded;  // += the tiles this launch loaded
};

template <int CH, bool SHIFT>
__global__ __launch_bounds__(SEL_W * 64) void ivf_scan_kernel(const IvfScanParams p) {
    constexpr int W = SEL_W;
    extern __shared__ __align__(16) unsigned char smem_iv[];
    __shared__ unsigned loadedS;
    const int S = p.qs_stride;
    float* mus = reinterpret_cast<float*>(smem_iv);  // [S]
    float* qs = mus + S;                             // [16][S]
    float* xn = qs + 16 * S;                         // [16]
    u64* lists = reinterpret_cast<u64*>(xn + 16);    // [W][16][kp]
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int q0 = (int)blockIdx.y * 16;
    const int nqt = min(16, p.nq - q0);
    const bool l2 = p.metric == ISE_METRIC_L2;
    const int kp = p.kpass;

    range_stage_queries<false, SHIFT>(RangeStage{p.q, p.mu, p.d, p.dp, S, p.tpr, p.vec_q}, q0, nqt, mus, qs, xn);
    u64* wl = lists + (size_t)w * 16 * kp;  // this wave's lists: lane i < kp owns entry i of each
    for (int i = lane; i < 16 * kp; i += 64) wl[i] = KEY_PAD;
    if (tid == 0) loadedS = 0u;
    __syncthreads();

    const float* qrow = qs + c * S + 4 * g;
    const float xq_n = xn[c];
    const bool qok = c < nqt;
    const uint32_t* gm = p.masks + (size_t)blockIdx.y * p.nlist;
    u64 tau = TAU0;  // query c's k-th key once its list is full (the same in the 4 lanes of query c)
    const u64 flo = p.floor_keys ? p.floor_keys[q0 + (qok ? c : 0)] : 0ull;
    unsigned nload = 0;  // wave-uniform

    // key kj of query qc (wave-uniform both) into the wave's list, if it is among the kp smallest: full keys compared
    auto insert = [&](int qc, u64 kj) {
        u64* l = wl + qc * kp;
        const u64 mine = lane < kp ? l[lane] : KEY_PAD;
        const int pos = __popcll(__ballot(mine < kj));
        if (pos >= kp) return;
        const u64 up = shfl_up1_u64(mine);
        const u64 nv = lane < pos ? mine : (lane == pos ? kj : up);
        if (lane < kp) l[lane] = nv;  // a lane reads and writes its own entry only
        const u64 kth = readlane_u64(nv, kp - 1);
        if (c == qc) tau = kth == KEY_PAD ? TAU0 : kth;
    };

    // Tiles are dealt round-robin: round r gives block b the W consecutive tiles from (r gridDim.x + b) W, wave w the
    // w-th of them, so the tiles of a probed list spread over all blocks.  A wave looks up 64 of its tiles at a time --
    // lane i the list and the mask of its i-th tile -- and visits only those somebody probes.
    const int stride = (int)gridDim.x * W;
    for (int base = (int)blockIdx.x * W + w; base < p.tiles_total; base += 64 * stride) {  // wave-uniform throughout
        const long long mine = (long long)base + (long long)lane * stride;
        const bool have = mine < p.tiles_total;
        const uint32_t myl = have ? p.tile_list[mine] : 0u;
        const uint32_t mym = have ? gm[myl] : 0u;
        u64 act = __ballot(mym != 0u);  // nobody probes the list: the tile is not read
        while (act) {
            const int i = __builtin_ctzll(act);
            act &= act - 1;
            const int tile = base + i * stride;
            const int li = __builtin_amdgcn_readlane((int)myl, i);
            const uint32_t qm = (uint32_t)__builtin_amdgcn_readlane((int)mym, i);
            const int lt0 = __builtin_amdgcn_readfirstlane((int)p.list_tile0[li]);
            const int lsz = __builtin_amdgcn_readfirstlane((int)p.list_size[li]);
            const bool probes = qok && ((qm >> c) & 1u);
            nload++;
            const f32x4 dot = range_tile_dots<CH, false, SHIFT>(p.xb, tile, p.row_slots, c, g, qrow, mus);
            const f32x4 yn = *reinterpret_cast<const f32x4*>(p.norms + (size_t)tile * 16 + 4 * g);
            const u32x4 idv = *reinterpret_cast<const u32x4*>(p.ids + (size_t)tile * 16 + 4 * g);
            const int pos0 = (tile - lt0) * 16 + 4 * g;  // position of this lane's first row within the list
            const float tau_d = unord_f32((uint32_t)(tau >> 32));  // FLT_MAX while the list is not full
            float val[4];
            bool sel[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                val[j] = range_pair_value<SHIFT>(l2, p.beta, xq_n, yn[j], dot[j]);
                sel[j] = probes && pos0 + j < lsz;
            }
            if constexpr (SHIFT) {
                // val = lo.  lo > tau_d: out (d >= lo > tau_d); lo == tau_d may still win its tie by id.  NaN: never
                u64 m[4];
#pragma unroll
                for (int j = 0; j < 4; j++) m[j] = __ballot(sel[j] && val[j] <= tau_d);
                if (!(m[0] | m[1] | m[2] | m[3])) continue;  // wave-uniform
#pragma unroll
                for (int gg = 0; gg < 4; gg++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        uint32_t hm = (uint32_t)(m[j] >> (16 * gg)) & 0xFFFFu;
                        const size_t slot = (size_t)tile * 16 + 4 * gg + j;
                        while (hm) {  // wave-uniform
                            const int qc = __builtin_ctz(hm);
                            hm &= hm - 1;
                            // the list may have tightened since the ballot
                            const float lo = __builtin_bit_cast(
                                float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val[j]), 16 * gg + qc));
                            const u64 tq = readlane_u64(tau, qc);
                            if (!(lo <= unord_f32((uint32_t)(tq >> 32)))) continue;
                            const float* rows[1] = {p.xb + slot * p.dp};
                            float dd[1];
                            exact_l2_rows<1>(rows, p.q + (size_t)(q0 + qc) * p.dp, p.dp, lane, dd);
                            const u64 kj = ((u64)ord_f32(dd[0]) << 32) | p.ids[slot];
                            if (dd[0] < FLT_MAX && kj > readlane_u64(flo, qc)) insert(qc, kj);
                        }
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float s = l2 ? val[j] : -val[j];
                    const u64 kj = ((u64)ord_f32(s) << 32) | idv[j];
                    u64 m = __ballot(sel[j] && s < FLT_MAX && kj < tau && kj > flo);
                    while (m) {  // wave-uniform; the keys are unique, so the order of insertion does not matter
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        insert(l & 15, readlane_u64(kj, l));
                    }
                }
            }
        }
    }
    if (lane == 0 && nload) atomicAdd(&loadedS, nload);  // LDS
    __syncthreads();
    if (tid == 0 && loadedS) atomicAdd(p.tiles_loaded, (unsigned long long)loadedS);
    // ---- the block's list of a query: the kp smallest of its 8 wave lists.  Wave w folds queries w and w + 8
    for (int qc = w; qc < 16; qc += W) {
        u64 kk[W * SEL_KPASS_MAX / 64];
#pragma unroll
        for (int e = 0; e < W * SEL_KPASS_MAX / 64; e++) {
            const int i = lane + 64 * e;  // wave i / kp, entry i % kp
            kk[e] = i < W * kp ? lists[((size_t)(i / kp) * 16 + qc) * kp + (i % kp)] : KEY_PAD;
        }
        u64* out = p.part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + qc) * kp;
        u64 kth_unused;
        const int nw = wave_select<W * SEL_KPASS_MAX / 64>(kk, W * kp, kp, out, &kth_unused);
        if (lane >= nw && lane < kp) out[lane] = KEY_PAD;
    }
}

// ---------------------------------------------------------------- rebuild (ise_ivf.hip)
// The rows move and scatter with the lists' own kernels (ivf_rebuild_launch, ise_ivf_tiles.hpp: 16-row tiles, 16-byte
// units); what follows is computed on the new array behind them.
//
// column sums of `rows` padded rows in `groups` row groups, then the mean over n real rows (pad slots are zero):
// fixed order, NaN / inf entries skipped (as the flat index's shift, ise_rows.hpp)
static __global__ __launch_bounds__(256) void ivf_col_sum_kernel(const float* x, long long rows, int d, int dp, int groups,
                                                          float* partial /* [groups][dp] */) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int gidx = blockIdx.y;
    if (j >= dp) return;
    const long long per = (rows + groups - 1) / groups;
    const long long r0 = gidx * per, r1 = min(rows, r0 + per);
    float s = 0.f;
    if (j < d)
        for (long long r = r0; r < r1; r++) {
            const float v = x[(size_t)r * dp + j];
            if (fabsf(v) <= FLT_MAX) s += v;
        }
    partial[(size_t)gidx * dp + j] = s;
}
static __global__ __launch_bounds__(256) void ivf_col_mean_kernel(const float* partial, long long n, int d, int dp, int groups,
                                                           float* mu) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dp) return;
    float s = 0.f;
    for (int gi = 0; gi < groups; gi++) s += partial[(size_t)gi * dp + j];
    const float m = s / (float)n;
    mu[j] = (j < d && fabsf(m) <= FLT_MAX) ? m : 0.f;
}

// |y - mu|^2 per slot, wave per slot: NaN for a row with a NaN or inf entry (ise_common.hpp, nonfinite_mark)
static __global__ __launch_bounds__(256) void ivf_norms_kernel(const float* x, long long slots, int dp, const float* mu,
                                                        float* out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= slots) return;
    const float* xr = x + (size_t)r * dp;
    float s = 0.f;
    for (int j = lane * 4; j < dp; j += 256) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(xr + j);
        const f32x4 v = y - *reinterpret_cast<const f32x4*>(mu + j);
        s = fmaf(v[0], v[0], s);
        s = fmaf(v[1], v[1], s);
        s = fmaf(v[2], v[2], s);
        s = fmaf(v[3], v[3], s);
        s += nonfinite_mark(y);
    }
    s = wave_sum_f32(s);
    if (lane == 0) out[r] = s;
}
