// ise_sel_scan.hpp -- selector-filtered search: the k best rows AMONG THOSE A SELECTOR NAMES (Faiss's
// SearchParameters(sel=...)), and the kernels that build a selector's device bitmap.
//
// A selector (ise_selector_t, ise_knn.hip) is a device bitmap of uint32 words, one bit per row: bit r & 31 of
// word r >> 5, so the 16 rows of an MFMA row tile are one half-word.  With it go the row WINDOW [r0, r1) from the
// first to the last selected row, the selected count and the number of non-empty tiles.
//
// sel_scan_kernel makes one pass per group of 16 queries (grid.y) over the row tiles of the window only:
//   work split   block b owns a contiguous slab of the window's tiles, its wave w a contiguous sub-slab, visited in
//                ascending order.  A clustered selection unbalances the blocks: accepted.
//   tile skip    a tile whose 16 mask bits are all zero is NOT LOADED: the half-word is read wave-uniformly before
//                the tile's loads are issued.
//   scoring      the range pass's device functions (ise_range.hpp: range_stage_queries, range_tile_dots,
//                range_pair_value), so a (query, row) pair has the bits search() and range_search() report.
//   selection    each wave keeps a sorted list of its kpass <= 32 best packed keys ord(score) << 32 | row per query
//                (LDS, lane i owns entry i: insertion by ballot rank, as ise_exact_scan.hpp).  A row enters only if
//                its mask bit is set, row < n and its score is strictly better than +-FLT_MAX: search()'s rule.
//                float32 L2: the row is keyed by the lower bound lo.  lo >= tau, the k-th exact distance of a FULL
//                list, proves the row out (d >= lo >= tau, and at d == tau the larger id loses the tie: a wave
//                visits its rows in ascending order).  Any other row (an overflowing norm's -FLT_MAX key included;
//                a NaN lo never) is re-evaluated at once with exact_l2_rows, and d is what enters the list: the
//                result is exact by construction -- no certificate, no fallback, no dependence on mu.
//                inner product / bf16 L2: the chain's value (minus the dot product; the clamped expanded form).
//   merge        the 8 wave lists of a query become the block's list (wave_select over 256 keys), written to
//                part [group][block][16][kpass]; merge_kernel (ise_merge.hpp) folds the blocks' lists.
//   k > 32       one pass per 32 results, floor-keyed with the last key of the previous pass (sel_scatter_kernel),
//                the scheme of exact_scan_kernel.
#pragma once
#include "ise_exact_scan.hpp"
#include "ise_range.hpp"

#define SEL_W RANGE_W    /* waves per block */
#define SEL_KPASS_MAX 32 /* = XPASS_MAX: most results per query of one pass */

struct SelScanParams {
    const void* xb;       // [cap][dp] float32 or bf16 rows
    const float* norms;   // [cap] |y - mu|^2 (L2)
    const float* mu;      // [dp] shift vector (float32 L2), zero padded
    const float* q;       // [nq][dp] float32 queries, zero padded to dp
    const uint32_t* bits; // the selector's bitmap
    long long n;
    int d, dp, qs_stride, row_slots, nq, metric;
    int tpr, vec_q;       // query staging of the streaming kernel for this index (as RangeParams)
    float beta;
    int tile0, tile1;     // the window's tiles
    int tiles_per_block;
    int kpass;            // <= SEL_KPASS_MAX, and as many as the wave lists' LDS holds beside the queries
    const u64* floor_keys;  // [nq] or null: only keys above it enter (k > 32)
    u64* part;            // [groups][gridDim.x][16][kpass] sorted keys per block
};

__host__ __device__ constexpr size_t sel_lds_bytes(int S, int kpass) {
    return range_lds_bytes(S) + (size_t)SEL_W * 16 * kpass * 8 /* wave lists */;
}

template <int CH, bool BF16, bool SHIFT>
__global__ __launch_bounds__(SEL_W * 64) void sel_scan_kernel(const SelScanParams p) {
    static_assert(!(BF16 && SHIFT), "the shift is applied to fp32 rows only");
    constexpr int W = SEL_W;
    extern __shared__ __align__(16) unsigned char smem_sl[];
    const int S = p.qs_stride;
    float* mus = reinterpret_cast<float*>(smem_sl);  // [S]
    float* qs = mus + S;                             // [16][S]
    float* xn = qs + 16 * S;                         // [16]
    u64* lists = reinterpret_cast<u64*>(xn + 16);    // [W][16][kp]; S is a multiple of 4: 8-byte aligned
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int q0 = (int)blockIdx.y * 16;
    const int nqt = min(16, p.nq - q0);
    const bool l2 = p.metric == ISE_METRIC_L2;
    const int kp = p.kpass;

    range_stage_queries<BF16, SHIFT>(RangeStage{p.q, p.mu, p.d, p.dp, S, p.tpr, p.vec_q}, q0, nqt, mus, qs, xn);
    u64* wl = lists + (size_t)w * 16 * kp;  // this wave's lists: lane i < kp owns entry i of each
    for (int i = lane; i < 16 * kp; i += 64) wl[i] = KEY_PAD;
    __syncthreads();

    const int t0 = p.tile0 + blockIdx.x * p.tiles_per_block;
    const int t1 = min(t0 + p.tiles_per_block, p.tile1);
    const int per_wave = (max(t1 - t0, 0) + W - 1) / W;
    const int tw0 = t0 + w * per_wave, tw1 = min(tw0 + per_wave, t1);
    const float* qrow = qs + c * S + 4 * g;
    const float xq_n = xn[c];
    const bool qok = c < nqt;
    u64 tau = TAU0;  // query c's k-th key once its list is full (the same in the 4 lanes of query c)
    const u64 flo = p.floor_keys ? p.floor_keys[q0 + (qok ? c : 0)] : 0ull;

    // key kj of query qc (wave-uniform both) into the wave's list, if it is among the kp smallest
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

    for (int tile = tw0; tile < tw1; tile++) {
        const uint32_t tb = __builtin_amdgcn_readfirstlane(sel_tile_bits(p.bits, tile));
        if (tb == 0u) continue;  // wave-uniform, before the tile's loads: an empty tile is not read
        const f32x4 dot = range_tile_dots<CH, BF16, SHIFT>(p.xb, tile, p.row_slots, c, g, qrow, mus);
        const f32x4 yn = *reinterpret_cast<const f32x4*>(p.norms + (size_t)tile * 16 + 4 * g);
        const long long row0 = (long long)tile * 16 + 4 * g;
        const float tau_d = unord_f32((uint32_t)(tau >> 32));  // FLT_MAX while the list is not full
        float val[4];
        bool sel[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            val[j] = range_pair_value<SHIFT>(l2, p.beta, xq_n, yn[j], dot[j]);
            sel[j] = ((tb >> (4 * g + j)) & 1u) && qok && row0 + j < p.n;
        }
        if constexpr (SHIFT) {
            // val = lo.  lo >= tau_d: out (d >= lo; FLT_MAX while the list is open is search()'s gate); NaN: never
            u64 m[4];
#pragma unroll
            for (int j = 0; j < 4; j++) m[j] = __ballot(sel[j] && val[j] < tau_d);
            if (!(m[0] | m[1] | m[2] | m[3])) continue;  // wave-uniform
            // rows in ascending order (the tie rule above): row 16 tile + 4 g' + j lives in the lanes 16 g' + c
#pragma unroll
            for (int gg = 0; gg < 4; gg++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t hm = (uint32_t)(m[j] >> (16 * gg)) & 0xFFFFu;
                    const long long row = (long long)tile * 16 + 4 * gg + j;
                    while (hm) {  // wave-uniform
                        const int qc = __builtin_ctz(hm);
                        hm &= hm - 1;
                        // the list may have tightened since the ballot
                        const float lo = __builtin_bit_cast(
                            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val[j]), 16 * gg + qc));
                        const u64 tq = readlane_u64(tau, qc);
                        if (!(lo < unord_f32((uint32_t)(tq >> 32)))) continue;
                        const float* rows[1] = {static_cast<const float*>(p.xb) + (size_t)row * p.dp};
                        float dd[1];
                        exact_l2_rows<1>(rows, p.q + (size_t)(q0 + qc) * p.dp, p.dp, lane, dd);
                        const u64 kj = ((u64)ord_f32(dd[0]) << 32) | (uint32_t)row;
                        if (dd[0] < FLT_MAX && kj > readlane_u64(flo, qc)) insert(qc, kj);
                    }
                }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float s = l2 ? val[j] : -val[j];
                const u64 kj = ((u64)ord_f32(s) << 32) | (uint32_t)(row0 + j);
                u64 m = __ballot(sel[j] && s < FLT_MAX && kj < tau && kj > flo);
                while (m) {  // wave-uniform; the keys are unique, so the order of insertion does not matter
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    insert(l & 15, readlane_u64(kj, l));
                }
            }
        }
    }
    __syncthreads();
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

// k > 32: one pass's merged keys [nq][kp] into the outputs at column `off`; each query's last key is the floor of
// the next pass (KEY_PAD when the selection ran out: later passes admit nothing)
static __global__ __launch_bounds__(256) void sel_scatter_kernel(const u64* pass_keys, int nq, int kp, int off, int k, int metric,
                                                          float* D, long long* I, u64* floor_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * kp) return;
    const int q = i / kp, r = i - q * kp;
    const u64 key = pass_keys[i];
    if (off + r < k) {
        const bool pad = key == KEY_PAD;
        const float sc = unord_f32((uint32_t)(key >> 32));
        const bool l2 = metric == ISE_METRIC_L2;
        D[(size_t)q * k + off + r] = pad ? (l2 ? FLT_MAX : -FLT_MAX) : (l2 ? sc : -sc);
        I[(size_t)q * k + off + r] = pad ? -1ll : (long long)(uint32_t)key;
    }
    if (r == kp - 1) floor_out[q] = key;
}

// queries [nq][d] -> [nq][dp], zero padded (the staging and exact_l2_rows read whole padded rows)
static __global__ __launch_bounds__(256) void sel_pad_queries_kernel(const float* q, int d, int dp, long long total, float* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long r = i / dp;
    const int j = (int)(i - r * dp);
    out[i] = j < d ? q[(size_t)r * d + j] : 0.f;
}

// ---------------------------------------------------------------- the bitmap
// bits of [i0, i1) set, every other bit of the nwords words clear (the padding words included)
static __global__ __launch_bounds__(256) void sel_fill_range_kernel(uint32_t* bits, long long nwords, long long i0, long long i1) {
    const long long wd = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (wd >= nwords) return;
    const long long a = max(i0, wd * 32) - wd * 32, b = min(i1, wd * 32 + 32) - wd * 32;  // [a, b) within the word
    uint32_t v = 0u;
    if (a < b) v = (b >= 32 ? ~0u : ((1u << b) - 1u)) & ~((1u << a) - 1u);
    bits[wd] = v;
}

// ids in any order, duplicates allowed; ids outside [0, n) are ignored.  set: the bit is raised, else cleared
static __global__ __launch_bounds__(256) void sel_scatter_ids_kernel(uint32_t* bits, const long long* ids, long long n_ids,
                                                              long long n, int set) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ids) return;
    const long long id = ids[i];
    if (id < 0 || id >= n) return;
    const uint32_t b = 1u << (id & 31);
    if (set) atomicOr(bits + (id >> 5), b);
    else atomicAnd(bits + (id >> 5), ~b);
}

// bits at or beyond n cleared (the user's bitmap), then the census: out[0] selected rows, out[1] non-empty tiles,
// out[2] first selected row (init: ~0), out[3] last selected row + 1 (init: 0)
static __global__ __launch_bounds__(256) void sel_census_kernel(uint32_t* bits, long long nwords, long long n, unsigned long long* out) {
    const long long wd = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cnt = 0, tiles = 0, lo = ~0ull, hi = 0;
    if (wd < nwords) {
        uint32_t v = bits[wd];
        const long long left = n - wd * 32;
        if (left < 32) {
            const uint32_t keep = left <= 0 ? 0u : ((1u << left) - 1u);
            if (v & ~keep) bits[wd] = v & keep;
            v &= keep;
        }
        if (v) {
            cnt = (unsigned long long)__popc(v);
            tiles = ((v & 0xFFFFu) ? 1u : 0u) + ((v >> 16) ? 1u : 0u);
            lo = (unsigned long long)(wd * 32 + (__ffs((int)v) - 1));
            hi = (unsigned long long)(wd * 32 + (32 - __clz((int)v)));
        }
    }
    // one atomic per wave and field
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        tiles += __shfl_xor(tiles, o);
        const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(out + 0, cnt);
        atomicAdd(out + 1, tiles);
        atomicMin(out + 2, lo);
        atomicMax(out + 3, hi);
    }
}

// launchers (ise_sel_scan.hip)
void ise_launch_sel_scan(int storage_bf16, int shift, int ch, dim3 grid, size_t lds, hipStream_t st, const SelScanParams& sp);
void ise_launch_range_masked(int storage_bf16, int shift, int ch, dim3 grid, size_t lds, hipStream_t st, const RangeParams& rp);
