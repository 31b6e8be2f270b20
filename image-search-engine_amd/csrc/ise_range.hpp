// ise_range.hpp -- range search: EVERY row within a radius, per query (Faiss's IndexFlat::range_search).
//
// One streaming pass over the index per group of 16 queries (one MFMA query tile, grid.y), on the scan
// kernel's arithmetic (ise_scan.hpp), so that every reported distance has the bits search() reports for the
// same (query, row) pair:
//   float32 L2   the row is keyed by the scan's rigorous lower bound lo (l2_lower_bound around mu).  lo >= radius
//                proves d >= lo >= radius: the row is out.  Any other row (an overflowing norm's -FLT_MAX key
//                included; a NaN lo never) is re-evaluated at once with the verifier's direct difference
//                d() (exact_l2_rows, ise_exact.hpp) and kept iff d < radius.  The result does not depend on mu.
//   inner product the dot product of the scan's two-accumulator v_mfma_f32_16x16x4f32 chain (float32) or
//                v_mfma_f32_16x16x32_bf16 chain (bf16), kept iff dot > radius.
//   bf16 L2      the scan's expanded form |x|^2 + |y|^2 - 2 x.y clamped at 0 (NaN kept), kept iff < radius;
//                queries are rounded to bf16 and |x|^2 is summed in the scan's order (threads per query row
//                and vector / scalar staging as the streaming kernel picks them for this index).
// Plain float comparisons: a NaN distance or radius keeps nothing, and the +-FLT_MAX gate of search() does not
// apply.
//
// Output order without a sort: block b owns the contiguous row tiles [b tpb, (b+1) tpb), its wave w the
// contiguous sub-slab w of those, and a wave visits its rows in ascending order.  Segment s = b W + w of a
// query therefore holds ascending ids, and concatenating the segments in s order gives the query's list.
//   pass 1 (mode 0)  each wave writes its hits per query into a staging segment of `cap` entries and records
//                    its full hit count, past the capacity too;
//   range_offsets    per query, an exclusive scan of the segment counts (+ an overflow flag);
//   range_lims       an exclusive scan of the query totals: lims.  The host reads lims (one synchronisation)
//                    and sizes the output;
//   range_compact    copies the segments to their offsets -- or, when a segment overflowed, pass 2 (mode 1)
//                    reads the index again and writes every hit straight to its now exact offset.
//
// The query staging, a tile's dot products and a pair's value are device functions (range_stage_queries,
// range_tile_dots, range_pair_value) that the masked k-best pass of ise_sel_scan.hpp calls too; MASK instantiations of
// this kernel restrict the pass to a selector's window and bitmap.
#pragma once
#include "ise_common.hpp"
#include "ise_exact.hpp"

#define RANGE_W 8 /* waves per block */

struct RangeParams {
    const void* xb;       // [cap][dp] float32 or bf16 rows
    const float* norms;   // [cap] |y - mu|^2 (L2)
    const float* mu;      // [dp] shift vector (float32 L2), zero padded
    const float* q;       // [nq][dp] float32 queries, zero padded to dp
    long long n;
    int d, dp, qs_stride, row_slots, nq, metric;
    int tpr, vec_q;       // query staging of the streaming kernel for this index: threads per query row, vector path
    float beta, radius;
    int tiles_total, tiles_per_block;
    int nseg;             // segments per query = gridDim.x * RANGE_W
    int cap;              // staging entries per segment
    int g0;               // first query group of this launch
    int mode;             // 0: stage + count, 1: write at the exact offsets
    unsigned* cnt;        // [nq][nseg] hits per segment (mode 0)
    float* sD;            // [nq][nseg][cap] staged distances (mode 0)
    uint32_t* sI;         // [nq][nseg][cap] staged row ids (mode 0)
    const long long* lims;    // [nq + 1] (mode 1)
    const long long* segoff;  // [nq][nseg] offset of a segment within its query (mode 1)
    float* D;             // [total] (mode 1)
    long long* I;         // [total] (mode 1)
    // MASK instantiations (a selector, ise_sel_scan.hpp): one bit per row, and the first tile of the selector's
    // window -- blocks then split the tiles [tile0, tiles_total)
    const uint32_t* bits;
    int tile0;
};

__host__ __device__ constexpr size_t range_lds_bytes(int S) {
    return (size_t)S * 4 /* mus */ + (size_t)16 * S * 4 /* qs */ + 16 * 4 /* xn */;
}

// ---- the pieces the range pass shares with the masked k-best pass (ise_sel_scan.hpp): both call these, so a
// (query, row) pair has the same bits in either
// the half-word of mask bits of one 16-row tile (bit r: row 16 tile + r)
__device__ __forceinline__ uint32_t sel_tile_bits(const uint32_t* bits, int tile) {
    return (bits[tile >> 1] >> ((tile & 1) << 4)) & 0xFFFFu;
}

// what the staging reads of an index and a query batch
struct RangeStage {
    const float* q;   // [nq][dp] float32 queries, zero padded to dp
    const float* mu;  // [dp] (SHIFT)
    int d, dp, S, tpr, vec_q;
};

// Query staging of the 16 queries from q0 (nqt of them real) into mus [S] | qs [16][S] | xn [16].  No barrier.
template <bool BF16, bool SHIFT>
__device__ __forceinline__ void range_stage_queries(const RangeStage p, int q0, int nqt, float* mus, float* qs, float* xn) {
    const int tid = threadIdx.x;
    const int S = p.S;
    // ---- query staging: the streaming kernel's values and |x|^2 summation order (ise_scan.hpp, step 2):
    // TPR threads per query row, thread t taking 16-byte slots (vector path) or 4-byte units (scalar path)
    // t, t + TPR, ..., then an xor butterfly over the TPR threads
    const int TPR = p.tpr;
    const int S4 = S >> 2;
    auto to_bf16_pair = [](float lo, float hi) -> uint32_t {
        const __bf16 a = (__bf16)lo, b = (__bf16)hi;
        return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
    };
    auto bf16_round = [](float v) -> float { return (float)(__bf16)v; };
    if (tid < 16 * TPR) {
        const int cc = tid / TPR, t = tid % TPR;
        const bool rowok = cc < nqt;
        const float* src = p.q + (size_t)(q0 + (rowok ? cc : 0)) * p.dp;  // zero padded: reads below dp need no test
        auto qval = [&](int j) -> float { return (rowok && j < p.d) ? src[j] : 0.f; };
        auto muval = [&](int j) -> float { return (SHIFT && j < p.d) ? p.mu[j] : 0.f; };
        float sn = 0.f;
        if (p.vec_q) {
            for (int j4 = t; j4 < S4; j4 += TPR) {
                if (BF16) {
                    float v0[4], v1[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        v0[e] = qval(8 * j4 + e);
                        v1[e] = qval(8 * j4 + 4 + e);
                    }
                    u32x4 o;
                    o[0] = to_bf16_pair(v0[0], v0[1]);
                    o[1] = to_bf16_pair(v0[2], v0[3]);
                    o[2] = to_bf16_pair(v1[0], v1[1]);
                    o[3] = to_bf16_pair(v1[2], v1[3]);
                    *reinterpret_cast<u32x4*>(qs + cc * S + 4 * j4) = o;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float r0 = bf16_round(v0[e]), r1 = bf16_round(v1[e]);
                        sn = fmaf(r0, r0, sn);
                        sn = fmaf(r1, r1, sn);
                    }
                } else {
                    f32x4 x, v;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        x[e] = qval(4 * j4 + e);
                        const float m = muval(4 * j4 + e);
                        v[e] = rowok ? x[e] - m : 0.f;  // padding rows stay zero
                        if (SHIFT && cc == 0) mus[4 * j4 + e] = m;
                    }
                    *reinterpret_cast<f32x4*>(qs + cc * S + 4 * j4) = v;
                    sn = fmaf(v[0], v[0], sn);
                    sn = fmaf(v[1], v[1], sn);
                    sn = fmaf(v[2], v[2], sn);
                    sn = fmaf(v[3], v[3], sn);
                    if (SHIFT) sn += nonfinite_mark(x);  // a non-finite entry: |x - mu|^2 = NaN
                }
            }
        } else {
            for (int j = t; j < S; j += TPR) {
                if (BF16) {
                    const float lo = qval(2 * j), hi = qval(2 * j + 1);
                    reinterpret_cast<uint32_t*>(qs)[cc * S + j] = to_bf16_pair(lo, hi);
                    const float r0 = bf16_round(lo), r1 = bf16_round(hi);
                    sn = fmaf(r0, r0, sn);
                    sn = fmaf(r1, r1, sn);
                } else {
                    const float x = qval(j), m = muval(j);
                    const float v = (rowok && j < p.d) ? x - m : 0.f;
                    qs[cc * S + j] = v;
                    if (SHIFT && cc == 0) mus[j] = m;
                    sn = fmaf(v, v, sn);
                    if (SHIFT) sn += nonfinite_mark(x);
                }
            }
        }
        for (int o = TPR / 2; o > 0; o >>= 1) sn += __shfl_xor(sn, o);
        if (t == 0) xn[cc] = sn;
    }
}

// the scan's dot products for (row 16 tile + 4 g + j, query c): two accumulator chains, k-steps in order
template <int CH, bool BF16, bool SHIFT>
__device__ __forceinline__ f32x4 range_tile_dots(const void* xb, int tile, int row_slots, int c, int g, const float* qrow,
                                                 const float* mus) {
    const int nsteps = row_slots >> 2;
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    const char* base = static_cast<const char*>(xb) + ((((size_t)tile * 16 + c) * row_slots + g) << 4);
    for (int s0 = 0; s0 < nsteps; s0 += CH) {
        f32x4 a[CH];
#pragma unroll
        for (int s = 0; s < CH; s++) a[s] = *reinterpret_cast<const f32x4*>(base + 64 * (s0 + s));
#pragma unroll
        for (int s = 0; s < CH; s++) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(qrow + 16 * (s0 + s));
            if (BF16) {
                const bf16x8 av = __builtin_bit_cast(bf16x8, a[s]), bv = __builtin_bit_cast(bf16x8, b);
                if (s & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc1, 0, 0, 0);
                else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc0, 0, 0, 0);
            } else {
                f32x4 as = a[s];
                if (SHIFT) as = as - *reinterpret_cast<const f32x4*>(mus + 4 * g + 16 * (s0 + s));
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(as[0], b[0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(as[1], b[1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(as[2], b[2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(as[3], b[3], acc1, 0, 0, 0);
            }
        }
    }
    return acc0 + acc1;
}

// one pair's value as both passes test it.  L2: the float32 rows' lower bound lo (SHIFT), or the expanded form
// clamped at 0 (NaN kept; Faiss: if (dis < 0) dis = 0); inner product: the dot product
template <bool SHIFT>
__device__ __forceinline__ float range_pair_value(bool l2, float beta, float xq_n, float yn, float dot) {
    if (l2) {
        const float tt = xq_n + yn;
        const float sc = tt - 2.f * dot;
        if (SHIFT) return l2_lower_bound(beta, tt, sc);
        return sc < 0.f ? 0.f : sc;
    }
    return dot;
}

// MASK: restricted to a selector (ise_sel_scan.hpp) -- the blocks split the tiles of its window [tile0, tiles_total), a
// tile whose 16 mask bits are all zero is not loaded, and a row is a hit only if its bit is set.  The segment layout
// and the ascending order within a segment are those of the unmasked pass.
template <int CH, bool BF16, bool SHIFT, bool MASK = false>
__global__ __launch_bounds__(RANGE_W * 64) void range_scan_kernel(const RangeParams p) {
    static_assert(!(BF16 && SHIFT), "the shift is applied to fp32 rows only");
    constexpr int W = RANGE_W;
    extern __shared__ __align__(16) unsigned char smem_rg[];
    const int S = p.qs_stride;
    float* mus = reinterpret_cast<float*>(smem_rg);  // [S]
    float* qs = mus + S;                             // [16][S]
    float* xn = qs + 16 * S;                         // [16]
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int q0 = (p.g0 + (int)blockIdx.y) * 16;
    const int nqt = min(16, p.nq - q0);
    const bool l2 = p.metric == ISE_METRIC_L2;

    range_stage_queries<BF16, SHIFT>(RangeStage{p.q, p.mu, p.d, p.dp, S, p.tpr, p.vec_q}, q0, nqt, mus, qs, xn);
    __syncthreads();

    // ---- this wave's contiguous sub-slab of the block's row tiles
    const int t0 = (MASK ? p.tile0 : 0) + blockIdx.x * p.tiles_per_block;
    const int t1 = min(t0 + p.tiles_per_block, p.tiles_total);
    const int per_wave = (max(t1 - t0, 0) + W - 1) / W;
    const int tw0 = t0 + w * per_wave, tw1 = min(tw0 + per_wave, t1);
    const int seg = blockIdx.x * W + w;
    const float* qrow = qs + c * S + 4 * g;
    const float xq_n = xn[c];
    const bool qok = c < nqt;
    const size_t segbase = ((size_t)(q0 + (qok ? c : 0)) * p.nseg + seg);
    unsigned cnt = 0;  // hits of query c in this segment (the same in the 4 lanes of query c)

    // one hit of query c (this lane's) at position cnt
    auto emit = [&](float dist, long long row) {
        if (p.mode == 0) {
            if (cnt < (unsigned)p.cap) {
                p.sD[segbase * p.cap + cnt] = dist;
                p.sI[segbase * p.cap + cnt] = (uint32_t)row;
            }
        } else {
            const long long o = p.lims[q0 + c] + p.segoff[segbase] + cnt;
            p.D[o] = dist;
            p.I[o] = row;
        }
    };

    for (int tile = tw0; tile < tw1; tile++) {
        uint32_t tb = 0xFFFFu;
        if (MASK) {
            tb = __builtin_amdgcn_readfirstlane(sel_tile_bits(p.bits, tile));  // wave-uniform, before the tile's loads
            if (tb == 0u) continue;
        }
        const f32x4 dot = range_tile_dots<CH, BF16, SHIFT>(p.xb, tile, p.row_slots, c, g, qrow, mus);
        const f32x4 yn = *reinterpret_cast<const f32x4*>(p.norms + (size_t)tile * 16 + 4 * g);
        const long long row0 = (long long)tile * 16 + 4 * g;
        float val[4];
        u64 m[4];
        u64 any = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            val[j] = range_pair_value<SHIFT>(l2, p.beta, xq_n, yn[j], dot[j]);
            bool pass = l2 ? val[j] < p.radius : val[j] > p.radius;  // false on NaN
            if (MASK) pass = pass && ((tb >> (4 * g + j)) & 1u);
            m[j] = __ballot(pass && qok && row0 + j < p.n);
            any |= m[j];
        }
        if (!any) continue;  // wave-uniform
        // rows in ascending order: row 16 tile + r, r = 4 g' + j, lives in the lanes 16 g' + c
#pragma unroll
        for (int gg = 0; gg < 4; gg++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t hm = (uint32_t)(m[j] >> (16 * gg)) & 0xFFFFu;
                const long long row = (long long)tile * 16 + 4 * gg + j;
                if (SHIFT) {
                    // candidates: the direct difference decides, one wave per (query, row) pair
                    while (hm) {
                        const int qc = __builtin_ctz(hm);
                        hm &= hm - 1;
                        const float* rows[1] = {static_cast<const float*>(p.xb) + (size_t)row * p.dp};
                        float dd[1];
                        exact_l2_rows<1>(rows, p.q + (size_t)(q0 + qc) * p.dp, p.dp, lane, dd);
                        if (dd[0] < p.radius) {  // wave-uniform
                            if (lane == qc) emit(dd[0], row);
                            if (c == qc) cnt++;
                        }
                    }
                } else {
                    if (hm) {
                        const float v = __shfl(val[j], 16 * gg + c);
                        if (g == 0 && ((hm >> c) & 1u)) emit(v, row);
                        cnt += (hm >> c) & 1u;
                    }
                }
            }
    }
    if (p.mode == 0 && g == 0 && qok) p.cnt[segbase] = cnt;
}

// per query (block y): exclusive scan of the segment counts -> segoff, the query's total -> tot; a segment
// past its capacity raises the overflow flag (plain stores of 1)
static __global__ __launch_bounds__(256) void range_offsets_kernel(const unsigned* cnt, int nseg, int cap, long long* segoff,
                                                            long long* tot, unsigned* overflow) {
    __shared__ long long part[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int per = (nseg + 255) / 256;
    const int s0 = min(tid * per, nseg), s1 = min(s0 + per, nseg);
    const unsigned* cq = cnt + (size_t)q * nseg;
    long long sum = 0;
    bool ovf = false;
    for (int s = s0; s < s1; s++) {
        sum += cq[s];
        ovf = ovf || cq[s] > (unsigned)cap;
    }
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive Hillis-Steele scan
        const long long v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = part[tid] - sum;
    for (int s = s0; s < s1; s++) {
        segoff[(size_t)q * nseg + s] = run;
        run += cq[s];
    }
    if (tid == 255) tot[q] = part[255];
    if (ovf) *overflow = 1u;
}

// lims[0] = 0, lims[i + 1] = lims[i] + tot[i] (one block)
static __global__ __launch_bounds__(1024) void range_lims_kernel(const long long* tot, int nq, long long* lims) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int per = (nq + 1023) / 1024;
    const int i0 = min(tid * per, nq), i1 = min(i0 + per, nq);
    long long sum = 0;
    for (int i = i0; i < i1; i++) sum += tot[i];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = part[tid] - sum;
    if (tid == 0) lims[0] = 0;
    for (int i = i0; i < i1; i++) {
        run += tot[i];
        lims[i + 1] = run;
    }
}

// staged segments -> their offsets: one wave per segment (grid.x: segments / 4, grid.y: queries)
static __global__ __launch_bounds__(256) void range_compact_kernel(const unsigned* cnt, const float* sD, const uint32_t* sI,
                                                            const long long* lims, const long long* segoff, int nseg,
                                                            int cap, float* D, long long* I) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), q = blockIdx.y, lane = threadIdx.x & 63;
    if (s >= nseg) return;
    const size_t sg = (size_t)q * nseg + s;
    const int m = (int)min(cnt[sg], (unsigned)cap);
    const long long o = lims[q] + segoff[sg];
    for (int i = lane; i < m; i += 64) {
        D[o + i] = sD[sg * cap + i];
        I[o + i] = (long long)sI[sg * cap + i];
    }
}
