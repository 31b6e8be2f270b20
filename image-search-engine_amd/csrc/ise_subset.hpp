// ise_subset.hpp -- subset scoring on the flat float32 index: exact scores of a PER-QUERY LIST of row ids, and the k
// best of them (Faiss's IndexRefineFlat re-ranks a base index's k * k_factor labels this way; compute_distance_subset
// hands the scores out as they are).  ise_index_search_subset_* / ise_index_distance_subset_* in include/ise_knn.h.
//
// The workload is a gather: nq x kc rows of dp floats named by id, each read once, little arithmetic (16 queries x
// 1000 candidates x 2 KiB = 32 MB).  One block per query -- the shape of rerank_kernel (ise_exact.hpp), which serves
// at most 36 candidates -- would leave one CU to fetch 2 MB alone, so the work is cut by CANDIDATE and spread over the
// device, and the selection is a second, small launch:
//
//   score   grid (ceil(n2 / SUB_CPB), nq), n2 = pow2(kc).  The block stages its query in LDS (zero padded to dp, as
//           the verifier and the range pass stage it) and scores SUB_CPB = 16 consecutive entries of the query's
//           candidate row:
//             float32 L2     four waves, each with its 4 candidate rows in flight at once, exact_l2_rows
//                            (ise_exact.hpp): the direct-difference value search() reports;
//             inner product  one wave: the tile of 16 gathered rows on the scan's two-accumulator
//                            v_mfma_f32_16x16x4f32 chain (range_tile_dots, ise_range.hpp), the k-steps in the same
//                            order: lane (c, g) reads row cand[c] where the scan reads row 16 tile + c, and all 16
//                            query columns hold the one query, so every column of the result is its dot product.
//           An entry outside [0, n) is not read (row 0 stands in for it in the loads) and scores nothing.  Each entry
//           writes its key ord(score) << 32 | id (of -score for inner product, as ivf_scan_kernel does; KEY_PAD when
//           the entry is ignored or the score is not strictly better than +-FLT_MAX, so NaN never enters) into the
//           workspace [nq][n2], and / or its raw score into dist [nq][kc].  One wave per query also counts the
//           query's valid entries for the statistics (one atomic per query).
//   select  one block per query: block_sort_u64 over the n2 keys (at most 2048 = 16 KiB of LDS), adjacent equal keys
//           -- an id named twice has the same score, hence the same key -- dropped by a prefix sum over the "first of
//           its run" flags, the first k written out.  Ascending key order is (score, id) order: ties by ascending id.
//
// Two launches rather than one with a last-block-finishes step: the hand-off would need a counter per query zeroed on
// the stream (a third node) and an agent-scope acquire in the last block before it reads the others' keys, to save
// one launch gap of a few microseconds on a pass that is bound by the latency of its gathered loads.
#pragma once
#include "ise_common.hpp"
#include "ise_exact.hpp"

#define SUB_W 4      /* waves per L2 score block */
#define SUB_CPB 16   /* candidate entries per score block: 4 rows in flight per wave (L2), one MFMA tile per block (IP) */
#define SUB_SORT_MAX_THREADS 1024

struct SubsetParams {
    const float* xb;        // [cap][dp] float32 rows
    const float* q;         // [nq][d] queries as the caller passed them
    const long long* cand;  // [nq][kc] row ids
    long long n;
    int d, dp, kc, n2;
    int ip;                 // inner product (else squared L2)
    u64* keys;              // [nq][n2] or null
    float* dist;            // [nq][kc] or null: raw scores, +-FLT_MAX for an ignored entry
    unsigned long long* valid;  // [1]: candidate entries inside [0, n) of the calls so far
};

// the block's query into LDS, zero padded to dp
__device__ __forceinline__ void subset_stage_query(const SubsetParams& p, int q, float* qs) {
    const float* src = p.q + (size_t)q * p.d;
    for (int j = threadIdx.x; j < p.dp; j += blockDim.x) qs[j] = j < p.d ? src[j] : 0.f;
    __syncthreads();
}

// the statistics' count of query q's entries inside [0, n): one wave and one atomic per query (an atomic per scoring
// wave would queue thousands of them on one address)
__device__ __forceinline__ void subset_count_valid(const SubsetParams& p, int q, int lane) {
    const long long* cq = p.cand + (size_t)q * p.kc;
    int cnt = 0;
    for (int c0 = 0; c0 < p.kc; c0 += 64) {
        const long long id = c0 + lane < p.kc ? cq[c0 + lane] : -1ll;
        cnt += __popcll(__ballot(id >= 0 && id < p.n));
    }
    if (lane == 0 && cnt) atomicAdd(p.valid, (unsigned long long)cnt);
}

__device__ __forceinline__ void subset_emit(const SubsetParams& p, int q, int c, bool ok, long long id, float score) {
    if (p.keys && c < p.n2) {
        const float s = p.ip ? -score : score;
        p.keys[(size_t)q * p.n2 + c] = (ok && s < FLT_MAX) ? (((u64)ord_f32(s) << 32) | (uint32_t)id) : KEY_PAD;  // false on NaN
    }
    if (p.dist && c < p.kc) p.dist[(size_t)q * p.kc + c] = ok ? score : (p.ip ? -FLT_MAX : FLT_MAX);
}

// float32 L2: wave w of the block scores the entries c0 + 4 w .. c0 + 4 w + 3
static __global__ __launch_bounds__(SUB_W * 64) void subset_score_l2_kernel(const SubsetParams p) {
    extern __shared__ __align__(16) unsigned char smem_sb[];
    float* qs = reinterpret_cast<float*>(smem_sb);
    const int q = blockIdx.y, lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    subset_stage_query(p, q, qs);
    constexpr int R = SUB_CPB / SUB_W;
    const int c0 = blockIdx.x * SUB_CPB + w * R;
    if (blockIdx.x == gridDim.x - 1 && w == SUB_W - 1) subset_count_valid(p, q, lane);
    if (c0 >= p.n2) return;  // wave-uniform; no barrier follows
    const long long* cq = p.cand + (size_t)q * p.kc;
    long long id[R];
    bool ok[R];
    const float* rows[R];
    bool any = false;
#pragma unroll
    for (int r = 0; r < R; r++) {
        id[r] = c0 + r < p.kc ? cq[c0 + r] : -1ll;
        ok[r] = id[r] >= 0 && id[r] < p.n;
        any = any || ok[r];
        rows[r] = p.xb + (size_t)(ok[r] ? id[r] : 0ll) * p.dp;
    }
    if (!any) {  // wave-uniform: nothing to read
        if (lane < R) subset_emit(p, q, c0 + lane, false, -1ll, 0.f);
        return;
    }
    float dd[R];
    exact_l2_rows<R>(rows, qs, p.dp, lane, dd);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; r++) subset_emit(p, q, c0 + r, ok[r], id[r], dd[r]);
    }
}

// inner product: one wave per tile of 16 entries, a block of one wave
static __global__ __launch_bounds__(64) void subset_score_ip_kernel(const SubsetParams p) {
    static_assert(SUB_CPB == 16, "one MFMA row tile per block");
    extern __shared__ __align__(16) unsigned char smem_sb[];
    float* qs = reinterpret_cast<float*>(smem_sb);
    const int q = blockIdx.y, lane = threadIdx.x;
    subset_stage_query(p, q, qs);
    const int c0 = blockIdx.x * SUB_CPB;  // below n2: the grid is ceil(n2 / SUB_CPB) wide
    if (blockIdx.x == gridDim.x - 1) subset_count_valid(p, q, lane);
    const int c = lane & 15, g = lane >> 4;
    const long long* cq = p.cand + (size_t)q * p.kc;
    const long long idc = c0 + c < p.kc ? cq[c0 + c] : -1ll;
    const bool okc = idc >= 0 && idc < p.n;
    if (!__ballot(okc)) {  // wave-uniform: nothing to read
        if (lane < 16) subset_emit(p, q, c0 + lane, false, -1ll, 0.f);
        return;
    }
    // range_tile_dots with a gathered row per lane: 16-byte slot g of every 64-byte k-step, two accumulator chains
    const int nsteps = p.dp >> 4;
    const char* base = reinterpret_cast<const char*>(p.xb + (size_t)(okc ? idc : 0ll) * p.dp) + (g << 4);
    const float* qrow = qs + 4 * g;
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < nsteps; s0 += 4) {
        f32x4 a[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
            if (s0 + s < nsteps) a[s] = *reinterpret_cast<const f32x4*>(base + 64 * (s0 + s));  // wave-uniform test
#pragma unroll
        for (int s = 0; s < 4; s++)
            if (s0 + s < nsteps) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(qrow + 16 * (s0 + s));
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][0], b[0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][1], b[1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][2], b[2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][3], b[3], acc1, 0, 0, 0);
            }
    }
    const f32x4 dot = acc0 + acc1;  // lane (c, g), element j: row 4 g + j of the tile against query column c
    // column j of the result gives row 4 g + j: the lanes c < 4 write one entry each
    if (c < 4) {
        const int r = 4 * g + c;
        const float v = c == 0 ? dot[0] : (c == 1 ? dot[1] : (c == 2 ? dot[2] : dot[3]));
        const long long id = c0 + r < p.kc ? cq[c0 + r] : -1ll;
        subset_emit(p, q, c0 + r, id >= 0 && id < p.n, id, v);
    }
}

// one block per query: sort the n2 keys, drop adjacent duplicates, write the first k
static __global__ __launch_bounds__(SUB_SORT_MAX_THREADS) void subset_select_kernel(const u64* keys, int n2, int k, int ip,
                                                                                  float* D, long long* I) {
    extern __shared__ __align__(16) unsigned char smem_ss[];
    u64* a = reinterpret_cast<u64*>(smem_ss);      // [n2]
    int* wtot = reinterpret_cast<int*>(a + n2);    // [SUB_SORT_MAX_THREADS / 64]
    const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < n2; i += nt) a[i] = keys[(size_t)q * n2 + i];
    block_sort_u64(a, n2, tid, nt);  // barriers inside, the first one before any key is read
    // thread t owns the contiguous entries [t per, (t + 1) per): count the keys that open a run of equal keys
    const int per = (n2 + nt - 1) / nt;
    const int i0 = min(tid * per, n2), i1 = min(i0 + per, n2);
    auto first = [&](int i) { return a[i] != KEY_PAD && (i == 0 || a[i] != a[i - 1]); };
    int mine = 0;
    for (int i = i0; i < i1; i++) mine += first(i) ? 1 : 0;
    int incl = mine;  // inclusive scan over the wave, then over the waves' totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    int pos = incl - mine, total = 0;
    for (int j = 0; j < (nt + 63) / 64; j++) {
        if (j < w) pos += wtot[j];
        total += wtot[j];
    }
    float* Dq = D + (size_t)q * k;
    long long* Iq = I + (size_t)q * k;
    for (int i = i0; i < i1 && pos < k; i++)
        if (first(i)) {
            const float sc = unord_f32((uint32_t)(a[i] >> 32));
            Dq[pos] = ip ? -sc : sc;
            Iq[pos] = (long long)(uint32_t)a[i];
            pos++;
        }
    for (int r = total + tid; r < k; r += nt) {
        Dq[r] = ip ? -FLT_MAX : FLT_MAX;
        Iq[r] = -1ll;
    }
}

__host__ __device__ constexpr size_t subset_select_lds_bytes(int n2) {
    return (size_t)n2 * 8 + (SUB_SORT_MAX_THREADS / 64) * 4;
}

// an empty index: every score is the ignored entry's
static __global__ __launch_bounds__(256) void subset_fill_dist_kernel(float* dist, long long total, int ip) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) dist[i] = ip ? -FLT_MAX : FLT_MAX;
}
