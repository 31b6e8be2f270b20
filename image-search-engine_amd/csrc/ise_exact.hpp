// ise_exact.hpp -- the VERIFIER of the exact float32 L2 search: direct-difference re-rank of the
// scan's candidates with a certificate, and the exact fallback scan for the queries it cannot prove.
//
// What Faiss computes for the reference's query shape (one query per call, backend/engine.py:50,55;
// nq < 20 in IndexFlatL2::search [upstream-faiss]) is the per-pair sum (x_i - y_i)^2 -- no
// expansion, no cancellation; the reference's own numpy restatement does the same
// (backend/siamese/test_index.py:62-64).  The streaming scan (ise_scan.hpp) evaluates the expanded
// form on the matrix core, which is fast but loses digits, so for float32 L2 indexes it is used as
// a FILTER only:
//
//   scan    keys every row by lo = s~ - beta (|x-mu|^2 + |y-mu|^2), a rigorous lower bound of the
//           direct-difference value d(x, y) as THIS file computes it, and keeps the kc = k + extra
//           rows of smallest (lo, id) per query.
//   rerank  (rerank_block, fused into the merge kernel) evaluates d for those kc rows, sorts them by
//           (d, id) and checks the certificate  lo_(kc) > d_(k):  every row outside the candidate
//           list has lo >= lo_(kc), hence d >= lo > d_(k), hence cannot enter the top k.  A list
//           with fewer than kc entries holds every admissible row and needs no check.
//   exact   queries whose certificate fails (dense near-ties, far-apart clusters, massive
//           duplicates: wherever beta (|x-mu|^2 + |y-mu|^2) exceeds the neighbour spacing) are put
//           on a per-launch list; exact_scan_kernel -- launched behind every rerank, exiting at
//           once when the list is empty -- recomputes them as a direct-difference scan of the whole
//           index with the same d(), i.e. Faiss's small-batch algorithm itself.
//
// Either way the reported distances are d(x, y) and the ids are the exact top k by (d, id): the
// result is independent of mu, of the grid shape and of which path produced it.
#pragma once
#include "ise_common.hpp"
#include "ise_select.hpp"

// d(x, y) = sum (y_i - x_i)^2 in float32, one wave per row, fixed order: lane l accumulates the
// elements 4l..4l+3 of every 256-element segment in sequence (fmaf chain), then an xor butterfly.
// row: dp floats (zero padded, 16-byte aligned); qs: the query in LDS, zero padded to dp.
// Every lane returns the same value.
template <int R>
__device__ __forceinline__ void exact_l2_rows(const float* const (&rows)[R], const float* qs, int dp, int lane,
                                              float (&out)[R]) {
    float s[R];
#pragma unroll
    for (int r = 0; r < R; r++) s[r] = 0.f;
    for (int j = lane * 4; j < dp; j += 256) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(qs + j);
        f32x4 y[R];
#pragma unroll
        for (int r = 0; r < R; r++) y[r] = *reinterpret_cast<const f32x4*>(rows[r] + j);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const f32x4 t = y[r] - x;
            s[r] = fmaf(t[0], t[0], s[r]);
            s[r] = fmaf(t[1], t[1], s[r]);
            s[r] = fmaf(t[2], t[2], s[r]);
            s[r] = fmaf(t[3], t[3], s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) out[r] = wave_sum_f32(s[r]);
}

struct ExactParams {
    const float* xb;   // [cap][dp] float32 rows
    const float* q;    // [nq][d]
    long long n;
    int d, dp, nq;
    int k;             // results per query
    int kc;            // candidates per query handed to the rerank (k < kc unless the index is short)
    uint32_t id_base;
    float* D;          // [nq][k] or null
    long long* I;      // [nq][k] or null
    u64* keys_out;     // [nq][k] or null: exact keys ord(d) << 32 | id
    // per-launch list of the queries whose certificate failed: state = launch seq << 32 | count
    u64* fl_state;
    int* fl_list;      // [nq]
    uint32_t seq;
    unsigned long long* stats;  // [0] queries reranked, [1] queries sent to the exact scan
    int force_fail;    // test knob ($ISE_FORCE_EXACT=1): fail every certificate
    // large-batch path: rows with lo > tau[q] never became candidates; the certificate covers them too
    const float* tau_bound;  // [nq] or null
};

// append query q to the launch's fallback list (the counter is tagged with the launch sequence
// number, so it needs no reset between launches)
__device__ __forceinline__ void fallback_list_push(const ExactParams& p, int q) {
    u64 old = __hip_atomic_load(p.fl_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const u64 want = ((uint32_t)(old >> 32) == p.seq) ? old + 1 : (((u64)p.seq << 32) | 1ull);
        if (__hip_atomic_compare_exchange_strong(p.fl_state, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
            p.fl_list[(uint32_t)want - 1] = q;
            return;
        }
    }
}

__device__ __forceinline__ void emit_exact(const ExactParams& p, size_t o, u64 key) {
    if (p.keys_out) p.keys_out[o] = key;
    if (p.D) {
        const bool pad = key == KEY_PAD;
        p.D[o] = pad ? FLT_MAX : unord_f32((uint32_t)(key >> 32));
        p.I[o] = pad ? -1ll : (long long)(uint32_t)key;
    }
}

// block-wide bitonic sort of n2 (a power of two) keys in LDS, ascending
__device__ __forceinline__ void block_sort_u64(u64* a, int n2, int tid, int nthreads) {
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < (n2 >> 1); i += nthreads) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const u64 x = a[lo], y = a[hi];
                if ((x > y) == up) {
                    a[lo] = y;
                    a[hi] = x;
                }
            }
        }
    __syncthreads();
}

// LDS image of one rerank block: qs [dp] floats | kin [kc] | kex [n2] (u64, 8-byte aligned)
__host__ __device__ constexpr int rerank_pow2(int kc) {
    int n2 = 1;
    while (n2 < kc) n2 <<= 1;
    return n2;
}
__host__ __device__ constexpr size_t rerank_lds_bytes(int dp, int kc) {
    return (size_t)dp * 4 + (size_t)kc * 8 + (size_t)rerank_pow2(kc) * 8;
}

// The query of a rerank block into LDS (zero padded to dp).  Separate from rerank_block so that the
// fused merge kernel can issue it before the lists are merged.
template <int NT>
__device__ __forceinline__ void rerank_stage_query(const ExactParams& p, int q, unsigned char* smem) {
    float* qs = reinterpret_cast<float*>(smem);
    const float* src = p.q + (size_t)q * p.d;
    for (int j = threadIdx.x; j < p.dp; j += NT) qs[j] = j < p.d ? src[j] : 0.f;
}

#define RERANK_ROWS 4 /* rows a re-rank wave scores side by side; two steps of them in flight: 8 loads, 32 VGPRs */

// Where a re-rank wave stands in its rows: group g of RERANK_ROWS candidates, column block j of nj.  The loads run two
// steps ahead of the arithmetic; each keeps one of these.
struct RerankCursor {
    int g = 0, j = 0;
    __device__ __forceinline__ void next(int nj) {
        if (++j == nj) {
            j = 0;
            g++;
        }
    }
};

// Re-rank the kc candidates of query q (kin: ascending lo-keys, KEY_PAD padded, in LDS behind the
// staged query) by their direct-difference distance; emit the top k; on a failed certificate put q
// on the fallback list.  Called by all NT threads of the block; smem is the block's dynamic LDS
// (rerank_lds_bytes).  keys_in_global: candidates to load first, or null when kin is already filled.
template <int NT>
__device__ __forceinline__ void rerank_block(const ExactParams& p, int q, unsigned char* smem,
                                             const u64* keys_in_global) {
    constexpr int NW = NT / 64;
    float* qs = reinterpret_cast<float*>(smem);
    u64* kin = reinterpret_cast<u64*>(qs + p.dp);
    u64* kex = kin + p.kc;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: a scalar
    const int n2 = rerank_pow2(p.kc);
    DBG_STAMP(p.stats ? p.stats + 8 : nullptr, 3);
    if (keys_in_global)
        for (int c = tid; c < p.kc; c += NT) kin[c] = keys_in_global[(size_t)q * p.kc + c];
    __syncthreads();
    // ---- the candidates' rows.  Wave w takes the candidates w, w + NW, .. in groups of RERANK_ROWS; a STEP is one
    // 256-float column block (16 bytes per lane) of the RERANK_ROWS rows of a group, and the ring holds two steps.
    // Fetching a row block by block, each used before the next is asked for, made the re-rank a chain of
    // dependent trips to rows that miss to HBM.  Here a wave asks for its first two steps together, the moment kin
    // is known (a pad is the largest key and ends the list, so the requests need no count), and for one step more
    // behind every step it uses: at dp = 512 all the rows of kc <= 32 (8 waves) come in ONE trip, longer rows and
    // lists go round the ring.  The lanes keep the wave's candidate keys in a register, 64 at a time, so that naming
    // a row costs a readlane and no trip to LDS.  A request is masked (a pad, a column at or beyond dp: nothing is read
    // -- and no row exists when the index is empty) and otherwise unconditional, like exact_scan_kernel's.
    // d() is exact_l2_rows' bit for bit: per lane the fmaf chain over the row's column blocks in ascending order
    // from 0.f, then wave_sum_f32 (the rows of a group are reduced side by side, each by its own butterfly).
    const int nj = (p.dp + 255) >> 8;
    int kb = 0;  // lane i holds the wave's (kb + i)-th candidate: 64 of them at a time
    auto lane_key = [&]() -> u64 { return (w + NW * (kb + lane)) < p.kc ? kin[w + NW * (kb + lane)] : KEY_PAD; };
    u64 lanekey = lane_key();
    f32x4 ring[2][RERANK_ROWS];
    RerankCursor ld;  // the next step to LOAD
    auto load_step = [&](f32x4(&y)[RERANK_ROWS]) {  // a slot keeps what it held where nothing is read (never used)
        const int j = (ld.j << 8) + lane * 4;
        if (ld.g * RERANK_ROWS - kb >= 64) {  // wave-uniform, once per 64 candidates of the wave
            kb += 64;
            lanekey = lane_key();
        }
#pragma unroll
        for (int r = 0; r < RERANK_ROWS; r++) {
            const u64 key = readlane_u64(lanekey, ld.g * RERANK_ROWS + r - kb);
            if (key != KEY_PAD && j < p.dp)
                y[r] = *reinterpret_cast<const f32x4*>(p.xb + (size_t)((uint32_t)key - p.id_base) * p.dp + j);
        }
        ld.next(nj);
    };
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int r = 0; r < RERANK_ROWS; r++) ring[h][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
        load_step(ring[h]);
    }
    // real entries come first (the list is sorted and pads are the largest key)
    int count = 0;
    for (int c0 = 0; c0 < p.kc; c0 += 64) {
        const bool real = (c0 + lane) < p.kc && kin[c0 + lane] != KEY_PAD;
        count += __popcll(__ballot(real));
    }
    DBG_STAMP(p.stats ? p.stats + 8 : nullptr, 4);
    for (int c = count + tid; c < n2; c += NT) kex[c] = KEY_PAD;
    {
        const int rows_w = count > w ? (count - w + NW - 1) / NW : 0;  // this wave's real candidates
        const int T = (rows_w + RERANK_ROWS - 1) / RERANK_ROWS * nj;    // ... and its steps
        RerankCursor use;  // the step being USED
        float s[RERANK_ROWS];
#pragma unroll
        for (int r = 0; r < RERANK_ROWS; r++) s[r] = 0.f;
        auto use_step = [&](f32x4(&slot)[RERANK_ROWS]) {
            f32x4 y[RERANK_ROWS];
#pragma unroll
            for (int r = 0; r < RERANK_ROWS; r++) y[r] = slot[r];
            load_step(slot);
            const int j = (use.j << 8) + lane * 4;
            if (j < p.dp) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(qs + j);
#pragma unroll
                for (int r = 0; r < RERANK_ROWS; r++) {
                    const f32x4 t = y[r] - x;
                    s[r] = fmaf(t[0], t[0], s[r]);
                    s[r] = fmaf(t[1], t[1], s[r]);
                    s[r] = fmaf(t[2], t[2], s[r]);
                    s[r] = fmaf(t[3], t[3], s[r]);
                }
            }
            if (use.j == nj - 1) {  // the group's rows are complete
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {  // wave_sum_f32 of every row, side by side
                    float t[RERANK_ROWS];
#pragma unroll
                    for (int r = 0; r < RERANK_ROWS; r++) t[r] = __shfl_xor(s[r], o);
#pragma unroll
                    for (int r = 0; r < RERANK_ROWS; r++) s[r] += t[r];
                }
#pragma unroll
                for (int r = 0; r < RERANK_ROWS; r++) {
                    const int i = use.g * RERANK_ROWS + r;
                    // Faiss's gate: a distance >= FLT_MAX (a candidate keyed -FLT_MAX for an overflowing norm, or
                    // one whose bound lay just below FLT_MAX) is not a result
                    if (lane == 0 && i < rows_w)
                        kex[w + NW * i] = s[r] < FLT_MAX ? (((u64)ord_f32(s[r]) << 32) | (uint32_t)kin[w + NW * i]) : KEY_PAD;
                    s[r] = 0.f;
                }
            }
            use.next(nj);
        };
        for (int t = 0; t < T; t += 2) {  // two steps per turn: the ring's registers are named statically
            use_step(ring[0]);
            if (t + 1 < T) use_step(ring[1]);
        }
    }
    DBG_STAMP(p.stats ? p.stats + 8 : nullptr, 5);
    if (n2 <= 64) {  // one wave ranks all pairs: no barrier per stage
        __syncthreads();
        if (w == 0) {
            const u64 mine = lane < n2 ? kex[lane] : KEY_PAD;
            int rk = 0;
            for (int j = 0; j < n2; j++) rk += readlane_u64(mine, j) < mine ? 1 : 0;
            // pads are equal: they keep their slots' worth of the tail in any order
            const u64 padm = __ballot(mine == KEY_PAD) & ((lane < 63 ? (1ull << (lane + 1)) : 0ull) - 1ull);
            if (mine == KEY_PAD) rk += __popcll(padm) - 1;
            wave_lds_fence();
            if (lane < n2) kex[rk] = mine;
        }
        __syncthreads();
    } else {
        block_sort_u64(kex, n2, tid, NT);
    }
    DBG_STAMP(p.stats ? p.stats + 8 : nullptr, 6);
    // certificate: lo of the last candidate strictly above the k-th direct distance.  A list that is
    // not full holds every row whose lo is not NaN: every row of finite entries, since an overflowing
    // norm is keyed lo = -FLT_MAX (ise_common.hpp, l2_lower_bound); NaN-normed rows hold a NaN or inf
    // entry and are never admissible.  A full list whose k-th slot is empty after the gate above (too
    // few candidates below FLT_MAX), or whose last lo is -FLT_MAX (every row overflowed, as for a query
    // with an overflowing |x - mu|^2), fails: d_k is NaN, or lo_last is not above it.
    bool ok = true;
    if (count == p.kc && p.n > p.kc) {
        const float lo_last = unord_f32((uint32_t)(kin[p.kc - 1] >> 32));
        const float d_k = unord_f32((uint32_t)(kex[p.k - 1] >> 32));
        ok = lo_last > d_k;  // false on NaN
    }
    if (p.tau_bound) {  // rows cut by the admit threshold have lo > tau: tau >= d_(k) keeps them out of the top k
        if (count >= p.k) ok = ok && p.tau_bound[q] >= unord_f32((uint32_t)(kex[p.k - 1] >> 32));
        else ok = ok && (long long)count >= p.n;  // fewer than k candidates and rows left outside: not a result
    }
    if (p.force_fail) ok = false;
    for (int r = tid; r < p.k; r += NT) emit_exact(p, (size_t)q * p.k + r, r < count ? kex[r] : KEY_PAD);
    DBG_STAMP(p.stats ? p.stats + 8 : nullptr, 7);
    if (tid == 0) {
        if (p.stats) atomicAdd(&p.stats[0], 1ull);
        if (!ok) {
            if (p.stats) atomicAdd(&p.stats[1], 1ull);
            fallback_list_push(p, q);
        }
    }
}

// standalone form: candidates [nq][kc] in HBM (the multi-pass path, kc > 32)
static __global__ __launch_bounds__(256) void rerank_kernel(const ExactParams p, const u64* keys_in) {
    extern __shared__ __align__(16) unsigned char smem_rr[];
    rerank_stage_query<256>(p, (int)blockIdx.x, smem_rr);
    rerank_block<256>(p, (int)blockIdx.x, smem_rr, keys_in);
}

