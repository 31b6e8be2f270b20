// ise_remove.hpp -- stable in-place compaction of the index rows: the device side of ise_index_remove_* (Faiss
// IndexFlatCodes::remove_ids; the reference never removes rows).  DESIGN.md section 4.8.
//
// Source map.  The host hands over the removed rows as T sorted, disjoint, non-adjacent runs (start_t, len_t) inside
// [0, n).  c_t = rows removed before run t; g_t = start_t - c_t is the DESTINATION row at which run t bites (strictly
// increasing); cend_t = c_t + len_t.  The row that ends up at destination j is
//     src(j) = j + cend_{u-1},   u = number of runs with g_t <= j   (one upper-bound search in g; u = 0 adds nothing)
// so src is strictly increasing, src(j) >= j, and src(j) = j below first = g_0 = start_0: those rows are never touched.
//
// In-place order.  Destination rows [first, n_new) are taken in ascending slabs [a, b).  Per slab, on ONE stream:
//   1. remove_src_kernel writes the slab's source rows once (u32 src_idx[b - a]); every array reuses them;
//   2. per array, a gather launch copies rows src(a) .. src(b - 1) into the bounce buffer;
//   3. a second launch copies the bounce buffer onto rows [a, b).
// The hand-off between the launches is stream order and nothing else: no atomics, no polling.  Why no launch ever
// reads a row that it or an earlier launch has overwritten:
//   - the gather launches write the bounce buffer only, and read rows src(j) >= src(a) >= a for j in [a, b);
//   - earlier slabs wrote only rows < a <= src(a), so everything this slab's gather reads is still original;
//   - this slab's copy-back writes rows < b, and every later slab reads rows src(j) >= src(b) >= b.
// Extra memory: the bounce buffer (one slab of the widest array) and src_idx, allocated per call by the host.
//
// Every row stride is a whole number of 64-byte k-steps, so the wide arrays (xb, the fp16 and the byte shadow rows)
// move as 16-byte units; the 4-byte arrays (norms, the three hmeta planes, bmeta) share one scalar gather kernel.
#pragma once
#include "ise_common.hpp"

#define REMOVE_MAX_PLANES 5   /* norms, hmeta x 3, bmeta */
#define REMOVE_UNROLL 4       /* independent 16-byte loads per lane in flight (1 KiB per wave-instruction) */

// src_idx[j - a] = src(j) for j in [a, b)
static __global__ __launch_bounds__(256) void remove_src_kernel(const uint32_t* __restrict__ g, const uint32_t* __restrict__ cend,
                                                         int n_runs, uint32_t a, uint32_t count,
                                                         uint32_t* __restrict__ src_idx) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const uint32_t j = a + i;
        int lo = 0, hi = n_runs;  // first run with g > j
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (g[mid] <= j) lo = mid + 1;
            else hi = mid;
        }
        src_idx[i] = j + (lo ? cend[lo - 1] : 0u);
    }
}

// Wide rows, as 16-byte units: dst unit i (rows x upr units, contiguous) <- unit i % upr of row (GATHER ? idx[i / upr]
// : i / upr) of src.  The units of a slab are dealt to the waves grid-stride in pieces of REMOVE_UNROLL wave-loads;
// a wave issues all of a piece's loads before its first store.  total <= 2^31 (the host bounds the slab).
template <bool GATHER>
__global__ __launch_bounds__(256) void remove_rows_kernel(const u32x4* __restrict__ src, const uint32_t* __restrict__ idx,
                                                          u32x4* __restrict__ dst, uint32_t total, uint32_t upr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const uint32_t piece = 64 * REMOVE_UNROLL;
    const uint32_t npieces = (total + piece - 1) / piece;
    for (uint32_t p = wave; p < npieces; p += nwaves) {
        const uint32_t base = p * piece + lane;
        // a piece's tail past `total` re-reads the last unit (no branch between the loads) and is not stored
        size_t s[REMOVE_UNROLL];
#pragma unroll
        for (int t = 0; t < REMOVE_UNROLL; t++) {  // every source row number first, so that the row loads go out together
            const uint32_t i = min(base + 64 * t, total - 1);
            s[t] = i;
            if (GATHER) {
                const uint32_t r = i / upr;
                s[t] = (size_t)idx[r] * upr + (i - r * upr);
            }
        }
        u32x4 v[REMOVE_UNROLL];
#pragma unroll
        for (int t = 0; t < REMOVE_UNROLL; t++) v[t] = __builtin_nontemporal_load(src + s[t]);
#pragma unroll
        for (int t = 0; t < REMOVE_UNROLL; t++) {
            const uint32_t i = base + 64 * t;
            if (i < total) dst[i] = v[t];
        }
    }
}

// The 4-byte arrays, one plane per blockIdx.y: dst[y][i] <- src[y][GATHER ? idx[i] : i], i < count.
struct RemovePlanes {
    const uint32_t* src[REMOVE_MAX_PLANES];
    uint32_t* dst[REMOVE_MAX_PLANES];
};
template <bool GATHER>
__global__ __launch_bounds__(256) void remove_words_kernel(RemovePlanes pl, const uint32_t* __restrict__ idx, uint32_t count) {
    const uint32_t* __restrict__ s = pl.src[blockIdx.y];
    uint32_t* __restrict__ d = pl.dst[blockIdx.y];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
        d[i] = s[GATHER ? idx[i] : i];
}
