// ise_ivf_tiles.hpp -- the kernels of the inverted lists that read nothing of a row's meaning, and their launches: the
// probe table's masks, the work list of the kinds that scan 64-row tiles, and the rebuild of all four kinds (float32
// rows, ise_ivf.hip; 8-bit rows, ise_ivfsq.hip; product-quantiser codes, ise_ivfpq.hip; bit codes, ise_binary_ivf.hip;
// DESIGN.md 4.12a).  A row is `row units`
// copy units of 16 or 8 bytes, a slot may carry an 8-byte side value (the 8-bit rows' row term) and carries a uint32
// id; list l owns the tiles [list_tile0[l], list_tile0[l + 1]) of ivf_plan_meta's table (ise_ivf_plan.hpp).  The host
// side is ise_ivf_lists.hpp; the launches have a second user, the test harnesses (tests/native/*_harness.hip), which
// therefore run the product's grids and not a copy of them.
#pragma once
#include "ise_common.hpp"
#include "ise_ivf_plan.hpp"

#define IVF_WORK_TILE 64 /* rows of a tile of the kinds that scan from a work list: a wave's unit */

// probes [nq][nprobe] (int64) -> masks [groups of 1 << qshift queries][nlist], bit c: query (group << qshift) + c probes
// the list; the masks are zero on entry.  -1 and out-of-range entries set nothing, a duplicate sets its bit twice
static __global__ __launch_bounds__(256) void ivf_mask_kernel(const long long* probes, long long total, int nprobe, int nlist,
                                                              int qshift, uint32_t* masks) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long l = probes[i];
    if (l < 0 || l >= nlist) return;
    const long long q = i / nprobe;
    atomicOr(masks + (size_t)(q >> qshift) * nlist + l, 1u << (q & ((1 << qshift) - 1)));
}

// ---------------------------------------------------------------- the work list (64-row tiles)
// one block per group: offs[group][l] = the tiles of the probed lists before l, count[group] = their total.  Thread t
// owns the lists [t per, (t + 1) per); the 256 partial sums are scanned in LDS
static __global__ __launch_bounds__(256) void ivf_offsets_kernel(const uint32_t* masks, const uint32_t* list_tile0, int nlist,
                                                                 uint32_t* offs, uint32_t* count) {
    __shared__ uint32_t part[256];
    const int t = threadIdx.x, grp = blockIdx.x;
    const uint32_t* gm = masks + (size_t)grp * nlist;
    uint32_t* go = offs + (size_t)grp * nlist;
    const int per = (nlist + 255) / 256;
    const int l0 = min(nlist, t * per), l1 = min(nlist, l0 + per);
    uint32_t s = 0;
    for (int l = l0; l < l1; l++) s += gm[l] ? list_tile0[l + 1] - list_tile0[l] : 0u;
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int l = l0; l < l1; l++) {
        go[l] = run;
        run += gm[l] ? list_tile0[l + 1] - list_tile0[l] : 0u;
    }
    if (t == 255) count[grp] = part[255];
}

// thread per (tile, group = blockIdx.y): the entry of a probed list's tile.  work: [groups][tiles]
static __global__ __launch_bounds__(256) void ivf_work_kernel(const uint32_t* masks, const uint32_t* offs,
                                                              const uint32_t* list_tile0, const uint32_t* list_size,
                                                              const uint32_t* tile_list, int nlist, uint32_t tiles,
                                                              u32x4* work) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles) return;
    const size_t grp = blockIdx.y;
    const uint32_t l = tile_list[t];
    const uint32_t m = masks[grp * nlist + l];
    if (!m) return;
    const uint32_t in_list = t - list_tile0[l];
    const uint32_t left = list_size[l] - in_list * IVF_WORK_TILE;  // >= 1: a list has no tile without a row
    work[grp * tiles + offs[grp * nlist + l] + in_list] = u32x4{t, left < IVF_WORK_TILE ? left : (uint32_t)IVF_WORK_TILE, m, 0u};
}

// Both launches below enqueue on st and return the first error of a memset; the caller takes hipGetLastError() for the
// kernels.  meta: ivf_plan_meta's table of nlist lists.
//
// the work lists of m queries' probes [m][nprobe]: masks [groups][nlist] (cleared here), offs [groups][nlist], counts
// [groups], work [groups][tiles], groups = ceil(m / 2^qshift).  m, nprobe >= 1; without a tile no entry is written
inline hipError_t ivf_work_list_launch(const long long* probes, int m, int nprobe, int nlist, int qshift, const uint32_t* meta,
                                       uint32_t tiles, uint32_t* masks, uint32_t* offs, uint32_t* counts, u32x4* work,
                                       hipStream_t st) {
    const int groups = (m + (1 << qshift) - 1) >> qshift;
    const hipError_t e = hipMemsetAsync(masks, 0, (size_t)groups * nlist * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const long long ptot = (long long)m * nprobe;
    hipLaunchKernelGGL(ivf_mask_kernel, dim3((unsigned)((ptot + 255) / 256)), dim3(256), 0, st, probes, ptot, nprobe, nlist, qshift,
                       masks);
    hipLaunchKernelGGL(ivf_offsets_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const uint32_t*)masks, meta, nlist, offs,
                       counts);
    if (tiles > 0)
        hipLaunchKernelGGL(ivf_work_kernel, dim3((tiles + 255) / 256, (unsigned)groups), dim3(256), 0, st, (const uint32_t*)masks,
                           (const uint32_t*)offs, meta, meta + ivf_meta_size_at((size_t)nlist),
                           meta + ivf_meta_tile_list_at((size_t)nlist), nlist, tiles, work);
    return hipSuccess;
}

// ---------------------------------------------------------------- the rebuild
// TILE rows a tile (16 or 64), U the copy unit (u32x4: 16 bytes; u64: 8 bytes, where a row may be half a 16-byte unit
// and a destination slot odd), ru units a row.  side: one 8-byte value per slot, or null in both kernels alike (the
// branch is uniform).
//
// one block per OLD tile: the tile moves, whole, to where its list now starts (side values, ids and pad slots with it)
template <int TILE, class U>
__global__ __launch_bounds__(256) void ivf_move_tiles_kernel(const U* __restrict__ src, const u64* __restrict__ src_side,
                                                             const uint32_t* __restrict__ src_ids,
                                                             const uint32_t* __restrict__ old_tile_list,
                                                             const uint32_t* __restrict__ old_tile0,
                                                             const uint32_t* __restrict__ new_tile0, int ru, U* __restrict__ dst,
                                                             u64* __restrict__ dst_side, uint32_t* __restrict__ dst_ids) {
    const size_t t = blockIdx.x;
    const uint32_t l = old_tile_list[t];
    const size_t nt = (size_t)new_tile0[l] + (t - old_tile0[l]);
    const U* s = src + t * TILE * ru;
    U* o = dst + nt * TILE * ru;
    for (int i = threadIdx.x; i < TILE * ru; i += 256) o[i] = s[i];
    if (threadIdx.x < TILE) {
        if (src_side) dst_side[nt * TILE + threadIdx.x] = src_side[t * TILE + threadIdx.x];
        dst_ids[nt * TILE + threadIdx.x] = src_ids[t * TILE + threadIdx.x];
    }
}

// wave per pending row i: to slot dest[i], with id id0 + i
template <class U>
__global__ __launch_bounds__(256) void ivf_scatter_rows_kernel(const U* __restrict__ pend, const u64* __restrict__ pend_side,
                                                               long long m, const uint32_t* __restrict__ dest, uint32_t id0, int ru,
                                                               U* __restrict__ dst, u64* __restrict__ dst_side,
                                                               uint32_t* __restrict__ dst_ids) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const size_t slot = dest[i];
    const U* s = pend + (size_t)i * ru;
    U* o = dst + slot * ru;
    for (int j = lane; j < ru; j += 64) o[j] = s[j];
    if (lane == 0) {
        if (pend_side) dst_side[slot] = pend_side[i];
        dst_ids[slot] = id0 + (uint32_t)i;
    }
}

// the arrays of one side of a rebuild: rows [slots][row_bytes], side [slots] 8-byte values or null, ids [slots]
struct IvfTileArrays {
    void* rows;
    void* side;
    uint32_t* ids;
};

template <int TILE, class U>
void ivf_rebuild_kernels_(size_t row_bytes, const IvfTileArrays& old, const uint32_t* meta, long long old_tiles,
                          const IvfTileArrays& pend, long long pend_n, const uint32_t* dest, uint32_t id0, int nlist,
                          const uint32_t* nmeta, const IvfTileArrays& nw, hipStream_t st) {
    const int ru = (int)(row_bytes / sizeof(U));
    if (old_tiles > 0)
        hipLaunchKernelGGL((ivf_move_tiles_kernel<TILE, U>), dim3((unsigned)old_tiles), dim3(256), 0, st, (const U*)old.rows,
                           (const u64*)old.side, (const uint32_t*)old.ids, meta + ivf_meta_tile_list_at((size_t)nlist), meta, nmeta, ru,
                           (U*)nw.rows, (u64*)nw.side, nw.ids);
    hipLaunchKernelGGL(ivf_scatter_rows_kernel<U>, dim3((unsigned)((pend_n + 3) / 4)), dim3(256), 0, st, (const U*)pend.rows,
                       (const u64*)pend.side, pend_n, dest, id0, ru, (U*)nw.rows, (u64*)nw.side, nw.ids);
}

// the new arrays nw of new_tiles tiles (table nmeta): cleared (pad slots are zero rows with a zero side value and id
// ~0), the old_tiles tiles of old (table meta; neither is read without an old tile) moved, the pend_n >= 1 pending
// rows of pend (its ids are not read) scattered to dest with the ids id0, id0 + 1, ..  (tile_rows, unit_bytes): (16,
// 16), (64, 16) or (64, 8), anything else is hipErrorInvalidValue; row_bytes: a multiple of unit_bytes
inline hipError_t ivf_rebuild_launch(int tile_rows, int unit_bytes, size_t row_bytes, const IvfTileArrays& old, const uint32_t* meta,
                                     long long old_tiles, const IvfTileArrays& pend, long long pend_n, const uint32_t* dest,
                                     uint32_t id0, int nlist, const uint32_t* nmeta, long long new_tiles, const IvfTileArrays& nw,
                                     hipStream_t st) {
    const int kind = tile_rows == 16 && unit_bytes == 16 ? 0 : tile_rows == 64 && unit_bytes == 16 ? 1 : tile_rows == 64 && unit_bytes == 8 ? 2 : -1;
    if (kind < 0) return hipErrorInvalidValue;
    const size_t slots = (size_t)new_tiles * tile_rows;
    hipError_t e = hipMemsetAsync(nw.rows, 0, slots * row_bytes, st);  // pad slots read as zero rows
    if (e == hipSuccess && nw.side) e = hipMemsetAsync(nw.side, 0, slots * sizeof(u64), st);
    if (e == hipSuccess) e = hipMemsetAsync(nw.ids, 0xFF, slots * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    auto* go = kind == 0 ? ivf_rebuild_kernels_<16, u32x4> : kind == 1 ? ivf_rebuild_kernels_<64, u32x4> : ivf_rebuild_kernels_<64, u64>;
    go(row_bytes, old, meta, old_tiles, pend, pend_n, dest, id0, nlist, nmeta, nw, st);
    return hipSuccess;
}
