// ise_ivfsq.hpp -- kernels of IndexIVFScalarQuantizer: inverted lists over the 8-bit rows of ise_sq.hpp and the pass
// that scans only the probed ones (include/ise_knn.h, ise_ivfsq_*).  Host side: ise_ivfsq.hip.
//
// Layout.  All lists live in ONE array: codes [slots][stride] (stride = d rounded up to 64, pad bytes zero), rterm
// [slots] float64 (ise_sq.hpp's row term) and ids [slots] uint32 (the row's insertion number).  List l owns the 64-row
// tiles [list_tile0[l], list_tile0[l + 1]) -- SQ_TILE rows, a wave's unit in the byte scan; inside a list the slots are
// in ascending id order, the slots behind list_size[l] rows are zero rows with id 0xFFFFFFFF, masked by position.
//
// A pass serves one group of QT = sq_qt(d) queries and 32 results:
//   masks      ivf_mask_kernel (ise_ivf_lists.hpp) turns the probe table [nq][nprobe] into one query mask per (group of
//              QT, list); -1 and out-of-range entries set nothing, a duplicate sets its bit twice.
//   work list  ivfsq_offsets_kernel scans the lists' tile counts under "mask != 0" into an offset per (group, list) and
//              a count per group; ivfsq_work_kernel, parallel over all tiles, writes for every tile of a probed list
//              the entry (tile, valid rows in it, the list's mask) at offset[list] + tile - list_tile0[list]: slot order,
//              so the list is the same whatever the launch does.
//   scan       ivfsq_scan_kernel is sq_scan_body (ise_sq.hpp) walking the entries instead of the tiles: wave w of block
//              b takes entries b SQ_WAVES + w + j gridDim.x SQ_WAVES.  The key is ord(score) << 32 | ids[slot]; keys are
//              unique and compared in full, so ties go by ascending id however the lists order the ids.
// The staging record, the selection (ise_cand.hpp), the pass's merge and the floor-keyed repeat for k > 32 are ise_sq.hpp's.
//
// The launches of the work list and of the rebuild are the two host functions at the end, ivfsq_work_list_launch and
// ivfsq_rebuild_launch: ise_ivfsq.hip calls them, and so does the test harness (tests/native/ivfsq_lists_harness.hip),
// which therefore runs the product's grids and not a copy of them.
#pragma once
#include "ise_ivf_lists.hpp"
#include "ise_sq.hpp"

struct SqIvfScanParams {
    const uint8_t* codes;   // [tiles * 64][stride]
    const double* rterm;    // [tiles * 64]
    const uint32_t* ids;    // [tiles * 64]
    int d, stride;
    const unsigned char* qrec;  // the group's first query's staged record, nqt of them
    int nqt, kp;
    int ip;
    const u64* lo;          // [nqt] floors, or null in the first pass
    u64* lists;             // [grid][QT][SQ_KPASS]
    const u32x4* work;      // the group's entries: (tile, valid rows, query mask, 0)
    const uint32_t* count;  // [1] entries of the group
    unsigned long long* tiles_loaded;  // += the entries this pass visits
};

template <int QT>
__global__ __launch_bounds__(SQ_WAVES * 64) void ivfsq_scan_kernel(const SqIvfScanParams p) {
    sq_scan_body<QT, true>(p);
}

// one block per group: offs[group][l] = the tiles of the probed lists before l, count[group] = their total.  Thread t
// owns the lists [t per, (t + 1) per); the 256 partial sums are scanned in LDS
static __global__ __launch_bounds__(256) void ivfsq_offsets_kernel(const uint32_t* masks, const uint32_t* list_tile0, int nlist,
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
static __global__ __launch_bounds__(256) void ivfsq_work_kernel(const uint32_t* masks, const uint32_t* offs,
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
    const uint32_t left = list_size[l] - in_list * SQ_TILE;  // >= 1: a list has no tile without a row
    work[grp * tiles + offs[grp * nlist + l] + in_list] = u32x4{t, left < SQ_TILE ? left : (uint32_t)SQ_TILE, m, 0u};
}

// ---------------------------------------------------------------- rebuild (ise_ivfsq.hip)
// one block per OLD tile: the tile moves, whole, to where its list now starts (row terms, ids and pad slots with it)
static __global__ __launch_bounds__(256) void ivfsq_move_tiles_kernel(const uint8_t* src, const double* src_rterm,
                                                                      const uint32_t* src_ids, const uint32_t* old_tile_list,
                                                                      const uint32_t* old_tile0, const uint32_t* new_tile0,
                                                                      int stride, uint8_t* dst, double* dst_rterm,
                                                                      uint32_t* dst_ids) {
    const size_t t = blockIdx.x;
    const uint32_t l = old_tile_list[t];
    const size_t nt = (size_t)new_tile0[l] + (t - old_tile0[l]);
    const u32x4* s = reinterpret_cast<const u32x4*>(src + t * SQ_TILE * stride);
    u32x4* o = reinterpret_cast<u32x4*>(dst + nt * SQ_TILE * stride);
    for (int i = threadIdx.x; i < SQ_TILE * stride / 16; i += 256) o[i] = s[i];
    if (threadIdx.x < SQ_TILE) {
        dst_rterm[nt * SQ_TILE + threadIdx.x] = src_rterm[t * SQ_TILE + threadIdx.x];
        dst_ids[nt * SQ_TILE + threadIdx.x] = src_ids[t * SQ_TILE + threadIdx.x];
    }
}

// wave per pending row i: to slot dest[i], with id id0 + i
static __global__ __launch_bounds__(256) void ivfsq_scatter_rows_kernel(const uint8_t* pend, const double* pend_rterm,
                                                                        long long m, const uint32_t* dest, uint32_t id0,
                                                                        int stride, uint8_t* dst, double* dst_rterm,
                                                                        uint32_t* dst_ids) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const size_t slot = dest[i];
    const u32x4* s = reinterpret_cast<const u32x4*>(pend + (size_t)i * stride);
    u32x4* o = reinterpret_cast<u32x4*>(dst + slot * stride);
    for (int j = lane; j < stride / 16; j += 64) o[j] = s[j];
    if (lane == 0) {
        dst_rterm[slot] = pend_rterm[i];
        dst_ids[slot] = id0 + (uint32_t)i;
    }
}

// ---------------------------------------------------------------- the launches (ise_ivfsq.hip and the test harness)
// Both enqueue on st and return the first error of a memset; the caller takes hipGetLastError() for the launches.
// meta: ivf_plan_meta's table (ise_ivf_plan.hpp) of nlist lists.
//
// the work lists of m queries' probes [m][nprobe]: masks [groups][nlist] (cleared here), offs [groups][nlist], counts
// [groups], work [groups][tiles], groups = ceil(m / 2^qshift).  m, nprobe >= 1; without a tile no entry is written
inline hipError_t ivfsq_work_list_launch(const long long* probes, int m, int nprobe, int nlist, int qshift, const uint32_t* meta,
                                         uint32_t tiles, uint32_t* masks, uint32_t* offs, uint32_t* counts, u32x4* work,
                                         hipStream_t st) {
    const int groups = (m + (1 << qshift) - 1) >> qshift;
    const hipError_t e = hipMemsetAsync(masks, 0, (size_t)groups * nlist * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const long long ptot = (long long)m * nprobe;
    hipLaunchKernelGGL(ivf_mask_kernel, dim3((unsigned)((ptot + 255) / 256)), dim3(256), 0, st, probes, ptot, nprobe, nlist, qshift,
                       masks);
    hipLaunchKernelGGL(ivfsq_offsets_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const uint32_t*)masks, meta, nlist, offs,
                       counts);
    if (tiles > 0)
        hipLaunchKernelGGL(ivfsq_work_kernel, dim3((tiles + 255) / 256, (unsigned)groups), dim3(256), 0, st, (const uint32_t*)masks,
                           (const uint32_t*)offs, meta, meta + ivf_meta_size_at((size_t)nlist),
                           meta + ivf_meta_tile_list_at((size_t)nlist), nlist, tiles, work);
    return hipSuccess;
}

// the new arrays nx / nr / nids of new_tiles tiles (table nmeta): cleared (pad slots are zero rows with id ~0), the
// old_tiles old tiles (table meta; not read without an old tile) moved, the pend_n >= 1 pending rows scattered to dest
// with the ids id0, id0 + 1, ..
inline hipError_t ivfsq_rebuild_launch(const uint8_t* codes, const double* rterm, const uint32_t* ids, const uint32_t* meta,
                                       long long old_tiles, const uint8_t* pend, const double* pend_rterm, long long pend_n,
                                       const uint32_t* dest, uint32_t id0, int stride, int nlist, const uint32_t* nmeta,
                                       long long new_tiles, uint8_t* nx, double* nr, uint32_t* nids, hipStream_t st) {
    const size_t slots = (size_t)new_tiles * SQ_TILE;
    hipError_t e = hipMemsetAsync(nx, 0, slots * stride, st);  // pad slots read as zero rows
    if (e == hipSuccess) e = hipMemsetAsync(nr, 0, slots * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(nids, 0xFF, slots * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    if (old_tiles > 0)
        hipLaunchKernelGGL(ivfsq_move_tiles_kernel, dim3((unsigned)old_tiles), dim3(256), 0, st, codes, rterm, ids,
                           meta + ivf_meta_tile_list_at((size_t)nlist), meta, nmeta, stride, nx, nr, nids);
    hipLaunchKernelGGL(ivfsq_scatter_rows_kernel, dim3((unsigned)((pend_n + 3) / 4)), dim3(256), 0, st, pend, pend_rterm, pend_n, dest,
                       id0, stride, nx, nr, nids);
    return hipSuccess;
}
