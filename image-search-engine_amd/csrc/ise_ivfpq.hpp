// ise_ivfpq.hpp -- kernels of IndexIVFPQ with by_residual = false: inverted lists over the code rows of ise_pq.hpp and
// the pass that scans only the probed ones (include/ise_knn.h, ise_ivfpq_*).  Host side: ise_ivfpq.hip.
//
// Layout.  All lists live in ONE array: codes [slots][stride] (stride = M rounded up to 16, pad bytes zero) and ids
// [slots] uint32 (the row's insertion number); no side value.  List l owns the 64-row tiles [list_tile0[l],
// list_tile0[l + 1]); inside a list the slots are in ascending id order, the slots behind list_size[l] rows are zero
// rows with id 0xFFFFFFFF.  A zero row is a VALID code (centroid 0 of every sub-quantiser) and may score best: the
// position mask of the entry (valid rows) is the only thing that keeps a pad slot out.
//
// A pass serves one group of QT = pq_qt(M) queries and 32 results:
//   tables     pq_table_kernel, as it is: one launch per chunk of PQ_TAB_CHUNK queries, [group][m][256][QT].
//   masks, work list   the lists' own kernels (ivf_work_list_launch, ise_ivf_tiles.hpp) with qshift =
//              log2(QT): per group the entries (tile, valid rows in it, the list's query mask) of the probed lists' tiles.
//   scan       ivfpq_scan_kernel is pq_scan_body (ise_pq.hpp) walking the entries instead of the tiles: wave w of block
//              b takes entries b PQ_WAVES + w + j gridDim.x PQ_WAVES, a lane owns slot tile * 64 + lane.  The key is
//              ord(score) << 32 | ids[slot]; keys are unique and compared in full, so ties go by ascending id however
//              the lists order the ids.  The gathers run in ascending m from +0.0f over the same tables as the flat
//              index's: a (query, row) pair scores the same bits in both.
// The selection (ise_cand.hpp), the pass's merge and the floor-keyed repeat for k > 32 are ise_pq.hpp's.  A rebuild
// (ivf_rebuild_launch, ise_ivf_tiles.hpp) moves rows in 16-byte units.
#pragma once
#include "ise_ivf_tiles.hpp"
#include "ise_pq.hpp"

static_assert(IVF_WORK_TILE == 64, "a lane owns slot tile * 64 + lane");
#define PQ_IVF_TILE 64 /* rows of a tile: a wave's unit in the scan */

struct PqIvfScanParams {
    const uint8_t* codes;  // [tiles * 64][stride]
    const uint32_t* ids;   // [tiles * 64]
    int M, stride;
    const float* tab;  // the pass's tables, [M][256][QT]
    int nqt, kp;
    int ip;
    const u64* lo;          // [nqt] floors, or null in the first pass
    u64* lists;             // [grid][QT][PQ_KPASS]
    const u32x4* work;      // the group's entries: (tile, valid rows, query mask, 0)
    const uint32_t* count;  // [1] entries of the group
    unsigned long long* tiles_loaded;  // += the entries this pass visits
};

template <int QT>
__global__ __launch_bounds__(PQ_WAVES * 64) void ivfpq_scan_kernel(const PqIvfScanParams p) {
    pq_scan_body<QT, true>(p);
}
