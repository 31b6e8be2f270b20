// ise_ivfsq.hpp -- kernels of IndexIVFScalarQuantizer: inverted lists over the 8-bit rows of ise_sq.hpp and the pass
// that scans only the probed ones (include/ise_knn.h, ise_ivfsq_*).  Host side: ise_ivfsq.hip.
//
// Layout.  All lists live in ONE array: codes [slots][stride] (stride = d rounded up to 64, pad bytes zero), rterm
// [slots] float64 (ise_sq.hpp's row term) and ids [slots] uint32 (the row's insertion number).  List l owns the 64-row
// tiles [list_tile0[l], list_tile0[l + 1]) -- SQ_TILE rows, a wave's unit in the byte scan; inside a list the slots are
// in ascending id order, the slots behind list_size[l] rows are zero rows with id 0xFFFFFFFF, masked by position.
//
// A pass serves one group of QT = sq_qt(d) queries and 32 results:
//   masks, work list   the lists' own kernels (ivf_work_list_launch, ise_ivf_tiles.hpp): per group of QT
//              queries the entries (tile, valid rows in it, the list's query mask) of the probed lists' tiles, in slot
//              order, so the list is the same whatever the launch does.
//   scan       ivfsq_scan_kernel is sq_scan_body (ise_sq.hpp) walking the entries instead of the tiles: wave w of block
//              b takes entries b SQ_WAVES + w + j gridDim.x SQ_WAVES.  The key is ord(score) << 32 | ids[slot]; keys are
//              unique and compared in full, so ties go by ascending id however the lists order the ids.
// The staging record, the selection (ise_cand.hpp), the pass's merge and the floor-keyed repeat for k > 32 are ise_sq.hpp's.
// A rebuild (ivf_rebuild_launch, ise_ivf_tiles.hpp) moves rows in 16-byte units, the row terms as the slots' side values.
#pragma once
#include "ise_ivf_tiles.hpp"
#include "ise_sq.hpp"

static_assert(SQ_TILE == IVF_WORK_TILE, "ivf_work_kernel counts a tile's valid rows in units of IVF_WORK_TILE");

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
