// ivfsq_lists_harness.hip -- test-only launchers around the work list and the rebuild of the 8-bit inverted lists
// (csrc/ise_ivf_tiles.hpp: ivf_mask_kernel, ivf_offsets_kernel, ivf_work_kernel, ivf_move_tiles_kernel<64, u32x4>,
// ivf_scatter_rows_kernel<u32x4>), and around the rebuild of any kind's lists (chk_ivf_rebuild: every instantiation of
// the two rebuild kernels, the float32 lists' 16-row tiles among them), so that tests/test_ivfsq_lists_gpu.py and
// tests/test_ivf_rebuild_gpu.py can hand them crafted probe tables and list tables and read every table they write.
// Built by csrc/Makefile into libise_ivfsq_check.so; never linked into libise_knn.so.  The header is included as it
// is, and the launches are the product's own (ivf_work_list_launch, ivf_rebuild_launch): whatever is wrong here is wrong
// in the product.
//
// Every launcher takes device pointers, launches on the null stream and returns hipGetLastError() as an int.  The
// callers validate the sizes of every array against the tables (tests/test_ivfsq_lists_gpu.py, the wrappers at its
// top); the kernels trust them.
#include "ise_ivf_tiles.hpp"

#define HARNESS_BAD_ARGS ((int)hipErrorInvalidValue)

// probes [nq][nprobe] int64; meta: list_tile0 [nlist + 1] | list_size [nlist] | tile_list [tiles]; masks, offs
// [groups][nlist], counts [groups], work [groups][tiles][4], groups = ceil(nq / 2^qshift)
extern "C" int chk_ivfsq_work_list(const long long* probes, int nq, int nprobe, int nlist, int qshift, const uint32_t* meta,
                                   long long tiles, uint32_t* masks, uint32_t* offs, uint32_t* counts, uint32_t* work) {
    if (nq <= 0 || nprobe <= 0 || nlist <= 0 || (qshift != 3 && qshift != 4) || tiles < 0 || tiles >= (1ll << 26)) return HARNESS_BAD_ARGS;
    const hipError_t e = ivf_work_list_launch(probes, nq, nprobe, nlist, qshift, meta, (uint32_t)tiles, masks, offs, counts,
                                                reinterpret_cast<u32x4*>(work), nullptr);
    return e != hipSuccess ? (int)e : (int)hipGetLastError();
}

// the old arrays codes [old_tiles 64][stride], rterm, ids [old_tiles 64] with their table meta; the pending rows pend
// [pend_n][stride], pend_rterm [pend_n] and their slots dest [pend_n]; the new table nmeta and the new arrays of
// new_tiles tiles.  stride: a multiple of 16
extern "C" int chk_ivfsq_rebuild(const uint8_t* codes, const double* rterm, const uint32_t* ids, const uint32_t* meta,
                                 long long old_tiles, const uint8_t* pend, const double* pend_rterm, long long pend_n,
                                 const uint32_t* dest, uint32_t id0, int stride, int nlist, const uint32_t* nmeta,
                                 long long new_tiles, uint8_t* nx, double* nr, uint32_t* nids) {
    if (old_tiles < 0 || pend_n <= 0 || stride <= 0 || stride % 16 != 0 || nlist <= 0 || new_tiles <= 0 || new_tiles >= (1ll << 26))
        return HARNESS_BAD_ARGS;
    const hipError_t e = ivf_rebuild_launch(64, 16, (size_t)stride, {(void*)codes, (void*)rterm, (uint32_t*)ids}, meta, old_tiles,
                                            {(void*)pend, (void*)pend_rterm, nullptr}, pend_n, dest, id0, nlist, nmeta, new_tiles,
                                            {nx, nr, nids}, nullptr);
    return e != hipSuccess ? (int)e : (int)hipGetLastError();
}

// the rebuild of any kind's lists: tile_rows rows a tile, rows of row_bytes moved in units of unit_bytes, no side value.
// The arrays as above: rows [tiles tile_rows][row_bytes], ids [tiles tile_rows]
extern "C" int chk_ivf_rebuild(int tile_rows, int unit_bytes, long long row_bytes, const void* rows, const uint32_t* ids,
                               const uint32_t* meta, long long old_tiles, const void* pend, long long pend_n, const uint32_t* dest,
                               uint32_t id0, int nlist, const uint32_t* nmeta, long long new_tiles, void* nx, uint32_t* nids) {
    if (old_tiles < 0 || pend_n <= 0 || unit_bytes <= 0 || row_bytes <= 0 || row_bytes % unit_bytes != 0 || row_bytes > (1 << 20) ||
        nlist <= 0 || new_tiles <= 0 || new_tiles >= (1ll << 26) || old_tiles > new_tiles)
        return HARNESS_BAD_ARGS;
    const hipError_t e = ivf_rebuild_launch(tile_rows, unit_bytes, (size_t)row_bytes, {(void*)rows, nullptr, (uint32_t*)ids}, meta,
                                            old_tiles, {(void*)pend, nullptr, nullptr}, pend_n, dest, id0, nlist, nmeta, new_tiles,
                                            {nx, nullptr, nids}, nullptr);
    return e != hipSuccess ? (int)e : (int)hipGetLastError();
}
