// ivfsq_lists_harness.hip -- test-only launchers around the work list and the rebuild of the 8-bit inverted lists
// (csrc/ise_ivf_lists.hpp: ivf_mask_kernel; csrc/ise_ivfsq.hpp: ivfsq_offsets_kernel, ivfsq_work_kernel,
// ivfsq_move_tiles_kernel, ivfsq_scatter_rows_kernel), so that tests/test_ivfsq_lists_gpu.py can hand them crafted
// probe tables and list tables and read every table they write.  Built by csrc/Makefile into libise_ivfsq_check.so;
// never linked into libise_knn.so.  The headers are included as they are, and the launches are the product's own
// (ivfsq_work_list_launch, ivfsq_rebuild_launch): whatever is wrong here is wrong in the product.
//
// Every launcher takes device pointers, launches on the null stream and returns hipGetLastError() as an int.  The
// callers validate the sizes of every array against the tables (tests/test_ivfsq_lists_gpu.py, the wrappers at its
// top); the kernels trust them.
#include "ise_ivf_lists.hpp"
#include "ise_ivfsq.hpp"

#define HARNESS_BAD_ARGS ((int)hipErrorInvalidValue)

// probes [nq][nprobe] int64; meta: list_tile0 [nlist + 1] | list_size [nlist] | tile_list [tiles]; masks, offs
// [groups][nlist], counts [groups], work [groups][tiles][4], groups = ceil(nq / 2^qshift)
extern "C" int chk_ivfsq_work_list(const long long* probes, int nq, int nprobe, int nlist, int qshift, const uint32_t* meta,
                                   long long tiles, uint32_t* masks, uint32_t* offs, uint32_t* counts, uint32_t* work) {
    if (nq <= 0 || nprobe <= 0 || nlist <= 0 || (qshift != 3 && qshift != 4) || tiles < 0 || tiles >= (1ll << 26)) return HARNESS_BAD_ARGS;
    const hipError_t e = ivfsq_work_list_launch(probes, nq, nprobe, nlist, qshift, meta, (uint32_t)tiles, masks, offs, counts,
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
    const hipError_t e = ivfsq_rebuild_launch(codes, rterm, ids, meta, old_tiles, pend, pend_rterm, pend_n, dest, id0, stride, nlist,
                                              nmeta, new_tiles, nx, nr, nids, nullptr);
    return e != hipSuccess ? (int)e : (int)hipGetLastError();
}
