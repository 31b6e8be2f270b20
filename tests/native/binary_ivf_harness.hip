// binary_ivf_harness.hip -- test-only launchers around one pass and the rebuild of the inverted lists over bit codes
// (csrc/ise_binary_ivf.hpp: binary_ivf_scan_kernel; csrc/ise_ivf_tiles.hpp: ivf_move_tiles_kernel<64, u64>,
// ivf_scatter_rows_kernel<u64>; csrc/ise_merge.hpp: pass_merge_kernel<int>), so that tests/test_binary_ivf_lists_gpu.py
// can hand them crafted work lists, floors and list tables and read every word they write.  Built by csrc/Makefile into
// libise_binary_ivf_check.so; never linked into libise_knn.so.  The headers are included as they are, and the launches
// are the product's own (binary_ivf_scan_launch, pass_merge_launch<int>, ivf_rebuild_launch): whatever is wrong here
// is wrong in the product.
//
// Every launcher takes device pointers, launches on the null stream and returns hipGetLastError() as an int.  The
// callers validate the sizes of every array against the tables (tests/test_binary_ivf_lists_gpu.py, the wrappers at
// its top); the kernels trust them.
#include "ise_binary_ivf.hpp"
#include "ise_pass_host.hpp"

#define HARNESS_BAD_ARGS ((int)hipErrorInvalidValue)

// One pass as search_enqueue runs it: the scan of the group's work list, then the merge of the blocks' lists.
// codes [tiles 64][ws], ids [tiles 64]; qpad [16][ws]; lo_in [nqt] or NULL (the first pass); lists [grid][16][32];
// work [count][4] (tile, valid rows, query mask, 0), count [1], tiles_loaded [1]; D, I [nqt][k], written at
// [off, off + kp); lo_out [nqt]
extern "C" int chk_binary_ivf_pass(const u64* codes, const uint32_t* ids, int ws, const u64* qpad, int nqt, int kp, const u64* lo_in,
                                   u64* lists, const uint32_t* work, const uint32_t* count, unsigned long long* tiles_loaded,
                                   int grid, int* D, long long* I, u64* lo_out, int k, int off) {
    if (ws < 1 || ws > BIN_MAX_WS || (ws != 1 && ws % 2 != 0) || nqt < 1 || nqt > BIN_QT || kp < 1 || kp > BIN_KPASS || grid < 1 ||
        grid > MERGE_LISTS_MAX || off < 0 || k < 1 || off > k - kp)
        return HARNESS_BAD_ARGS;
    BinIvfScanParams sp{};
    sp.codes = codes;
    sp.ids = ids;
    sp.ws = ws;
    sp.qpad = qpad;
    sp.nqt = nqt;
    sp.kp = kp;
    sp.lo = lo_in;
    sp.lists = lists;
    sp.work = reinterpret_cast<const u32x4*>(work);
    sp.count = count;
    sp.tiles_loaded = tiles_loaded;
    binary_ivf_scan_launch(ws == 1 ? 1 : ws == 2 ? 2 : 0, (unsigned)grid, ws, nullptr, sp);
    pass_merge_launch<int>(lists, BIN_QT, BIN_KPASS, (unsigned)grid, nqt, kp, D, I, lo_out, k, off, 0, nullptr);
    return (int)hipGetLastError();
}

// the old arrays codes [old_tiles 64][ws], ids [old_tiles 64] with their table meta (not read without an old tile); the
// pending rows pend [pend_n][ws] and their slots dest [pend_n]; the new table nmeta and the new arrays of new_tiles tiles
extern "C" int chk_binary_ivf_rebuild(const u64* codes, const uint32_t* ids, const uint32_t* meta, long long old_tiles, const u64* pend,
                                      long long pend_n, const uint32_t* dest, uint32_t id0, int ws, int nlist, const uint32_t* nmeta,
                                      long long new_tiles, u64* nx, uint32_t* nids) {
    if (old_tiles < 0 || pend_n <= 0 || ws < 1 || ws > BIN_MAX_WS || (ws != 1 && ws % 2 != 0) || nlist <= 0 || new_tiles <= 0 ||
        new_tiles >= (1ll << 26) || old_tiles > new_tiles)
        return HARNESS_BAD_ARGS;
    const hipError_t e = ivf_rebuild_launch(BIN_IVF_TILE, sizeof(u64), (size_t)ws * sizeof(u64), {(void*)codes, nullptr, (uint32_t*)ids},
                                            meta, old_tiles, {(void*)pend, nullptr, nullptr}, pend_n, dest, id0, nlist, nmeta, new_tiles,
                                            {nx, nullptr, nids}, nullptr);
    return e != hipSuccess ? (int)e : (int)hipGetLastError();
}
