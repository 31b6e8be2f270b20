// ise_binary_ivf.hip -- host side and C ABI of the inverted-list index over bit codes (include/ise_knn.h,
// ise_binary_ivf_*; kernels in ise_binary_ivf.hpp).  faiss.IndexBinaryIVF.
//
// The lists are the 8-bit lists' (IvfLists, ise_ivf_lists.hpp) with 64-row tiles: rows come in with their list numbers
// (the coarse quantiser lives with the caller), add() pads them to ws words at once into a PENDING buffer; the first
// call that reads the lists afterwards (search, list_host) rebuilds: the host's counting sort (ise_ivf_plan.hpp) says
// where every pending row goes, the old tiles move to where their lists now start, the pending rows are scattered
// behind them.  Codes, ids and the tables go into fresh buffers that are swapped in together (a pass still in flight on
// another stream keeps a consistent set); the old ones and the pending buffer are freed when it is done.
//
// Calls on one handle run one at a time (a mutex).  The handle has ONE set of search workspaces: a search waits for
// the one before and marks its end once a pass may be enqueued (CallOrder, ise_host.hpp), and a workspace that has to
// grow is replaced by the after-event rule (grow_after_event, ise_host.hpp).
#include "ise_binary_ivf.hpp"
#include "ise_ivf_lists.hpp"

struct ise_binary_ivf {
    int d_bits = 0, code_size = 0, ws = 0;
    IvfCore c;            // the sorted codes are c.rows: [c.inv.tiles * 64][ws] words, no side value
    DevBuf<uint8_t> raw;  // add_host: the codes as passed
    IvfTiledWs w;         // one set of search workspaces; w.stage: one chunk's padded queries
};

namespace {
int check_handle(const ise_binary_ivf* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "binary inverted-list index handle is NULL"); }

void free_own(ise_binary_ivf* h) {
    buf_free(h->raw);
    h->w.free();
}

// pending rows [at, at + m) <- x_dev's m codes of code_size bytes, padded to ws words (every word written)
int pad_pending(ise_binary_ivf* h, const uint8_t* x_dev, long long at, long long m, hipStream_t st) {
    const long long total = m * h->ws;
    hipLaunchKernelGGL(binary_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x_dev, h->code_size,
                       h->c.pend_row<u64>(at), h->ws, m);
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// mu_ held.  The shell is the lists' (ivf_tiled_search): this is how a chunk's queries are padded and what a pass is handed.
// Blocks of a pass: the flat Hamming pass's rule (ise_binary_scan.hip) on the lists' tiles in all: about two tiles per
// wave, at most two blocks per CU
int search_enqueue(ise_binary_ivf* h, const uint8_t* q_dev, long long nq, int k, const long long* probes_dev, int nprobe, int* D_dev,
                   long long* I_dev, hipStream_t st) {
    const int ws = h->ws, wt = ws == 1 ? 1 : ws == 2 ? 2 : 0;
    const size_t qbytes = (size_t)BIN_IVF_CHUNK * ws * sizeof(u64);
    const IvfTiledShape shape{BIN_IVF_CHUNK, BIN_QT, 4, BIN_KPASS, 2, BIN_WAVES, 2, qbytes};
    auto qpad = [&]() { return reinterpret_cast<u64*>(h->w.stage.p); };
    return ivf_tiled_search(
        h->c, h->w, shape, nq, k, probes_dev, nprobe, D_dev, I_dev, 0, st,
        [&](long long c0, int m) {
            // all 64 rows are written: a pass reads [16][ws] words whatever its group holds
            HIP_TRY(hipMemsetAsync(qpad(), 0, qbytes, st));
            hipLaunchKernelGGL(binary_pad_kernel, dim3((unsigned)(((long long)m * ws + 255) / 256)), dim3(256), 0, st,
                               q_dev + (size_t)c0 * h->code_size, h->code_size, qpad(), ws, (long long)m);
            return (int)ISE_OK;
        },
        [&](const IvfPass& ps) {
            BinIvfScanParams sp{};
            sp.codes = h->c.rows_as<u64>();
            sp.ids = h->c.inv.ids;
            sp.ws = ws;
            sp.qpad = qpad() + (size_t)ps.g * BIN_QT * ws;
            sp.nqt = ps.nqt;
            sp.kp = ps.kp;
            sp.lo = ps.lo;
            sp.lists = ps.lists;
            sp.work = ps.work;
            sp.count = ps.count;
            sp.tiles_loaded = h->c.stats_dev;
            binary_ivf_scan_launch(wt, ps.grid, ws, st, sp);
        });
}

int check_search_args(const ise_binary_ivf* h, const void* q, long long nq, int k, const void* probes, int nprobe, const void* D,
                      const void* I) {
    const int rc = check_ivf_knn_args(q, nq, k, probes, nprobe, D, I);
    return rc ? rc : check_handle(h);
}

int check_add_args(const ise_binary_ivf* h, const void* x, const void* list_no, long long n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !list_no)) return ise_fail_(ISE_E_INVALID, "codes or list numbers pointer is NULL");
    return check_handle(h);
}
}  // namespace

extern "C" int ise_binary_ivf_create(ise_binary_ivf_t** out, int d_bits, int nlist, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d_bits <= 0 || d_bits % 8 != 0 || d_bits > ISE_BINARY_MAX_BITS)
        return ise_fail_(ISE_E_INVALID, "d_bits must be a positive multiple of 8, at most ISE_BINARY_MAX_BITS");
    if (nlist <= 0) return ise_fail_(ISE_E_INVALID, "nlist must be positive");
    return ivf_create(out, nlist, device, "binary inverted-list index setup",
                      [&](ise_binary_ivf* h) {
                          h->d_bits = d_bits;
                          h->code_size = d_bits / 8;
                          const int w = (h->code_size + 7) / 8;
                          h->ws = w == 1 ? 1 : (w + 1) / 2 * 2;
                          h->c.tile_rows = BIN_IVF_TILE;
                          h->c.unit_bytes = sizeof(u64);
                          h->c.row_bytes = (size_t)h->ws * sizeof(u64);
                          return hipSuccess;
                      },
                      free_own);
}

extern "C" int ise_binary_ivf_destroy(ise_binary_ivf_t* h) { return ivf_destroy(h, free_own); }

extern "C" int ise_binary_ivf_reset(ise_binary_ivf_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    return ivf_reset(h->c, []() {});
}

extern "C" int ise_binary_ivf_info(const ise_binary_ivf_t* h, int* d_bits, int* nlist, int64_t* ntotal, int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d_bits) *d_bits = h->d_bits;
    if (nlist) *nlist = h->c.inv.nlist;
    if (ntotal) *ntotal = h->c.inv.n;
    if (device) *device = h->c.device;
    return ISE_OK;
}

extern "C" int ise_binary_ivf_add_host(ise_binary_ivf_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, codes, list_no, n);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (n == 0) return ISE_OK;
    if ((rc = h->c.inv.check_lists(list_no, n)) || (rc = en.check())) return rc;
    hipStream_t st = h->c.stream;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    const long long step = upload_step((size_t)h->code_size);
    if ((rc = grow_after_event(h->raw, (size_t)std::min<long long>(step, n) * h->code_size, nullptr))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {  // nothing is counted in before the last piece is in place
        const long long m = std::min<long long>(step, n - i0);
        HIP_TRY(hipMemcpyAsync(h->raw.p, codes + (size_t)i0 * h->code_size, (size_t)m * h->code_size, hipMemcpyHostToDevice, st));
        if ((rc = pad_pending(h, h->raw.p, h->c.inv.pend_n + i0, m, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));  // the next piece overwrites raw
    }
    h->c.inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_binary_ivf_add_device(ise_binary_ivf_t* h, const uint8_t* codes_dev, const int64_t* list_no_dev, int64_t n,
                                         void* stream) {
    int rc = check_add_args(h, codes_dev, list_no_dev, n);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    IvfEntry en(h->c);
    if (n == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    std::vector<int64_t> lists;
    if ((rc = h->c.download_lists(list_no_dev, n, st, &lists))) return rc;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    if ((rc = pad_pending(h, codes_dev, h->c.inv.pend_n, n, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // the pending rows are in place: the caller may free its codes, a rebuild may run on any stream
    h->c.inv.add(lists.data(), n);
    return ISE_OK;
}

extern "C" int ise_binary_ivf_list_sizes_host(ise_binary_ivf_t* h, int64_t* sizes) {
    if (!sizes) return ise_fail_(ISE_E_INVALID, "sizes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    h->c.inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_binary_ivf_list_host(ise_binary_ivf_t* h, int list, int64_t* ids, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (list < 0 || list >= h->c.inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    IvfEntry en(h->c);
    int rc = en.check();
    if (rc || (rc = ivf_rebuild_locked(h->c, h->c.stream, ivf_no_hook))) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->c.inv.list_ids_host(list, BIN_IVF_TILE, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    if (codes)
        HIP_TRY(hipMemcpy2D(codes, (size_t)h->code_size, h->c.rows_as<u64>() + slot0 * h->ws, (size_t)h->ws * sizeof(u64),
                            (size_t)h->code_size, m, hipMemcpyDeviceToHost));
    return ISE_OK;
}

extern "C" int ise_binary_ivf_search_device(ise_binary_ivf_t* h, const uint8_t* q_dev, int64_t nq, int k, const int64_t* probes_dev,
                                            int nprobe, int32_t* D_dev, int64_t* I_dev, void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (nq == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    return search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, (int*)D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_binary_ivf_search_host(ise_binary_ivf_t* h, const uint8_t* q, int64_t nq, int k, const int64_t* probes, int nprobe,
                                          int32_t* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (nq == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    return ivf_search_staged(h->code_size, h->c.stream, q, nq, k, probes, nprobe, (int*)D, I,
                             [&](const uint8_t* q_dev, long long m, const long long* p_dev, int* D_dev, long long* I_dev) {
                                 return search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->c.stream);
                             });
}

extern "C" int ise_binary_ivf_stats(ise_binary_ivf_t* h, uint64_t* out3) {
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    IvfEntry en(h->c);
    const int rc = en.check();
    return rc ? rc : h->c.stats(out3);
}
