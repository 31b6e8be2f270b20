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
#include "ise_pass_host.hpp"

struct ise_binary_ivf {
    int d_bits = 0, code_size = 0, ws = 0, device = 0, num_cu = 256;
    IvfLists inv;          // the lists' counts, ids and table; the sorted array has [inv.tiles * 64] slots
    u64* codes = nullptr;  // [inv.tiles * 64][ws]
    // rows added since the last rebuild, in insertion order (inv.pend_n of them)
    u64* pend = nullptr;  // [pend_cap][ws]
    long long pend_cap = 0;
    DevBuf<uint8_t> raw;  // add_host: the codes as passed
    // one set of search workspaces
    DevBuf<u64> qpad;        // one chunk's padded queries
    DevBuf<u64> lo, lists;
    DevBuf<uint32_t> masks;  // [groups][nlist]
    DevBuf<uint32_t> offs;   // [groups][nlist] | count [groups]
    DevBuf<u32x4> work;      // [groups][tiles]
    CallOrder order;
    unsigned long long* stats_dev = nullptr;  // [1] work-list entries (64-row tiles) the passes visited
    unsigned long long batches = 0, passes = 0;
    hipStream_t stream = nullptr;
    std::mutex mu_;
};

namespace {
int check_handle(const ise_binary_ivf* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "binary inverted-list index handle is NULL"); }

int bin_wt(const ise_binary_ivf* h) { return h->ws == 1 ? 1 : h->ws == 2 ? 2 : 0; }

void free_rows(ise_binary_ivf* h) {
    if (h->codes) (void)hipFree(h->codes);
    if (h->pend) (void)hipFree(h->pend);
    h->codes = nullptr;
    h->pend = nullptr;
    h->pend_cap = 0;
    h->inv.free_rows();
}

void free_all(ise_binary_ivf* h) {
    free_rows(h);
    for (void* p : {(void*)h->raw.p, (void*)h->qpad.p, (void*)h->lo.p, (void*)h->lists.p, (void*)h->masks.p, (void*)h->offs.p,
                    (void*)h->work.p, (void*)h->stats_dev})
        if (p) (void)hipFree(p);
    h->order.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

// room for n more pending rows (mu_ held): the buffer at least doubles
int reserve_pending(ise_binary_ivf* h, long long n, hipStream_t st) {
    const long long need = h->inv.pend_n + n;
    if (need <= h->pend_cap) return ISE_OK;
    const long long cap = std::max(need, 2 * h->pend_cap);
    const size_t rb = (size_t)h->ws * sizeof(u64);
    u64* nx = nullptr;
    HIP_TRY(hipMalloc((void**)&nx, (size_t)cap * rb));
    hipError_t e = hipSuccess;
    if (h->inv.pend_n > 0) {
        e = hipMemcpyAsync(nx, h->pend, (size_t)h->inv.pend_n * rb, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        (void)hipFree(nx);
        return ise_fail_(ISE_E_HIP, std::string("growing the pending rows: ") + hipGetErrorString(e));
    }
    if (h->pend) (void)hipFree(h->pend);
    h->pend = nx;
    h->pend_cap = cap;
    return ISE_OK;
}

// pending rows [at, at + m) <- x_dev's m codes of code_size bytes, padded to ws words (every word written)
int pad_pending(ise_binary_ivf* h, const uint8_t* x_dev, long long at, long long m, hipStream_t st) {
    const long long total = m * h->ws;
    hipLaunchKernelGGL(binary_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x_dev, h->code_size,
                       h->pend + (size_t)at * h->ws, h->ws, m);
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// the pending rows into the lists (mu_ held).  Blocks.  Nothing changes if an allocation fails
int rebuild_locked(ise_binary_ivf* h, hipStream_t st) {
    IvfLists& inv = h->inv;
    if (inv.pend_n == 0) return ISE_OK;
    IvfPlan pl;
    if (!inv.plan(&pl, BIN_IVF_TILE)) return ise_fail_(ISE_E_INVALID, "the lists' 64-row tiles no longer fit 32-bit slot numbers");
    const size_t slots = (size_t)pl.tile0[(size_t)inv.nlist] * BIN_IVF_TILE;
    u64* nx = nullptr;
    uint32_t *nids = nullptr, *nmeta = nullptr, *dest = nullptr;
    DevFreeList<4> fr{{(void**)&nx, (void**)&nids, (void**)&nmeta, (void**)&dest}};
    std::vector<uint32_t> meta_host;
    HIP_TRY(hipMalloc((void**)&nx, slots * h->ws * sizeof(u64)));
    int rc = inv.begin_rebuild(pl, BIN_IVF_TILE, st, meta_host, &nids, &nmeta, &dest);
    if (rc) return rc;
    HIP_TRY(binary_ivf_rebuild_launch(h->codes, inv.ids, inv.meta, inv.tiles, h->pend, inv.pend_n, dest, (uint32_t)(inv.n - inv.pend_n),
                                      h->ws, inv.nlist, nmeta, (long long)pl.tile0[(size_t)inv.nlist], nx, nids, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::swap(h->codes, nx);  // the old array goes with the guard (hipFree waits for the passes that still read it)
    inv.finish_rebuild(pl, &nids, &nmeta);
    if (h->pend) (void)hipFree(h->pend);
    h->pend = nullptr;
    h->pend_cap = 0;
    return ISE_OK;
}

// blocks of a pass: the flat Hamming pass's rule (ise_binary_scan.hip) on the lists' tiles in all (the host does not know
// how many a group's work list holds without a wait): about two tiles per wave, at most two blocks per CU and the merge's
// list count
unsigned pass_grid(const ise_binary_ivf* h) { return coded_grid(h->inv.tiles, 2, BIN_WAVES, 2, h->num_cu); }

// mu_ held.  Enqueues only, unless rows are pending (the rebuild blocks) or a workspace has to grow
int search_enqueue(ise_binary_ivf* h, const uint8_t* q_dev, long long nq, int k, const long long* probes_dev, int nprobe, int* D_dev,
                   long long* I_dev, hipStream_t st) {
    h->batches++;
    // a search still in flight on another stream comes first on the device: before the rebuild and before the
    // workspaces are written
    int rc = h->order.wait(st);
    if (rc) return rc;
    if ((rc = rebuild_locked(h, st))) return rc;
    const IvfLists& inv = h->inv;
    if (inv.tiles == 0) {  // an empty index: padding, no pass
        knn_fill_launch(D_dev, I_dev, nq * k, 0, st);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    const int gmax = BIN_IVF_CHUNK / BIN_QT;
    const unsigned grid = pass_grid(h);
    const size_t nl = (size_t)inv.nlist;
    const hipEvent_t busy = h->order.busy();
    if ((rc = grow_after_event(h->qpad, (size_t)BIN_IVF_CHUNK * h->ws, busy))) return rc;
    if ((rc = grow_after_event(h->lo, (size_t)BIN_QT, busy))) return rc;
    if ((rc = grow_after_event(h->lists, (size_t)grid * BIN_QT * BIN_KPASS, busy))) return rc;
    if ((rc = grow_after_event(h->masks, (size_t)gmax * nl, busy))) return rc;
    if ((rc = grow_after_event(h->offs, (size_t)gmax * nl + gmax, busy))) return rc;
    if ((rc = grow_after_event(h->work, (size_t)gmax * inv.tiles, busy))) return rc;
    CallOrder::Scope release{h->order, st};
    uint32_t* counts = h->offs.p + (size_t)gmax * nl;
    const int wt = bin_wt(h);
    for (long long c0 = 0; c0 < nq; c0 += BIN_IVF_CHUNK) {
        // the chunk's padded queries, masks and work lists (in stream order behind the passes that read the last chunk's)
        const int m = (int)std::min<long long>(BIN_IVF_CHUNK, nq - c0);
        const int groups = (m + BIN_QT - 1) / BIN_QT;
        // all 64 rows are written: a pass reads [16][ws] words whatever its group holds
        HIP_TRY(hipMemsetAsync(h->qpad.p, 0, (size_t)BIN_IVF_CHUNK * h->ws * sizeof(u64), st));
        hipLaunchKernelGGL(binary_pad_kernel, dim3((unsigned)(((long long)m * h->ws + 255) / 256)), dim3(256), 0, st,
                           q_dev + (size_t)c0 * h->code_size, h->code_size, h->qpad.p, h->ws, (long long)m);
        HIP_TRY(ivfsq_work_list_launch(probes_dev + (size_t)c0 * nprobe, m, nprobe, inv.nlist, 4, inv.meta, (uint32_t)inv.tiles,
                                       h->masks.p, h->offs.p, counts, h->work.p, st));
        for (int g = 0; g < groups; g++) {
            const long long q0 = c0 + (long long)g * BIN_QT;
            const int nqt = (int)std::min<long long>(BIN_QT, nq - q0);
            for (int off = 0; off < k; off += BIN_KPASS) {
                const int kp = std::min(BIN_KPASS, k - off);
                BinIvfScanParams sp{};
                sp.codes = h->codes;
                sp.ids = inv.ids;
                sp.ws = h->ws;
                sp.qpad = h->qpad.p + (size_t)g * BIN_QT * h->ws;
                sp.nqt = nqt;
                sp.kp = kp;
                sp.lo = off == 0 ? nullptr : h->lo.p;  // the merge of the pass before wrote it
                sp.lists = h->lists.p;
                sp.work = h->work.p + (size_t)g * inv.tiles;
                sp.count = counts + g;
                sp.tiles_loaded = h->stats_dev;
                binary_ivf_scan_launch(wt, grid, h->ws, st, sp);
                pass_merge_launch(h->lists.p, BIN_QT, BIN_KPASS, grid, nqt, kp, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, h->lo.p, k,
                                  off, 0, st);
                h->passes++;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
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
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_binary_ivf* h = new (std::nothrow) ise_binary_ivf();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d_bits = d_bits;
    h->code_size = d_bits / 8;
    const int w = (h->code_size + 7) / 8;
    h->ws = w == 1 ? 1 : (w + 1) / 2 * 2;
    h->device = device;
    h->num_cu = num_cu;
    h->inv.nlist = nlist;
    h->inv.clear();
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->order.create();
    if (e == hipSuccess) e = hipMalloc((void**)&h->stats_dev, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->stats_dev, 0, sizeof(unsigned long long));
    if (e != hipSuccess) {
        free_all(h);
        delete h;
        return ise_fail_(ISE_E_HIP, std::string("binary inverted-list index setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_binary_ivf_destroy(ise_binary_ivf_t* h) {
    if (!h) return ISE_OK;
    {
        DeviceGuard gd(h->device);
        (void)hipDeviceSynchronize();
        free_all(h);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_binary_ivf_reset(ise_binary_ivf_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());
    free_rows(h);
    h->order.forget();  // the device has drained
    return ISE_OK;
}

extern "C" int ise_binary_ivf_info(const ise_binary_ivf_t* h, int* d_bits, int* nlist, int64_t* ntotal, int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d_bits) *d_bits = h->d_bits;
    if (nlist) *nlist = h->inv.nlist;
    if (ntotal) *ntotal = h->inv.n;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_binary_ivf_add_host(ise_binary_ivf_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, codes, list_no, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (n == 0) return ISE_OK;
    if ((rc = h->inv.check_lists(list_no, n))) return rc;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    if ((rc = reserve_pending(h, n, st))) return rc;
    const long long step = upload_step((size_t)h->code_size);
    if ((rc = grow_after_event(h->raw, (size_t)std::min<long long>(step, n) * h->code_size, nullptr))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {  // nothing is counted in before the last piece is in place
        const long long m = std::min<long long>(step, n - i0);
        HIP_TRY(hipMemcpyAsync(h->raw.p, codes + (size_t)i0 * h->code_size, (size_t)m * h->code_size, hipMemcpyHostToDevice, st));
        if ((rc = pad_pending(h, h->raw.p, h->inv.pend_n + i0, m, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));  // the next piece overwrites raw
    }
    h->inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_binary_ivf_add_device(ise_binary_ivf_t* h, const uint8_t* codes_dev, const int64_t* list_no_dev, int64_t n,
                                         void* stream) {
    int rc = check_add_args(h, codes_dev, list_no_dev, n);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::vector<int64_t> lists((size_t)n);
    HIP_TRY(hipMemcpyAsync(lists.data(), list_no_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = h->inv.check_lists(lists.data(), n))) return rc;
    if ((rc = reserve_pending(h, n, st))) return rc;
    if ((rc = pad_pending(h, codes_dev, h->inv.pend_n, n, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // the pending rows are in place: the caller may free its codes, a rebuild may run on any stream
    h->inv.add(lists.data(), n);
    return ISE_OK;
}

extern "C" int ise_binary_ivf_list_sizes_host(ise_binary_ivf_t* h, int64_t* sizes) {
    if (!sizes) return ise_fail_(ISE_E_INVALID, "sizes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    h->inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_binary_ivf_list_host(ise_binary_ivf_t* h, int list, int64_t* ids, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (list < 0 || list >= h->inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = rebuild_locked(h, h->stream);
    if (rc) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->inv.list_ids_host(list, BIN_IVF_TILE, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    if (codes)
        HIP_TRY(hipMemcpy2D(codes, (size_t)h->code_size, h->codes + slot0 * h->ws, (size_t)h->ws * sizeof(u64), (size_t)h->code_size, m,
                            hipMemcpyDeviceToHost));
    return ISE_OK;
}

extern "C" int ise_binary_ivf_search_device(ise_binary_ivf_t* h, const uint8_t* q_dev, int64_t nq, int k, const int64_t* probes_dev,
                                            int nprobe, int32_t* D_dev, int64_t* I_dev, void* stream) {
    const int rc = check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, (int*)D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_binary_ivf_search_host(ise_binary_ivf_t* h, const uint8_t* q, int64_t nq, int k, const int64_t* probes, int nprobe,
                                          int32_t* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return ivf_search_staged(h->code_size, h->stream, q, nq, k, probes, nprobe, (int*)D, I,
                             [&](const uint8_t* q_dev, long long m, const long long* p_dev, int* D_dev, long long* I_dev) {
                                 return search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->stream);
                             });
}

extern "C" int ise_binary_ivf_stats(ise_binary_ivf_t* h, uint64_t* out3) {
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    unsigned long long loaded = 0;
    HIP_TRY(hipDeviceSynchronize());  // the passes enqueued so far have added their entries
    HIP_TRY(hipMemcpy(&loaded, h->stats_dev, sizeof(loaded), hipMemcpyDeviceToHost));
    out3[0] = h->batches;
    out3[1] = h->passes;
    out3[2] = loaded;
    return ISE_OK;
}
