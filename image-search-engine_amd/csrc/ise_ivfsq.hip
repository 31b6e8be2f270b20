// ise_ivfsq.hip -- host side and C ABI of the inverted-list index over 8-bit rows (include/ise_knn.h, ise_ivfsq_*;
// kernels in ise_ivfsq.hpp and ise_sq.hpp).  faiss.IndexIVFScalarQuantizer with by_residual = false.
//
// The codec is the flat scalar-quantised index's (SqCodec, ise_sq_host.hpp): the trained state comes from the caller,
// rows are encoded on the device by sq_encode_kernel.  The lists are the float32 lists' (IvfLists, ise_ivf_lists.hpp):
// rows come in with their list numbers (the coarse quantiser lives with the caller), add() encodes them at once into a
// PENDING buffer of codes and row terms and reads the encoder's non-finite flag back before anything is counted in; the
// first call that reads the lists afterwards (search, list_host) rebuilds: the host's counting sort (ise_ivf_plan.hpp,
// 64-row tiles) says where every pending row goes, the old tiles move to where their lists now start, the pending rows
// are scattered behind them.  Codes, row terms, ids and the tables go into fresh buffers that are swapped in together
// (a pass still in flight on another stream keeps a consistent set); the old ones and the pending buffer are freed when
// it is done.
//
// Calls on one handle run one at a time (a mutex).  The handle has ONE set of search workspaces: a search waits for
// the one before and marks its end once a pass may be enqueued (CallOrder, ise_host.hpp), and a workspace that has to
// grow is replaced by the after-event rule (grow_after_event, ise_host.hpp).
#include "ise_ivf_lists.hpp"
#include "ise_ivfsq.hpp"
#include "ise_sq_host.hpp"

struct ise_ivfsq {
    int d = 0, stride = 0, qt = 0, qshift = 0, metric = ISE_METRIC_L2, device = 0, num_cu = 256;
    SqCodec codec;
    IvfLists inv;  // the lists' counts, ids and table; the sorted array has [inv.tiles * SQ_TILE] slots
    uint8_t* codes = nullptr;
    double* rterm = nullptr;
    // rows added since the last rebuild, in insertion order (inv.pend_n of them)
    uint8_t* pend = nullptr;        // [pend_cap][stride]
    double* pend_rterm = nullptr;   // [pend_cap]
    long long pend_cap = 0;
    // host forms (they return with the stream drained): rows or queries as passed | codes as passed
    DevBuf<float> xraw;
    DevBuf<uint8_t> craw;
    // one set of search workspaces
    DevBuf<uint8_t> qrec;    // one chunk's staged queries
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
int check_handle(const ise_ivfsq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "inverted-list scalar-quantiser index handle is NULL"); }

void free_rows(ise_ivfsq* h) {
    for (void* p : {(void*)h->codes, (void*)h->rterm, (void*)h->pend, (void*)h->pend_rterm})
        if (p) (void)hipFree(p);
    h->codes = nullptr; h->rterm = nullptr; h->pend = nullptr; h->pend_rterm = nullptr;
    h->pend_cap = 0;
    h->inv.free_rows();
}

void free_all(ise_ivfsq* h) {
    free_rows(h);
    h->codec.destroy();
    for (void* p : {(void*)h->xraw.p, (void*)h->craw.p, (void*)h->qrec.p, (void*)h->lo.p, (void*)h->lists.p,
                    (void*)h->masks.p, (void*)h->offs.p, (void*)h->work.p, (void*)h->stats_dev})
        if (p) (void)hipFree(p);
    h->order.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

// room for n more pending rows (mu_ held): the buffers at least double
int reserve_pending(ise_ivfsq* h, long long n, hipStream_t st) {
    const long long need = h->inv.pend_n + n;
    if (need <= h->pend_cap) return ISE_OK;
    const long long cap = std::max(need, 2 * h->pend_cap);
    uint8_t* nx = nullptr;
    double* nr = nullptr;
    HIP_TRY(hipMalloc((void**)&nx, (size_t)cap * h->stride));
    hipError_t e = hipMalloc((void**)&nr, (size_t)cap * sizeof(double));
    if (e == hipSuccess && h->inv.pend_n > 0) {
        e = hipMemcpyAsync(nx, h->pend, (size_t)h->inv.pend_n * h->stride, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nr, h->pend_rterm, (size_t)h->inv.pend_n * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        (void)hipFree(nx);
        if (nr) (void)hipFree(nr);
        return ise_fail_(e == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP, std::string("growing the pending rows: ") + hipGetErrorString(e));
    }
    if (h->pend) (void)hipFree(h->pend);
    if (h->pend_rterm) (void)hipFree(h->pend_rterm);
    h->pend = nx;
    h->pend_rterm = nr;
    h->pend_cap = cap;
    return ISE_OK;
}

// pending rows [at, at + m) <- the codes and row terms of x_dev's rows (pad bytes zero); sets the codec's bad flag on a non-finite entry
int encode_pending(ise_ivfsq* h, const float* x_dev, long long at, long long m, hipStream_t st) {
    uint8_t* dst = h->pend + (size_t)at * h->stride;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)m * h->stride, st));
    h->codec.encode_launch(x_dev, m, dst, h->stride, h->pend_rterm + at, st);
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// the pending rows into the lists (mu_ held).  Blocks.  Nothing changes if an allocation fails
int rebuild_locked(ise_ivfsq* h, hipStream_t st) {
    IvfLists& inv = h->inv;
    if (inv.pend_n == 0) return ISE_OK;
    IvfPlan pl;
    if (!inv.plan(&pl, SQ_TILE)) return ise_fail_(ISE_E_INVALID, "the lists' 64-row tiles no longer fit 32-bit slot numbers");
    const size_t slots = (size_t)pl.tile0[(size_t)inv.nlist] * SQ_TILE;
    uint8_t* nx = nullptr;
    double* nr = nullptr;
    uint32_t *nids = nullptr, *nmeta = nullptr, *dest = nullptr;
    DevFreeList<5> fr{{(void**)&nx, (void**)&nr, (void**)&nids, (void**)&nmeta, (void**)&dest}};
    std::vector<uint32_t> meta_host;
    HIP_TRY(hipMalloc((void**)&nx, slots * h->stride));
    HIP_TRY(hipMalloc((void**)&nr, slots * sizeof(double)));
    int rc = inv.begin_rebuild(pl, SQ_TILE, st, meta_host, &nids, &nmeta, &dest);
    if (rc) return rc;
    HIP_TRY(ivfsq_rebuild_launch(h->codes, h->rterm, inv.ids, inv.meta, inv.tiles, h->pend, h->pend_rterm, inv.pend_n, dest,
                                 (uint32_t)(inv.n - inv.pend_n), h->stride, inv.nlist, nmeta, (long long)pl.tile0[(size_t)inv.nlist], nx,
                                 nr, nids, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::swap(h->codes, nx);  // the old arrays go with the guard (hipFree waits for the passes that still read them)
    std::swap(h->rterm, nr);
    inv.finish_rebuild(pl, &nids, &nmeta);
    if (h->pend) (void)hipFree(h->pend);
    if (h->pend_rterm) (void)hipFree(h->pend_rterm);
    h->pend = nullptr;
    h->pend_rterm = nullptr;
    h->pend_cap = 0;
    return ISE_OK;
}

void launch_scan(int qt, unsigned grid, size_t lds, hipStream_t st, const SqIvfScanParams& sp) {
    static LdsAttrOnce attr[2];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), SQ_LDS_LIMIT);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SQ_WAVES * 64), lds, st, sp);
    };
    if (qt == 16) go(ivfsq_scan_kernel<16>, attr[0]);
    else go(ivfsq_scan_kernel<8>, attr[1]);
}

// blocks of a pass: ise_sq.hip's rule on the lists' tiles in all (the host does not know how many a group's work list
// holds without a wait): about SQ_BLOCK_TILES tiles per wave, at most what the CUs hold at once and the merge's list count
unsigned pass_grid(const ise_ivfsq* h) {
    const long long per_cu = std::max<long long>(1, (long long)SQ_LDS_LIMIT / (long long)sq_lds_bytes(h->d, h->qt));
    return coded_grid(h->inv.tiles, SQ_BLOCK_TILES, SQ_WAVES, per_cu, h->num_cu);
}

// mu_ held, trained.  Enqueues only, unless rows are pending (the rebuild blocks) or a workspace has to grow
int search_enqueue(ise_ivfsq* h, const float* q_dev, long long nq, int k, const long long* probes_dev, int nprobe, float* D_dev,
                   long long* I_dev, hipStream_t st) {
    h->batches++;
    // a search still in flight on another stream comes first on the device: before the rebuild and before the
    // workspaces are written
    int rc = h->order.wait(st);
    if (rc) return rc;
    if ((rc = rebuild_locked(h, st))) return rc;
    const IvfLists& inv = h->inv;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT;
    if (inv.tiles == 0) {  // an empty index: padding, no pass
        knn_fill_launch(D_dev, I_dev, nq * k, ip, st);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    const int qt = h->qt, gmax = SQ_STAGE_CHUNK / qt;
    const unsigned grid = pass_grid(h);
    const size_t rec = sq_rec_bytes(h->d), nl = (size_t)inv.nlist;
    const hipEvent_t busy = h->order.busy();
    if ((rc = grow_after_event(h->qrec, (size_t)std::min<long long>(nq, SQ_STAGE_CHUNK) * rec, busy))) return rc;
    if ((rc = grow_after_event(h->lo, (size_t)qt, busy))) return rc;
    if ((rc = grow_after_event(h->lists, (size_t)grid * qt * SQ_KPASS, busy))) return rc;
    if ((rc = grow_after_event(h->masks, (size_t)gmax * nl, busy))) return rc;
    if ((rc = grow_after_event(h->offs, (size_t)gmax * nl + gmax, busy))) return rc;
    if ((rc = grow_after_event(h->work, (size_t)gmax * inv.tiles, busy))) return rc;
    CallOrder::Scope release{h->order, st};
    uint32_t* counts = h->offs.p + (size_t)gmax * nl;
    const size_t lds = sq_lds_bytes(h->d, qt);
    for (long long c0 = 0; c0 < nq; c0 += SQ_STAGE_CHUNK) {
        // the chunk's records, masks and work lists (in stream order behind the passes that read the last chunk's)
        const int m = (int)std::min<long long>(SQ_STAGE_CHUNK, nq - c0);
        const int groups = (m + qt - 1) / qt;
        h->codec.stage_launch(q_dev + (size_t)c0 * h->d, m, ip, h->qrec.p, st);
        HIP_TRY(ivfsq_work_list_launch(probes_dev + (size_t)c0 * nprobe, m, nprobe, inv.nlist, h->qshift, inv.meta, (uint32_t)inv.tiles,
                                       h->masks.p, h->offs.p, counts, h->work.p, st));
        for (int g = 0; g < groups; g++) {
            const long long q0 = c0 + (long long)g * qt;
            const int nqt = (int)std::min<long long>(qt, nq - q0);
            for (int off = 0; off < k; off += SQ_KPASS) {
                const int kp = std::min(SQ_KPASS, k - off);
                SqIvfScanParams sp{};
                sp.codes = h->codes;
                sp.rterm = h->rterm;
                sp.ids = inv.ids;
                sp.d = h->d;
                sp.stride = h->stride;
                sp.qrec = h->qrec.p + (size_t)g * qt * rec;
                sp.nqt = nqt;
                sp.kp = kp;
                sp.ip = ip;
                sp.lo = off == 0 ? nullptr : h->lo.p;  // the merge of the pass before wrote it
                sp.lists = h->lists.p;
                sp.work = h->work.p + (size_t)g * inv.tiles;
                sp.count = counts + g;
                sp.tiles_loaded = h->stats_dev;
                launch_scan(qt, grid, lds, st, sp);
                pass_merge_launch(h->lists.p, qt, SQ_KPASS, grid, nqt, kp, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, h->lo.p, k, off, ip, st);
                h->passes++;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

int check_search_args(const ise_ivfsq* h, const void* q, long long nq, int k, const void* probes, int nprobe, const void* D,
                      const void* I) {
    const int rc = check_ivf_knn_args(q, nq, k, probes, nprobe, D, I);
    return rc ? rc : check_handle(h);
}

int check_add_args(const ise_ivfsq* h, const void* x, const void* list_no, long long n, const char* what) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !list_no)) return ise_fail_(ISE_E_INVALID, std::string(what) + " or list numbers pointer is NULL");
    return check_handle(h);
}
}  // namespace

extern "C" int ise_ivfsq_create(ise_ivfsq_t** out, int d, int qtype, int metric, int nlist, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (d > ISE_SQ_MAX_D) return ise_fail_(ISE_E_INVALID, "d must be at most ISE_SQ_MAX_D");
    if (nlist <= 0) return ise_fail_(ISE_E_INVALID, "nlist must be positive");
    if (qtype != ISE_SQ_8BIT && qtype != ISE_SQ_8BIT_UNIFORM)
        return ise_fail_(ISE_E_INVALID, "qtype must be ISE_SQ_8BIT or ISE_SQ_8BIT_UNIFORM: only the 8-bit types are provided");
    if (metric != ISE_METRIC_L2 && metric != ISE_METRIC_INNER_PRODUCT)
        return ise_fail_(ISE_E_INVALID, "metric must be ISE_METRIC_L2 or ISE_METRIC_INNER_PRODUCT");
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_ivfsq* h = new (std::nothrow) ise_ivfsq();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d = d;
    h->stride = sq_stride(d);
    h->qt = sq_qt(d);
    h->qshift = h->qt == 16 ? 4 : 3;
    h->metric = metric;
    h->device = device;
    h->num_cu = num_cu;
    h->inv.nlist = nlist;
    h->inv.clear();
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->order.create();
    if (e == hipSuccess) e = h->codec.create(d, qtype);
    if (e == hipSuccess) e = hipMalloc((void**)&h->stats_dev, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->stats_dev, 0, sizeof(unsigned long long));
    if (e != hipSuccess) {
        free_all(h);
        delete h;
        return ise_fail_(ISE_E_HIP, std::string("inverted-list scalar-quantiser index setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_ivfsq_destroy(ise_ivfsq_t* h) {
    if (!h) return ISE_OK;
    {
        DeviceGuard gd(h->device);
        (void)hipDeviceSynchronize();
        free_all(h);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_ivfsq_reset(ise_ivfsq_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());
    free_rows(h);
    return ISE_OK;
}

extern "C" int ise_ivfsq_info(const ise_ivfsq_t* h, int* d, int* qtype, int* metric, int* nlist, int64_t* ntotal, int* is_trained,
                              int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d) *d = h->d;
    if (qtype) *qtype = h->codec.qtype;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->inv.nlist;
    if (ntotal) *ntotal = h->inv.n;
    if (is_trained) *is_trained = h->codec.trained ? 1 : 0;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_ivfsq_set_trained_host(ise_ivfsq_t* h, const float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->inv.n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the trained state in place (reset first)");
    return h->codec.set_trained(t, h->device);
}

extern "C" int ise_ivfsq_get_trained_host(ise_ivfsq_t* h, float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    return h->codec.get_trained(t);
}

extern "C" int ise_ivfsq_add_host(ise_ivfsq_t* h, const float* x, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, x, list_no, n, "rows");
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = h->inv.check_lists(list_no, n))) return rc;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    if ((rc = reserve_pending(h, n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    if ((rc = grow_after_event(h->xraw, (size_t)std::min<long long>(step, n) * h->d, nullptr))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {  // nothing is counted in before the last piece's verdict
        const long long m = std::min<long long>(step, n - i0);
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = encode_pending(h, h->xraw.p, h->inv.pend_n + i0, m, st))) return rc;
    }
    if ((rc = h->codec.bad.check(st))) return rc;
    h->inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_add_device(ise_ivfsq_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream) {
    int rc = check_add_args(h, x_dev, list_no_dev, n, "rows");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::vector<int64_t> lists((size_t)n);
    HIP_TRY(hipMemcpyAsync(lists.data(), list_no_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = h->inv.check_lists(lists.data(), n))) return rc;
    if ((rc = reserve_pending(h, n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    if ((rc = encode_pending(h, x_dev, h->inv.pend_n, n, st))) return rc;
    if ((rc = h->codec.bad.check(st))) return rc;
    h->inv.add(lists.data(), n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_add_codes_host(ise_ivfsq_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, codes, list_no, n, "codes");
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = h->inv.check_lists(list_no, n))) return rc;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    if ((rc = reserve_pending(h, n, st))) return rc;
    uint8_t* dst = h->pend + (size_t)h->inv.pend_n * h->stride;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * h->stride, st));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->stride, codes, (size_t)h->d, (size_t)h->d, (size_t)n, hipMemcpyHostToDevice, st));
    h->codec.rowterm_launch(dst, h->stride, n, h->pend_rterm + h->inv.pend_n, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    h->inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_list_sizes_host(ise_ivfsq_t* h, int64_t* sizes) {
    if (!sizes) return ise_fail_(ISE_E_INVALID, "sizes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    h->inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_ivfsq_list_host(ise_ivfsq_t* h, int list, int64_t* ids, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (list < 0 || list >= h->inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = rebuild_locked(h, h->stream);
    if (rc) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->inv.list_ids_host(list, SQ_TILE, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    if (codes)
        HIP_TRY(hipMemcpy2D(codes, (size_t)h->d, h->codes + slot0 * h->stride, (size_t)h->stride, (size_t)h->d, m, hipMemcpyDeviceToHost));
    return ISE_OK;
}

extern "C" int ise_ivfsq_search_device(ise_ivfsq_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                                       float* D_dev, int64_t* I_dev, void* stream) {
    const int rc = check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_ivfsq_search_host(ise_ivfsq_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                                     int64_t* I) {
    int rc = check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return ivf_search_staged(h->d, h->stream, q, nq, k, probes, nprobe, D, I,
                             [&](const float* q_dev, long long m, const long long* p_dev, float* D_dev, long long* I_dev) {
                                 return search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->stream);
                             });
}

extern "C" int ise_ivfsq_stats(ise_ivfsq_t* h, uint64_t* out3) {
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
