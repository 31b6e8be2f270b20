// ise_pq.hip -- host side and C ABI of the product-quantised index (include/ise_knn.h, ise_pq_*; kernels in
// ise_pq.hpp).  faiss.IndexPQ with 8-bit sub-quantisers: the codebook comes from the caller
// (set_centroids; the k-means lives in faiss_compat.IndexPQ.train), rows are encoded on the device and kept as codes
// only, search builds the queries' lookup tables and scans the codes.
//
// Calls on one handle run one at a time (a mutex; the host forms hold it until their results are back, the device
// forms while they enqueue).  The handle has ONE set of workspaces: every call that touches them waits for the call
// before and marks its own end (CallOrder, ise_host.hpp), and a workspace that has to grow is replaced by the drained
// rule (grow_drained, ise_host.hpp).
#include <cmath>

#include "ise_pq_host.hpp"

struct ise_pq {
    int metric = ISE_METRIC_L2, device = 0, num_cu = 256;
    PqCodec codec;  // d, M, dsub, stride, qt, the codebook and the encoders' flag
    long long n = 0, cap = 0;
    uint8_t* codes = nullptr;  // [cap][stride]; bytes [M, stride) of every row are zero
    hipStream_t stream = nullptr;
    CallOrder order;
    mutable std::mutex mu;
    DevBuf<float> xraw, tab, oD;  // host forms: rows or queries as passed | one chunk's tables | results
    DevBuf<uint8_t> craw;         // host forms: codes as passed or to hand back, packed [n][M]
    DevBuf<u64> lo, lists;
    DevBuf<long long> oI;
    uint64_t st_search = 0, st_passes = 0, st_tables = 0;
};

namespace {
int check_handle(const ise_pq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "product-quantiser index handle is NULL"); }
int check_trained(const ise_pq* h) { return h->codec.check_trained(); }

PqScanLaunch<PqScanParams> launch_scan{{pq_scan_kernel<16>, pq_scan_kernel<8>, pq_scan_kernel<4>, pq_scan_kernel<2>}, {}};

// blocks of a pass: about two tiles per wave on a short index, at most what the CUs hold at once (their LDS)
unsigned pq_grid(const ise_pq* h) {
    return coded_grid((h->n + 63) / 64, 2, PQ_WAVES, h->codec.blocks_per_cu(), h->num_cu);
}

int reserve_rows(ise_pq* h, long long need, hipStream_t st) {
    return reserve_code_rows(&h->codes, (size_t)h->codec.stride, h->n, &h->cap, need, 64, st);
}

int check_rows_fit(const ise_pq* h, long long n) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "a product-quantiser index holds fewer than 2^32 rows");
    return ISE_OK;
}

// q_dev: nq x d floats on the device; D_dev / I_dev: nq x k.  mu held, the index trained
int search_enqueue(ise_pq* h, const float* q_dev, long long nq, int k, float* D_dev, long long* I_dev, hipStream_t st) {
    int rc = h->order.wait(st);
    if (rc) return rc;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT;
    if (h->n == 0) {  // nothing to rank: a fill, no table, no pass
        h->st_search++;
        knn_fill_launch(D_dev, I_dev, nq * k, ip, st);
        HIP_TRY(hipGetLastError());
        return h->order.mark(st);
    }
    const int qt = h->codec.qt;
    const unsigned grid = pq_grid(h);
    const size_t tab_q = h->codec.tab_floats();  // floats of one query's tables
    if ((rc = grow_drained(h->tab, (size_t)std::min<long long>((nq + qt - 1) / qt * qt, PQ_TAB_CHUNK) * tab_q))) return rc;
    if ((rc = grow_drained(h->lo, (size_t)PQ_TAB_CHUNK))) return rc;
    if ((rc = grow_drained(h->lists, (size_t)grid * qt * PQ_KPASS))) return rc;
    h->st_search++;  // counted once the batch is certain to be enqueued
    const size_t lds = h->codec.lds_bytes();
    for (long long c0 = 0; c0 < nq; c0 += PQ_TAB_CHUNK) {
        const int mc = (int)std::min<long long>(PQ_TAB_CHUNK, nq - c0);
        const int groups = (mc + qt - 1) / qt;
        h->codec.table_launch(q_dev + (size_t)c0 * h->codec.d, mc, ip, h->tab.p, st);
        h->st_tables++;
        for (int g = 0; g < groups; g++) {
            const long long q0 = c0 + (long long)g * qt;
            const int nqt = (int)std::min<long long>(qt, nq - q0);
            for (int off = 0; off < k; off += PQ_KPASS) {
                const int kp = std::min(PQ_KPASS, k - off);
                PqScanParams sp{};
                sp.codes = h->codes;
                sp.M = h->codec.M;
                sp.stride = h->codec.stride;
                sp.n = h->n;
                sp.tab = h->tab.p + (size_t)g * qt * tab_q;
                sp.nqt = nqt;
                sp.kp = kp;
                sp.ip = ip;
                sp.lo = off == 0 ? nullptr : h->lo.p + g * qt;  // the merge of the pass before wrote it
                sp.lists = h->lists.p;
                launch_scan(qt, grid, lds, st, sp);
                pass_merge_launch(h->lists.p, qt, PQ_KPASS, grid, nqt, kp, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k,
                                  h->lo.p + g * qt, k, off, ip, st);
                h->st_passes++;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return h->order.mark(st);
}

int check_search_args(const ise_pq* h, const void* q, long long nq, int k, const void* D, const void* I) {
    const int rc = check_knn_args(q, nq, k, D, I);
    return rc ? rc : check_handle(h);
}

// mu held, trained, n > 0 rows at x_dev: encode them behind the stored rows and, if every entry was finite, count
// them in.  Blocks (the flag is read back)
int add_device_locked(ise_pq* h, const float* x_dev, long long n, hipStream_t st) {
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = h->order.wait(st))) return rc;
    if ((rc = reserve_rows(h, h->n + n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    h->codec.encode_launch(x_dev, n, h->codes + (size_t)h->n * h->codec.stride, h->codec.stride, st);
    HIP_TRY(hipGetLastError());
    if ((rc = h->order.mark(st))) return rc;
    if ((rc = h->codec.bad.check(st))) return rc;
    h->n += n;
    return ISE_OK;
}

void free_buffers(ise_pq* h) {
    for (void* p : {(void*)h->xraw.p, (void*)h->tab.p, (void*)h->oD.p, (void*)h->craw.p, (void*)h->lo.p, (void*)h->lists.p,
                    (void*)h->oI.p, (void*)h->codes})
        if (p) (void)hipFree(p);
    h->codec.destroy();
}
}  // namespace

extern "C" int ise_pq_create(ise_pq_t** out, int d, int M, int nbits, int metric, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (M <= 0) return ise_fail_(ISE_E_INVALID, "M must be positive");
    if (M > ISE_PQ_MAX_M) return ise_fail_(ISE_E_INVALID, "M must be at most ISE_PQ_MAX_M");
    if (d % M != 0) return ise_fail_(ISE_E_INVALID, "d must be a multiple of M");
    if (nbits != 8) return ise_fail_(ISE_E_INVALID, "nbits must be 8: only 8-bit sub-quantisers are provided");
    if (metric != ISE_METRIC_L2 && metric != ISE_METRIC_INNER_PRODUCT)
        return ise_fail_(ISE_E_INVALID, "metric must be ISE_METRIC_L2 or ISE_METRIC_INNER_PRODUCT");
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_pq* h = new (std::nothrow) ise_pq();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->metric = metric;
    h->device = device;
    h->num_cu = num_cu;
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->order.create();
    if (e == hipSuccess) e = h->codec.create(d, M);
    if (e != hipSuccess) {
        free_buffers(h);
        h->order.destroy();
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return ise_fail_(ISE_E_HIP, std::string("product-quantiser index setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_pq_destroy(ise_pq_t* h) {
    if (!h) return ISE_OK;
    {
        DeviceGuard gd(h->device);
        (void)hipDeviceSynchronize();
        free_buffers(h);
        h->order.destroy();
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_pq_reset(ise_pq_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->n = 0;  // capacity is kept; stale rows are masked by row number, their pad bytes are zero already
    return ISE_OK;
}

extern "C" int ise_pq_info(const ise_pq_t* h, int* d, int* M, int* nbits, int* metric, int64_t* ntotal, int* is_trained,
                           int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (d) *d = h->codec.d;
    if (M) *M = h->codec.M;
    if (nbits) *nbits = 8;
    if (metric) *metric = h->metric;
    if (ntotal) *ntotal = h->n;
    if (is_trained) *is_trained = h->codec.trained ? 1 : 0;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_pq_set_centroids_host(ise_pq_t* h, const float* c) {
    if (!c) return ise_fail_(ISE_E_INVALID, "centroid pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the centroids in place (reset first)");
    return h->codec.set_centroids(c, h->device);
}

extern "C" int ise_pq_get_centroids_host(ise_pq_t* h, float* c) {
    if (!c) return ise_fail_(ISE_E_INVALID, "centroid pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->codec.get_centroids(c, h->device);
}

extern "C" int ise_pq_encode_device(ise_pq_t* h, const float* x_dev, int64_t n, uint8_t* codes_dev, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x_dev || !codes_dev)) return ise_fail_(ISE_E_INVALID, "rows or codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = h->order.wait(st);
    if (rc) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    h->codec.encode_launch(x_dev, n, codes_dev, h->codec.M, st);
    HIP_TRY(hipGetLastError());
    if ((rc = h->order.mark(st))) return rc;
    return h->codec.bad.check(st);
}

extern "C" int ise_pq_encode_host(ise_pq_t* h, const float* x, int64_t n, uint8_t* codes) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !codes)) return ise_fail_(ISE_E_INVALID, "rows or codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->codec.d * sizeof(float));
    int rc = h->order.wait(st);
    if (rc) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->codec.d))) return rc;
        if ((rc = grow_drained(h->craw, (size_t)m * h->codec.M))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->codec.d, (size_t)m * h->codec.d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = h->codec.bad.clear(st))) return rc;
        h->codec.encode_launch(h->xraw.p, m, h->craw.p, h->codec.M, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(codes + (size_t)i0 * h->codec.M, h->craw.p, (size_t)m * h->codec.M, hipMemcpyDeviceToHost, st));
        if ((rc = h->order.mark(st))) return rc;
        if ((rc = h->codec.bad.check(st))) return rc;
    }
    return ISE_OK;
}

extern "C" int ise_pq_decode_host(ise_pq_t* h, const uint8_t* codes, int64_t n, float* x) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!codes || !x)) return ise_fail_(ISE_E_INVALID, "codes or rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->codec.d * sizeof(float));
    int rc = h->order.wait(st);
    if (rc) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->codec.d))) return rc;
        if ((rc = grow_drained(h->craw, (size_t)m * h->codec.M))) return rc;
        HIP_TRY(hipMemcpyAsync(h->craw.p, codes + (size_t)i0 * h->codec.M, (size_t)m * h->codec.M, hipMemcpyHostToDevice, st));
        h->codec.decode_launch(h->craw.p, h->codec.M, m, h->xraw.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x + (size_t)i0 * h->codec.d, h->xraw.p, (size_t)m * h->codec.d * sizeof(float), hipMemcpyDeviceToHost, st));
        if ((rc = h->order.mark(st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_pq_add_device(ise_pq_t* h, const float* x_dev, int64_t n, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !x_dev) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return add_device_locked(h, x_dev, n, (hipStream_t)stream);
}

extern "C" int ise_pq_add_host(ise_pq_t* h, const float* x, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !x) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    struct Undo {  // a non-finite row (or an error) in a later piece takes the earlier pieces back out
        ise_pq* h;
        long long n0;
        bool keep = false;
        ~Undo() {
            if (!keep) h->n = n0;
        }
    } undo{h, h->n};
    const long long step = upload_step((size_t)h->codec.d * sizeof(float));
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = reserve_rows(h, h->n + n, h->stream))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->codec.d))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->codec.d, (size_t)m * h->codec.d * sizeof(float), hipMemcpyHostToDevice,
                               h->stream));
        if ((rc = add_device_locked(h, h->xraw.p, m, h->stream))) return rc;
    }
    undo.keep = true;
    return ISE_OK;
}

extern "C" int ise_pq_add_codes_host(ise_pq_t* h, const uint8_t* codes, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !codes) return ise_fail_(ISE_E_INVALID, "codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = h->order.wait(st))) return rc;
    if ((rc = reserve_rows(h, h->n + n, st))) return rc;
    // the pad bytes of the fresh rows are zero already (reserve_code_rows); only bytes below M are ever written
    HIP_TRY(hipMemcpy2DAsync(h->codes + (size_t)h->n * h->codec.stride, (size_t)h->codec.stride, codes, (size_t)h->codec.M, (size_t)h->codec.M, (size_t)n,
                             hipMemcpyHostToDevice, st));
    if ((rc = h->order.mark(st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    h->n += n;
    return ISE_OK;
}

extern "C" int ise_pq_codes_host(ise_pq_t* h, int64_t i0, int64_t n, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 < 0 || n < 0 || i0 + n > h->n) return ise_fail_(ISE_E_INVALID, "row range out of bounds");
    if (n == 0) return ISE_OK;
    if (!codes) return ise_fail_(ISE_E_INVALID, "codes pointer is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    int rc = h->order.wait(st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(codes, (size_t)h->codec.M, h->codes + (size_t)i0 * h->codec.stride, (size_t)h->codec.stride, (size_t)h->codec.M, (size_t)n,
                             hipMemcpyDeviceToHost, st));
    if ((rc = h->order.mark(st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return ISE_OK;
}

extern "C" int ise_pq_reconstruct_host(ise_pq_t* h, int64_t i0, int64_t n, float* x) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 < 0 || n < 0 || i0 + n > h->n) return ise_fail_(ISE_E_INVALID, "row range out of bounds");
    if (n == 0) return ISE_OK;
    if (!x) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->codec.d * sizeof(float));
    int rc = h->order.wait(st);
    if (rc) return rc;
    for (long long j0 = 0; j0 < n; j0 += step) {
        const long long m = std::min<long long>(step, n - j0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->codec.d))) return rc;
        h->codec.decode_launch(h->codes + (size_t)(i0 + j0) * h->codec.stride, h->codec.stride, m, h->xraw.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x + (size_t)j0 * h->codec.d, h->xraw.p, (size_t)m * h->codec.d * sizeof(float), hipMemcpyDeviceToHost, st));
        if ((rc = h->order.mark(st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_pq_search_device(ise_pq_t* h, const float* q_dev, int64_t nq, int k, float* D_dev, int64_t* I_dev,
                                    void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return search_enqueue(h, q_dev, nq, k, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_pq_search_host(ise_pq_t* h, const float* q, int64_t nq, int k, float* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k, D, I);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long batch = std::min<long long>(nq, 4096);
    if ((rc = grow_drained(h->xraw, (size_t)batch * h->codec.d))) return rc;
    if ((rc = grow_drained(h->oD, (size_t)batch * k))) return rc;
    if ((rc = grow_drained(h->oI, (size_t)batch * k))) return rc;
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        if ((rc = h->order.wait(st))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, q + (size_t)i0 * h->codec.d, (size_t)m * h->codec.d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = search_enqueue(h, h->xraw.p, m, k, h->oD.p, h->oI.p, st))) return rc;
        HIP_TRY(hipMemcpyAsync(D + (size_t)i0 * k, h->oD.p, (size_t)m * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, h->oI.p, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_pq_stats(ise_pq_t* h, uint64_t* out4) {
    if (!out4) return ise_fail_(ISE_E_INVALID, "out4 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    out4[0] = h->st_search;
    out4[1] = h->st_passes;
    out4[2] = h->st_tables;
    out4[3] = (uint64_t)h->cap * (uint64_t)h->codec.stride;
    return ISE_OK;
}
