// ise_sq.hip -- host side and C ABI of the scalar-quantised index (include/ise_knn.h, ise_sq_*; kernels in
// ise_sq.hpp).  faiss.IndexScalarQuantizer with the 8-bit types: the trained state (per-dimension or
// uniform vmin / vdiff) comes from the caller (set_trained; the min/max pass lives in
// faiss_compat.IndexScalarQuantizer.train), rows are encoded on the device and kept as one byte per entry plus one
// float64 row term, search stages the queries' weights and scans the bytes on the matrix cores.
//
// Calls on one handle run one at a time (a mutex; the host forms hold it until their results are back, the device
// forms while they enqueue).  The handle has ONE set of workspaces: every call that touches them waits for the call
// before and marks its own end (CallOrder, ise_host.hpp), and a workspace that has to grow is replaced by the drained
// rule (grow_drained, ise_host.hpp).  The codec's host state is ise_sq_host.hpp's.
#include "ise_sq_host.hpp"

struct ise_sq {
    int d = 0, stride = 0, qt = 0, metric = ISE_METRIC_L2, device = 0, num_cu = 256;
    long long n = 0, cap = 0;
    uint8_t* codes = nullptr;  // [cap][stride]; bytes [d, stride) of every row are zero
    double* rterm = nullptr;   // [cap] sum_j (s_j c_j)^2
    SqCodec codec;
    hipStream_t stream = nullptr;
    CallOrder order;
    mutable std::mutex mu;
    DevBuf<float> xraw, oD;  // host forms: rows or queries as passed | results
    DevBuf<uint8_t> craw;    // host forms: codes as passed or to hand back, packed [n][d]
    DevBuf<uint8_t> qrec;    // one chunk's staged queries
    DevBuf<u64> lo, lists;
    DevBuf<long long> oI;
    uint64_t st_search = 0, st_passes = 0;
};

namespace {
int check_handle(const ise_sq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "scalar-quantiser index handle is NULL"); }

void launch_scan(int qt, unsigned grid, size_t lds, hipStream_t st, const SqScanParams& sp) {
    static LdsAttrOnce attr[2];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), SQ_LDS_LIMIT);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SQ_WAVES * 64), lds, st, sp);
    };
    if (qt == 16) go(sq_scan_kernel<16>, attr[0]);
    else go(sq_scan_kernel<8>, attr[1]);
}

// blocks of a pass: about SQ_BLOCK_TILES tiles per wave on a short index, at most what the CUs hold at once (their LDS)
unsigned sq_grid(const ise_sq* h) {
    const long long per_cu = std::max<long long>(1, (long long)SQ_LDS_LIMIT / (long long)sq_lds_bytes(h->d, h->qt));
    return coded_grid((h->n + SQ_TILE - 1) / SQ_TILE, SQ_BLOCK_TILES, SQ_WAVES, per_cu, h->num_cu);
}

// the codes and, beside them, the row terms
int reserve_rows(ise_sq* h, long long need, hipStream_t st) {
    return reserve_code_rows(&h->codes, (size_t)h->stride, h->n, &h->cap, need, SQ_TILE, st, &h->rterm, sizeof(double));
}

int check_rows_fit(const ise_sq* h, long long n) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "a scalar-quantiser index holds fewer than 2^32 rows");
    return ISE_OK;
}

// q_dev: nq x d floats on the device; D_dev / I_dev: nq x k.  mu held, the index trained
int search_enqueue(ise_sq* h, const float* q_dev, long long nq, int k, float* D_dev, long long* I_dev, hipStream_t st) {
    int rc = h->order.wait(st);
    if (rc) return rc;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT;
    if (h->n == 0) {  // nothing to rank: a fill, no pass
        h->st_search++;
        knn_fill_launch(D_dev, I_dev, nq * k, ip, st);
        HIP_TRY(hipGetLastError());
        return h->order.mark(st);
    }
    const int qt = h->qt;
    const unsigned grid = sq_grid(h);
    const size_t rec = sq_rec_bytes(h->d);
    if ((rc = grow_drained(h->qrec, (size_t)std::min<long long>(nq, SQ_STAGE_CHUNK) * rec))) return rc;
    if ((rc = grow_drained(h->lo, (size_t)qt))) return rc;
    if ((rc = grow_drained(h->lists, (size_t)grid * qt * SQ_KPASS))) return rc;
    h->st_search++;  // counted once the batch is certain to be enqueued
    const size_t lds = sq_lds_bytes(h->d, qt);
    for (long long q0 = 0; q0 < nq; q0 += qt) {
        if (q0 % SQ_STAGE_CHUNK == 0) {  // the next chunk's records (in stream order behind the passes that read the last)
            h->codec.stage_launch(q_dev + (size_t)q0 * h->d, (int)std::min<long long>(SQ_STAGE_CHUNK, nq - q0), ip, h->qrec.p, st);
        }
        const int nqt = (int)std::min<long long>(qt, nq - q0);
        for (int off = 0; off < k; off += SQ_KPASS) {
            const int kp = std::min(SQ_KPASS, k - off);
            SqScanParams sp{};
            sp.codes = h->codes;
            sp.rterm = h->rterm;
            sp.d = h->d;
            sp.stride = h->stride;
            sp.n = h->n;
            sp.qrec = h->qrec.p + (size_t)(q0 % SQ_STAGE_CHUNK) * rec;
            sp.nqt = nqt;
            sp.kp = kp;
            sp.ip = ip;
            sp.lo = off == 0 ? nullptr : h->lo.p;  // the merge of the pass before wrote it
            sp.lists = h->lists.p;
            launch_scan(qt, grid, lds, st, sp);
            pass_merge_launch(h->lists.p, qt, SQ_KPASS, grid, nqt, kp, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, h->lo.p, k, off, ip, st);
            h->st_passes++;
        }
    }
    HIP_TRY(hipGetLastError());
    return h->order.mark(st);
}

int check_search_args(const ise_sq* h, const void* q, long long nq, int k, const void* D, const void* I) {
    const int rc = check_knn_args(q, nq, k, D, I);
    return rc ? rc : check_handle(h);
}

// mu held, trained, n > 0 rows at x_dev: encode them behind the stored rows and, if every entry was finite, count
// them in.  Blocks (the flag is read back)
int add_device_locked(ise_sq* h, const float* x_dev, long long n, hipStream_t st) {
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = h->order.wait(st))) return rc;
    if ((rc = reserve_rows(h, h->n + n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    h->codec.encode_launch(x_dev, n, h->codes + (size_t)h->n * h->stride, h->stride, h->rterm + h->n, st);
    HIP_TRY(hipGetLastError());
    if ((rc = h->order.mark(st))) return rc;
    if ((rc = h->codec.bad.check(st))) return rc;
    h->n += n;
    return ISE_OK;
}

void free_buffers(ise_sq* h) {
    for (void* p : {(void*)h->xraw.p, (void*)h->oD.p, (void*)h->craw.p, (void*)h->qrec.p, (void*)h->lo.p, (void*)h->lists.p, (void*)h->oI.p,
                    (void*)h->codes, (void*)h->rterm})
        if (p) (void)hipFree(p);
    h->codec.destroy();
}
}  // namespace

extern "C" int ise_sq_create(ise_sq_t** out, int d, int qtype, int metric, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (d > ISE_SQ_MAX_D) return ise_fail_(ISE_E_INVALID, "d must be at most ISE_SQ_MAX_D");
    if (qtype != ISE_SQ_8BIT && qtype != ISE_SQ_8BIT_UNIFORM)
        return ise_fail_(ISE_E_INVALID, "qtype must be ISE_SQ_8BIT or ISE_SQ_8BIT_UNIFORM: only the 8-bit types are provided");
    if (metric != ISE_METRIC_L2 && metric != ISE_METRIC_INNER_PRODUCT)
        return ise_fail_(ISE_E_INVALID, "metric must be ISE_METRIC_L2 or ISE_METRIC_INNER_PRODUCT");
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_sq* h = new (std::nothrow) ise_sq();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d = d;
    h->stride = sq_stride(d);
    h->qt = sq_qt(d);
    h->metric = metric;
    h->device = device;
    h->num_cu = num_cu;
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->order.create();
    if (e == hipSuccess) e = h->codec.create(d, qtype);
    if (e != hipSuccess) {
        free_buffers(h);
        h->order.destroy();
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return ise_fail_(ISE_E_HIP, std::string("scalar-quantiser index setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_sq_destroy(ise_sq_t* h) {
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

extern "C" int ise_sq_reset(ise_sq_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->n = 0;  // capacity is kept; stale rows are masked by row number, their pad bytes are zero already
    return ISE_OK;
}

extern "C" int ise_sq_info(const ise_sq_t* h, int* d, int* qtype, int* metric, int64_t* ntotal, int* is_trained, int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (d) *d = h->d;
    if (qtype) *qtype = h->codec.qtype;
    if (metric) *metric = h->metric;
    if (ntotal) *ntotal = h->n;
    if (is_trained) *is_trained = h->codec.trained ? 1 : 0;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_sq_set_trained_host(ise_sq_t* h, const float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the trained state in place (reset first)");
    return h->codec.set_trained(t, h->device);
}

extern "C" int ise_sq_get_trained_host(ise_sq_t* h, float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->codec.get_trained(t);
    return ISE_OK;
}

extern "C" int ise_sq_encode_device(ise_sq_t* h, const float* x_dev, int64_t n, uint8_t* codes_dev, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x_dev || !codes_dev)) return ise_fail_(ISE_E_INVALID, "rows or codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = h->order.wait(st);
    if (rc) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    h->codec.encode_launch(x_dev, n, codes_dev, h->d, nullptr, st);
    HIP_TRY(hipGetLastError());
    if ((rc = h->order.mark(st))) return rc;
    return h->codec.bad.check(st);
}

extern "C" int ise_sq_encode_host(ise_sq_t* h, const float* x, int64_t n, uint8_t* codes) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !codes)) return ise_fail_(ISE_E_INVALID, "rows or codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    int rc = h->order.wait(st);
    if (rc) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->d))) return rc;
        if ((rc = grow_drained(h->craw, (size_t)m * h->d))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = h->codec.bad.clear(st))) return rc;
        h->codec.encode_launch(h->xraw.p, m, h->craw.p, h->d, nullptr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(codes + (size_t)i0 * h->d, h->craw.p, (size_t)m * h->d, hipMemcpyDeviceToHost, st));
        if ((rc = h->order.mark(st))) return rc;
        if ((rc = h->codec.bad.check(st))) return rc;
    }
    return ISE_OK;
}

extern "C" int ise_sq_decode_host(ise_sq_t* h, const uint8_t* codes, int64_t n, float* x) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!codes || !x)) return ise_fail_(ISE_E_INVALID, "codes or rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    int rc = h->order.wait(st);
    if (rc) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->d))) return rc;
        if ((rc = grow_drained(h->craw, (size_t)m * h->d))) return rc;
        HIP_TRY(hipMemcpyAsync(h->craw.p, codes + (size_t)i0 * h->d, (size_t)m * h->d, hipMemcpyHostToDevice, st));
        h->codec.decode_launch(h->craw.p, h->d, m, h->xraw.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x + (size_t)i0 * h->d, h->xraw.p, (size_t)m * h->d * sizeof(float), hipMemcpyDeviceToHost, st));
        if ((rc = h->order.mark(st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_sq_add_device(ise_sq_t* h, const float* x_dev, int64_t n, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !x_dev) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return add_device_locked(h, x_dev, n, (hipStream_t)stream);
}

extern "C" int ise_sq_add_host(ise_sq_t* h, const float* x, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !x) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    struct Undo {  // a non-finite row (or an error) in a later piece takes the earlier pieces back out
        ise_sq* h;
        long long n0;
        bool keep = false;
        ~Undo() {
            if (!keep) h->n = n0;
        }
    } undo{h, h->n};
    const long long step = upload_step((size_t)h->d * sizeof(float));
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = reserve_rows(h, h->n + n, h->stream))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->d))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice,
                               h->stream));
        if ((rc = add_device_locked(h, h->xraw.p, m, h->stream))) return rc;
    }
    undo.keep = true;
    return ISE_OK;
}

extern "C" int ise_sq_add_codes_host(ise_sq_t* h, const uint8_t* codes, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !codes) return ise_fail_(ISE_E_INVALID, "codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = h->order.wait(st))) return rc;
    if ((rc = reserve_rows(h, h->n + n, st))) return rc;
    // the pad bytes of the fresh rows are zero already (reserve_code_rows); only bytes below d are ever written
    uint8_t* dst = h->codes + (size_t)h->n * h->stride;
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->stride, codes, (size_t)h->d, (size_t)h->d, (size_t)n, hipMemcpyHostToDevice, st));
    h->codec.rowterm_launch(dst, h->stride, n, h->rterm + h->n, st);
    HIP_TRY(hipGetLastError());
    if ((rc = h->order.mark(st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    h->n += n;
    return ISE_OK;
}

extern "C" int ise_sq_codes_host(ise_sq_t* h, int64_t i0, int64_t n, uint8_t* codes) {
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
    HIP_TRY(hipMemcpy2DAsync(codes, (size_t)h->d, h->codes + (size_t)i0 * h->stride, (size_t)h->stride, (size_t)h->d, (size_t)n,
                             hipMemcpyDeviceToHost, st));
    if ((rc = h->order.mark(st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return ISE_OK;
}

extern "C" int ise_sq_reconstruct_host(ise_sq_t* h, int64_t i0, int64_t n, float* x) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 < 0 || n < 0 || i0 + n > h->n) return ise_fail_(ISE_E_INVALID, "row range out of bounds");
    if (n == 0) return ISE_OK;
    if (!x) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    int rc = h->order.wait(st);
    if (rc) return rc;
    for (long long j0 = 0; j0 < n; j0 += step) {
        const long long m = std::min<long long>(step, n - j0);
        if ((rc = grow_drained(h->xraw, (size_t)m * h->d))) return rc;
        h->codec.decode_launch(h->codes + (size_t)(i0 + j0) * h->stride, h->stride, m, h->xraw.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x + (size_t)j0 * h->d, h->xraw.p, (size_t)m * h->d * sizeof(float), hipMemcpyDeviceToHost, st));
        if ((rc = h->order.mark(st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_sq_search_device(ise_sq_t* h, const float* q_dev, int64_t nq, int k, float* D_dev, int64_t* I_dev,
                                    void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return search_enqueue(h, q_dev, nq, k, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_sq_search_host(ise_sq_t* h, const float* q, int64_t nq, int k, float* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k, D, I);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long batch = std::min<long long>(nq, 4096);
    if ((rc = grow_drained(h->xraw, (size_t)batch * h->d))) return rc;
    if ((rc = grow_drained(h->oD, (size_t)batch * k))) return rc;
    if ((rc = grow_drained(h->oI, (size_t)batch * k))) return rc;
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        if ((rc = h->order.wait(st))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, q + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = search_enqueue(h, h->xraw.p, m, k, h->oD.p, h->oI.p, st))) return rc;
        HIP_TRY(hipMemcpyAsync(D + (size_t)i0 * k, h->oD.p, (size_t)m * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, h->oI.p, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_sq_stats(ise_sq_t* h, uint64_t* out3) {
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    out3[0] = h->st_search;
    out3[1] = h->st_passes;
    out3[2] = (uint64_t)h->cap * (uint64_t)h->stride;
    return ISE_OK;
}
