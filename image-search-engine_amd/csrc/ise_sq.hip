// ise_sq.hip -- host side and C ABI of the scalar-quantised index (include/ise_knn.h, ise_sq_*; kernels in
// ise_sq.hpp).  faiss.IndexScalarQuantizer with the 8-bit types: the trained state (per-dimension or
// uniform vmin / vdiff) comes from the caller (set_trained; the min/max pass lives in
// faiss_compat.IndexScalarQuantizer.train), rows are encoded on the device and kept as one byte per entry plus one
// float64 row term, search stages the queries' weights and scans the bytes on the matrix cores.
//
// Calls on one handle run one at a time (a mutex; the host forms hold it until their results are back, the device
// forms while they enqueue).  The handle has ONE set of workspaces: work enqueued on another stream than the previous
// call's waits for that call through an event, and a workspace that has to grow is replaced only after the device
// has drained.
#include <cmath>

#include "ise_host.hpp"
#include "ise_sq.hpp"

namespace {
// rule: device-wide drain before a free (any stream may still use the handle's ONE set), and half again on top so growth drains rarely
template <class T>
int sq_grow(DevBuf<T>& b, size_t need) {
    if (b.p && need <= b.n) return ISE_OK;
    if (b.p) {
        HIP_TRY(hipDeviceSynchronize());  // work in flight on any stream may still use the old one
        (void)hipFree(b.p);
    }
    b.p = nullptr;
    b.n = 0;
    const size_t want = std::max<size_t>(need + need / 2, 16);
    HIP_TRY(hipMalloc((void**)&b.p, want * sizeof(T)));
    b.n = want;
    return ISE_OK;
}
}  // namespace

struct ise_sq {
    int d = 0, qtype = ISE_SQ_8BIT, stride = 0, qt = 0, metric = ISE_METRIC_L2, device = 0, num_cu = 256;
    bool trained = false;
    long long n = 0, cap = 0;
    uint8_t* codes = nullptr;  // [cap][stride]; bytes [d, stride) of every row are zero
    double* rterm = nullptr;   // [cap] sum_j (s_j c_j)^2
    float* par = nullptr;      // [3][d]: vmin | s | o = vmin + s / 2
    std::vector<float> trained_host;  // Faiss's layout: [vmin.., vdiff..] (2 d) or [vmin, vdiff] (uniform)
    unsigned int* bad = nullptr;      // [1] set by an encode that met a NaN or inf entry
    hipStream_t stream = nullptr;
    hipEvent_t last = nullptr;  // the end of the previous call's device work
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    mutable std::mutex mu;
    DevBuf<float> xraw, oD;  // host forms: rows or queries as passed | results
    DevBuf<uint8_t> craw;    // host forms: codes as passed or to hand back, packed [n][d]
    DevBuf<uint8_t> qrec;    // one chunk's staged queries
    DevBuf<u64> lo, lists;
    DevBuf<long long> oI;
    uint64_t st_search = 0, st_passes = 0;
    const float* vmin() const { return par; }
    const float* step() const { return par + d; }
    const float* off() const { return par + 2 * (size_t)d; }
};

namespace {
const char* const NONFINITE_MSG = "a row has a NaN or inf entry: nothing was encoded or added";

// order this call's device work behind the previous call's, and mark its own end
int sq_begin(ise_sq* h, hipStream_t st) {
    if (h->last_valid && h->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, h->last, 0));
    return ISE_OK;
}
int sq_end(ise_sq* h, hipStream_t st) {
    HIP_TRY(hipEventRecord(h->last, st));
    h->last_stream = st;
    h->last_valid = true;
    return ISE_OK;
}

int check_handle(const ise_sq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "scalar-quantiser index handle is NULL"); }
int check_trained(const ise_sq* h) {
    return h->trained ? ISE_OK : ise_fail_(ISE_E_INVALID, "the index is not trained: set the trained state first");
}
bool uniform(const ise_sq* h) { return h->qtype == ISE_SQ_8BIT_UNIFORM; }
size_t trained_count(const ise_sq* h) { return uniform(h) ? 2 : 2 * (size_t)h->d; }

void launch_scan(int qt, unsigned grid, size_t lds, hipStream_t st, const SqScanParams& sp) {
    static LdsAttrOnce attr[2];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), SQ_LDS_LIMIT);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SQ_WAVES * 64), lds, st, sp);
    };
    if (qt == 16) go(sq_scan_kernel<16>, attr[0]);
    else go(sq_scan_kernel<8>, attr[1]);
}

// blocks of a pass: about SQ_BLOCK_TILES tiles per wave on a short index, at most what the CUs hold at once (their
// LDS) and the merge's list count
unsigned sq_grid(const ise_sq* h) {
    const long long tiles = (h->n + SQ_TILE - 1) / SQ_TILE;
    const long long per_cu = std::max<long long>(1, (long long)SQ_LDS_LIMIT / (long long)sq_lds_bytes(h->d, h->qt));
    long long g = (tiles + SQ_BLOCK_TILES * SQ_WAVES - 1) / (SQ_BLOCK_TILES * SQ_WAVES);
    g = std::min<long long>(g, std::min<long long>(per_cu * h->num_cu, MERGE_LISTS_MAX));
    return (unsigned)std::max<long long>(g, 1);
}

int reserve_codes(ise_sq* h, long long need, hipStream_t st) {
    if (need <= h->cap) return ISE_OK;
    long long want = need;
    if (h->cap > 0 && want < h->cap + h->cap / 2) want = h->cap + h->cap / 2;  // geometric growth on re-add
    want = (want + SQ_TILE - 1) / SQ_TILE * SQ_TILE;
    const size_t rb = (size_t)h->stride;
    uint8_t* nx = nullptr;
    double* nr = nullptr;
    HIP_TRY(hipMalloc((void**)&nx, (size_t)want * rb));
    hipError_t e = hipMalloc((void**)&nr, (size_t)want * sizeof(double));
    if (e == hipSuccess && h->n > 0) e = hipMemcpyAsync(nx, h->codes, (size_t)h->n * rb, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && h->n > 0) e = hipMemcpyAsync(nr, h->rterm, (size_t)h->n * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(nx + (size_t)h->n * rb, 0, (size_t)(want - h->n) * rb, st);
    if (e == hipSuccess) e = hipMemsetAsync(nr + h->n, 0, (size_t)(want - h->n) * sizeof(double), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h->codes) e = hipDeviceSynchronize();  // searches in flight still read the old storage
    if (e != hipSuccess) {
        (void)hipFree(nx);
        if (nr) (void)hipFree(nr);
        return ise_fail_(e == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP, std::string("growing the code storage: ") + hipGetErrorString(e));
    }
    if (h->codes) (void)hipFree(h->codes);
    if (h->rterm) (void)hipFree(h->rterm);
    h->codes = nx;
    h->rterm = nr;
    h->cap = want;
    return ISE_OK;
}

// rows [0, n) of dst (row stride `stride`) <- the codes of x's rows, rterm (may be null) <- their row terms; sets
// *h->bad on a non-finite entry
void encode_launch(ise_sq* h, const float* x_dev, long long n, uint8_t* dst, int stride, double* rterm, hipStream_t st) {
    hipLaunchKernelGGL(sq_encode_kernel, dim3((unsigned)((n + SQ_ENC_ROWS - 1) / SQ_ENC_ROWS)), dim3(SQ_WAVES * 64), 0, st, x_dev,
                       n, h->d, h->vmin(), h->step(), dst, stride, rterm, h->bad);
}

int bad_clear(ise_sq* h, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(unsigned int), st));
    return ISE_OK;
}
// waits for st; ISE_E_INVALID when an encode since bad_clear met a non-finite entry
int bad_check(ise_sq* h, hipStream_t st) {
    unsigned int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->bad, sizeof(flag), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return flag ? ise_fail_(ISE_E_INVALID, NONFINITE_MSG) : ISE_OK;
}

int check_rows_fit(const ise_sq* h, long long n) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "a scalar-quantiser index holds fewer than 2^32 rows");
    return ISE_OK;
}

// rows of `step` at most so that one upload is 256 MiB at most
long long upload_step(size_t row_bytes) { return std::max<long long>(1, (1ll << 28) / (long long)row_bytes); }

void decode_launch(const ise_sq* h, const uint8_t* codes, int stride, long long n, float* x_dev, hipStream_t st) {
    const long long tot = n * h->d;
    hipLaunchKernelGGL(sq_decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, codes, stride, n, h->d, h->vmin(),
                       h->step(), x_dev);
}

// q_dev: nq x d floats on the device; D_dev / I_dev: nq x k.  mu held, the index trained
int search_enqueue(ise_sq* h, const float* q_dev, long long nq, int k, float* D_dev, long long* I_dev, hipStream_t st) {
    int rc = sq_begin(h, st);
    if (rc) return rc;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT;
    if (h->n == 0) {  // nothing to rank: a fill, no pass
        h->st_search++;
        const long long cnt = nq * k;
        hipLaunchKernelGGL(sq_fill_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, D_dev, I_dev, cnt, ip);
        HIP_TRY(hipGetLastError());
        return sq_end(h, st);
    }
    const int qt = h->qt;
    const unsigned grid = sq_grid(h);
    const size_t rec = sq_rec_bytes(h->d);
    if ((rc = sq_grow(h->qrec, (size_t)std::min<long long>(nq, SQ_STAGE_CHUNK) * rec))) return rc;
    if ((rc = sq_grow(h->lo, (size_t)qt))) return rc;
    if ((rc = sq_grow(h->lists, (size_t)grid * qt * SQ_KPASS))) return rc;
    h->st_search++;  // counted once the batch is certain to be enqueued
    const size_t lds = sq_lds_bytes(h->d, qt);
    for (long long q0 = 0; q0 < nq; q0 += qt) {
        if (q0 % SQ_STAGE_CHUNK == 0) {  // the next chunk's records (in stream order behind the passes that read the last)
            SqStageParams gp{};
            gp.q = q_dev + (size_t)q0 * h->d;
            gp.nq = (int)std::min<long long>(SQ_STAGE_CHUNK, nq - q0);
            gp.d = h->d;
            gp.ip = ip;
            gp.step = h->step();
            gp.off = h->off();
            gp.rec = h->qrec.p;
            hipLaunchKernelGGL(sq_stage_kernel, dim3((unsigned)gp.nq), dim3(64), 0, st, gp);
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
            MergeParams mp{};
            mp.lists = h->lists.p;
            mp.stride_list = (long long)qt * SQ_KPASS;
            mp.stride_qtile = 0;
            mp.qt = qt;
            mp.n_lists = (int)grid;
            mp.nq = nqt;
            mp.k = kp;
            SqMergeOut mo{};
            mo.D = D_dev + (size_t)q0 * k;
            mo.I = I_dev + (size_t)q0 * k;
            mo.lo = h->lo.p;
            mo.k = k;
            mo.off = off;
            mo.ip = ip;
            hipLaunchKernelGGL(sq_merge_kernel, dim3((unsigned)nqt), dim3(MERGE_THREADS), 0, st, mp, mo);
            h->st_passes++;
        }
    }
    HIP_TRY(hipGetLastError());
    return sq_end(h, st);
}

int check_search_args(const ise_sq* h, const void* q, long long nq, int k, const void* D, const void* I) {
    if (nq < 0) return ise_fail_(ISE_E_INVALID, "nq must be >= 0");
    if (k < 1 || k > ISE_MAX_K) return ise_fail_(ISE_E_INVALID, "k must be in [1, ISE_MAX_K]");
    if (nq > 0 && !q) return ise_fail_(ISE_E_INVALID, "query pointer is NULL");
    if (nq > 0 && (!D || !I)) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    if (nq * (long long)k >= (1ll << 40)) return ise_fail_(ISE_E_INVALID, "nq * k is too large");
    return check_handle(h);
}

// mu held, trained, n > 0 rows at x_dev: encode them behind the stored rows and, if every entry was finite, count
// them in.  Blocks (the flag is read back)
int add_device_locked(ise_sq* h, const float* x_dev, long long n, hipStream_t st) {
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = sq_begin(h, st))) return rc;
    if ((rc = reserve_codes(h, h->n + n, st))) return rc;
    if ((rc = bad_clear(h, st))) return rc;
    encode_launch(h, x_dev, n, h->codes + (size_t)h->n * h->stride, h->stride, h->rterm + h->n, st);
    HIP_TRY(hipGetLastError());
    if ((rc = sq_end(h, st))) return rc;
    if ((rc = bad_check(h, st))) return rc;
    h->n += n;
    return ISE_OK;
}

void free_buffers(ise_sq* h) {
    for (void* p : {(void*)h->xraw.p, (void*)h->oD.p, (void*)h->craw.p, (void*)h->qrec.p, (void*)h->lo.p, (void*)h->lists.p, (void*)h->oI.p,
                    (void*)h->codes, (void*)h->rterm, (void*)h->par, (void*)h->bad})
        if (p) (void)hipFree(p);
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ise_fail_(ISE_E_NODEVICE, "no HIP device visible: the kNN path needs an MI355X (gfx950) GPU");
    if (device < 0 || device >= ndev) return ise_fail_(ISE_E_INVALID, "device out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ise_fail_(ISE_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    ise_sq* h = new (std::nothrow) ise_sq();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d = d;
    h->qtype = qtype;
    h->stride = sq_stride(d);
    h->qt = sq_qt(d);
    h->metric = metric;
    h->device = device;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&h->par, 3 * (size_t)d * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->bad, sizeof(unsigned int));
    if (e != hipSuccess) {
        free_buffers(h);
        if (h->last) (void)hipEventDestroy(h->last);
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
        if (h->last) (void)hipEventDestroy(h->last);
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
    if (qtype) *qtype = h->qtype;
    if (metric) *metric = h->metric;
    if (ntotal) *ntotal = h->n;
    if (is_trained) *is_trained = h->trained ? 1 : 0;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_sq_set_trained_host(ise_sq_t* h, const float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the trained state in place (reset first)");
    const size_t cnt = trained_count(h), half = cnt / 2;
    for (size_t i = 0; i < cnt; i++)
        if (!(std::fabs(t[i]) <= FLT_MAX)) return ise_fail_(ISE_E_INVALID, "the trained state has a NaN or inf entry");
    for (size_t i = half; i < cnt; i++)
        if (t[i] < 0.f) return ise_fail_(ISE_E_INVALID, "the trained state has a negative vdiff");
    const size_t d = (size_t)h->d;
    std::vector<float> par(3 * d);
    for (size_t j = 0; j < d; j++) {
        const float vmin = t[uniform(h) ? 0 : j], vdiff = t[uniform(h) ? 1 : d + j];
        const float s = vdiff / 255.0f;
        par[j] = vmin;
        par[d + j] = s;
        par[2 * d + j] = std::fmaf(0.5f, s, vmin);
    }
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // an encode or a scan in flight still reads the old state
    HIP_TRY(hipMemcpy(h->par, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice));
    h->trained_host.assign(t, t + cnt);
    h->trained = true;
    return ISE_OK;
}

extern "C" int ise_sq_get_trained_host(ise_sq_t* h, float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    std::copy(h->trained_host.begin(), h->trained_host.end(), t);
    return ISE_OK;
}

extern "C" int ise_sq_encode_device(ise_sq_t* h, const float* x_dev, int64_t n, uint8_t* codes_dev, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x_dev || !codes_dev)) return ise_fail_(ISE_E_INVALID, "rows or codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = sq_begin(h, st);
    if (rc) return rc;
    if ((rc = bad_clear(h, st))) return rc;
    encode_launch(h, x_dev, n, codes_dev, h->d, nullptr, st);
    HIP_TRY(hipGetLastError());
    if ((rc = sq_end(h, st))) return rc;
    return bad_check(h, st);
}

extern "C" int ise_sq_encode_host(ise_sq_t* h, const float* x, int64_t n, uint8_t* codes) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !codes)) return ise_fail_(ISE_E_INVALID, "rows or codes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    int rc = sq_begin(h, st);
    if (rc) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = sq_grow(h->xraw, (size_t)m * h->d))) return rc;
        if ((rc = sq_grow(h->craw, (size_t)m * h->d))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = bad_clear(h, st))) return rc;
        encode_launch(h, h->xraw.p, m, h->craw.p, h->d, nullptr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(codes + (size_t)i0 * h->d, h->craw.p, (size_t)m * h->d, hipMemcpyDeviceToHost, st));
        if ((rc = sq_end(h, st))) return rc;
        if ((rc = bad_check(h, st))) return rc;
    }
    return ISE_OK;
}

extern "C" int ise_sq_decode_host(ise_sq_t* h, const uint8_t* codes, int64_t n, float* x) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!codes || !x)) return ise_fail_(ISE_E_INVALID, "codes or rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    int rc = sq_begin(h, st);
    if (rc) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = sq_grow(h->xraw, (size_t)m * h->d))) return rc;
        if ((rc = sq_grow(h->craw, (size_t)m * h->d))) return rc;
        HIP_TRY(hipMemcpyAsync(h->craw.p, codes + (size_t)i0 * h->d, (size_t)m * h->d, hipMemcpyHostToDevice, st));
        decode_launch(h, h->craw.p, h->d, m, h->xraw.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x + (size_t)i0 * h->d, h->xraw.p, (size_t)m * h->d * sizeof(float), hipMemcpyDeviceToHost, st));
        if ((rc = sq_end(h, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_sq_add_device(ise_sq_t* h, const float* x_dev, int64_t n, void* stream) {
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

extern "C" int ise_sq_add_host(ise_sq_t* h, const float* x, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && !x) return ise_fail_(ISE_E_INVALID, "rows pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
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
    if ((rc = reserve_codes(h, h->n + n, h->stream))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = sq_grow(h->xraw, (size_t)m * h->d))) return rc;
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
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    int rc = check_rows_fit(h, n);
    if (rc) return rc;
    if ((rc = sq_begin(h, st))) return rc;
    if ((rc = reserve_codes(h, h->n + n, st))) return rc;
    // the pad bytes of the fresh rows are zero already (reserve_codes); only bytes below d are ever written
    uint8_t* dst = h->codes + (size_t)h->n * h->stride;
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->stride, codes, (size_t)h->d, (size_t)h->d, (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sq_rowterm_kernel, dim3((unsigned)((n + SQ_ENC_ROWS - 1) / SQ_ENC_ROWS)), dim3(SQ_WAVES * 64), 0, st,
                       (const uint8_t*)dst, h->stride, (long long)n, h->d, h->step(), h->rterm + h->n);
    HIP_TRY(hipGetLastError());
    if ((rc = sq_end(h, st))) return rc;
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
    int rc = sq_begin(h, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(codes, (size_t)h->d, h->codes + (size_t)i0 * h->stride, (size_t)h->stride, (size_t)h->d, (size_t)n,
                             hipMemcpyDeviceToHost, st));
    if ((rc = sq_end(h, st))) return rc;
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
    int rc = sq_begin(h, st);
    if (rc) return rc;
    for (long long j0 = 0; j0 < n; j0 += step) {
        const long long m = std::min<long long>(step, n - j0);
        if ((rc = sq_grow(h->xraw, (size_t)m * h->d))) return rc;
        decode_launch(h, h->codes + (size_t)(i0 + j0) * h->stride, h->stride, m, h->xraw.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x + (size_t)j0 * h->d, h->xraw.p, (size_t)m * h->d * sizeof(float), hipMemcpyDeviceToHost, st));
        if ((rc = sq_end(h, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_sq_search_device(ise_sq_t* h, const float* q_dev, int64_t nq, int k, float* D_dev, int64_t* I_dev,
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

extern "C" int ise_sq_search_host(ise_sq_t* h, const float* q, int64_t nq, int k, float* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k, D, I);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (check_trained(h)) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long batch = std::min<long long>(nq, 4096);
    if ((rc = sq_grow(h->xraw, (size_t)batch * h->d))) return rc;
    if ((rc = sq_grow(h->oD, (size_t)batch * k))) return rc;
    if ((rc = sq_grow(h->oI, (size_t)batch * k))) return rc;
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        if ((rc = sq_begin(h, st))) return rc;
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
