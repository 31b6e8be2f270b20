// ise_binary_scan.hip -- host side of the binary flat index (include/ise_knn.h, ise_binary_index_*): storage,
// launches of the kernels of ise_binary_scan.hpp, the C entry points.  faiss.IndexBinaryFlat: exact Hamming kNN and
// range search; the reference's DHASH method (backend/engine.py:82-91) asks it for "every image within r bits".
//
// Calls on one handle run one at a time (a mutex; the host forms hold it until their results are back, the device
// forms while they enqueue).  The handle has ONE set of workspaces: work enqueued on another stream than the previous
// call's waits for that call through an event, and a workspace that has to grow is replaced only after the device
// has drained.
#include "ise_binary_scan.hpp"

extern int ise_fail_(int code, const std::string& msg);  // ise_knn.hip: sets the thread-local message

#define BIN_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ise_fail_(e_ == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP,                  \
                             std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

#define BIN_RANGE_NQ_CHUNK 256 /* queries per range batch: one host synchronisation each */
static_assert(BIN_RANGE_NQ_CHUNK <= 256, "binary_lims_kernel scans a batch's totals in one block of 256 threads");

namespace {
template <class T>
struct BinBuf {  // grown lazily, contents not kept
    T* p = nullptr;
    size_t n = 0;
};

template <class T>
int bin_grow(BinBuf<T>& b, size_t need) {
    if (b.p && need <= b.n) return ISE_OK;
    if (b.p) {
        BIN_TRY(hipDeviceSynchronize());  // work in flight on any stream may still use the old one
        (void)hipFree(b.p);
    }
    b.p = nullptr;
    b.n = 0;
    const size_t want = std::max<size_t>(need + need / 2, 16);
    BIN_TRY(hipMalloc((void**)&b.p, want * sizeof(T)));
    b.n = want;
    return ISE_OK;
}
}  // namespace

struct ise_binary_index {
    int d_bits = 0, code_size = 0, ws = 0, device = 0, num_cu = 256;
    long long n = 0, cap = 0;
    u64* codes = nullptr;  // [cap][ws]; bytes past code_size of every row are zero
    hipStream_t stream = nullptr;
    hipEvent_t last = nullptr;  // the end of the previous call's device work
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    mutable std::mutex mu;
    BinBuf<uint8_t> raw;       // host forms: the queries as passed
    BinBuf<u64> qpad, lo, lists;
    BinBuf<int> oD, counts, rD;
    BinBuf<long long> oI, offs, totals, lims, rI;
    uint64_t st_search = 0, st_passes = 0, st_range = 0;
};

struct ise_binary_range_result {
    std::vector<int64_t> lims;
    std::vector<int32_t> D;
    std::vector<int64_t> I;
};

namespace {
int bin_wt(const ise_binary_index* h) { return h->ws == 1 ? 1 : h->ws == 2 ? 2 : 0; }
size_t bin_query_lds(const ise_binary_index* h) { return bin_wt(h) == 0 ? (size_t)BIN_QT * h->ws * 8 : 0; }

// order this call's device work behind the previous call's, and mark its own end
int bin_begin(ise_binary_index* h, hipStream_t st) {
    if (h->last_valid && h->last_stream != st) BIN_TRY(hipStreamWaitEvent(st, h->last, 0));
    return ISE_OK;
}
int bin_end(ise_binary_index* h, hipStream_t st) {
    BIN_TRY(hipEventRecord(h->last, st));
    h->last_stream = st;
    h->last_valid = true;
    return ISE_OK;
}

void launch_scan(int wt, unsigned grid, size_t lds, hipStream_t st, const BinScanParams& sp) {
    static LdsAttrOnce attr[3];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), BIN_LDS_MAX);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(BIN_WAVES * 64), lds, st, sp);
    };
    if (wt == 1) go(binary_scan_kernel<1>, attr[0]);
    else if (wt == 2) go(binary_scan_kernel<2>, attr[1]);
    else go(binary_scan_kernel<0>, attr[2]);
}

template <bool FILL>
void launch_range(int wt, unsigned grid, size_t lds, hipStream_t st, const BinRangeParams& rp) {
    if (wt == 1) hipLaunchKernelGGL((binary_range_kernel<1, FILL>), dim3(grid), dim3(BIN_WAVES * 64), lds, st, rp);
    else if (wt == 2) hipLaunchKernelGGL((binary_range_kernel<2, FILL>), dim3(grid), dim3(BIN_WAVES * 64), lds, st, rp);
    else hipLaunchKernelGGL((binary_range_kernel<0, FILL>), dim3(grid), dim3(BIN_WAVES * 64), lds, st, rp);
}

// blocks of a pass over the rows: about two 64-row tiles per wave on a short index, at most two blocks per CU
unsigned bin_grid(const ise_binary_index* h) {
    const long long tiles = (h->n + 63) / 64;
    long long g = (tiles + 2 * BIN_WAVES - 1) / (2 * BIN_WAVES);
    g = std::min<long long>(g, std::min<long long>(2ll * h->num_cu, MERGE_LISTS_MAX));
    return (unsigned)std::max<long long>(g, 1);
}

int reserve_codes(ise_binary_index* h, long long need, hipStream_t st) {
    if (need <= h->cap) return ISE_OK;
    long long want = need;
    if (h->cap > 0 && want < h->cap + h->cap / 2) want = h->cap + h->cap / 2;  // geometric growth on re-add
    want = (want + 63) / 64 * 64;
    const size_t rb = (size_t)h->ws * 8;
    u64* nx = nullptr;
    BIN_TRY(hipMalloc((void**)&nx, (size_t)want * rb));
    hipError_t e = hipSuccess;
    if (h->n > 0) e = hipMemcpyAsync(nx, h->codes, (size_t)h->n * rb, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync((char*)nx + (size_t)h->n * rb, 0, (size_t)(want - h->n) * rb, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h->codes) e = hipDeviceSynchronize();  // searches in flight still read the old storage
    if (e != hipSuccess) {
        (void)hipFree(nx);
        return ise_fail_(ISE_E_HIP, std::string("growing the code storage: ") + hipGetErrorString(e));
    }
    if (h->codes) (void)hipFree(h->codes);
    h->codes = nx;
    h->cap = want;
    return ISE_OK;
}

void pad_rows(const uint8_t* src_dev, int code_size, u64* dst, int ws, long long n, hipStream_t st) {
    const long long total = n * ws;
    hipLaunchKernelGGL(binary_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src_dev, code_size, dst,
                       ws, n);
}

int add_device_locked(ise_binary_index* h, const uint8_t* x_dev, long long n, hipStream_t st) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "a binary index holds fewer than 2^32 rows");
    int rc = bin_begin(h, st);
    if (rc) return rc;
    rc = reserve_codes(h, h->n + n, st);
    if (rc) return rc;
    pad_rows(x_dev, h->code_size, h->codes + (size_t)h->n * h->ws, h->ws, n, st);
    BIN_TRY(hipGetLastError());
    h->n += n;
    return bin_end(h, st);
}

// q_dev: nq x code_size bytes on the device; D_dev / I_dev: nq x k
int search_enqueue(ise_binary_index* h, const uint8_t* q_dev, long long nq, int k, int* D_dev, long long* I_dev,
                   hipStream_t st) {
    int rc = bin_begin(h, st);
    if (rc) return rc;
    if (h->n == 0) {
        h->st_search++;
        const long long cnt = nq * k;
        hipLaunchKernelGGL(binary_fill_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, D_dev, I_dev, cnt);
        BIN_TRY(hipGetLastError());
        return bin_end(h, st);
    }
    const unsigned grid = bin_grid(h);
    const long long nq16 = (nq + BIN_QT - 1) / BIN_QT * BIN_QT;
    if ((rc = bin_grow(h->qpad, (size_t)nq16 * h->ws))) return rc;
    if ((rc = bin_grow(h->lo, (size_t)nq16))) return rc;
    if ((rc = bin_grow(h->lists, (size_t)grid * BIN_QT * BIN_KPASS))) return rc;
    h->st_search++;  // counted once the batch is certain to be enqueued
    pad_rows(q_dev, h->code_size, h->qpad.p, h->ws, nq, st);
    const int wt = bin_wt(h);
    const size_t lds = BIN_BUF_BYTES + BIN_CNT_BYTES + bin_query_lds(h);
    for (long long q0 = 0; q0 < nq; q0 += BIN_QT) {
        const int nqt = (int)std::min<long long>(BIN_QT, nq - q0);
        for (int off = 0; off < k; off += BIN_KPASS) {
            const int kp = std::min(BIN_KPASS, k - off);
            BinScanParams sp{};
            sp.codes = h->codes;
            sp.ws = h->ws;
            sp.n = h->n;
            sp.qpad = h->qpad.p + (size_t)q0 * h->ws;
            sp.nqt = nqt;
            sp.kp = kp;
            sp.lo = off == 0 ? nullptr : h->lo.p + q0;  // the merge of the pass before wrote it
            sp.lists = h->lists.p;
            launch_scan(wt, grid, lds, st, sp);
            MergeParams mp{};
            mp.lists = h->lists.p;
            mp.stride_list = (long long)BIN_QT * BIN_KPASS;
            mp.stride_qtile = 0;
            mp.qt = BIN_QT;
            mp.n_lists = (int)grid;
            mp.nq = nqt;
            mp.k = kp;
            BinMergeOut mo{};
            mo.D = D_dev + (size_t)q0 * k;
            mo.I = I_dev + (size_t)q0 * k;
            mo.lo = h->lo.p + q0;
            mo.k = k;
            mo.off = off;
            hipLaunchKernelGGL(binary_merge_kernel, dim3((unsigned)nqt), dim3(MERGE_THREADS), 0, st, mp, mo);
            h->st_passes++;
        }
    }
    BIN_TRY(hipGetLastError());
    return bin_end(h, st);
}

int check_handle(const ise_binary_index* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "binary index handle is NULL"); }

int check_search_args(const ise_binary_index* h, const void* q, long long nq, int k) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (nq < 0) return ise_fail_(ISE_E_INVALID, "nq must be >= 0");
    if (k < 1 || k > ISE_MAX_K) return ise_fail_(ISE_E_INVALID, "k must be in [1, ISE_MAX_K]");
    if (nq > 0 && !q) return ise_fail_(ISE_E_INVALID, "query pointer is NULL");
    if (nq * (long long)k >= (1ll << 40)) return ise_fail_(ISE_E_INVALID, "nq * k is too large");
    return ISE_OK;
}

// one batch of m <= BIN_RANGE_NQ_CHUNK queries (host pointer) appended to the result
int range_batch(ise_binary_index* h, hipStream_t st, const uint8_t* q, long long m, int radius, ise_binary_range_result* res) {
    int rc;
    const long long m16 = (m + BIN_QT - 1) / BIN_QT * BIN_QT;
    const unsigned grid = bin_grid(h);
    const int S = (int)grid * BIN_WAVES;
    long long seg_rows = (h->n + S - 1) / S;
    seg_rows = (seg_rows + 63) / 64 * 64;
    const long long M = m * S;
    if ((rc = bin_grow(h->raw, (size_t)m * h->code_size))) return rc;
    if ((rc = bin_grow(h->qpad, (size_t)m16 * h->ws))) return rc;
    if ((rc = bin_grow(h->counts, (size_t)M))) return rc;
    if ((rc = bin_grow(h->offs, (size_t)M))) return rc;
    if ((rc = bin_grow(h->lims, (size_t)m + 1))) return rc;
    if ((rc = bin_grow(h->totals, (size_t)m))) return rc;
    BIN_TRY(hipMemcpyAsync(h->raw.p, q, (size_t)m * h->code_size, hipMemcpyHostToDevice, st));
    pad_rows(h->raw.p, h->code_size, h->qpad.p, h->ws, m, st);
    const int wt = bin_wt(h);
    const size_t lds = bin_query_lds(h);
    BinRangeParams rp{};
    rp.codes = h->codes;
    rp.ws = h->ws;
    rp.n = h->n;
    rp.radius = radius;
    rp.seg_rows = seg_rows;
    rp.S = S;
    for (long long q0 = 0; q0 < m; q0 += BIN_QT) {
        rp.qpad = h->qpad.p + (size_t)q0 * h->ws;
        rp.nqt = (int)std::min<long long>(BIN_QT, m - q0);
        rp.counts = h->counts.p + (size_t)q0 * S;
        launch_range<false>(wt, grid, lds, st, rp);
    }
    hipLaunchKernelGGL(binary_offsets_kernel, dim3((unsigned)m), dim3(BIN_SCAN_THREADS), 0, st, h->counts.p, S, h->offs.p,
                       h->totals.p);
    hipLaunchKernelGGL(binary_lims_kernel, dim3(1), dim3(256), 0, st, h->totals.p, (int)m, h->lims.p);
    BIN_TRY(hipGetLastError());
    std::vector<long long> lims((size_t)m + 1);
    BIN_TRY(hipMemcpyAsync(lims.data(), h->lims.p, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, st));
    BIN_TRY(hipStreamSynchronize(st));  // the one host synchronisation that sizes the result
    const long long total = lims[(size_t)m];
    const size_t at = res->D.size();
    for (long long i = 1; i <= m; i++) res->lims.push_back((int64_t)at + lims[(size_t)i]);
    if (total == 0) return ISE_OK;
    if ((rc = bin_grow(h->rD, (size_t)total))) return rc;
    if ((rc = bin_grow(h->rI, (size_t)total))) return rc;
    rp.D = h->rD.p;
    rp.I = h->rI.p;
    for (long long q0 = 0; q0 < m; q0 += BIN_QT) {
        rp.qpad = h->qpad.p + (size_t)q0 * h->ws;
        rp.nqt = (int)std::min<long long>(BIN_QT, m - q0);
        rp.offs = h->offs.p + (size_t)q0 * S;
        rp.lims = h->lims.p + q0;
        launch_range<true>(wt, grid, lds, st, rp);
    }
    BIN_TRY(hipGetLastError());
    res->D.resize(at + (size_t)total);
    res->I.resize(at + (size_t)total);
    BIN_TRY(hipMemcpyAsync(res->D.data() + at, h->rD.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    BIN_TRY(hipMemcpyAsync(res->I.data() + at, h->rI.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    BIN_TRY(hipStreamSynchronize(st));
    return ISE_OK;
}

void free_buffers(ise_binary_index* h) {
    auto drop = [](auto& b) {
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr;
        b.n = 0;
    };
    drop(h->raw); drop(h->qpad); drop(h->lo); drop(h->lists); drop(h->oD); drop(h->counts); drop(h->rD);
    drop(h->oI); drop(h->offs); drop(h->totals); drop(h->lims); drop(h->rI);
    if (h->codes) (void)hipFree(h->codes);
    h->codes = nullptr;
}
}  // namespace

extern "C" int ise_binary_index_create(ise_binary_index_t** out, int d_bits, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d_bits <= 0 || d_bits % 8 != 0 || d_bits > ISE_BINARY_MAX_BITS)
        return ise_fail_(ISE_E_INVALID, "d_bits must be a positive multiple of 8, at most ISE_BINARY_MAX_BITS");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ise_fail_(ISE_E_NODEVICE, "no HIP device visible: the kNN path needs an MI355X (gfx950) GPU");
    if (device < 0 || device >= ndev) return ise_fail_(ISE_E_INVALID, "device out of range");
    hipDeviceProp_t prop;
    BIN_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ise_fail_(ISE_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    ise_binary_index* h = new (std::nothrow) ise_binary_index();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d_bits = d_bits;
    h->code_size = d_bits / 8;
    const int w = (h->code_size + 7) / 8;
    h->ws = w == 1 ? 1 : (w + 1) / 2 * 2;
    h->device = device;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    DeviceGuard gd(device);
    if (!gd.ok) {
        delete h;
        return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    }
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->last, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return ise_fail_(ISE_E_HIP, std::string("binary index setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_binary_index_destroy(ise_binary_index_t* h) {
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

extern "C" int ise_binary_index_reset(ise_binary_index_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->n = 0;  // capacity is kept; stale rows are masked by row number, their pad bytes are zero already
    return ISE_OK;
}

extern "C" int ise_binary_index_info(const ise_binary_index_t* h, int* d_bits, int64_t* ntotal, int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (d_bits) *d_bits = h->d_bits;
    if (ntotal) *ntotal = h->n;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_binary_index_add_device(ise_binary_index_t* h, const uint8_t* codes_dev, int64_t n, void* stream) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (n < 0 || (n > 0 && !codes_dev)) return ise_fail_(ISE_E_INVALID, "bad codes / n");
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    return add_device_locked(h, codes_dev, n, (hipStream_t)stream);
}

extern "C" int ise_binary_index_add_host(ise_binary_index_t* h, const uint8_t* codes, int64_t n) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (n < 0 || (n > 0 && !codes)) return ise_fail_(ISE_E_INVALID, "bad codes / n");
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    const long long step = std::max<long long>(1, (1ll << 28) / h->code_size);  // 256 MiB of codes per upload
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        int rc = bin_grow(h->raw, (size_t)m * h->code_size);
        if (rc) return rc;
        BIN_TRY(hipMemcpyAsync(h->raw.p, codes + (size_t)i0 * h->code_size, (size_t)m * h->code_size, hipMemcpyHostToDevice,
                               h->stream));
        rc = add_device_locked(h, h->raw.p, m, h->stream);
        if (rc) return rc;
        BIN_TRY(hipStreamSynchronize(h->stream));
    }
    return ISE_OK;
}

extern "C" int ise_binary_index_reconstruct_host(ise_binary_index_t* h, int64_t i0, int64_t n, uint8_t* out) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 < 0 || n < 0 || i0 + n > h->n) return ise_fail_(ISE_E_INVALID, "row range out of bounds");
    if (n == 0) return ISE_OK;
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = bin_begin(h, h->stream);
    if (rc) return rc;
    BIN_TRY(hipMemcpy2DAsync(out, (size_t)h->code_size, h->codes + (size_t)i0 * h->ws, (size_t)h->ws * 8, (size_t)h->code_size,
                             (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if ((rc = bin_end(h, h->stream))) return rc;
    BIN_TRY(hipStreamSynchronize(h->stream));
    return ISE_OK;
}

extern "C" int ise_binary_index_search_device(ise_binary_index_t* h, const uint8_t* q_dev, int64_t nq, int k, int32_t* D_dev,
                                              int64_t* I_dev, void* stream) {
    int rc = check_search_args(h, q_dev, nq, k);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    if (!D_dev || !I_dev) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    return search_enqueue(h, q_dev, nq, k, (int*)D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_binary_index_search_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int k, int32_t* D,
                                            int64_t* I) {
    int rc = check_search_args(h, q, nq, k);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    if (!D || !I) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t cnt = (size_t)nq * k;
    if ((rc = bin_grow(h->raw, (size_t)nq * h->code_size))) return rc;
    if ((rc = bin_grow(h->oD, cnt))) return rc;
    if ((rc = bin_grow(h->oI, cnt))) return rc;
    if ((rc = bin_begin(h, h->stream))) return rc;
    BIN_TRY(hipMemcpyAsync(h->raw.p, q, (size_t)nq * h->code_size, hipMemcpyHostToDevice, h->stream));
    if ((rc = search_enqueue(h, h->raw.p, nq, k, h->oD.p, h->oI.p, h->stream))) return rc;
    BIN_TRY(hipMemcpyAsync(D, h->oD.p, cnt * 4, hipMemcpyDeviceToHost, h->stream));
    BIN_TRY(hipMemcpyAsync(I, h->oI.p, cnt * 8, hipMemcpyDeviceToHost, h->stream));
    BIN_TRY(hipStreamSynchronize(h->stream));
    return ISE_OK;
}

extern "C" int ise_binary_index_range_search_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int32_t radius,
                                                  ise_binary_range_result_t** out) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (check_handle(h)) return ISE_E_INVALID;
    if (nq < 0 || (nq > 0 && !q)) return ise_fail_(ISE_E_INVALID, "bad queries / nq");
    ise_binary_range_result* res = new (std::nothrow) ise_binary_range_result();
    if (!res) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    int rc = ISE_OK;
    try {
        res->lims.reserve((size_t)nq + 1);
        res->lims.push_back(0);
        DeviceGuard gd(h->device);
        if (!gd.ok) rc = ise_fail_(ISE_E_HIP, "hipSetDevice failed");
        std::lock_guard<std::mutex> lk(h->mu);
        if (!rc && (h->n == 0 || radius <= 0)) {
            res->lims.resize((size_t)nq + 1, 0);  // nothing can match: no pass
        } else if (!rc) {
            rc = bin_begin(h, h->stream);
            for (long long q0 = 0; q0 < nq && !rc; q0 += BIN_RANGE_NQ_CHUNK) {
                const long long m = std::min<long long>(BIN_RANGE_NQ_CHUNK, nq - q0);
                h->st_range++;
                rc = range_batch(h, h->stream, q + (size_t)q0 * h->code_size, m, radius, res);
            }
            if (!rc) rc = bin_end(h, h->stream);  // the workspaces' last user, as after every other call
        }
    } catch (const std::bad_alloc&) {
        rc = ise_fail_(ISE_E_NOMEM, "host allocation of the range result failed");
    }
    if (rc) {
        delete res;
        return rc;
    }
    *out = res;
    return ISE_OK;
}

extern "C" int ise_binary_range_result_get(const ise_binary_range_result_t* r, int64_t* nq, const int64_t** lims,
                                           const int32_t** D, const int64_t** I) {
    if (!r) return ise_fail_(ISE_E_INVALID, "range result is NULL");
    if (nq) *nq = (int64_t)r->lims.size() - 1;
    if (lims) *lims = r->lims.data();
    if (D) *D = r->D.data();
    if (I) *I = r->I.data();
    return ISE_OK;
}

extern "C" int ise_binary_range_result_destroy(ise_binary_range_result_t* r) {
    delete r;
    return ISE_OK;
}

extern "C" int ise_binary_index_stats(ise_binary_index_t* h, uint64_t* out3) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    out3[0] = h->st_search;
    out3[1] = h->st_passes;
    out3[2] = h->st_range;
    return ISE_OK;
}
