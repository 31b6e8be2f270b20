// ise_ivfpq.hip -- host side and C ABI of the inverted-list index over product-quantiser codes (include/ise_knn.h,
// ise_ivfpq_*; kernels in ise_ivfpq.hpp and ise_pq.hpp).  faiss.IndexIVFPQ with by_residual = false.
//
// The codec is the flat product-quantised index's (PqCodec, ise_pq_host.hpp): the codebook comes from the caller, rows
// are encoded on the device by pq_encode_kernel.  The lists are the other kinds' (IvfCore, ise_ivf_lists.hpp): rows come
// in with their list numbers (the coarse quantiser lives with the caller), add() encodes them at once into a PENDING
// buffer of code rows and reads the encoder's non-finite flag back before anything is counted in; the first call that
// reads the lists afterwards (search, list_host) rebuilds them (ivf_rebuild_locked; 64-row tiles, 16-byte units, no
// side value).
//
// Calls on one handle run one at a time (a mutex).  The handle has ONE set of search workspaces: a search waits for
// the one before and marks its end once a pass may be enqueued (CallOrder, ise_host.hpp), and a workspace that has to
// grow is replaced by the after-event rule (grow_after_event, ise_host.hpp).
#include "ise_ivf_lists.hpp"
#include "ise_ivfpq.hpp"
#include "ise_pq_host.hpp"

struct ise_ivfpq {
    int qshift = 0, metric = ISE_METRIC_L2;
    PqCodec codec;
    IvfCore c;  // the sorted codes are c.rows: [c.inv.tiles * 64][stride]
    // host forms (they return with the stream drained): rows as passed
    DevBuf<float> xraw;
    IvfTiledWs w;  // one set of search workspaces; w.stage: one chunk's tables
    unsigned long long tables = 0;  // pq_table_kernel launches
};

namespace {
int check_handle(const ise_ivfpq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "inverted-list product-quantiser index handle is NULL"); }

void free_own(ise_ivfpq* h) {
    h->codec.destroy();
    buf_free(h->xraw);
    h->w.free();
}

// pending rows [at, at + m) <- the codes of x_dev's rows (pad bytes zero); sets the codec's bad flag on a non-finite entry
int encode_pending(ise_ivfpq* h, const float* x_dev, long long at, long long m, hipStream_t st) {
    uint8_t* dst = h->c.pend_row<uint8_t>(at);
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)m * h->codec.stride, st));
    h->codec.encode_launch(x_dev, m, dst, h->codec.stride, st);
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

PqScanLaunch<PqIvfScanParams> launch_scan{{ivfpq_scan_kernel<16>, ivfpq_scan_kernel<8>, ivfpq_scan_kernel<4>, ivfpq_scan_kernel<2>}, {}};

// mu_ held, trained.  The shell is the lists' (ivf_tiled_search): a chunk's staging is its tables (one pq_table_kernel
// launch), a pass is handed the group's tables.  Blocks of a pass: ise_pq.hip's rule on the lists' tiles in all: about
// two tiles per wave, at most what the CUs hold at once (their LDS)
int search_enqueue(ise_ivfpq* h, const float* q_dev, long long nq, int k, const long long* probes_dev, int nprobe, float* D_dev,
                   long long* I_dev, hipStream_t st) {
    const PqCodec& cd = h->codec;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT, qt = cd.qt;
    const size_t tab_q = cd.tab_floats(), lds = cd.lds_bytes();
    const IvfTiledShape shape{PQ_TAB_CHUNK, qt, h->qshift, PQ_KPASS, 2, PQ_WAVES, cd.blocks_per_cu(),
                              (size_t)std::min<long long>((nq + qt - 1) / qt * qt, PQ_TAB_CHUNK) * tab_q * sizeof(float)};
    return ivf_tiled_search(
        h->c, h->w, shape, nq, k, probes_dev, nprobe, D_dev, I_dev, ip, st,
        [&](long long c0, int m) {
            cd.table_launch(q_dev + (size_t)c0 * cd.d, m, ip, reinterpret_cast<float*>(h->w.stage.p), st);
            h->tables++;
            return (int)ISE_OK;
        },
        [&](const IvfPass& ps) {
            PqIvfScanParams sp{};
            sp.codes = h->c.rows_as<uint8_t>();
            sp.ids = h->c.inv.ids;
            sp.M = cd.M;
            sp.stride = cd.stride;
            sp.tab = reinterpret_cast<const float*>(h->w.stage.p) + (size_t)ps.g * qt * tab_q;
            sp.nqt = ps.nqt;
            sp.kp = ps.kp;
            sp.ip = ip;
            sp.lo = ps.lo;
            sp.lists = ps.lists;
            sp.work = ps.work;
            sp.count = ps.count;
            sp.tiles_loaded = h->c.stats_dev;
            launch_scan(qt, ps.grid, lds, st, sp);
        });
}

int check_search_args(const ise_ivfpq* h, const void* q, long long nq, int k, const void* probes, int nprobe, const void* D,
                      const void* I) {
    const int rc = check_ivf_knn_args(q, nq, k, probes, nprobe, D, I);
    return rc ? rc : check_handle(h);
}

int check_add_args(const ise_ivfpq* h, const void* x, const void* list_no, long long n, const char* what) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !list_no)) return ise_fail_(ISE_E_INVALID, std::string(what) + " or list numbers pointer is NULL");
    return check_handle(h);
}
}  // namespace

extern "C" int ise_ivfpq_create(ise_ivfpq_t** out, int d, int M, int nbits, int metric, int nlist, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (M <= 0) return ise_fail_(ISE_E_INVALID, "M must be positive");
    if (M > ISE_PQ_MAX_M) return ise_fail_(ISE_E_INVALID, "M must be at most ISE_PQ_MAX_M");
    if (d % M != 0) return ise_fail_(ISE_E_INVALID, "d must be a multiple of M");
    if (nbits != 8) return ise_fail_(ISE_E_INVALID, "nbits must be 8: only 8-bit sub-quantisers are provided");
    if (nlist <= 0) return ise_fail_(ISE_E_INVALID, "nlist must be positive");
    if (metric != ISE_METRIC_L2 && metric != ISE_METRIC_INNER_PRODUCT)
        return ise_fail_(ISE_E_INVALID, "metric must be ISE_METRIC_L2 or ISE_METRIC_INNER_PRODUCT");
    return ivf_create(out, nlist, device, "inverted-list product-quantiser index setup",
                      [&](ise_ivfpq* h) {
                          const hipError_t e = h->codec.create(d, M);
                          const int qt = h->codec.qt;
                          h->qshift = qt == 16 ? 4 : qt == 8 ? 3 : qt == 4 ? 2 : 1;
                          h->metric = metric;
                          h->c.tile_rows = PQ_IVF_TILE;
                          h->c.unit_bytes = 16;
                          h->c.row_bytes = (size_t)h->codec.stride;
                          h->c.with_side = false;
                          return e;
                      },
                      free_own);
}

extern "C" int ise_ivfpq_destroy(ise_ivfpq_t* h) { return ivf_destroy(h, free_own); }

extern "C" int ise_ivfpq_reset(ise_ivfpq_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    return ivf_reset(h->c, []() {});
}

extern "C" int ise_ivfpq_info(const ise_ivfpq_t* h, int* d, int* M, int* nbits, int* metric, int* nlist, int64_t* ntotal,
                              int* is_trained, int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d) *d = h->codec.d;
    if (M) *M = h->codec.M;
    if (nbits) *nbits = 8;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->c.inv.nlist;
    if (ntotal) *ntotal = h->c.inv.n;
    if (is_trained) *is_trained = h->codec.trained ? 1 : 0;
    if (device) *device = h->c.device;
    return ISE_OK;
}

extern "C" int ise_ivfpq_set_centroids_host(ise_ivfpq_t* h, const float* c) {
    if (!c) return ise_fail_(ISE_E_INVALID, "centroid pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    if (h->c.inv.n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the centroids in place (reset first)");
    return h->codec.set_centroids(c, h->c.device);
}

extern "C" int ise_ivfpq_get_centroids_host(ise_ivfpq_t* h, float* c) {
    if (!c) return ise_fail_(ISE_E_INVALID, "centroid pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    return h->codec.get_centroids(c, h->c.device);
}

extern "C" int ise_ivfpq_add_host(ise_ivfpq_t* h, const float* x, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, x, list_no, n, "rows");
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = h->c.inv.check_lists(list_no, n)) || (rc = en.check())) return rc;
    hipStream_t st = h->c.stream;
    const int d = h->codec.d;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    const long long step = upload_step((size_t)d * sizeof(float));
    if ((rc = grow_after_event(h->xraw, (size_t)std::min<long long>(step, n) * d, nullptr))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {  // nothing is counted in before the last piece's verdict
        const long long m = std::min<long long>(step, n - i0);
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * d, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = encode_pending(h, h->xraw.p, h->c.inv.pend_n + i0, m, st))) return rc;
    }
    if ((rc = h->codec.bad.check(st))) return rc;
    h->c.inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfpq_add_device(ise_ivfpq_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream) {
    int rc = check_add_args(h, x_dev, list_no_dev, n, "rows");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    std::vector<int64_t> lists;
    if ((rc = h->c.download_lists(list_no_dev, n, st, &lists))) return rc;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    if ((rc = encode_pending(h, x_dev, h->c.inv.pend_n, n, st))) return rc;
    if ((rc = h->codec.bad.check(st))) return rc;
    h->c.inv.add(lists.data(), n);
    return ISE_OK;
}

extern "C" int ise_ivfpq_add_codes_host(ise_ivfpq_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, codes, list_no, n, "codes");
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = h->c.inv.check_lists(list_no, n)) || (rc = en.check())) return rc;
    hipStream_t st = h->c.stream;
    const size_t M = (size_t)h->codec.M, stride = (size_t)h->codec.stride;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    uint8_t* dst = h->c.pend_row<uint8_t>(h->c.inv.pend_n);
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * stride, st));
    HIP_TRY(hipMemcpy2DAsync(dst, stride, codes, M, M, (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->c.inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfpq_list_sizes_host(ise_ivfpq_t* h, int64_t* sizes) {
    if (!sizes) return ise_fail_(ISE_E_INVALID, "sizes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    h->c.inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_ivfpq_list_host(ise_ivfpq_t* h, int list, int64_t* ids, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (list < 0 || list >= h->c.inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    IvfEntry en(h->c);
    int rc = en.check();
    if (rc || (rc = ivf_rebuild_locked(h->c, h->c.stream, ivf_no_hook))) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->c.inv.list_ids_host(list, PQ_IVF_TILE, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    const size_t M = (size_t)h->codec.M, stride = (size_t)h->codec.stride;
    if (codes) HIP_TRY(hipMemcpy2D(codes, M, h->c.rows_as<uint8_t>() + slot0 * stride, stride, M, m, hipMemcpyDeviceToHost));
    return ISE_OK;
}

extern "C" int ise_ivfpq_search_device(ise_ivfpq_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                                       float* D_dev, int64_t* I_dev, void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    return search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_ivfpq_search_host(ise_ivfpq_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                                     int64_t* I) {
    int rc = check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    return ivf_search_staged(h->codec.d, h->c.stream, q, nq, k, probes, nprobe, D, I,
                             [&](const float* q_dev, long long m, const long long* p_dev, float* D_dev, long long* I_dev) {
                                 return search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->c.stream);
                             });
}

extern "C" int ise_ivfpq_stats(ise_ivfpq_t* h, uint64_t* out4) {
    if (!out4) return ise_fail_(ISE_E_INVALID, "out4 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    IvfEntry en(h->c);
    const int rc = en.check();
    if (rc) return rc;
    out4[3] = h->tables;
    return h->c.stats(out4);
}
