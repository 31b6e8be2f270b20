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
    int d = 0, stride = 0, qt = 0, qshift = 0, metric = ISE_METRIC_L2;
    SqCodec codec;
    IvfCore c;  // the sorted codes are c.rows: [c.inv.tiles * SQ_TILE][stride], their row terms c.side (float64)
    // host forms (they return with the stream drained): rows or queries as passed | codes as passed
    DevBuf<float> xraw;
    DevBuf<uint8_t> craw;
    IvfTiledWs w;  // one set of search workspaces; w.stage: one chunk's staged query records
};

namespace {
int check_handle(const ise_ivfsq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "inverted-list scalar-quantiser index handle is NULL"); }

void free_own(ise_ivfsq* h) {
    h->codec.destroy();
    buf_free(h->xraw, h->craw);
    h->w.free();
}

uint8_t* pend_codes(const ise_ivfsq* h, long long at) { return h->c.pend_row<uint8_t>(at); }
double* pend_rterm(const ise_ivfsq* h, long long at) { return reinterpret_cast<double*>(h->c.pend_side) + at; }

// pending rows [at, at + m) <- the codes and row terms of x_dev's rows (pad bytes zero); sets the codec's bad flag on a non-finite entry
int encode_pending(ise_ivfsq* h, const float* x_dev, long long at, long long m, hipStream_t st) {
    uint8_t* dst = pend_codes(h, at);
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)m * h->stride, st));
    h->codec.encode_launch(x_dev, m, dst, h->stride, pend_rterm(h, at), st);
    HIP_TRY(hipGetLastError());
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

// mu_ held, trained.  The shell is the lists' (ivf_tiled_search): this is how a chunk's queries are staged and what a
// pass is handed.  Blocks of a pass: ise_sq.hip's rule on the lists' tiles in all: about SQ_BLOCK_TILES tiles per wave,
// at most what the CUs hold at once
int search_enqueue(ise_ivfsq* h, const float* q_dev, long long nq, int k, const long long* probes_dev, int nprobe, float* D_dev,
                   long long* I_dev, hipStream_t st) {
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT, qt = h->qt;
    const size_t rec = sq_rec_bytes(h->d), lds = sq_lds_bytes(h->d, qt);
    const long long per_cu = std::max<long long>(1, (long long)SQ_LDS_LIMIT / (long long)lds);
    const IvfTiledShape shape{SQ_STAGE_CHUNK, qt, h->qshift, SQ_KPASS, SQ_BLOCK_TILES, SQ_WAVES, per_cu,
                              (size_t)std::min<long long>(nq, SQ_STAGE_CHUNK) * rec};
    return ivf_tiled_search(
        h->c, h->w, shape, nq, k, probes_dev, nprobe, D_dev, I_dev, ip, st,
        [&](long long c0, int m) {
            h->codec.stage_launch(q_dev + (size_t)c0 * h->d, m, ip, h->w.stage.p, st);
            return (int)ISE_OK;
        },
        [&](const IvfPass& ps) {
            SqIvfScanParams sp{};
            sp.codes = h->c.rows_as<uint8_t>();
            sp.rterm = reinterpret_cast<const double*>(h->c.side);
            sp.ids = h->c.inv.ids;
            sp.d = h->d;
            sp.stride = h->stride;
            sp.qrec = h->w.stage.p + (size_t)ps.g * qt * rec;
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
    return ivf_create(out, nlist, device, "inverted-list scalar-quantiser index setup",
                      [&](ise_ivfsq* h) {
                          h->d = d;
                          h->stride = sq_stride(d);
                          h->qt = sq_qt(d);
                          h->qshift = h->qt == 16 ? 4 : 3;
                          h->metric = metric;
                          h->c.tile_rows = SQ_TILE;
                          h->c.unit_bytes = 16;
                          h->c.row_bytes = (size_t)h->stride;
                          h->c.with_side = true;
                          return h->codec.create(d, qtype);
                      },
                      free_own);
}

extern "C" int ise_ivfsq_destroy(ise_ivfsq_t* h) { return ivf_destroy(h, free_own); }

extern "C" int ise_ivfsq_reset(ise_ivfsq_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    return ivf_reset(h->c, []() {});
}

extern "C" int ise_ivfsq_info(const ise_ivfsq_t* h, int* d, int* qtype, int* metric, int* nlist, int64_t* ntotal, int* is_trained,
                              int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d) *d = h->d;
    if (qtype) *qtype = h->codec.qtype;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->c.inv.nlist;
    if (ntotal) *ntotal = h->c.inv.n;
    if (is_trained) *is_trained = h->codec.trained ? 1 : 0;
    if (device) *device = h->c.device;
    return ISE_OK;
}

extern "C" int ise_ivfsq_set_trained_host(ise_ivfsq_t* h, const float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    if (h->c.inv.n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the trained state in place (reset first)");
    return h->codec.set_trained(t, h->c.device);
}

extern "C" int ise_ivfsq_get_trained_host(ise_ivfsq_t* h, float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    return h->codec.get_trained(t);
}

extern "C" int ise_ivfsq_add_host(ise_ivfsq_t* h, const float* x, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, x, list_no, n, "rows");
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = h->c.inv.check_lists(list_no, n)) || (rc = en.check())) return rc;
    hipStream_t st = h->c.stream;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    if ((rc = h->codec.bad.clear(st))) return rc;
    const long long step = upload_step((size_t)h->d * sizeof(float));
    if ((rc = grow_after_event(h->xraw, (size_t)std::min<long long>(step, n) * h->d, nullptr))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {  // nothing is counted in before the last piece's verdict
        const long long m = std::min<long long>(step, n - i0);
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = encode_pending(h, h->xraw.p, h->c.inv.pend_n + i0, m, st))) return rc;
    }
    if ((rc = h->codec.bad.check(st))) return rc;
    h->c.inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_add_device(ise_ivfsq_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream) {
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

extern "C" int ise_ivfsq_add_codes_host(ise_ivfsq_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, codes, list_no, n, "codes");
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = h->c.inv.check_lists(list_no, n)) || (rc = en.check())) return rc;
    hipStream_t st = h->c.stream;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    uint8_t* dst = pend_codes(h, h->c.inv.pend_n);
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * h->stride, st));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->stride, codes, (size_t)h->d, (size_t)h->d, (size_t)n, hipMemcpyHostToDevice, st));
    h->codec.rowterm_launch(dst, h->stride, n, pend_rterm(h, h->c.inv.pend_n), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    h->c.inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_list_sizes_host(ise_ivfsq_t* h, int64_t* sizes) {
    if (!sizes) return ise_fail_(ISE_E_INVALID, "sizes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->c.mu_);
    h->c.inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_ivfsq_list_host(ise_ivfsq_t* h, int list, int64_t* ids, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (list < 0 || list >= h->c.inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    IvfEntry en(h->c);
    int rc = en.check();
    if (rc || (rc = ivf_rebuild_locked(h->c, h->c.stream, ivf_no_hook))) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->c.inv.list_ids_host(list, SQ_TILE, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    if (codes)
        HIP_TRY(hipMemcpy2D(codes, (size_t)h->d, h->c.rows_as<uint8_t>() + slot0 * h->stride, (size_t)h->stride, (size_t)h->d, m,
                            hipMemcpyDeviceToHost));
    return ISE_OK;
}

extern "C" int ise_ivfsq_search_device(ise_ivfsq_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                                       float* D_dev, int64_t* I_dev, void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    return search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_ivfsq_search_host(ise_ivfsq_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                                     int64_t* I) {
    int rc = check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    IvfEntry en(h->c);
    if (h->codec.check_trained()) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    if ((rc = en.check())) return rc;
    return ivf_search_staged(h->d, h->c.stream, q, nq, k, probes, nprobe, D, I,
                             [&](const float* q_dev, long long m, const long long* p_dev, float* D_dev, long long* I_dev) {
                                 return search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->c.stream);
                             });
}

extern "C" int ise_ivfsq_stats(ise_ivfsq_t* h, uint64_t* out3) {
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    IvfEntry en(h->c);
    const int rc = en.check();
    return rc ? rc : h->c.stats(out3);
}
