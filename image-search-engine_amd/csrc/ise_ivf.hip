// ise_ivf.hip -- host side and C ABI of the inverted-list index (include/ise_knn.h, ise_ivf_*; kernels in
// ise_ivf.hpp).  Own translation unit so the kernel families compile in parallel.
//
// Rows come in with their list numbers (the coarse quantiser lives with the caller).  add() checks the numbers and
// appends the rows, in insertion order, to a PENDING buffer; the first call that reads the lists afterwards (search,
// list_host) rebuilds: the host works out where every pending row goes (ise_ivf_plan.hpp, a stable counting sort of the
// list numbers), a new row array of exactly the needed tiles is allocated, the old tiles move to where their lists now
// start, the pending rows are scattered behind them, and the shift vector and the norms are recomputed.  One rebuild
// therefore moves the whole index.  Rows, ids, norms, the table and the shift vector all go into fresh buffers that are
// swapped in together (a pass still in flight on another stream keeps a consistent set); the old ones and the pending
// buffer are freed when it is done.  Between calls the index holds the sorted array (exact size) plus the pending
// buffer (at most twice the pending rows).  The lists' counts, ids and table are IvfLists (ise_ivf_lists.hpp), shared
// with the lists over 8-bit rows; the rows, the norms and the shift vector are this file's.
//
// Calls on one handle run one at a time (a mutex).  The handle has ONE set of search workspaces: a search waits for
// the one before and marks its end once a pass may be enqueued (CallOrder, ise_host.hpp), and a workspace that has to
// grow is replaced by the after-event rule (grow_after_event, ise_host.hpp).
#include "ise_geometry.hpp"
#include "ise_scan_params.hpp"
#include "ise_ivf.hpp"
#include "ise_ivf_lists.hpp"

#define IVF_NQ_CHUNK 64 /* queries per launch (4 groups of 16): bounds the per-block lists */

struct ise_ivf {
    int d = 0, dp = 0, metric = ISE_METRIC_L2;
    IvfCore c;  // the sorted rows are c.rows: [c.inv.tiles * 16][dp] float32, no side value
    float* norms = nullptr;  // [c.inv.tiles * 16] |y - mu|^2 (L2)
    float* mu = nullptr;     // [dp]
    // one set of search workspaces: *_device calls on different streams are ordered one behind the other
    DevBuf<float> q;         // [chunk][dp] padded queries
    DevBuf<u64> part;        // [groups][blocks][16][kpass]
    DevBuf<u64> keys;        // [chunk][32] one pass's merged keys (k > 32) | [chunk] floors
    DevBuf<uint32_t> masks;  // [groups][nlist]
};

static void ivf_free_norms(ise_ivf* h) {
    if (h->norms) (void)hipFree(h->norms);
    h->norms = nullptr;
}

static void ivf_free_own(ise_ivf* h) {
    ivf_free_norms(h);
    if (h->mu) (void)hipFree(h->mu);
    buf_free(h->q, h->part, h->keys, h->masks);
}

extern "C" int ise_ivf_create(ise_ivf_t** out, int d, int metric, int nlist, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (nlist <= 0) return ise_fail_(ISE_E_INVALID, "nlist must be positive");
    if (metric != ISE_METRIC_L2 && metric != ISE_METRIC_INNER_PRODUCT)
        return ise_fail_(ISE_E_INVALID, "metric must be ISE_METRIC_L2 or ISE_METRIC_INNER_PRODUCT");
    return ivf_create(out, nlist, device, "inverted-list index setup",
                      [&](ise_ivf* h) {
                          h->d = d;
                          h->dp = pad_dim(d, ISE_STORE_F32);
                          h->metric = metric;
                          h->c.tile_rows = 16;
                          h->c.unit_bytes = 16;
                          h->c.row_bytes = (size_t)h->dp * sizeof(float);
                          const hipError_t e = hipMalloc((void**)&h->mu, h->c.row_bytes);
                          return e == hipSuccess ? hipMemset(h->mu, 0, h->c.row_bytes) : e;
                      },
                      ivf_free_own);
}

extern "C" int ise_ivf_destroy(ise_ivf_t* h) { return ivf_destroy(h, ivf_free_own); }

extern "C" int ise_ivf_reset(ise_ivf_t* h) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    return ivf_reset(h->c, [&]() { ivf_free_norms(h); });
}

extern "C" int ise_ivf_info(const ise_ivf_t* h, int* d, int* metric, int* nlist, int64_t* ntotal, int* device) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (d) *d = h->d;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->c.inv.nlist;
    if (ntotal) *ntotal = h->c.inv.n;
    if (device) *device = h->c.device;
    return ISE_OK;
}

// ---------------------------------------------------------------- add
extern "C" int ise_ivf_add_host(ise_ivf_t* h, const float* x, const int64_t* list_no, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !list_no)) return ise_fail_(ISE_E_INVALID, "rows or list numbers pointer is NULL");
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (n == 0) return ISE_OK;
    IvfEntry en(h->c);
    int rc = h->c.inv.check_lists(list_no, n);
    if (rc || (rc = en.check())) return rc;
    hipStream_t st = h->c.stream;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    float* dst = h->c.pend_row<float>(h->c.inv.pend_n);
    if (h->dp != h->d) HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * h->dp * sizeof(float), st));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->dp * sizeof(float), x, (size_t)h->d * sizeof(float), (size_t)h->d * sizeof(float),
                             (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->c.inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivf_add_device(ise_ivf_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x_dev || !list_no_dev)) return ise_fail_(ISE_E_INVALID, "rows or list numbers pointer is NULL");
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (n == 0) return ISE_OK;
    hipStream_t st = (hipStream_t)stream;
    IvfEntry en(h->c);
    int rc = en.check();
    if (rc) return rc;
    std::vector<int64_t> lists;
    if ((rc = h->c.download_lists(list_no_dev, n, st, &lists))) return rc;
    if ((rc = h->c.reserve_pending(n, st))) return rc;
    const long long tot = (long long)n * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x_dev, h->d, h->dp, tot,
                       h->c.pend_row<float>(h->c.inv.pend_n));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    h->c.inv.add(lists.data(), n);
    return ISE_OK;
}

// ---------------------------------------------------------------- rebuild
// the lists' rebuild (ivf_rebuild_locked, ise_ivf_lists.hpp) with this kind's hook: the shift vector and the norms are
// computed on the new array before the stream drains, into buffers of their own that go in together with the rows -- a
// pass still in flight keeps the mu its norms belong to.  One rebuild therefore moves the whole index
static int ivf_rebuild_with_norms(ise_ivf* h, hipStream_t st) {
    float *nn = nullptr, *partial = nullptr, *nmu = nullptr;
    DevFreeList<3> fr{{(void**)&nn, (void**)&partial, (void**)&nmu}};
    bool rebuilt = false;
    const int rc = ivf_rebuild_locked(
        h->c, st,
        [&](char* rows, size_t slots) {
            const float* nx = reinterpret_cast<const float*>(rows);
            HIP_TRY(hipMalloc((void**)&nn, slots * sizeof(float)));
            if (h->metric != ISE_METRIC_L2) {
                HIP_TRY(hipMemsetAsync(nn, 0, slots * sizeof(float), st));
                return (int)ISE_OK;
            }
            // the shift vector: the column mean of the rows as they stand (it decides how tight the bounds are, nothing else)
            const int groups = (int)std::min<long long>(1024, std::max<long long>(1, (long long)slots / 256));
            HIP_TRY(hipMalloc((void**)&nmu, (size_t)h->dp * sizeof(float)));
            HIP_TRY(hipMalloc((void**)&partial, (size_t)groups * h->dp * sizeof(float)));
            const unsigned gx = (unsigned)((h->dp + 255) / 256);
            hipLaunchKernelGGL(ivf_col_sum_kernel, dim3(gx, (unsigned)groups), dim3(256), 0, st, nx, (long long)slots, h->d, h->dp,
                               groups, partial);
            hipLaunchKernelGGL(ivf_col_mean_kernel, dim3(gx), dim3(256), 0, st, (const float*)partial, h->c.inv.n, h->d, h->dp, groups,
                               nmu);
            hipLaunchKernelGGL(ivf_norms_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, st, nx, (long long)slots, h->dp,
                               (const float*)nmu, nn);
            return (int)ISE_OK;
        },
        &rebuilt);
    if (rebuilt) {  // the old ones go with the guard
        std::swap(h->norms, nn);
        if (nmu) std::swap(h->mu, nmu);
    }
    return rc;
}

extern "C" int ise_ivf_list_sizes_host(ise_ivf_t* h, int64_t* sizes) {
    if (!h || !sizes) return ise_fail_(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->c.mu_);
    h->c.inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_ivf_list_host(ise_ivf_t* h, int list, int64_t* ids, float* rows) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (list < 0 || list >= h->c.inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    IvfEntry en(h->c);
    int rc = en.check();
    if (rc || (rc = ivf_rebuild_with_norms(h, h->c.stream))) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->c.inv.list_ids_host(list, 16, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    if (rows)
        HIP_TRY(hipMemcpy2D(rows, (size_t)h->d * sizeof(float), h->c.rows_as<float>() + slot0 * h->dp, (size_t)h->dp * sizeof(float),
                            (size_t)h->d * sizeof(float), m, hipMemcpyDeviceToHost));
    return ISE_OK;
}

// ---------------------------------------------------------------- search
template <bool SHIFT>
static void launch_ivf_v(int ch, dim3 grid, size_t lds, hipStream_t st, const IvfScanParams& sp) {
    static LdsAttrOnce attr[3];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), LDS_LIMIT);
        hipLaunchKernelGGL(kern, grid, dim3(SEL_W * 64), lds, st, sp);
    };
    if (ch >= 4) go(ivf_scan_kernel<4, SHIFT>, attr[0]);
    else if (ch == 2) go(ivf_scan_kernel<2, SHIFT>, attr[1]);
    else go(ivf_scan_kernel<1, SHIFT>, attr[2]);
}

// one chunk of m <= IVF_NQ_CHUNK queries (mu_ held, the lists rebuilt and not empty): pad the queries, build the
// masks, then per 32 results one pass + the merge of its per-block lists
static int ivf_chunk_enqueue(ise_ivf* h, const float* q_dev, long long m, int k, const long long* probes_dev, int nprobe,
                             float* D_dev, long long* I_dev, hipStream_t st) {
    const bool l2 = h->metric == ISE_METRIC_L2;
    IvfScanParams sp{};
    sp.xb = h->c.rows_as<float>(); sp.norms = h->norms; sp.mu = h->mu; sp.ids = h->c.inv.ids;
    sp.list_tile0 = h->c.inv.list_tile0_dev(); sp.list_size = h->c.inv.list_size_dev(); sp.tile_list = h->c.inv.tile_list_dev();
    sp.nlist = h->c.inv.nlist; sp.d = h->d; sp.dp = h->dp;
    sp.qs_stride = qs_stride_units(h->dp);
    sp.row_slots = h->dp / 4;
    sp.nq = (int)m; sp.metric = h->metric;
    sp.beta = l2 ? exact_beta_dp(h->dp) : 0.f;
    range_staging_rule(SEL_W, false, h->d, sp.qs_stride, &sp.tpr, &sp.vec_q);  // the pass's own 8 waves stage the queries
    sp.tiles_loaded = h->c.stats_dev;
    const int ch = std::min(chunk_steps_rb((size_t)h->dp * sizeof(float)), 4);
    // at least a tile per wave, at most two blocks per CU (what their LDS lets a CU hold) and the merge's list count
    const int span = (int)h->c.inv.tiles;
    const int nb = std::max(1, std::min({(span + SEL_W - 1) / SEL_W, 2 * h->c.num_cu, MERGE_LISTS_MAX}));
    sp.tiles_total = span;
    const int groups = (int)((m + 15) / 16);
    // results per pass: 32, or what the wave lists' LDS holds beside long query rows
    const long long lds_left = (long long)LDS_LIMIT - (long long)range_lds_bytes(sp.qs_stride);
    const int kp = (int)std::min<long long>(std::min(k, SEL_KPASS_MAX), lds_left / (SEL_W * 16 * 8));
    if (kp < 1) return ise_fail_(ISE_E_INVALID, "rows too long for the inverted-list search");
    const hipEvent_t busy = h->c.order.busy();
    int rc = grow_after_event(h->q, (size_t)m * h->dp, busy);
    if (!rc) rc = grow_after_event(h->part, (size_t)groups * nb * 16 * kp, busy);
    if (!rc) rc = grow_after_event(h->masks, (size_t)groups * h->c.inv.nlist, busy);
    if (!rc && k > kp) rc = grow_after_event(h->keys, (size_t)m * kp + (size_t)m, busy);
    if (rc) return rc;
    const long long qtot = m * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((qtot + 255) / 256)), dim3(256), 0, st, q_dev, h->d, h->dp, qtot,
                       h->q.p);
    HIP_TRY(hipMemsetAsync(h->masks.p, 0, (size_t)groups * h->c.inv.nlist * sizeof(uint32_t), st));
    const long long ptot = m * nprobe;
    hipLaunchKernelGGL(ivf_mask_kernel, dim3((unsigned)((ptot + 255) / 256)), dim3(256), 0, st, probes_dev, ptot, nprobe, h->c.inv.nlist,
                       4, h->masks.p);
    sp.q = h->q.p;
    sp.masks = h->masks.p;
    sp.part = h->part.p;
    sp.kpass = kp;
    MergeParams mp{};
    mp.lists = h->part.p; mp.qt = 16; mp.n_lists = nb; mp.nq = (int)m; mp.k = kp; mp.metric = h->metric;
    mp.stride_list = 16ll * kp; mp.stride_qtile = (long long)nb * 16 * kp;
    const ExactParams xp{};
    const dim3 grid((unsigned)nb, (unsigned)groups);
    const size_t lds = sel_lds_bytes(sp.qs_stride, kp);
    auto scan = [&]() {
        if (l2) launch_ivf_v<true>(ch, grid, lds, st, sp);
        else launch_ivf_v<false>(ch, grid, lds, st, sp);
        h->c.passes++;
    };
    if (k <= kp) {
        sp.floor_keys = nullptr;
        scan();
        mp.D = D_dev; mp.I = I_dev;
        hipLaunchKernelGGL((merge_kernel<false>), dim3((unsigned)m), dim3(MERGE_THREADS), 0, st, mp, xp);
    } else {
        u64* pass_keys = h->keys.p;
        u64* floors = pass_keys + (size_t)m * kp;
        for (int off = 0; off < k; off += kp) {
            sp.floor_keys = off ? floors : nullptr;
            scan();
            mp.keys_out = pass_keys;
            hipLaunchKernelGGL((merge_kernel<false>), dim3((unsigned)m), dim3(MERGE_THREADS), 0, st, mp, xp);
            const long long tot = m * kp;
            hipLaunchKernelGGL(sel_scatter_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const u64*)pass_keys,
                               (int)m, kp, off, k, h->metric, D_dev, I_dev, floors);
        }
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// mu_ held.  Enqueues only, unless rows are pending (the rebuild blocks)
static int ivf_search_enqueue(ise_ivf* h, const float* q_dev, long long nq, int k, const long long* probes_dev, int nprobe,
                              float* D_dev, long long* I_dev, hipStream_t st) {
    h->c.batches++;
    // a search still in flight on another stream comes first on the device: before the rebuild and before the
    // workspaces are written.  (The host waits only where a buffer is replaced: grow_after_event, the rebuild.)
    int rc = h->c.order.wait(st);
    if (rc) return rc;
    if ((rc = ivf_rebuild_with_norms(h, st))) return rc;
    if (h->c.inv.tiles == 0) {  // an empty index: padding, no pass
        knn_fill_launch(D_dev, I_dev, nq * k, h->metric != ISE_METRIC_L2, st);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    CallOrder::Scope release{h->c.order, st};
    for (long long i0 = 0; i0 < nq; i0 += IVF_NQ_CHUNK) {
        const long long m = std::min<long long>(IVF_NQ_CHUNK, nq - i0);
        rc = ivf_chunk_enqueue(h, q_dev + (size_t)i0 * h->d, m, k, probes_dev + (size_t)i0 * nprobe, nprobe,
                               D_dev + (size_t)i0 * k, I_dev + (size_t)i0 * k, st);
        if (rc) return rc;
    }
    return ISE_OK;
}

static int ivf_check_search_args(const ise_ivf* h, const void* q, long long nq, int k, const void* probes, int nprobe,
                                 const void* D, const void* I) {
    const int rc = check_ivf_knn_args(q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    return ISE_OK;
}

extern "C" int ise_ivf_search_device(ise_ivf_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                                     float* D_dev, int64_t* I_dev, void* stream) {
    int rc = ivf_check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    IvfEntry en(h->c);
    if ((rc = en.check())) return rc;
    return ivf_search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_ivf_search_host(ise_ivf_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                                   int64_t* I) {
    int rc = ivf_check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    IvfEntry en(h->c);
    if ((rc = en.check())) return rc;
    return ivf_search_staged(h->d, h->c.stream, q, nq, k, probes, nprobe, D, I,
                             [&](const float* q_dev, long long m, const long long* p_dev, float* D_dev, long long* I_dev) {
                                 return ivf_search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->c.stream);
                             });
}

extern "C" int ise_ivf_stats(ise_ivf_t* h, uint64_t* out3) {
    if (!h || !out3) return ise_fail_(ISE_E_INVALID, "NULL argument");
    IvfEntry en(h->c);
    const int rc = en.check();
    return rc ? rc : h->c.stats(out3);
}
