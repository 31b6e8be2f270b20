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
#include "ise_pass_host.hpp"

#define IVF_NQ_CHUNK 64 /* queries per launch (4 groups of 16): bounds the per-block lists */

struct ise_ivf {
    int d = 0, dp = 0, metric = ISE_METRIC_L2, device = 0, num_cu = 256;
    IvfLists inv;  // the lists' counts, ids and table; the sorted array has [inv.tiles * 16] slots
    float* xb = nullptr;
    float* norms = nullptr;
    float* mu = nullptr;       // [dp]
    // rows added since the last rebuild, in insertion order (inv.pend_n of them)
    float* pend = nullptr;  // [pend_cap][dp]
    long long pend_cap = 0;
    // one set of search workspaces: *_device calls on different streams are ordered one behind the other
    DevBuf<float> q;         // [chunk][dp] padded queries
    DevBuf<u64> part;        // [groups][blocks][16][kpass]
    DevBuf<u64> keys;        // [chunk][32] one pass's merged keys (k > 32) | [chunk] floors
    DevBuf<uint32_t> masks;  // [groups][nlist]
    CallOrder order;
    unsigned long long* stats_dev = nullptr;  // [1] tiles loaded
    unsigned long long batches = 0, passes = 0;
    hipStream_t stream = nullptr;  // add / rebuild from the host entry points / list_host
    std::mutex mu_;
};

static void ivf_free_rows(ise_ivf* h) {
    for (void* p : {(void*)h->xb, (void*)h->norms, (void*)h->pend})
        if (p) (void)hipFree(p);
    h->xb = nullptr; h->norms = nullptr; h->pend = nullptr;
    h->pend_cap = 0;
    h->inv.free_rows();
}

extern "C" int ise_ivf_create(ise_ivf_t** out, int d, int metric, int nlist, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (nlist <= 0) return ise_fail_(ISE_E_INVALID, "nlist must be positive");
    if (metric != ISE_METRIC_L2 && metric != ISE_METRIC_INNER_PRODUCT)
        return ise_fail_(ISE_E_INVALID, "metric must be ISE_METRIC_L2 or ISE_METRIC_INNER_PRODUCT");
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_ivf* h = new (std::nothrow) ise_ivf();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d = d;
    h->dp = pad_dim(d, ISE_STORE_F32);
    h->metric = metric;
    h->device = device;
    h->num_cu = num_cu;
    h->inv.nlist = nlist;
    h->inv.clear();
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->order.create();
    if (e == hipSuccess) e = hipMalloc((void**)&h->mu, (size_t)h->dp * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->mu, 0, (size_t)h->dp * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->stats_dev, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->stats_dev, 0, sizeof(unsigned long long));
    if (e != hipSuccess) {
        if (h->stream) (void)hipStreamDestroy(h->stream);
        h->order.destroy();
        if (h->mu) (void)hipFree(h->mu);
        if (h->stats_dev) (void)hipFree(h->stats_dev);
        delete h;
        return ise_fail_(ISE_E_HIP, std::string("inverted-list index setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_ivf_destroy(ise_ivf_t* h) {
    if (!h) return ISE_OK;
    {
        DeviceGuard gd(h->device);
        (void)hipDeviceSynchronize();
        ivf_free_rows(h);
        for (void* p : {(void*)h->q.p, (void*)h->part.p, (void*)h->keys.p, (void*)h->masks.p, (void*)h->mu, (void*)h->stats_dev})
            if (p) (void)hipFree(p);
        h->order.destroy();
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_ivf_reset(ise_ivf_t* h) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());
    ivf_free_rows(h);
    return ISE_OK;
}

extern "C" int ise_ivf_info(const ise_ivf_t* h, int* d, int* metric, int* nlist, int64_t* ntotal, int* device) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (d) *d = h->d;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->inv.nlist;
    if (ntotal) *ntotal = h->inv.n;
    if (device) *device = h->device;
    return ISE_OK;
}

// ---------------------------------------------------------------- add
// room for n more pending rows (mu_ held): the buffer at least doubles, so it is never more than twice its rows
static int ivf_reserve_pending(ise_ivf* h, long long n, hipStream_t st) {
    const long long need = h->inv.pend_n + n;
    if (need <= h->pend_cap) return ISE_OK;
    const long long cap = std::max(need, 2 * h->pend_cap);
    float* nx = nullptr;
    HIP_TRY(hipMalloc((void**)&nx, (size_t)cap * h->dp * sizeof(float)));
    if (h->inv.pend_n > 0) {
        hipError_t e = hipMemcpyAsync(nx, h->pend, (size_t)h->inv.pend_n * h->dp * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(nx);
            return ise_fail_(ISE_E_HIP, std::string("growing the pending rows: ") + hipGetErrorString(e));
        }
    }
    if (h->pend) (void)hipFree(h->pend);
    h->pend = nx;
    h->pend_cap = cap;
    return ISE_OK;
}

extern "C" int ise_ivf_add_host(ise_ivf_t* h, const float* x, const int64_t* list_no, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !list_no)) return ise_fail_(ISE_E_INVALID, "rows or list numbers pointer is NULL");
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (n == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    int rc = h->inv.check_lists(list_no, n);
    if (rc) return rc;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    rc = ivf_reserve_pending(h, n, h->stream);
    if (rc) return rc;
    float* dst = h->pend + (size_t)h->inv.pend_n * h->dp;
    if (h->dp != h->d) HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * h->dp * sizeof(float), h->stream));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->dp * sizeof(float), x, (size_t)h->d * sizeof(float), (size_t)h->d * sizeof(float),
                             (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->inv.add(list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivf_add_device(ise_ivf_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x_dev || !list_no_dev)) return ise_fail_(ISE_E_INVALID, "rows or list numbers pointer is NULL");
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (n == 0) return ISE_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::vector<int64_t> lists((size_t)n);
    HIP_TRY(hipMemcpyAsync(lists.data(), list_no_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int rc = h->inv.check_lists(lists.data(), n);
    if (rc) return rc;
    rc = ivf_reserve_pending(h, n, st);
    if (rc) return rc;
    const long long tot = (long long)n * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x_dev, h->d, h->dp, tot,
                       h->pend + (size_t)h->inv.pend_n * h->dp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    h->inv.add(lists.data(), n);
    return ISE_OK;
}

// ---------------------------------------------------------------- rebuild
// the pending rows into the lists (mu_ held).  Blocks: the host's tables are copied from pageable memory and the old
// array is freed behind the kernels.  Nothing changes if an allocation fails
static int ivf_rebuild_locked(ise_ivf* h, hipStream_t st) {
    IvfLists& inv = h->inv;
    if (inv.pend_n == 0) return ISE_OK;
    IvfPlan pl;
    if (!inv.plan(&pl, 16)) return ise_fail_(ISE_E_INVALID, "the lists' 16-row tiles no longer fit 32-bit slot numbers");
    const size_t slots = (size_t)pl.tile0[(size_t)inv.nlist] * 16;
    const int groups = (int)std::min<long long>(1024, std::max<long long>(1, (long long)slots / 256));
    float *nx = nullptr, *nn = nullptr, *partial = nullptr, *nmu = nullptr;
    uint32_t *nids = nullptr, *nmeta = nullptr, *dest = nullptr;
    DevFreeList<7> fr{{(void**)&nx, (void**)&nn, (void**)&partial, (void**)&nids, (void**)&nmeta, (void**)&dest, (void**)&nmu}};
    std::vector<uint32_t> meta_host;
    HIP_TRY(hipMalloc((void**)&nx, slots * h->dp * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&nn, slots * sizeof(float)));
    int rc = inv.begin_rebuild(pl, 16, st, meta_host, &nids, &nmeta, &dest);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(nx, 0, slots * h->dp * sizeof(float), st));   // pad slots read as zero rows
    HIP_TRY(hipMemsetAsync(nids, 0xFF, slots * sizeof(uint32_t), st));
    if (inv.tiles > 0)
        hipLaunchKernelGGL(ivf_move_tiles_kernel, dim3((unsigned)inv.tiles), dim3(256), 0, st, (const float*)h->xb,
                           (const uint32_t*)inv.ids, inv.tile_list_dev(), inv.list_tile0_dev(), (const uint32_t*)nmeta, h->dp, nx, nids);
    hipLaunchKernelGGL(ivf_scatter_rows_kernel, dim3((unsigned)((inv.pend_n + 3) / 4)), dim3(256), 0, st, (const float*)h->pend,
                       inv.pend_n, (const uint32_t*)dest, (uint32_t)(inv.n - inv.pend_n), h->dp, nx, nids);
    if (h->metric == ISE_METRIC_L2) {
        // the shift vector: the column mean of the rows as they stand (it decides how tight the bounds are, nothing else)
        // into a buffer of its own, swapped in with the rows: a pass still in flight keeps the mu its norms belong to
        HIP_TRY(hipMalloc((void**)&nmu, (size_t)h->dp * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&partial, (size_t)groups * h->dp * sizeof(float)));
        const unsigned gx = (unsigned)((h->dp + 255) / 256);
        hipLaunchKernelGGL(ivf_col_sum_kernel, dim3(gx, (unsigned)groups), dim3(256), 0, st, (const float*)nx, (long long)slots,
                           h->d, h->dp, groups, partial);
        hipLaunchKernelGGL(ivf_col_mean_kernel, dim3(gx), dim3(256), 0, st, (const float*)partial, inv.n, h->d, h->dp, groups,
                           nmu);
        hipLaunchKernelGGL(ivf_norms_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, st, (const float*)nx, (long long)slots,
                           h->dp, (const float*)nmu, nn);
    } else {
        HIP_TRY(hipMemsetAsync(nn, 0, slots * sizeof(float), st));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::swap(h->xb, nx);  // the old arrays go with the guard (hipFree waits for the passes that still read them)
    if (nmu) std::swap(h->mu, nmu);
    std::swap(h->norms, nn);
    inv.finish_rebuild(pl, &nids, &nmeta);
    if (h->pend) (void)hipFree(h->pend);
    h->pend = nullptr;
    h->pend_cap = 0;
    return ISE_OK;
}

extern "C" int ise_ivf_list_sizes_host(ise_ivf_t* h, int64_t* sizes) {
    if (!h || !sizes) return ise_fail_(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu_);
    h->inv.list_sizes_host(sizes);
    return ISE_OK;
}

extern "C" int ise_ivf_list_host(ise_ivf_t* h, int list, int64_t* ids, float* rows) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (list < 0 || list >= h->inv.nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = ivf_rebuild_locked(h, h->stream);
    if (rc) return rc;
    size_t m = 0, slot0 = 0;
    if ((rc = h->inv.list_ids_host(list, 16, ids, &m, &slot0))) return rc;
    if (m == 0) return ISE_OK;
    if (rows)
        HIP_TRY(hipMemcpy2D(rows, (size_t)h->d * sizeof(float), h->xb + slot0 * h->dp, (size_t)h->dp * sizeof(float),
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
    sp.xb = h->xb; sp.norms = h->norms; sp.mu = h->mu; sp.ids = h->inv.ids;
    sp.list_tile0 = h->inv.list_tile0_dev(); sp.list_size = h->inv.list_size_dev(); sp.tile_list = h->inv.tile_list_dev();
    sp.nlist = h->inv.nlist; sp.d = h->d; sp.dp = h->dp;
    sp.qs_stride = qs_stride_units(h->dp);
    sp.row_slots = h->dp / 4;
    sp.nq = (int)m; sp.metric = h->metric;
    sp.beta = l2 ? exact_beta_dp(h->dp) : 0.f;
    range_staging_rule(SEL_W, false, h->d, sp.qs_stride, &sp.tpr, &sp.vec_q);  // the pass's own 8 waves stage the queries
    sp.tiles_loaded = h->stats_dev;
    const int ch = std::min(chunk_steps_rb((size_t)h->dp * sizeof(float)), 4);
    // at least a tile per wave, at most two blocks per CU (what their LDS lets a CU hold) and the merge's list count
    const int span = (int)h->inv.tiles;
    const int nb = std::max(1, std::min({(span + SEL_W - 1) / SEL_W, 2 * h->num_cu, MERGE_LISTS_MAX}));
    sp.tiles_total = span;
    const int groups = (int)((m + 15) / 16);
    // results per pass: 32, or what the wave lists' LDS holds beside long query rows
    const long long lds_left = (long long)LDS_LIMIT - (long long)range_lds_bytes(sp.qs_stride);
    const int kp = (int)std::min<long long>(std::min(k, SEL_KPASS_MAX), lds_left / (SEL_W * 16 * 8));
    if (kp < 1) return ise_fail_(ISE_E_INVALID, "rows too long for the inverted-list search");
    const hipEvent_t busy = h->order.busy();
    int rc = grow_after_event(h->q, (size_t)m * h->dp, busy);
    if (!rc) rc = grow_after_event(h->part, (size_t)groups * nb * 16 * kp, busy);
    if (!rc) rc = grow_after_event(h->masks, (size_t)groups * h->inv.nlist, busy);
    if (!rc && k > kp) rc = grow_after_event(h->keys, (size_t)m * kp + (size_t)m, busy);
    if (rc) return rc;
    const long long qtot = m * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((qtot + 255) / 256)), dim3(256), 0, st, q_dev, h->d, h->dp, qtot,
                       h->q.p);
    HIP_TRY(hipMemsetAsync(h->masks.p, 0, (size_t)groups * h->inv.nlist * sizeof(uint32_t), st));
    const long long ptot = m * nprobe;
    hipLaunchKernelGGL(ivf_mask_kernel, dim3((unsigned)((ptot + 255) / 256)), dim3(256), 0, st, probes_dev, ptot, nprobe, h->inv.nlist,
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
        h->passes++;
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
    h->batches++;
    // a search still in flight on another stream comes first on the device: before the rebuild and before the
    // workspaces are written.  (The host waits only where a buffer is replaced: grow_after_event, ivf_rebuild_locked.)
    int rc = h->order.wait(st);
    if (rc) return rc;
    if ((rc = ivf_rebuild_locked(h, st))) return rc;
    if (h->inv.tiles == 0) {  // an empty index: padding, no pass
        knn_fill_launch(D_dev, I_dev, nq * k, h->metric != ISE_METRIC_L2, st);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    CallOrder::Scope release{h->order, st};
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
    const int rc = ivf_check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return ivf_search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_ivf_search_host(ise_ivf_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                                   int64_t* I) {
    int rc = ivf_check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return ivf_search_staged(h->d, h->stream, q, nq, k, probes, nprobe, D, I,
                             [&](const float* q_dev, long long m, const long long* p_dev, float* D_dev, long long* I_dev) {
                                 return ivf_search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, h->stream);
                             });
}

extern "C" int ise_ivf_stats(ise_ivf_t* h, uint64_t* out3) {
    if (!h || !out3) return ise_fail_(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    unsigned long long loaded = 0;
    HIP_TRY(hipDeviceSynchronize());  // the passes enqueued so far have added their tiles
    HIP_TRY(hipMemcpy(&loaded, h->stats_dev, sizeof(loaded), hipMemcpyDeviceToHost));
    out3[0] = h->batches;
    out3[1] = h->passes;
    out3[2] = loaded;
    return ISE_OK;
}
