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
// buffer (at most twice the pending rows).
#include "ise_host.hpp"
#include "ise_geometry.hpp"
#include "ise_scan_params.hpp"
#include "ise_ivf.hpp"
#include "ise_ivf_plan.hpp"

#define IVF_NQ_CHUNK 64 /* queries per launch (4 groups of 16): bounds the per-block lists */

namespace {

// busy: the event behind the last pass that used the workspaces, or null -- waited for only when the buffer really has
// to be replaced (then the call blocks)
// rule: a free waits for that one event only -- every pass that used the workspaces is ordered before it
template <class T>
int grow(DevBuf<T>& b, size_t need, hipEvent_t busy) {
    if (need <= b.n) return ISE_OK;
    if (b.p && busy) HIP_TRY(hipEventSynchronize(busy));
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
    HIP_TRY(hipMalloc((void**)&b.p, need * sizeof(T)));
    b.n = need;
    return ISE_OK;
}

}  // namespace

struct ise_ivf {
    int d = 0, dp = 0, metric = ISE_METRIC_L2, nlist = 0, device = 0, num_cu = 256;
    long long n = 0;  // rows in all, the pending ones included
    // the sorted array: [tiles * 16] slots
    float* xb = nullptr;
    uint32_t* ids = nullptr;
    float* norms = nullptr;
    uint32_t* meta = nullptr;  // list_tile0 [nlist + 1] | list_size [nlist] | tile_list [tiles]
    long long tiles = 0;
    float* mu = nullptr;       // [dp]
    std::vector<long long> size;      // [nlist] rows per list in the sorted array
    std::vector<long long> size_all;  // ... with the pending rows
    std::vector<uint32_t> tile0;      // [nlist + 1] host copy
    // rows added since the last rebuild, in insertion order
    float* pend = nullptr;  // [pend_cap][dp]
    long long pend_n = 0, pend_cap = 0;
    std::vector<int32_t> pend_list;
    // one set of search workspaces: *_device calls on different streams are ordered one behind the other
    DevBuf<float> q;         // [chunk][dp] padded queries
    DevBuf<u64> part;        // [groups][blocks][16][kpass]
    DevBuf<u64> keys;        // [chunk][32] one pass's merged keys (k > 32) | [chunk] floors
    DevBuf<uint32_t> masks;  // [groups][nlist]
    hipEvent_t done = nullptr;
    bool used = false;
    hipStream_t last_stream = nullptr;
    unsigned long long* stats_dev = nullptr;  // [1] tiles loaded
    unsigned long long batches = 0, passes = 0;
    hipStream_t stream = nullptr;  // add / rebuild from the host entry points / list_host
    std::mutex mu_;

    const uint32_t* list_tile0_dev() const { return meta; }
    const uint32_t* list_size_dev() const { return meta + nlist + 1; }
    const uint32_t* tile_list_dev() const { return meta + 2 * (size_t)nlist + 1; }
};

static void ivf_free_rows(ise_ivf* h) {
    for (void* p : {(void*)h->xb, (void*)h->ids, (void*)h->norms, (void*)h->meta, (void*)h->pend})
        if (p) (void)hipFree(p);
    h->xb = nullptr; h->ids = nullptr; h->norms = nullptr; h->meta = nullptr; h->pend = nullptr;
    h->tiles = 0;
    h->n = 0;
    h->pend_n = h->pend_cap = 0;
    h->pend_list.clear();
    h->size.assign((size_t)h->nlist, 0);
    h->size_all.assign((size_t)h->nlist, 0);
    h->tile0.assign((size_t)h->nlist + 1, 0u);
}

extern "C" int ise_ivf_create(ise_ivf_t** out, int d, int metric, int nlist, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d <= 0) return ise_fail_(ISE_E_INVALID, "d must be positive");
    if (nlist <= 0) return ise_fail_(ISE_E_INVALID, "nlist must be positive");
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
    ise_ivf* h = new (std::nothrow) ise_ivf();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d = d;
    h->dp = pad_dim(d, ISE_STORE_F32);
    h->metric = metric;
    h->nlist = nlist;
    h->device = device;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->size.assign((size_t)nlist, 0);
    h->size_all.assign((size_t)nlist, 0);
    h->tile0.assign((size_t)nlist + 1, 0u);
    DeviceGuard gd(device);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&h->mu, (size_t)h->dp * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->mu, 0, (size_t)h->dp * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->stats_dev, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->stats_dev, 0, sizeof(unsigned long long));
    if (e != hipSuccess) {
        if (h->stream) (void)hipStreamDestroy(h->stream);
        if (h->done) (void)hipEventDestroy(h->done);
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
        if (h->done) (void)hipEventDestroy(h->done);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_ivf_reset(ise_ivf_t* h) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    HIP_TRY(hipDeviceSynchronize());
    ivf_free_rows(h);
    return ISE_OK;
}

extern "C" int ise_ivf_info(const ise_ivf_t* h, int* d, int* metric, int* nlist, int64_t* ntotal, int* device) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (d) *d = h->d;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->nlist;
    if (ntotal) *ntotal = h->n;
    if (device) *device = h->device;
    return ISE_OK;
}

// ---------------------------------------------------------------- add
// room for n more pending rows (mu_ held): the buffer at least doubles, so it is never more than twice its rows
static int ivf_reserve_pending(ise_ivf* h, long long n, hipStream_t st) {
    const long long need = h->pend_n + n;
    if (need <= h->pend_cap) return ISE_OK;
    const long long cap = std::max(need, 2 * h->pend_cap);
    float* nx = nullptr;
    HIP_TRY(hipMalloc((void**)&nx, (size_t)cap * h->dp * sizeof(float)));
    if (h->pend_n > 0) {
        hipError_t e = hipMemcpyAsync(nx, h->pend, (size_t)h->pend_n * h->dp * sizeof(float), hipMemcpyDeviceToDevice, st);
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

// list numbers on the host, checked before anything changes
static int ivf_check_lists(const ise_ivf* h, const int64_t* list_no, long long n) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "an inverted-list index holds fewer than 2^32 rows");
    for (long long i = 0; i < n; i++)
        if (list_no[i] < 0 || list_no[i] >= h->nlist)
            return ise_fail_(ISE_E_INVALID, "list number " + std::to_string((long long)list_no[i]) + " of row " + std::to_string(i) +
                                                " is outside [0, nlist = " + std::to_string(h->nlist) + "): nothing was added");
    return ISE_OK;
}

// the rows are in the pending buffer: book them (mu_ held)
static void ivf_commit_add(ise_ivf* h, const int64_t* list_no, long long n) {
    h->pend_list.reserve(h->pend_list.size() + (size_t)n);
    for (long long i = 0; i < n; i++) {
        h->pend_list.push_back((int32_t)list_no[i]);
        h->size_all[(size_t)list_no[i]]++;
    }
    h->pend_n += n;
    h->n += n;
}

extern "C" int ise_ivf_add_host(ise_ivf_t* h, const float* x, const int64_t* list_no, int64_t n) {
    if (n < 0) return ise_fail_(ISE_E_INVALID, "n must be >= 0");
    if (n > 0 && (!x || !list_no)) return ise_fail_(ISE_E_INVALID, "rows or list numbers pointer is NULL");
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (n == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    int rc = ivf_check_lists(h, list_no, n);
    if (rc) return rc;
    DeviceGuard gd(h->device);
    rc = ivf_reserve_pending(h, n, h->stream);
    if (rc) return rc;
    float* dst = h->pend + (size_t)h->pend_n * h->dp;
    if (h->dp != h->d) HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * h->dp * sizeof(float), h->stream));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->dp * sizeof(float), x, (size_t)h->d * sizeof(float), (size_t)h->d * sizeof(float),
                             (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ivf_commit_add(h, list_no, n);
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
    std::vector<int64_t> lists((size_t)n);
    HIP_TRY(hipMemcpyAsync(lists.data(), list_no_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int rc = ivf_check_lists(h, lists.data(), n);
    if (rc) return rc;
    rc = ivf_reserve_pending(h, n, st);
    if (rc) return rc;
    const long long tot = (long long)n * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x_dev, h->d, h->dp, tot,
                       h->pend + (size_t)h->pend_n * h->dp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    ivf_commit_add(h, lists.data(), n);
    return ISE_OK;
}

// ---------------------------------------------------------------- rebuild
// the pending rows into the lists (mu_ held).  Blocks: the host's tables are copied from pageable memory and the old
// array is freed behind the kernels.  Nothing changes if an allocation fails
static int ivf_rebuild_locked(ise_ivf* h, hipStream_t st) {
    if (h->pend_n == 0) return ISE_OK;
    IvfPlan pl;
    if (!ivf_plan_rebuild(h->size, h->pend_list.data(), h->pend_n, &pl))
        return ise_fail_(ISE_E_INVALID, "the lists' 16-row tiles no longer fit 32-bit slot numbers");
    const size_t nlist = (size_t)h->nlist;
    const long long tiles = pl.tile0[nlist];
    const size_t slots = (size_t)tiles * 16;
    const int groups = (int)std::min<long long>(1024, std::max<long long>(1, (long long)slots / 256));
    float *nx = nullptr, *nn = nullptr, *partial = nullptr, *nmu = nullptr;
    uint32_t *nids = nullptr, *nmeta = nullptr, *dest = nullptr;
    struct Free {
        void** p[7];
        ~Free() {
            for (void** q : p)
                if (*q) (void)hipFree(*q);
        }
    } fr{{(void**)&nx, (void**)&nn, (void**)&partial, (void**)&nids, (void**)&nmeta, (void**)&dest, (void**)&nmu}};
    const size_t nmeta_n = 2 * nlist + 1 + (size_t)tiles;
    HIP_TRY(hipMalloc((void**)&nx, slots * h->dp * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&nn, slots * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&nids, slots * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&nmeta, nmeta_n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&dest, (size_t)h->pend_n * sizeof(uint32_t)));
    std::vector<uint32_t> meta_host(nmeta_n);
    std::copy(pl.tile0.begin(), pl.tile0.end(), meta_host.begin());
    for (size_t l = 0; l < nlist; l++) meta_host[nlist + 1 + l] = (uint32_t)pl.size[l];
    std::copy(pl.tile_list.begin(), pl.tile_list.end(), meta_host.begin() + 2 * nlist + 1);
    HIP_TRY(hipMemcpyAsync(nmeta, meta_host.data(), nmeta_n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dest, pl.dest.data(), (size_t)h->pend_n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(nx, 0, slots * h->dp * sizeof(float), st));   // pad slots read as zero rows
    HIP_TRY(hipMemsetAsync(nids, 0xFF, slots * sizeof(uint32_t), st));
    if (h->tiles > 0)
        hipLaunchKernelGGL(ivf_move_tiles_kernel, dim3((unsigned)h->tiles), dim3(256), 0, st, (const float*)h->xb,
                           (const uint32_t*)h->ids, h->tile_list_dev(), h->list_tile0_dev(), (const uint32_t*)nmeta, h->dp, nx, nids);
    hipLaunchKernelGGL(ivf_scatter_rows_kernel, dim3((unsigned)((h->pend_n + 3) / 4)), dim3(256), 0, st, (const float*)h->pend,
                       h->pend_n, (const uint32_t*)dest, (uint32_t)(h->n - h->pend_n), h->dp, nx, nids);
    if (h->metric == ISE_METRIC_L2) {
        // the shift vector: the column mean of the rows as they stand (it decides how tight the bounds are, nothing else)
        // into a buffer of its own, swapped in with the rows: a pass still in flight keeps the mu its norms belong to
        HIP_TRY(hipMalloc((void**)&nmu, (size_t)h->dp * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&partial, (size_t)groups * h->dp * sizeof(float)));
        const unsigned gx = (unsigned)((h->dp + 255) / 256);
        hipLaunchKernelGGL(ivf_col_sum_kernel, dim3(gx, (unsigned)groups), dim3(256), 0, st, (const float*)nx, (long long)slots,
                           h->d, h->dp, groups, partial);
        hipLaunchKernelGGL(ivf_col_mean_kernel, dim3(gx), dim3(256), 0, st, (const float*)partial, h->n, h->d, h->dp, groups,
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
    std::swap(h->ids, nids);
    std::swap(h->meta, nmeta);
    if (h->pend) (void)hipFree(h->pend);
    h->pend = nullptr;
    h->pend_n = h->pend_cap = 0;
    h->pend_list.clear();
    h->pend_list.shrink_to_fit();
    h->tiles = tiles;
    h->size = pl.size;
    h->tile0 = pl.tile0;
    return ISE_OK;
}

extern "C" int ise_ivf_list_sizes_host(ise_ivf_t* h, int64_t* sizes) {
    if (!h || !sizes) return ise_fail_(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu_);
    for (int l = 0; l < h->nlist; l++) sizes[l] = h->size_all[(size_t)l];
    return ISE_OK;
}

extern "C" int ise_ivf_list_host(ise_ivf_t* h, int list, int64_t* ids, float* rows) {
    if (!h) return ise_fail_(ISE_E_INVALID, "handle is NULL");
    if (list < 0 || list >= h->nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    int rc = ivf_rebuild_locked(h, h->stream);
    if (rc) return rc;
    const size_t m = (size_t)h->size[(size_t)list];
    if (m == 0) return ISE_OK;
    const size_t slot0 = (size_t)h->tile0[(size_t)list] * 16;
    if (ids) {
        std::vector<uint32_t> tmp(m);
        HIP_TRY(hipMemcpy(tmp.data(), h->ids + slot0, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++) ids[i] = (int64_t)tmp[i];
    }
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
    sp.xb = h->xb; sp.norms = h->norms; sp.mu = h->mu; sp.ids = h->ids;
    sp.list_tile0 = h->list_tile0_dev(); sp.list_size = h->list_size_dev(); sp.tile_list = h->tile_list_dev();
    sp.nlist = h->nlist; sp.d = h->d; sp.dp = h->dp;
    sp.qs_stride = qs_stride_units(h->dp);
    sp.row_slots = h->dp / 4;
    sp.nq = (int)m; sp.metric = h->metric;
    sp.beta = l2 ? exact_beta_dp(h->dp) : 0.f;
    range_staging_rule(SEL_W, false, h->d, sp.qs_stride, &sp.tpr, &sp.vec_q);  // the pass's own 8 waves stage the queries
    sp.tiles_loaded = h->stats_dev;
    const int ch = std::min(chunk_steps_rb((size_t)h->dp * sizeof(float)), 4);
    // at least a tile per wave, at most two blocks per CU (what their LDS lets a CU hold) and the merge's list count
    const int span = (int)h->tiles;
    const int nb = std::max(1, std::min({(span + SEL_W - 1) / SEL_W, 2 * h->num_cu, MERGE_LISTS_MAX}));
    sp.tiles_total = span;
    const int groups = (int)((m + 15) / 16);
    // results per pass: 32, or what the wave lists' LDS holds beside long query rows
    const long long lds_left = (long long)LDS_LIMIT - (long long)range_lds_bytes(sp.qs_stride);
    const int kp = (int)std::min<long long>(std::min(k, SEL_KPASS_MAX), lds_left / (SEL_W * 16 * 8));
    if (kp < 1) return ise_fail_(ISE_E_INVALID, "rows too long for the inverted-list search");
    const hipEvent_t busy = h->used ? h->done : nullptr;
    int rc = grow(h->q, (size_t)m * h->dp, busy);
    if (!rc) rc = grow(h->part, (size_t)groups * nb * 16 * kp, busy);
    if (!rc) rc = grow(h->masks, (size_t)groups * h->nlist, busy);
    if (!rc && k > kp) rc = grow(h->keys, (size_t)m * kp + (size_t)m, busy);
    if (rc) return rc;
    const long long qtot = m * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((qtot + 255) / 256)), dim3(256), 0, st, q_dev, h->d, h->dp, qtot,
                       h->q.p);
    HIP_TRY(hipMemsetAsync(h->masks.p, 0, (size_t)groups * h->nlist * sizeof(uint32_t), st));
    const long long ptot = m * nprobe;
    hipLaunchKernelGGL(ivf_mask_kernel, dim3((unsigned)((ptot + 255) / 256)), dim3(256), 0, st, probes_dev, ptot, nprobe, h->nlist,
                       h->masks.p);
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
    // workspaces are written.  (The host waits only where a buffer is replaced: grow, ivf_rebuild_locked.)
    if (h->used && h->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
    int rc = ivf_rebuild_locked(h, st);
    if (rc) return rc;
    if (h->tiles == 0) {  // an empty index: padding, no pass
        const long long tot = nq * k;
        hipLaunchKernelGGL(sel_fill_pad_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, D_dev, I_dev, tot, h->metric);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    struct Release {  // whatever path returns, a later user on another stream waits for this call
        ise_ivf* h;
        hipStream_t st;
        ~Release() {
            if (hipEventRecord(h->done, st) == hipSuccess) { h->used = true; h->last_stream = st; }
        }
    } release{h, st};
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
    if (nq < 0) return ise_fail_(ISE_E_INVALID, "nq must be >= 0");
    if (k < 1 || k > ISE_MAX_K) return ise_fail_(ISE_E_INVALID, "k must be in [1, ISE_MAX_K]");
    if (nprobe < 1) return ise_fail_(ISE_E_INVALID, "nprobe must be positive");
    if (nq > 0 && (!q || !probes)) return ise_fail_(ISE_E_INVALID, "query or probe pointer is NULL");
    if (nq > 0 && (!D || !I)) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    if (nq * (long long)k >= (1ll << 40)) return ise_fail_(ISE_E_INVALID, "nq * k is too large");
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
    return ivf_search_enqueue(h, q_dev, nq, k, (const long long*)probes_dev, nprobe, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_ivf_search_host(ise_ivf_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                                   int64_t* I) {
    int rc = ivf_check_search_args(h, q, nq, k, probes, nprobe, D, I);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    const long long batch = std::min<long long>(nq, 4096);
    float *q_dev = nullptr, *D_dev = nullptr;
    long long *p_dev = nullptr, *I_dev = nullptr;
    struct Free {
        void** p[4];
        ~Free() {
            for (void** x : p)
                if (*x) (void)hipFree(*x);
        }
    } fr{{(void**)&q_dev, (void**)&D_dev, (void**)&p_dev, (void**)&I_dev}};
    HIP_TRY(hipMalloc((void**)&q_dev, (size_t)batch * h->d * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&p_dev, (size_t)batch * nprobe * sizeof(long long)));
    HIP_TRY(hipMalloc((void**)&D_dev, (size_t)batch * k * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&I_dev, (size_t)batch * k * sizeof(long long)));
    hipStream_t st = h->stream;
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        HIP_TRY(hipMemcpyAsync(q_dev, q + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(p_dev, probes + (size_t)i0 * nprobe, (size_t)m * nprobe * sizeof(long long), hipMemcpyHostToDevice,
                               st));
        rc = ivf_search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, st);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(D + (size_t)i0 * k, D_dev, (size_t)m * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, I_dev, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_ivf_stats(ise_ivf_t* h, uint64_t* out3) {
    if (!h || !out3) return ise_fail_(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    unsigned long long loaded = 0;
    HIP_TRY(hipDeviceSynchronize());  // the passes enqueued so far have added their tiles
    HIP_TRY(hipMemcpy(&loaded, h->stats_dev, sizeof(loaded), hipMemcpyDeviceToHost));
    out3[0] = h->batches;
    out3[1] = h->passes;
    out3[2] = loaded;
    return ISE_OK;
}
