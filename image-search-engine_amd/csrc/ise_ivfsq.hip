// ise_ivfsq.hip -- host side and C ABI of the inverted-list index over 8-bit rows (include/ise_knn.h, ise_ivfsq_*;
// kernels in ise_ivfsq.hpp and ise_sq.hpp).  faiss.IndexIVFScalarQuantizer with by_residual = false.
//
// The codec is ise_sq.hip's: the trained state comes from the caller, rows are encoded on the device by
// sq_encode_kernel.  The lists are ise_ivf.hip's: rows come in with their list numbers (the coarse quantiser lives with
// the caller), add() encodes them at once into a PENDING buffer of codes and row terms and reads the encoder's
// non-finite flag back before anything is counted in; the first call that reads the lists afterwards (search,
// list_host) rebuilds: the host's counting sort (ise_ivf_plan.hpp, 64-row tiles) says where every pending row goes, the
// old tiles move to where their lists now start, the pending rows are scattered behind them.  Codes, row terms, ids and
// the tables go into fresh buffers that are swapped in together (a pass still in flight on another stream keeps a
// consistent set); the old ones and the pending buffer are freed when it is done.
//
// Calls on one handle run one at a time (a mutex).  The handle has ONE set of search workspaces: a search enqueued on
// another stream than the previous one waits for it through an event, and a workspace that has to grow waits for that
// event before the old buffer is freed.
#include <cmath>

#include "ise_host.hpp"
#include "ise_ivfsq.hpp"
#include "ise_ivf_plan.hpp"

namespace {
// busy: the event behind the last pass that used the workspaces, or null
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

struct ise_ivfsq {
    int d = 0, qtype = ISE_SQ_8BIT, stride = 0, qt = 0, qshift = 0, metric = ISE_METRIC_L2, nlist = 0, device = 0, num_cu = 256;
    bool trained = false;
    long long n = 0;  // rows in all, the pending ones included
    // the sorted array: [tiles * SQ_TILE] slots
    uint8_t* codes = nullptr;
    double* rterm = nullptr;
    uint32_t* ids = nullptr;
    uint32_t* meta = nullptr;  // list_tile0 [nlist + 1] | list_size [nlist] | tile_list [tiles]
    long long tiles = 0;
    std::vector<long long> size;      // [nlist] rows per list in the sorted array
    std::vector<long long> size_all;  // ... with the pending rows
    std::vector<uint32_t> tile0;      // [nlist + 1] host copy
    // rows added since the last rebuild, in insertion order
    uint8_t* pend = nullptr;        // [pend_cap][stride]
    double* pend_rterm = nullptr;   // [pend_cap]
    long long pend_n = 0, pend_cap = 0;
    std::vector<int32_t> pend_list;
    // the codec
    float* par = nullptr;  // [3][d]: vmin | s | o = vmin + s / 2
    std::vector<float> trained_host;
    unsigned int* bad = nullptr;  // [1] set by an encode that met a NaN or inf entry
    // host forms (they return with the stream drained): rows or queries as passed | codes as passed
    DevBuf<float> xraw;
    DevBuf<uint8_t> craw;
    // one set of search workspaces
    DevBuf<uint8_t> qrec;    // one chunk's staged queries
    DevBuf<u64> lo, lists;
    DevBuf<uint32_t> masks;  // [groups][nlist]
    DevBuf<uint32_t> offs;   // [groups][nlist] | count [groups]
    DevBuf<u32x4> work;      // [groups][tiles]
    hipEvent_t done = nullptr;
    bool used = false;
    hipStream_t last_stream = nullptr;
    unsigned long long* stats_dev = nullptr;  // [1] work-list entries (64-row tiles) the passes visited
    unsigned long long batches = 0, passes = 0;
    hipStream_t stream = nullptr;
    std::mutex mu_;

    const float* vmin() const { return par; }
    const float* step() const { return par + d; }
    const float* off() const { return par + 2 * (size_t)d; }
    const uint32_t* list_tile0_dev() const { return meta; }
    const uint32_t* list_size_dev() const { return meta + nlist + 1; }
    const uint32_t* tile_list_dev() const { return meta + 2 * (size_t)nlist + 1; }
};

namespace {
const char* const NONFINITE_MSG = "a row has a NaN or inf entry: nothing was encoded or added";

int check_handle(const ise_ivfsq* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "inverted-list scalar-quantiser index handle is NULL"); }
int check_trained(const ise_ivfsq* h) {
    return h->trained ? ISE_OK : ise_fail_(ISE_E_INVALID, "the index is not trained: set the trained state first");
}
bool uniform(const ise_ivfsq* h) { return h->qtype == ISE_SQ_8BIT_UNIFORM; }
size_t trained_count(const ise_ivfsq* h) { return uniform(h) ? 2 : 2 * (size_t)h->d; }

void free_rows(ise_ivfsq* h) {
    for (void* p : {(void*)h->codes, (void*)h->rterm, (void*)h->ids, (void*)h->meta, (void*)h->pend, (void*)h->pend_rterm})
        if (p) (void)hipFree(p);
    h->codes = nullptr; h->rterm = nullptr; h->ids = nullptr; h->meta = nullptr; h->pend = nullptr; h->pend_rterm = nullptr;
    h->tiles = 0;
    h->n = 0;
    h->pend_n = h->pend_cap = 0;
    h->pend_list.clear();
    h->size.assign((size_t)h->nlist, 0);
    h->size_all.assign((size_t)h->nlist, 0);
    h->tile0.assign((size_t)h->nlist + 1, 0u);
}

void free_all(ise_ivfsq* h) {
    free_rows(h);
    for (void* p : {(void*)h->par, (void*)h->bad, (void*)h->xraw.p, (void*)h->craw.p, (void*)h->qrec.p, (void*)h->lo.p, (void*)h->lists.p,
                    (void*)h->masks.p, (void*)h->offs.p, (void*)h->work.p, (void*)h->stats_dev})
        if (p) (void)hipFree(p);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

// rows of `step` at most so that one upload is 256 MiB at most
long long upload_step(size_t row_bytes) { return std::max<long long>(1, (1ll << 28) / (long long)row_bytes); }

// room for n more pending rows (mu_ held): the buffers at least double
int reserve_pending(ise_ivfsq* h, long long n, hipStream_t st) {
    const long long need = h->pend_n + n;
    if (need <= h->pend_cap) return ISE_OK;
    const long long cap = std::max(need, 2 * h->pend_cap);
    uint8_t* nx = nullptr;
    double* nr = nullptr;
    HIP_TRY(hipMalloc((void**)&nx, (size_t)cap * h->stride));
    hipError_t e = hipMalloc((void**)&nr, (size_t)cap * sizeof(double));
    if (e == hipSuccess && h->pend_n > 0) {
        e = hipMemcpyAsync(nx, h->pend, (size_t)h->pend_n * h->stride, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nr, h->pend_rterm, (size_t)h->pend_n * sizeof(double), hipMemcpyDeviceToDevice, st);
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

// list numbers on the host, checked before anything changes
int check_lists(const ise_ivfsq* h, const int64_t* list_no, long long n) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "an inverted-list index holds fewer than 2^32 rows");
    for (long long i = 0; i < n; i++)
        if (list_no[i] < 0 || list_no[i] >= h->nlist)
            return ise_fail_(ISE_E_INVALID, "list number " + std::to_string((long long)list_no[i]) + " of row " + std::to_string(i) +
                                                " is outside [0, nlist = " + std::to_string(h->nlist) + "): nothing was added");
    return ISE_OK;
}

// the rows' codes and row terms are in the pending buffer: book them (mu_ held)
void commit_add(ise_ivfsq* h, const int64_t* list_no, long long n) {
    h->pend_list.reserve(h->pend_list.size() + (size_t)n);
    for (long long i = 0; i < n; i++) {
        h->pend_list.push_back((int32_t)list_no[i]);
        h->size_all[(size_t)list_no[i]]++;
    }
    h->pend_n += n;
    h->n += n;
}

// pending rows [at, at + m) <- the codes and row terms of x_dev's rows (pad bytes zero); sets *h->bad on a non-finite entry
int encode_pending(ise_ivfsq* h, const float* x_dev, long long at, long long m, hipStream_t st) {
    uint8_t* dst = h->pend + (size_t)at * h->stride;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)m * h->stride, st));
    hipLaunchKernelGGL(sq_encode_kernel, dim3((unsigned)((m + SQ_ENC_ROWS - 1) / SQ_ENC_ROWS)), dim3(SQ_WAVES * 64), 0, st, x_dev, m,
                       h->d, h->vmin(), h->step(), dst, h->stride, h->pend_rterm + at, h->bad);
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// waits for st; ISE_E_INVALID when an encode since the flag was cleared met a non-finite entry
int bad_check(ise_ivfsq* h, hipStream_t st) {
    unsigned int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->bad, sizeof(flag), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return flag ? ise_fail_(ISE_E_INVALID, NONFINITE_MSG) : ISE_OK;
}

// the pending rows into the lists (mu_ held).  Blocks.  Nothing changes if an allocation fails
int rebuild_locked(ise_ivfsq* h, hipStream_t st) {
    if (h->pend_n == 0) return ISE_OK;
    IvfPlan pl;
    if (!ivf_plan_rebuild(h->size, h->pend_list.data(), h->pend_n, &pl, SQ_TILE))
        return ise_fail_(ISE_E_INVALID, "the lists' 64-row tiles no longer fit 32-bit slot numbers");
    const size_t nlist = (size_t)h->nlist;
    const long long tiles = pl.tile0[nlist];
    const size_t slots = (size_t)tiles * SQ_TILE;
    uint8_t* nx = nullptr;
    double* nr = nullptr;
    uint32_t *nids = nullptr, *nmeta = nullptr, *dest = nullptr;
    struct Free {
        void** p[5];
        ~Free() {
            for (void** q : p)
                if (*q) (void)hipFree(*q);
        }
    } fr{{(void**)&nx, (void**)&nr, (void**)&nids, (void**)&nmeta, (void**)&dest}};
    const size_t nmeta_n = 2 * nlist + 1 + (size_t)tiles;
    HIP_TRY(hipMalloc((void**)&nx, slots * h->stride));
    HIP_TRY(hipMalloc((void**)&nr, slots * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&nids, slots * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&nmeta, nmeta_n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&dest, (size_t)h->pend_n * sizeof(uint32_t)));
    std::vector<uint32_t> meta_host(nmeta_n);
    std::copy(pl.tile0.begin(), pl.tile0.end(), meta_host.begin());
    for (size_t l = 0; l < nlist; l++) meta_host[nlist + 1 + l] = (uint32_t)pl.size[l];
    std::copy(pl.tile_list.begin(), pl.tile_list.end(), meta_host.begin() + 2 * nlist + 1);
    HIP_TRY(hipMemcpyAsync(nmeta, meta_host.data(), nmeta_n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dest, pl.dest.data(), (size_t)h->pend_n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(nx, 0, slots * h->stride, st));  // pad slots read as zero rows
    HIP_TRY(hipMemsetAsync(nr, 0, slots * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(nids, 0xFF, slots * sizeof(uint32_t), st));
    if (h->tiles > 0)
        hipLaunchKernelGGL(ivfsq_move_tiles_kernel, dim3((unsigned)h->tiles), dim3(256), 0, st, (const uint8_t*)h->codes,
                           (const double*)h->rterm, (const uint32_t*)h->ids, h->tile_list_dev(), h->list_tile0_dev(),
                           (const uint32_t*)nmeta, h->stride, nx, nr, nids);
    hipLaunchKernelGGL(ivfsq_scatter_rows_kernel, dim3((unsigned)((h->pend_n + 3) / 4)), dim3(256), 0, st, (const uint8_t*)h->pend,
                       (const double*)h->pend_rterm, h->pend_n, (const uint32_t*)dest, (uint32_t)(h->n - h->pend_n), h->stride, nx, nr,
                       nids);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::swap(h->codes, nx);  // the old arrays go with the guard (hipFree waits for the passes that still read them)
    std::swap(h->rterm, nr);
    std::swap(h->ids, nids);
    std::swap(h->meta, nmeta);
    if (h->pend) (void)hipFree(h->pend);
    if (h->pend_rterm) (void)hipFree(h->pend_rterm);
    h->pend = nullptr;
    h->pend_rterm = nullptr;
    h->pend_n = h->pend_cap = 0;
    h->pend_list.clear();
    h->pend_list.shrink_to_fit();
    h->tiles = tiles;
    h->size = pl.size;
    h->tile0 = pl.tile0;
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
    long long g = (h->tiles + SQ_BLOCK_TILES * SQ_WAVES - 1) / (SQ_BLOCK_TILES * SQ_WAVES);
    g = std::min<long long>(g, std::min<long long>(per_cu * h->num_cu, MERGE_LISTS_MAX));
    return (unsigned)std::max<long long>(g, 1);
}

// mu_ held, trained.  Enqueues only, unless rows are pending (the rebuild blocks) or a workspace has to grow
int search_enqueue(ise_ivfsq* h, const float* q_dev, long long nq, int k, const long long* probes_dev, int nprobe, float* D_dev,
                   long long* I_dev, hipStream_t st) {
    h->batches++;
    // a search still in flight on another stream comes first on the device: before the rebuild and before the
    // workspaces are written
    if (h->used && h->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
    int rc = rebuild_locked(h, st);
    if (rc) return rc;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT;
    if (h->tiles == 0) {  // an empty index: padding, no pass
        const long long cnt = nq * k;
        hipLaunchKernelGGL(sq_fill_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, D_dev, I_dev, cnt, ip);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    const int qt = h->qt, gmax = SQ_STAGE_CHUNK / qt;
    const unsigned grid = pass_grid(h);
    const size_t rec = sq_rec_bytes(h->d), nl = (size_t)h->nlist;
    const hipEvent_t busy = h->used ? h->done : nullptr;
    if ((rc = grow(h->qrec, (size_t)std::min<long long>(nq, SQ_STAGE_CHUNK) * rec, busy))) return rc;
    if ((rc = grow(h->lo, (size_t)qt, busy))) return rc;
    if ((rc = grow(h->lists, (size_t)grid * qt * SQ_KPASS, busy))) return rc;
    if ((rc = grow(h->masks, (size_t)gmax * nl, busy))) return rc;
    if ((rc = grow(h->offs, (size_t)gmax * nl + gmax, busy))) return rc;
    if ((rc = grow(h->work, (size_t)gmax * h->tiles, busy))) return rc;
    struct Release {  // whatever path returns, a later user on another stream waits for this call
        ise_ivfsq* h;
        hipStream_t st;
        ~Release() {
            if (hipEventRecord(h->done, st) == hipSuccess) { h->used = true; h->last_stream = st; }
        }
    } release{h, st};
    uint32_t* counts = h->offs.p + (size_t)gmax * nl;
    const size_t lds = sq_lds_bytes(h->d, qt);
    for (long long c0 = 0; c0 < nq; c0 += SQ_STAGE_CHUNK) {
        // the chunk's records, masks and work lists (in stream order behind the passes that read the last chunk's)
        const int m = (int)std::min<long long>(SQ_STAGE_CHUNK, nq - c0);
        const int groups = (m + qt - 1) / qt;
        SqStageParams gp{};
        gp.q = q_dev + (size_t)c0 * h->d;
        gp.nq = m;
        gp.d = h->d;
        gp.ip = ip;
        gp.step = h->step();
        gp.off = h->off();
        gp.rec = h->qrec.p;
        hipLaunchKernelGGL(sq_stage_kernel, dim3((unsigned)m), dim3(64), 0, st, gp);
        HIP_TRY(hipMemsetAsync(h->masks.p, 0, (size_t)groups * nl * sizeof(uint32_t), st));
        const long long ptot = (long long)m * nprobe;
        hipLaunchKernelGGL(ivfsq_mask_kernel, dim3((unsigned)((ptot + 255) / 256)), dim3(256), 0, st, probes_dev + (size_t)c0 * nprobe,
                           ptot, nprobe, h->nlist, h->qshift, h->masks.p);
        hipLaunchKernelGGL(ivfsq_offsets_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const uint32_t*)h->masks.p,
                           h->list_tile0_dev(), h->nlist, h->offs.p, counts);
        hipLaunchKernelGGL(ivfsq_work_kernel, dim3((unsigned)((h->tiles + 255) / 256), (unsigned)groups), dim3(256), 0, st,
                           (const uint32_t*)h->masks.p, (const uint32_t*)h->offs.p, h->list_tile0_dev(), h->list_size_dev(),
                           h->tile_list_dev(), h->nlist, (uint32_t)h->tiles, h->work.p);
        for (int g = 0; g < groups; g++) {
            const long long q0 = c0 + (long long)g * qt;
            const int nqt = (int)std::min<long long>(qt, nq - q0);
            for (int off = 0; off < k; off += SQ_KPASS) {
                const int kp = std::min(SQ_KPASS, k - off);
                SqIvfScanParams sp{};
                sp.codes = h->codes;
                sp.rterm = h->rterm;
                sp.ids = h->ids;
                sp.d = h->d;
                sp.stride = h->stride;
                sp.qrec = h->qrec.p + (size_t)g * qt * rec;
                sp.nqt = nqt;
                sp.kp = kp;
                sp.ip = ip;
                sp.lo = off == 0 ? nullptr : h->lo.p;  // the merge of the pass before wrote it
                sp.lists = h->lists.p;
                sp.work = h->work.p + (size_t)g * h->tiles;
                sp.count = counts + g;
                sp.tiles_loaded = h->stats_dev;
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
                h->passes++;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

int check_search_args(const ise_ivfsq* h, const void* q, long long nq, int k, const void* probes, int nprobe, const void* D,
                      const void* I) {
    if (nq < 0) return ise_fail_(ISE_E_INVALID, "nq must be >= 0");
    if (k < 1 || k > ISE_MAX_K) return ise_fail_(ISE_E_INVALID, "k must be in [1, ISE_MAX_K]");
    if (nprobe < 1) return ise_fail_(ISE_E_INVALID, "nprobe must be positive");
    if (nq > 0 && (!q || !probes)) return ise_fail_(ISE_E_INVALID, "query or probe pointer is NULL");
    if (nq > 0 && (!D || !I)) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    if (nq * (long long)k >= (1ll << 40)) return ise_fail_(ISE_E_INVALID, "nq * k is too large");
    return check_handle(h);
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ise_fail_(ISE_E_NODEVICE, "no HIP device visible: the kNN path needs an MI355X (gfx950) GPU");
    if (device < 0 || device >= ndev) return ise_fail_(ISE_E_INVALID, "device out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ise_fail_(ISE_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    ise_ivfsq* h = new (std::nothrow) ise_ivfsq();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d = d;
    h->qtype = qtype;
    h->stride = sq_stride(d);
    h->qt = sq_qt(d);
    h->qshift = h->qt == 16 ? 4 : 3;
    h->metric = metric;
    h->nlist = nlist;
    h->device = device;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->size.assign((size_t)nlist, 0);
    h->size_all.assign((size_t)nlist, 0);
    h->tile0.assign((size_t)nlist + 1, 0u);
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&h->par, 3 * (size_t)d * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->bad, sizeof(unsigned int));
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
    HIP_TRY(hipDeviceSynchronize());
    free_rows(h);
    return ISE_OK;
}

extern "C" int ise_ivfsq_info(const ise_ivfsq_t* h, int* d, int* qtype, int* metric, int* nlist, int64_t* ntotal, int* is_trained,
                              int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d) *d = h->d;
    if (qtype) *qtype = h->qtype;
    if (metric) *metric = h->metric;
    if (nlist) *nlist = h->nlist;
    if (ntotal) *ntotal = h->n;
    if (is_trained) *is_trained = h->trained ? 1 : 0;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_ivfsq_set_trained_host(ise_ivfsq_t* h, const float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (h->n > 0) return ise_fail_(ISE_E_INVALID, "the index holds rows: their codes belong to the trained state in place (reset first)");
    const size_t cnt = trained_count(h), half = cnt / 2;
    for (size_t i = 0; i < cnt; i++)
        if (!(std::fabs(t[i]) <= FLT_MAX)) return ise_fail_(ISE_E_INVALID, "the trained state has a NaN or inf entry");
    for (size_t i = half; i < cnt; i++)
        if (t[i] < 0.f) return ise_fail_(ISE_E_INVALID, "the trained state has a negative vdiff");
    const size_t d = (size_t)h->d;
    std::vector<float> par(3 * d);
    for (size_t j = 0; j < d; j++) {  // ise_sq_set_trained_host's arithmetic: the same step and offset bits
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

extern "C" int ise_ivfsq_get_trained_host(ise_ivfsq_t* h, float* t) {
    if (!t) return ise_fail_(ISE_E_INVALID, "trained pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (check_trained(h)) return ISE_E_INVALID;
    std::copy(h->trained_host.begin(), h->trained_host.end(), t);
    return ISE_OK;
}

extern "C" int ise_ivfsq_add_host(ise_ivfsq_t* h, const float* x, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, x, list_no, n, "rows");
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = check_lists(h, list_no, n))) return rc;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    if ((rc = reserve_pending(h, n, st))) return rc;
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(unsigned int), st));
    const long long step = upload_step((size_t)h->d * sizeof(float));
    if ((rc = grow(h->xraw, (size_t)std::min<long long>(step, n) * h->d, nullptr))) return rc;
    for (long long i0 = 0; i0 < n; i0 += step) {  // nothing is counted in before the last piece's verdict
        const long long m = std::min<long long>(step, n - i0);
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = encode_pending(h, h->xraw.p, h->pend_n + i0, m, st))) return rc;
    }
    if ((rc = bad_check(h, st))) return rc;
    commit_add(h, list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_add_device(ise_ivfsq_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream) {
    int rc = check_add_args(h, x_dev, list_no_dev, n, "rows");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::vector<int64_t> lists((size_t)n);
    HIP_TRY(hipMemcpyAsync(lists.data(), list_no_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_lists(h, lists.data(), n))) return rc;
    if ((rc = reserve_pending(h, n, st))) return rc;
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(unsigned int), st));
    if ((rc = encode_pending(h, x_dev, h->pend_n, n, st))) return rc;
    if ((rc = bad_check(h, st))) return rc;
    commit_add(h, lists.data(), n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_add_codes_host(ise_ivfsq_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n) {
    int rc = check_add_args(h, codes, list_no, n, "codes");
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (check_trained(h)) return ISE_E_INVALID;
    if (n == 0) return ISE_OK;
    if ((rc = check_lists(h, list_no, n))) return rc;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    if ((rc = reserve_pending(h, n, st))) return rc;
    uint8_t* dst = h->pend + (size_t)h->pend_n * h->stride;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * h->stride, st));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)h->stride, codes, (size_t)h->d, (size_t)h->d, (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sq_rowterm_kernel, dim3((unsigned)((n + SQ_ENC_ROWS - 1) / SQ_ENC_ROWS)), dim3(SQ_WAVES * 64), 0, st,
                       (const uint8_t*)dst, h->stride, (long long)n, h->d, h->step(), h->pend_rterm + h->pend_n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    commit_add(h, list_no, n);
    return ISE_OK;
}

extern "C" int ise_ivfsq_list_sizes_host(ise_ivfsq_t* h, int64_t* sizes) {
    if (!sizes) return ise_fail_(ISE_E_INVALID, "sizes pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu_);
    for (int l = 0; l < h->nlist; l++) sizes[l] = h->size_all[(size_t)l];
    return ISE_OK;
}

extern "C" int ise_ivfsq_list_host(ise_ivfsq_t* h, int list, int64_t* ids, uint8_t* codes) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (list < 0 || list >= h->nlist) return ise_fail_(ISE_E_INVALID, "list out of range");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    int rc = rebuild_locked(h, h->stream);
    if (rc) return rc;
    const size_t m = (size_t)h->size[(size_t)list];
    if (m == 0) return ISE_OK;
    const size_t slot0 = (size_t)h->tile0[(size_t)list] * SQ_TILE;
    if (ids) {
        std::vector<uint32_t> tmp(m);
        HIP_TRY(hipMemcpy(tmp.data(), h->ids + slot0, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++) ids[i] = (int64_t)tmp[i];
    }
    if (codes)
        HIP_TRY(hipMemcpy2D(codes, (size_t)h->d, h->codes + slot0 * h->stride, (size_t)h->stride, (size_t)h->d, m, hipMemcpyDeviceToHost));
    return ISE_OK;
}

extern "C" int ise_ivfsq_search_device(ise_ivfsq_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                                       float* D_dev, int64_t* I_dev, void* stream) {
    const int rc = check_search_args(h, q_dev, nq, k, probes_dev, nprobe, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu_);
    if (check_trained(h)) return ISE_E_INVALID;
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
    if (check_trained(h)) return ISE_E_INVALID;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
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
        HIP_TRY(hipMemcpyAsync(p_dev, probes + (size_t)i0 * nprobe, (size_t)m * nprobe * sizeof(long long), hipMemcpyHostToDevice, st));
        if ((rc = search_enqueue(h, q_dev, m, k, p_dev, nprobe, D_dev, I_dev, st))) return rc;
        HIP_TRY(hipMemcpyAsync(D + (size_t)i0 * k, D_dev, (size_t)m * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, I_dev, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
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
