// ise_binary_scan.hip -- host side of the binary flat index (include/ise_knn.h, ise_binary_index_*): storage,
// launches of the kernels of ise_binary_scan.hpp, the C entry points.  faiss.IndexBinaryFlat: exact Hamming kNN and
// range search; the reference's DHASH method (backend/engine.py:82-91) asks it for "every image within r bits".
//
// Calls on one handle run one at a time (a mutex; the host forms hold it until their results are back, the device
// forms while they enqueue).  The handle has ONE set of workspaces: every call that touches them waits for the call
// before and marks its own end (CallOrder, ise_host.hpp), and a workspace that has to grow is replaced by the drained
// rule (grow_drained, ise_host.hpp).
//
// Selectors and removal mirror the float index (ise_knn.hip): a selector is a device bitmap bound to
// the handle, its ntotal and its ROW EPOCH (bumped by whatever removes rows: a reset of a non-empty index, a removal
// that removes something; never by add); every filtered entry point checks the three before anything else.  A removal
// holds the mutex from its device-wide synchronisation to the end of its last copy: other calls on the handle run
// entirely before or entirely after it.
#include "ise_binary_scan.hpp"
#include "ise_pass_host.hpp"
#include "ise_remove.hpp"
#include "ise_remove_plan.hpp"
#include "ise_selector.hpp"

#define BIN_RANGE_NQ_CHUNK 256 /* queries per range batch: one host synchronisation each */
static_assert(BIN_RANGE_NQ_CHUNK <= 256, "binary_lims_kernel scans a batch's totals in one block of 256 threads");

struct ise_binary_index {
    int d_bits = 0, code_size = 0, ws = 0, device = 0, num_cu = 256;
    long long n = 0, cap = 0;
    u64* codes = nullptr;  // [cap][ws]; bytes past code_size of every row are zero
    hipStream_t stream = nullptr;
    CallOrder order;
    mutable std::mutex mu;
    DevBuf<uint8_t> raw;       // host forms: the queries as passed
    DevBuf<u64> qpad, lo, lists;
    DevBuf<int> oD, counts, rD;
    DevBuf<long long> oI, offs, totals, lims, rI;
    uint64_t st_search = 0, st_passes = 0, st_range = 0;
    unsigned long long row_epoch = 0;  // bumped when rows go or are renumbered: selectors made before are stale
    uint64_t st_sel = 0, st_sel_passes = 0, st_sel_range = 0;    // filtered batches, masked passes, filtered range batches
    uint64_t st_rm_calls = 0, st_rm_rows = 0, st_rm_moved = 0;   // removals that removed something, rows removed, rows moved
};

// a device bitmap over the rows of ONE binary index at ONE (ntotal, row epoch); bits: 2 * max(1, ceil(ntotal / 64))
// words, one aligned 8-byte word per 64-row tile
struct ise_binary_selector : SelectorBase {};

struct ise_binary_range_result {
    std::vector<int64_t> lims;
    std::vector<int32_t> D;
    std::vector<int64_t> I;
};

namespace {
int bin_wt(const ise_binary_index* h) { return h->ws == 1 ? 1 : h->ws == 2 ? 2 : 0; }
size_t bin_query_lds(const ise_binary_index* h) { return bin_wt(h) == 0 ? (size_t)BIN_QT * h->ws * 8 : 0; }

// mk: the selector's mask and window (the masked kernels), or null
void launch_scan(int wt, unsigned grid, size_t lds, hipStream_t st, const BinScanParams& sp, const BinMask* mk) {
    static LdsAttrOnce attr[6];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), BIN_LDS_MAX);
        if constexpr (std::is_invocable_v<decltype(kern), BinScanParams, BinMask>)
            hipLaunchKernelGGL(kern, dim3(grid), dim3(BIN_WAVES * 64), lds, st, sp, *mk);
        else
            hipLaunchKernelGGL(kern, dim3(grid), dim3(BIN_WAVES * 64), lds, st, sp);
    };
    if (mk) {
        if (wt == 1) go(binary_scan_masked_kernel<1>, attr[3]);
        else if (wt == 2) go(binary_scan_masked_kernel<2>, attr[4]);
        else go(binary_scan_masked_kernel<0>, attr[5]);
    } else if (wt == 1) go(binary_scan_kernel<1>, attr[0]);
    else if (wt == 2) go(binary_scan_kernel<2>, attr[1]);
    else go(binary_scan_kernel<0>, attr[2]);
}

template <bool FILL>
void launch_range(int wt, unsigned grid, size_t lds, hipStream_t st, const BinRangeParams& rp, const BinMask* mk) {
    const dim3 g(grid), b(BIN_WAVES * 64);
    if (mk) {
        if (wt == 1) hipLaunchKernelGGL((binary_range_masked_kernel<1, FILL>), g, b, lds, st, rp, *mk);
        else if (wt == 2) hipLaunchKernelGGL((binary_range_masked_kernel<2, FILL>), g, b, lds, st, rp, *mk);
        else hipLaunchKernelGGL((binary_range_masked_kernel<0, FILL>), g, b, lds, st, rp, *mk);
    } else if (wt == 1) hipLaunchKernelGGL((binary_range_kernel<1, FILL>), g, b, lds, st, rp);
    else if (wt == 2) hipLaunchKernelGGL((binary_range_kernel<2, FILL>), g, b, lds, st, rp);
    else hipLaunchKernelGGL((binary_range_kernel<0, FILL>), g, b, lds, st, rp);
}

// blocks of a pass over `tiles` 64-row tiles: about two per wave on a short index, at most two blocks per CU
unsigned bin_grid_tiles(const ise_binary_index* h, long long tiles) { return coded_grid(tiles, 2, BIN_WAVES, 2, h->num_cu); }
unsigned bin_grid(const ise_binary_index* h) { return bin_grid_tiles(h, (h->n + 63) / 64); }

// mu held.  A selector is good for the handle it was made from while ntotal and the row epoch stand
int selector_check_locked(const ise_binary_index* h, const ise_binary_selector* sel) {
    if (!sel) return ise_fail_(ISE_E_INVALID, "selector is NULL");
    if (sel->owner != h) return ise_fail_(ISE_E_INVALID, "the selector was made for another index");
    if (sel->epoch != h->row_epoch)
        return ise_fail_(ISE_E_INVALID,
                         "stale selector: rows were removed from the index (row epoch changed) since it was made");
    if (sel->ntotal != h->n)
        return ise_fail_(ISE_E_INVALID, "stale selector: ntotal changed (" + std::to_string(sel->ntotal) + " -> " +
                                            std::to_string(h->n) + ") since it was made");
    return ISE_OK;
}

BinMask selector_mask(const ise_binary_selector* sel) {
    BinMask mk{};
    mk.words = reinterpret_cast<const u64*>(sel->bits);
    mk.tile0 = sel->r0 >> 6;
    mk.tile1 = (sel->r1 + 63) >> 6;
    return mk;
}

void pad_rows(const uint8_t* src_dev, int code_size, u64* dst, int ws, long long n, hipStream_t st) {
    const long long total = n * ws;
    hipLaunchKernelGGL(binary_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src_dev, code_size, dst,
                       ws, n);
}

int add_device_locked(ise_binary_index* h, const uint8_t* x_dev, long long n, hipStream_t st) {
    if (h->n + n >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "a binary index holds fewer than 2^32 rows");
    int rc = h->order.wait(st);
    if (rc) return rc;
    rc = reserve_code_rows(&h->codes, (size_t)h->ws * 8, h->n, &h->cap, h->n + n, 64, st);
    if (rc) return rc;
    pad_rows(x_dev, h->code_size, h->codes + (size_t)h->n * h->ws, h->ws, n, st);
    HIP_TRY(hipGetLastError());
    h->n += n;
    return h->order.mark(st);
}

// q_dev: nq x code_size bytes on the device; D_dev / I_dev: nq x k.  sel: among the selector's rows only (checked by
// the caller; the masked kernels over its window), or null
int search_enqueue(ise_binary_index* h, const uint8_t* q_dev, long long nq, int k, int* D_dev, long long* I_dev,
                   hipStream_t st, const ise_binary_selector* sel = nullptr) {
    int rc = h->order.wait(st);
    if (rc) return rc;
    uint64_t& st_batches = sel ? h->st_sel : h->st_search;
    uint64_t& st_pass = sel ? h->st_sel_passes : h->st_passes;
    if (h->n == 0 || (sel && sel->count == 0)) {  // nothing to rank: a fill, no pass
        st_batches++;
        knn_fill_launch(D_dev, I_dev, nq * k, 0, st);
        HIP_TRY(hipGetLastError());
        return h->order.mark(st);
    }
    BinMask mk{};
    if (sel) mk = selector_mask(sel);
    const unsigned grid = sel ? bin_grid_tiles(h, mk.tile1 - mk.tile0) : bin_grid(h);
    const long long nq16 = (nq + BIN_QT - 1) / BIN_QT * BIN_QT;
    if ((rc = grow_drained(h->qpad, (size_t)nq16 * h->ws))) return rc;
    if ((rc = grow_drained(h->lo, (size_t)nq16))) return rc;
    if ((rc = grow_drained(h->lists, (size_t)grid * BIN_QT * BIN_KPASS))) return rc;
    st_batches++;  // counted once the batch is certain to be enqueued
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
            launch_scan(wt, grid, lds, st, sp, sel ? &mk : nullptr);
            pass_merge_launch(h->lists.p, BIN_QT, BIN_KPASS, grid, nqt, kp, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k,
                              h->lo.p + q0, k, off, 0, st);
            st_pass++;
        }
    }
    HIP_TRY(hipGetLastError());
    return h->order.mark(st);
}

int check_handle(const ise_binary_index* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "binary index handle is NULL"); }

int check_search_args(const ise_binary_index* h, const void* q, long long nq, int k, const void* D, const void* I) {
    if (check_handle(h)) return ISE_E_INVALID;
    return check_knn_args(q, nq, k, D, I);
}

// one batch of m <= BIN_RANGE_NQ_CHUNK queries (host pointer) appended to the result.  sel: the segments cut the
// selector's window (whole tiles) instead of [0, n), or null
int range_batch(ise_binary_index* h, hipStream_t st, const uint8_t* q, long long m, int radius, ise_binary_range_result* res,
                const ise_binary_selector* sel) {
    int rc;
    const long long m16 = (m + BIN_QT - 1) / BIN_QT * BIN_QT;
    BinMask mkv{};
    if (sel) mkv = selector_mask(sel);
    const BinMask* mk = sel ? &mkv : nullptr;
    const unsigned grid = sel ? bin_grid_tiles(h, mkv.tile1 - mkv.tile0) : bin_grid(h);
    const int S = (int)grid * BIN_WAVES;
    long long seg_rows = ((sel ? (mkv.tile1 - mkv.tile0) * 64 : h->n) + S - 1) / S;
    seg_rows = (seg_rows + 63) / 64 * 64;
    const long long M = m * S;
    if ((rc = grow_drained(h->raw, (size_t)m * h->code_size))) return rc;
    if ((rc = grow_drained(h->qpad, (size_t)m16 * h->ws))) return rc;
    if ((rc = grow_drained(h->counts, (size_t)M))) return rc;
    if ((rc = grow_drained(h->offs, (size_t)M))) return rc;
    if ((rc = grow_drained(h->lims, (size_t)m + 1))) return rc;
    if ((rc = grow_drained(h->totals, (size_t)m))) return rc;
    HIP_TRY(hipMemcpyAsync(h->raw.p, q, (size_t)m * h->code_size, hipMemcpyHostToDevice, st));
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
        launch_range<false>(wt, grid, lds, st, rp, mk);
    }
    hipLaunchKernelGGL(binary_offsets_kernel, dim3((unsigned)m), dim3(BIN_SCAN_THREADS), 0, st, h->counts.p, S, h->offs.p,
                       h->totals.p);
    hipLaunchKernelGGL(binary_lims_kernel, dim3(1), dim3(256), 0, st, h->totals.p, (int)m, h->lims.p);
    HIP_TRY(hipGetLastError());
    std::vector<long long> lims((size_t)m + 1);
    HIP_TRY(hipMemcpyAsync(lims.data(), h->lims.p, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the one host synchronisation that sizes the result
    const long long total = lims[(size_t)m];
    const size_t at = res->D.size();
    for (long long i = 1; i <= m; i++) res->lims.push_back((int64_t)at + lims[(size_t)i]);
    if (total == 0) return ISE_OK;
    if ((rc = grow_drained(h->rD, (size_t)total))) return rc;
    if ((rc = grow_drained(h->rI, (size_t)total))) return rc;
    rp.D = h->rD.p;
    rp.I = h->rI.p;
    for (long long q0 = 0; q0 < m; q0 += BIN_QT) {
        rp.qpad = h->qpad.p + (size_t)q0 * h->ws;
        rp.nqt = (int)std::min<long long>(BIN_QT, m - q0);
        rp.offs = h->offs.p + (size_t)q0 * S;
        rp.lims = h->lims.p + q0;
        launch_range<true>(wt, grid, lds, st, rp, mk);
    }
    HIP_TRY(hipGetLastError());
    res->D.resize(at + (size_t)total);
    res->I.resize(at + (size_t)total);
    HIP_TRY(hipMemcpyAsync(res->D.data() + at, h->rD.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(res->I.data() + at, h->rI.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
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
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_binary_index* h = new (std::nothrow) ise_binary_index();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->d_bits = d_bits;
    h->code_size = d_bits / 8;
    const int w = (h->code_size + 7) / 8;
    h->ws = w == 1 ? 1 : (w + 1) / 2 * 2;
    h->device = device;
    h->num_cu = num_cu;
    DeviceGuard gd(device);
    if (!gd.ok) {
        delete h;
        return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    }
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->order.create();
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
        h->order.destroy();
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_binary_index_reset(ise_binary_index_t* h) {
    if (check_handle(h)) return ISE_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->n > 0) h->row_epoch++;  // rows went: selectors made before are stale
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
    const long long step = upload_step((size_t)h->code_size);
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        int rc = grow_drained(h->raw, (size_t)m * h->code_size);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(h->raw.p, codes + (size_t)i0 * h->code_size, (size_t)m * h->code_size, hipMemcpyHostToDevice,
                               h->stream));
        rc = add_device_locked(h, h->raw.p, m, h->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
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
    int rc = h->order.wait(h->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)h->code_size, h->codes + (size_t)i0 * h->ws, (size_t)h->ws * 8, (size_t)h->code_size,
                             (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if ((rc = h->order.mark(h->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ISE_OK;
}

extern "C" int ise_binary_index_search_device(ise_binary_index_t* h, const uint8_t* q_dev, int64_t nq, int k, int32_t* D_dev,
                                              int64_t* I_dev, void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, D_dev, I_dev);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    return search_enqueue(h, q_dev, nq, k, (int*)D_dev, (long long*)I_dev, (hipStream_t)stream);
}

extern "C" int ise_binary_index_search_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int k, int32_t* D,
                                            int64_t* I) {
    int rc = check_search_args(h, q, nq, k, D, I);
    if (rc) return rc;
    if (nq == 0) return ISE_OK;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t cnt = (size_t)nq * k;
    if ((rc = grow_drained(h->raw, (size_t)nq * h->code_size))) return rc;
    if ((rc = grow_drained(h->oD, cnt))) return rc;
    if ((rc = grow_drained(h->oI, cnt))) return rc;
    if ((rc = h->order.wait(h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(h->raw.p, q, (size_t)nq * h->code_size, hipMemcpyHostToDevice, h->stream));
    if ((rc = search_enqueue(h, h->raw.p, nq, k, h->oD.p, h->oI.p, h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(D, h->oD.p, cnt * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(I, h->oI.p, cnt * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ISE_OK;
}

// filtered: sel must be a selector (checked first, under the mutex, also for nq == 0 or an empty index)
static int range_search_impl(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int32_t radius, bool filtered,
                             const ise_binary_selector* sel, ise_binary_range_result_t** out) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (check_handle(h)) return ISE_E_INVALID;
    if (filtered && !sel) return ise_fail_(ISE_E_INVALID, "selector is NULL");
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
        if (!rc && filtered) rc = selector_check_locked(h, sel);
        if (!rc && (h->n == 0 || radius <= 0 || (filtered && sel->count == 0))) {
            res->lims.resize((size_t)nq + 1, 0);  // nothing can match: no pass
        } else if (!rc) {
            rc = h->order.wait(h->stream);
            for (long long q0 = 0; q0 < nq && !rc; q0 += BIN_RANGE_NQ_CHUNK) {
                const long long m = std::min<long long>(BIN_RANGE_NQ_CHUNK, nq - q0);
                (filtered ? h->st_sel_range : h->st_range)++;
                rc = range_batch(h, h->stream, q + (size_t)q0 * h->code_size, m, radius, res, sel);
            }
            if (!rc) rc = h->order.mark(h->stream);  // the workspaces' last user, as after every other call
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

extern "C" int ise_binary_index_range_search_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int32_t radius,
                                                  ise_binary_range_result_t** out) {
    return range_search_impl(h, q, nq, radius, false, nullptr, out);
}

extern "C" int ise_binary_index_range_search_sel_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int32_t radius,
                                                      const ise_binary_selector_t* sel, ise_binary_range_result_t** out) {
    return range_search_impl(h, q, nq, radius, true, sel, out);
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

// ---- selectors
namespace {
// a new selector for h as it stands (mu held): one 8-byte word per 64-row tile, at least one
SelectorFor selector_for(const ise_binary_index* h) {
    return SelectorFor{h, h->device, h->n, h->row_epoch, h->stream, 2 * std::max<long long>(1, (h->n + 63) / 64)};
}
void selector_census_launch(SelectorBase* s, hipStream_t st, unsigned long long* out4) {
    const long long nw64 = s->nwords / 2;
    hipLaunchKernelGGL(binary_sel_census_kernel, dim3((unsigned)((nw64 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<u64*>(s->bits), nw64, s->ntotal, out4);
}
}  // namespace

extern "C" int ise_binary_selector_create_range(ise_binary_index_t* h, int64_t i0, int64_t i1, ise_binary_selector_t** out) {
    if (!out) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (check_handle(h)) return ISE_E_INVALID;
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    const long long a = std::max<long long>(i0, 0), b = std::min<long long>(i1, h->n);
    return selector_create(selector_for(h), [&](SelectorBase* s) { return selector_fill_range(s, h->stream, a, b); },
                           selector_census_launch, out);
}

extern "C" int ise_binary_selector_create_ids(ise_binary_index_t* h, const int64_t* ids, int64_t n_ids, int invert,
                                              ise_binary_selector_t** out) {
    if (!out) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (check_handle(h)) return ISE_E_INVALID;
    if (n_ids < 0 || (n_ids > 0 && !ids)) return ise_fail_(ISE_E_INVALID, "ids is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    DevFree ids_dev;
    return selector_create(selector_for(h),
                           [&](SelectorBase* s) { return selector_scatter_ids(s, h->stream, ids, n_ids, invert, &ids_dev); },
                           selector_census_launch, out);
}

extern "C" int ise_binary_selector_create_bitmap(ise_binary_index_t* h, const uint32_t* words, int64_t n_words,
                                                 ise_binary_selector_t** out) {
    if (!out) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (check_handle(h)) return ISE_E_INVALID;
    if (n_words < 0 || (n_words > 0 && !words)) return ise_fail_(ISE_E_INVALID, "words is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    if (n_words != (h->n + 31) / 32)
        return ise_fail_(ISE_E_INVALID, "the bitmap must have ceil(ntotal / 32) = " + std::to_string((h->n + 31) / 32) + " words");
    return selector_create(selector_for(h), [&](SelectorBase* s) { return selector_copy_bitmap(s, h->stream, words, n_words); },
                           selector_census_launch, out);  // the census clears the bits at or beyond ntotal
}

extern "C" int ise_binary_selector_info(const ise_binary_selector_t* sel, int64_t* out5) { return selector_info(sel, out5); }

extern "C" int ise_binary_selector_destroy(ise_binary_selector_t* sel) {
    if (!sel) return ISE_OK;
    DeviceGuard gd(sel->device);
    selector_free(sel);
    return ISE_OK;
}

extern "C" int ise_binary_index_search_sel_device(ise_binary_index_t* h, const uint8_t* q_dev, int64_t nq, int k,
                                                  const ise_binary_selector_t* sel, int32_t* D_dev, int64_t* I_dev,
                                                  void* stream) {
    int rc = check_search_args(h, q_dev, nq, k, D_dev, I_dev);
    if (rc) return rc;
    if (!sel) return ise_fail_(ISE_E_INVALID, "selector is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    if ((rc = selector_check_locked(h, sel))) return rc;  // first, and also for nq == 0 or an empty index
    if (nq == 0) return ISE_OK;
    return search_enqueue(h, q_dev, nq, k, (int*)D_dev, (long long*)I_dev, (hipStream_t)stream, sel);
}

extern "C" int ise_binary_index_search_sel_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int k,
                                                const ise_binary_selector_t* sel, int32_t* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k, D, I);
    if (rc) return rc;
    if (!sel) return ise_fail_(ISE_E_INVALID, "selector is NULL");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(h->mu);
    if ((rc = selector_check_locked(h, sel))) return rc;
    if (nq == 0) return ISE_OK;
    const size_t cnt = (size_t)nq * k;
    if ((rc = grow_drained(h->raw, (size_t)nq * h->code_size))) return rc;
    if ((rc = grow_drained(h->oD, cnt))) return rc;
    if ((rc = grow_drained(h->oI, cnt))) return rc;
    if ((rc = h->order.wait(h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(h->raw.p, q, (size_t)nq * h->code_size, hipMemcpyHostToDevice, h->stream));
    if ((rc = search_enqueue(h, h->raw.p, nq, k, h->oD.p, h->oI.p, h->stream, sel))) return rc;
    HIP_TRY(hipMemcpyAsync(D, h->oD.p, cnt * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(I, h->oI.p, cnt * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ISE_OK;
}

extern "C" int ise_binary_index_sel_stats(ise_binary_index_t* h, uint64_t* out3) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    out3[0] = h->st_sel;
    out3[1] = h->st_sel_passes;
    out3[2] = h->st_sel_range;
    return ISE_OK;
}

// ---- remove_ids: stable in-place compaction of the code rows (ise_remove.hpp)
namespace {
// everything a removal allocates for the duration of the call
struct BinRemoveScratch {
    uint32_t* g = nullptr;        // [T] destination row at which run t bites
    uint32_t* cend = nullptr;     // [T] rows removed up to and including run t
    uint32_t* src_idx = nullptr;  // [slab] source rows of the current slab
    char* bounce = nullptr;       // one slab of rows
    ~BinRemoveScratch() {
        for (void* p : {(void*)g, (void*)cend, (void*)src_idx, (void*)bounce})
            if (p) (void)hipFree(p);
    }
};

// runs: sorted, disjoint, non-adjacent, non-empty, inside [0, h->n).  mu held.
int remove_runs_locked(ise_binary_index* h, const std::vector<RemoveRun>& runs, long long removed) {
    const long long n_old = h->n, n_new = n_old - removed, first = runs[0].start;
    const long long moved = n_new - first;  // destination rows [first, n_new) get a new row
    hipStream_t st = h->stream;
    HIP_TRY(hipDeviceSynchronize());  // nothing in flight reads the rows while they move
    if (moved > 0) {
        BinRemoveScratch sc;
        const long long T = (long long)runs.size();
        std::vector<uint32_t> g, cend;
        remove_plan_tables(runs, &g, &cend);
        // slab: at most 256 MiB of rows in the bounce buffer, as the float index; a slab's units (16 bytes, or the
        // 8-byte rows of ws == 1) stay below 2^31 whatever $ISE_REMOVE_SLAB_ROWS says
        const size_t rb = (size_t)h->ws * 8;
        const uint32_t upr = (uint32_t)std::max(1, h->ws / 2);
        const long long slab = remove_plan_slab_rows(ise_remove_slab_rows_(), (long long)rb, (long long)upr, moved);
        HIP_TRY(hipMalloc((void**)&sc.g, (size_t)T * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&sc.cend, (size_t)T * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&sc.src_idx, (size_t)slab * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&sc.bounce, (size_t)slab * rb));
        HIP_TRY(hipMemcpyAsync(sc.g, g.data(), (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sc.cend, cend.data(), (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // g and cend are pageable host vectors
        for (long long a = first; a < n_new; a += slab) {
            const long long m = std::min(slab, n_new - a);
            const unsigned gw = (unsigned)std::min<long long>((m + 255) / 256, (long long)h->num_cu * 8);
            hipLaunchKernelGGL(remove_src_kernel, dim3(gw), dim3(256), 0, st, (const uint32_t*)sc.g, (const uint32_t*)sc.cend,
                               (int)T, (uint32_t)a, (uint32_t)m, sc.src_idx);
            // rows src_idx[0 .. m) -> bounce -> rows [a, a + m)
            const uint32_t total = (uint32_t)(m * upr);
            const uint32_t per = 64 * (h->ws == 1 ? BIN_REMOVE_UNROLL : REMOVE_UNROLL);
            const uint32_t pieces = (total + per - 1) / per;
            const unsigned grid = std::max(1u, std::min((pieces + 3) / 4, (unsigned)h->num_cu * 4u));  // 16 waves per CU
            if (h->ws == 1) {
                hipLaunchKernelGGL(binary_remove_words_kernel<true>, dim3(grid), dim3(256), 0, st, (const u64*)h->codes,
                                   (const uint32_t*)sc.src_idx, (u64*)sc.bounce, total);
                hipLaunchKernelGGL(binary_remove_words_kernel<false>, dim3(grid), dim3(256), 0, st, (const u64*)sc.bounce,
                                   (const uint32_t*)nullptr, h->codes + a, total);
            } else {
                hipLaunchKernelGGL(remove_rows_kernel<true>, dim3(grid), dim3(256), 0, st, (const u32x4*)h->codes,
                                   (const uint32_t*)sc.src_idx, (u32x4*)sc.bounce, total, upr);
                hipLaunchKernelGGL(remove_rows_kernel<false>, dim3(grid), dim3(256), 0, st, (const u32x4*)sc.bounce,
                                   (const uint32_t*)nullptr, (u32x4*)(h->codes + (size_t)a * h->ws), total, upr);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(st));  // before the scratch is freed; a removal blocks
    }
    // the tail [n_new, n_old) keeps its stale rows: masked by row number, like the rows a reset leaves behind
    h->n = n_new;
    h->row_epoch++;  // rows were renumbered: selectors made before are stale
    h->order.forget();  // the device has drained
    h->st_rm_calls++;
    h->st_rm_rows += (uint64_t)removed;
    h->st_rm_moved += (uint64_t)moved;
    return ISE_OK;
}
}  // namespace

extern "C" int ise_binary_index_remove_range(ise_binary_index_t* h, int64_t i0, int64_t i1, int64_t* n_removed) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (n_removed) *n_removed = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const long long a = std::max<long long>(i0, 0), b = std::min<long long>(i1, h->n);
    if (a >= b) return ISE_OK;  // nothing to remove: no synchronisation, no counters
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    const int rc = remove_runs_locked(h, {RemoveRun{a, b - a}}, b - a);
    if (rc == ISE_OK && n_removed) *n_removed = b - a;
    return rc;
}

extern "C" int ise_binary_index_remove_ids_host(ise_binary_index_t* h, const int64_t* ids, int64_t n_ids, int64_t* n_removed) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (n_removed) *n_removed = 0;
    if (n_ids < 0 || (n_ids > 0 && !ids)) return ise_fail_(ISE_E_INVALID, "ids is NULL");
    if (n_ids == 0) return ISE_OK;
    std::vector<long long> v;
    std::vector<RemoveRun> runs;
    long long removed = 0;
    try {
        v = remove_plan_ids(ids, n_ids);
    } catch (const std::bad_alloc&) {
        return ise_fail_(ISE_E_NOMEM, "remove_ids: host allocation failed");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    try {
        removed = remove_plan_runs(v, h->n, &runs);
    } catch (const std::bad_alloc&) {
        return ise_fail_(ISE_E_NOMEM, "remove_ids: host allocation failed");
    }
    if (removed == 0) return ISE_OK;  // nothing to remove: no synchronisation, no counters
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    const int rc = remove_runs_locked(h, runs, removed);
    if (rc == ISE_OK && n_removed) *n_removed = removed;
    return rc;
}

extern "C" int ise_binary_index_remove_stats(ise_binary_index_t* h, uint64_t* out3) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    out3[0] = h->st_rm_calls;
    out3[1] = h->st_rm_rows;
    out3[2] = h->st_rm_moved;
    return ISE_OK;
}
