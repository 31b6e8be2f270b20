// ise_flat_sel.hip -- the float index's selector objects and its selector-filtered search (ise_sel_scan.hpp; ise_flat.hpp: the handle).
#include "ise_flat.hpp"
#include "ise_pass_host.hpp"
#include "ise_scan_params.hpp"
#include "ise_selector.hpp"

// ---- selectors (ise_sel_scan.hpp): a device bitmap over the rows of ONE index at ONE (ntotal, row epoch)
// mu_ held.  A selector is good for the handle it was made from while ntotal and the row epoch stand
int selector_check_locked(const ise_index* h, const ise_selector* sel) {
    if (!sel) return fail(ISE_E_INVALID, "selector is NULL");
    if (sel->owner != h) return fail(ISE_E_INVALID, "the selector was made for another index");
    if (sel->epoch != h->row_epoch)
        return fail(ISE_E_INVALID, "stale selector: rows were removed from the index (row epoch changed) since it was made");
    if (sel->ntotal != h->n)
        return fail(ISE_E_INVALID, "stale selector: ntotal changed (" + std::to_string(sel->ntotal) + " -> " +
                                       std::to_string(h->n) + ") since it was made");
    return ISE_OK;
}

// ---- selector objects and the selector-filtered search (ise_sel_scan.hpp)
#define SEL_NQ_CHUNK 64 /* queries per masked launch (4 groups of 16): bounds the per-block lists of a slot */

// a new selector for h as it stands (mu_ held): ceil(n / 32) words and a word of padding, so that the half-word of
// every tile below the capacity's last one is there to read, zero
static SelectorFor selector_for(const ise_index* h) {
    return SelectorFor{h, h->device, h->n, h->row_epoch, h->stream, (h->n + 31) / 32 + 1};
}
static void selector_census_launch(SelectorBase* s, hipStream_t st, unsigned long long* out4) {
    hipLaunchKernelGGL(sel_census_kernel, dim3((unsigned)((s->nwords + 255) / 256)), dim3(256), 0, st, s->bits, s->nwords,
                       s->ntotal, out4);
}

extern "C" int ise_selector_create_range(ise_index_t* h, int64_t i0, int64_t i1, ise_selector_t** out) {
    if (!out) return fail(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (!h) return fail(ISE_E_INVALID, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    const long long a = std::max<long long>(i0, 0), b = std::min<long long>(i1, h->n);
    return selector_create(selector_for(h), [&](SelectorBase* s) { return selector_fill_range(s, h->stream, a, b); },
                           selector_census_launch, out);
}

extern "C" int ise_selector_create_ids(ise_index_t* h, const int64_t* ids, int64_t n_ids, int invert, ise_selector_t** out) {
    if (!out) return fail(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (!h) return fail(ISE_E_INVALID, "handle is NULL");
    if (n_ids < 0 || (n_ids > 0 && !ids)) return fail(ISE_E_INVALID, "ids is NULL");
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    DevFree ids_dev;
    return selector_create(selector_for(h),
                           [&](SelectorBase* s) { return selector_scatter_ids(s, h->stream, ids, n_ids, invert, &ids_dev); },
                           selector_census_launch, out);
}

extern "C" int ise_selector_create_bitmap(ise_index_t* h, const uint32_t* words, int64_t n_words, ise_selector_t** out) {
    if (!out) return fail(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (!h) return fail(ISE_E_INVALID, "handle is NULL");
    if (n_words < 0 || (n_words > 0 && !words)) return fail(ISE_E_INVALID, "words is NULL");
    std::lock_guard<std::mutex> lk(h->mu_);
    if (n_words != (h->n + 31) / 32)
        return fail(ISE_E_INVALID, "the bitmap must have ceil(ntotal / 32) = " + std::to_string((h->n + 31) / 32) + " words");
    DeviceGuard gd(h->device);
    return selector_create(selector_for(h), [&](SelectorBase* s) { return selector_copy_bitmap(s, h->stream, words, n_words); },
                           selector_census_launch, out);  // the census clears the bits at or beyond ntotal
}

extern "C" int ise_selector_info(const ise_selector_t* sel, int64_t* out5) { return selector_info(sel, out5); }

extern "C" int ise_selector_destroy(ise_selector_t* sel) {
    if (sel) selector_free(sel);  // waits for the device: a masked pass still in flight has finished reading the bitmap
    return ISE_OK;
}

// one chunk of m <= SEL_NQ_CHUNK queries (mu_ held, the selector checked, the shift prepared): pad the queries, then
// per 32 results one masked pass + the merge of its per-block lists
static int sel_chunk_enqueue(ise_index* h, ise_index::SelSlot* sl, const ise_selector* sel, const float* q_dev, long long m,
                             int k, float* D_dev, long long* I_dev, hipStream_t st) {
    SelScanParams sp{};
    sp.xb = h->xb; sp.norms = h->norms; sp.mu = h->mu; sp.bits = sel->bits;
    sp.n = h->n; sp.d = h->d; sp.dp = h->dp;
    sp.qs_stride = qs_stride_for(h);
    sp.row_slots = (int)(row_bytes(h) / 16);
    sp.nq = (int)m; sp.metric = h->metric;
    sp.beta = uses_shift(h) ? exact_beta(h) : 0.f;
    int rc = range_staging(h, sp.qs_stride, &sp.tpr, &sp.vec_q);
    if (rc) return rc;
    const int ch = std::min(chunk_steps(h), 4);
    // the grid comes from the window's tiles, not from the index: at least a tile per wave, at most two blocks per CU
    // (what their LDS lets a CU hold) and the merge's list count
    sp.tile0 = (int)(sel->r0 / 16);
    sp.tile1 = (int)((sel->r1 + 15) / 16);
    const int span = sp.tile1 - sp.tile0;
    int nb = std::max(1, std::min({(span + SEL_W - 1) / SEL_W, 2 * h->num_cu, MERGE_LISTS_MAX}));
    sp.tiles_per_block = (span + nb - 1) / nb;
    nb = (span + sp.tiles_per_block - 1) / sp.tiles_per_block;
    const int groups = (int)((m + 15) / 16);
    // results per pass: XPASS_MAX, or what the wave lists' LDS holds beside long query rows (float32 d = 2048: 23; the
    // longest rows, float32 d = 2240 and bf16 d = 4480: 10).  The kp < 1 test below is not reachable on this index:
    // range_staging above has failed with make_plan's "d too large" for every row longer than those, whose stride of
    // 2248 units still leaves 10 results.  It stays as the guard of this function's own LDS arithmetic
    // (tests/test_flat_shapes_gpu.py, test_rows_too_long_are_refused_by_the_plan)
    static_assert(XPASS_MAX == SEL_KPASS_MAX, "one masked pass yields what one exact pass yields");
    const long long lds_left = (long long)LDS_LIMIT - (long long)range_lds_bytes(sp.qs_stride);
    const int kp = (int)std::min<long long>(std::min(k, XPASS_MAX), lds_left / (SEL_W * 16 * 8));
    if (kp < 1) return fail(ISE_E_INVALID, "rows too long for the selector-filtered search");
    rc = grow_owned(sl->q, (size_t)m * h->dp);
    if (!rc) rc = grow_owned(sl->part, (size_t)groups * nb * 16 * kp);
    if (!rc && k > kp) rc = grow_owned(sl->keys, (size_t)m * kp + (size_t)m);
    if (rc) return rc;
    const long long qtot = m * h->dp;
    hipLaunchKernelGGL(sel_pad_queries_kernel, dim3((unsigned)((qtot + 255) / 256)), dim3(256), 0, st, q_dev, h->d, h->dp,
                       qtot, sl->q.p);
    sp.q = sl->q.p;
    sp.part = sl->part.p;
    sp.kpass = kp;
    MergeParams mp{};
    mp.lists = sl->part.p; mp.qt = 16; mp.n_lists = nb; mp.nq = (int)m; mp.k = kp; mp.metric = h->metric;
    mp.stride_list = 16ll * kp; mp.stride_qtile = (long long)nb * 16 * kp;
    const ExactParams xp{};
    auto merge = [&] { hipLaunchKernelGGL((merge_kernel<false>), dim3((unsigned)m), dim3(MERGE_THREADS), 0, st, mp, xp); };
    const dim3 grid((unsigned)nb, (unsigned)groups);
    const size_t lds = sel_lds_bytes(sp.qs_stride, kp);
    const int bf16 = h->storage == ISE_STORE_BF16, shift = uses_shift(h);
    if (k <= kp) {
        sp.floor_keys = nullptr;
        ise_launch_sel_scan(bf16, shift, ch, grid, lds, st, sp);
        mp.D = D_dev; mp.I = I_dev;
        merge();
        h->sel_passes++;
    } else {
        u64* pass_keys = sl->keys.p;
        u64* floors = pass_keys + (size_t)m * kp;
        for (int off = 0; off < k; off += kp) {
            sp.floor_keys = off ? floors : nullptr;
            ise_launch_sel_scan(bf16, shift, ch, grid, lds, st, sp);
            mp.keys_out = pass_keys;
            merge();
            const long long tot = m * kp;
            hipLaunchKernelGGL(sel_scatter_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st,
                               (const u64*)pass_keys, (int)m, kp, off, k, h->metric, D_dev, I_dev, floors);
            h->sel_passes++;
        }
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// mu_ held.  Enqueues only
static int search_sel_enqueue(ise_index* h, const ise_selector* sel, const float* q_dev, long long nq, int k, float* D_dev,
                              long long* I_dev, hipStream_t st) {
    int rc = selector_check_locked(h, sel);
    if (rc) return rc;
    h->sel_batches++;
    if (sel->count == 0) {  // an empty window: padding, no pass
        knn_fill_launch(D_dev, I_dev, nq * k, h->metric != ISE_METRIC_L2, st);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    rc = prepare_shift_locked(h, st);
    if (rc) return rc;
    ise_index::SelSlot* sl = nullptr;
    bool waited = false;
    if ((rc = take_slot(h->ss, &h->ss_next, st, &sl, &waited))) return rc;
    if (!sl->order.ev) HIP_TRY(sl->order.create());  // a slot never used: nothing was waited for
    // its buffers may grow (free + allocate) below: the other stream's passes have to be through with them
    if (waited) HIP_TRY(hipEventSynchronize(sl->order.ev));
    CallOrder::Scope release{sl->order, st};
    for (long long i0 = 0; i0 < nq; i0 += SEL_NQ_CHUNK) {
        const long long m = std::min<long long>(SEL_NQ_CHUNK, nq - i0);
        rc = sel_chunk_enqueue(h, sl, sel, q_dev + (size_t)i0 * h->d, m, k, D_dev + (size_t)i0 * k, I_dev + (size_t)i0 * k, st);
        if (rc) return rc;
    }
    return ISE_OK;
}

extern "C" int ise_index_search_sel_device(ise_index_t* h, const float* q_dev, int64_t nq, int k, const ise_selector_t* sel,
                                           float* D_dev, int64_t* I_dev, void* stream) {
    int rc = check_search_args(h, q_dev, nq, k);
    if (rc) return rc;
    if (!sel) return fail(ISE_E_INVALID, "selector is NULL");
    if (nq > 0 && (!D_dev || !I_dev)) return fail(ISE_E_INVALID, "output pointer is NULL");
    std::lock_guard<std::mutex> lk(h->mu_);
    if (nq == 0) return selector_check_locked(h, sel);
    DeviceGuard gd(h->device);
    return search_sel_enqueue(h, sel, q_dev, nq, k, D_dev, (long long*)I_dev, (hipStream_t)stream);
}

// blocks; on one of the host contexts, never through the request combiner: a filtered call is not merged with others
extern "C" int ise_index_search_sel_host(ise_index_t* h, const float* q, int64_t nq, int k, const ise_selector_t* sel,
                                         float* D, int64_t* I) {
    int rc = check_search_args(h, q, nq, k);
    if (rc) return rc;
    if (!sel) return fail(ISE_E_INVALID, "selector is NULL");
    if (nq > 0 && (!D || !I)) return fail(ISE_E_INVALID, "output pointer is NULL");
    if (nq == 0) {
        std::lock_guard<std::mutex> lk(h->mu_);
        return selector_check_locked(h, sel);
    }
    return search_host_staged(h, q, nq, k, 1024, D, (long long*)I, [&](ise_index::HostCtx* c, long long m) {
        return search_sel_enqueue(h, sel, c->q_dev.p, m, k, c->D_dev.p, c->I_dev.p, c->stream);
    });
}

extern "C" int ise_index_sel_stats(ise_index_t* h, uint64_t* out3) {
    if (!h || !out3) return fail(ISE_E_INVALID, "NULL argument");
    {
        std::lock_guard<std::mutex> lk(h->mu_);
        out3[0] = h->sel_batches;
        out3[1] = h->sel_passes;
    }
    std::lock_guard<std::mutex> lk(h->rg_mu);
    out3[2] = h->sel_range_batches;
    return ISE_OK;
}
