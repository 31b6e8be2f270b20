// ise_flat_range.hip -- the float index's range search, plain and masked by a selector (ise_range.hpp; ise_flat.hpp: the handle).
#include <memory>
#include "ise_flat.hpp"
#include "ise_scan_params.hpp"
#include "ise_range.hpp"
#include "ise_selector.hpp"

// ---- range search (ise_range.hpp): index.range_search(x, radius) -> (lims, D, I)
struct ise_range_result {
    std::vector<int64_t> lims;
    std::vector<float> D;
    std::vector<int64_t> I;
};

#define RANGE_NQ_CHUNK 256          /* queries per batch: one host synchronisation (and 16 passes over the index) each */
#define RANGE_STAGE_CAP 16          /* default staging entries per (query, wave segment) */
#define RANGE_STAGE_MAX (1ll << 23) /* most staged entries per batch (64 MiB): a smaller capacity beyond that */

template <bool BF16, bool SHIFT>
static void launch_range_v(int ch, dim3 grid, size_t lds, hipStream_t st, const RangeParams& rp) {
    static LdsAttrOnce attr[3];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), LDS_LIMIT);
        hipLaunchKernelGGL(kern, grid, dim3(RANGE_W * 64), lds, st, rp);
    };
    if (ch >= 4) go(range_scan_kernel<4, BF16, SHIFT>, attr[0]);
    else if (ch == 2) go(range_scan_kernel<2, BF16, SHIFT>, attr[1]);
    else go(range_scan_kernel<1, BF16, SHIFT>, attr[2]);
}
static void launch_range(const ise_index* h, int ch, dim3 grid, size_t lds, hipStream_t st, const RangeParams& rp) {
    if (h->storage == ISE_STORE_BF16) launch_range_v<true, false>(ch, grid, lds, st, rp);
    else if (uses_shift(h)) launch_range_v<false, true>(ch, grid, lds, st, rp);
    else launch_range_v<false, false>(ch, grid, lds, st, rp);
}

// the index as the range kernels read it (mu_ held, shift prepared)
static void range_params_index(const ise_index* h, RangeParams* rp) {
    rp->xb = h->xb;
    rp->norms = h->norms;
    rp->mu = h->mu;
    rp->d = h->d;
    rp->dp = h->dp;
    rp->qs_stride = qs_stride_for(h);
    rp->row_slots = (int)(row_bytes(h) / 16);
    rp->metric = h->metric;
    rp->beta = uses_shift(h) ? exact_beta(h) : 0.f;
}

// one batch of m <= RANGE_NQ_CHUNK queries, appended to r (rg_mu held).  sel: restricted to a selector's window and
// mask (the MASK instantiations), or null
static int range_batch(ise_index* h, hipStream_t st, const float* q, long long m, float radius, const ise_selector* sel,
                       ise_range_result* r) {
    auto& ws = h->rg;
    const int dp = h->dp, d = h->d;
    // queries zero padded to dp: the staging reads them per row, the direct difference as exact_l2_rows does
    int rc = grow_owned(ws.q_pin, (size_t)m * dp);
    if (!rc) rc = grow_owned(ws.q, (size_t)m * dp);
    if (rc) return rc;
    for (long long i = 0; i < m; i++) {
        memcpy(ws.q_pin.p + (size_t)i * dp, q + (size_t)i * d, (size_t)d * sizeof(float));
        memset(ws.q_pin.p + (size_t)i * dp + d, 0, (size_t)(dp - d) * sizeof(float));
    }
    HIP_TRY(hipMemcpyAsync(ws.q.p, ws.q_pin.p, (size_t)m * dp * sizeof(float), hipMemcpyHostToDevice, st));

    RangeParams rp{};
    dim3 grid;
    size_t lds = 0;
    int ch = 1;
    long long n0 = 0;
    {
        std::lock_guard<std::mutex> lk(h->mu_);
        rc = prepare_shift_locked(h, st);
        if (rc) return rc;
        n0 = h->n;
        if (n0 == 0) {  // an empty index (a reset since the caller looked): every list is empty
            r->lims.resize(r->lims.size() + (size_t)m, r->lims.back());
            return ISE_OK;
        }
        if (sel) {
            rc = selector_check_locked(h, sel);
            if (rc) return rc;
            if (sel->count == 0) {  // an empty selection: every list is empty
                r->lims.resize(r->lims.size() + (size_t)m, r->lims.back());
                h->sel_range_batches++;
                return ISE_OK;
            }
        }
        range_params_index(h, &rp);
        rc = range_staging(h, rp.qs_stride, &rp.tpr, &rp.vec_q);
        if (rc) return rc;
        ch = std::min(chunk_steps(h), 4);
        // blocks own contiguous slabs of row tiles (of the selector's window), up to 4 blocks per CU
        rp.tile0 = sel ? (int)(sel->r0 / 16) : 0;
        rp.bits = sel ? sel->bits : nullptr;
        rp.tiles_total = sel ? (int)((sel->r1 + 15) / 16) : (int)((n0 + 15) / 16);
        const int span = rp.tiles_total - rp.tile0;
        int nb = std::max(1, std::min(span, 4 * h->num_cu));
        rp.tiles_per_block = (span + nb - 1) / nb;
        nb = (span + rp.tiles_per_block - 1) / rp.tiles_per_block;
        rp.nseg = nb * RANGE_W;
        rp.n = n0;
        rp.nq = (int)m;
        rp.radius = radius;
        int cap = knobs().range_stage_cap.load(std::memory_order_relaxed);
        if (cap <= 0) cap = RANGE_STAGE_CAP;
        rp.cap = (int)std::max<long long>(1, std::min<long long>(cap, RANGE_STAGE_MAX / (m * rp.nseg)));
        const size_t segs = (size_t)m * rp.nseg;
        rc = grow_owned(ws.cnt, segs);
        if (!rc) rc = grow_owned(ws.segoff, segs);
        if (!rc) rc = grow_owned(ws.sD, segs * rp.cap);
        if (!rc) rc = grow_owned(ws.sI, segs * rp.cap);
        if (!rc) rc = grow_owned(ws.tot, (size_t)m);
        if (!rc) rc = grow_owned(ws.lims, (size_t)m + 1);
        if (!rc) rc = grow_owned(ws.flag, 1);
        if (!rc) rc = grow_owned(ws.lims_pin, (size_t)m + 2);
        if (rc) return rc;
        rp.q = ws.q.p;
        rp.cnt = ws.cnt.p;
        rp.sD = ws.sD.p;
        rp.sI = ws.sI.p;
        rp.mode = 0;
        rp.g0 = 0;
        grid = dim3((unsigned)nb, (unsigned)((m + 15) / 16));
        lds = range_lds_bytes(rp.qs_stride);
        HIP_TRY(hipMemsetAsync(ws.flag.p, 0, sizeof(unsigned), st));
        if (sel) ise_launch_range_masked(h->storage == ISE_STORE_BF16, uses_shift(h), ch, grid, lds, st, rp);
        else launch_range(h, ch, grid, lds, st, rp);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(range_offsets_kernel, dim3((unsigned)m), dim3(256), 0, st, ws.cnt.p, rp.nseg, rp.cap,
                       ws.segoff.p, ws.tot.p, ws.flag.p);
    hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(1024), 0, st, ws.tot.p, (int)m, ws.lims.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ws.lims_pin.p, ws.lims.p, (size_t)(m + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ws.lims_pin.p + m + 1, ws.flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the one synchronisation: the total sizes the output
    const long long total = ws.lims_pin.p[m];
    const bool overflow = *reinterpret_cast<const unsigned*>(ws.lims_pin.p + m + 1) != 0;
    if (total > 0) {
        rc = grow_owned(ws.D, (size_t)total);
        if (!rc) rc = grow_owned(ws.I, (size_t)total);
        if (!rc) rc = grow_owned(ws.D_pin, (size_t)total);
        if (!rc) rc = grow_owned(ws.I_pin, (size_t)total);
        if (rc) return rc;
        if (overflow) {  // a segment overflowed: read the index once more, every hit straight to its exact offset
            std::lock_guard<std::mutex> lk(h->mu_);
            rc = prepare_shift_locked(h, st);
            if (rc) return rc;
            if (h->n < n0 || !h->xb) return fail(ISE_E_INVALID, "the index was reset during range_search");
            if (sel) {  // an add since the first pass: the selector no longer names this index's rows
                rc = selector_check_locked(h, sel);
                if (rc) return rc;
            }
            range_params_index(h, &rp);
            rp.mode = 1;
            rp.lims = ws.lims.p;
            rp.segoff = ws.segoff.p;
            rp.D = ws.D.p;
            rp.I = ws.I.p;
            if (sel) ise_launch_range_masked(h->storage == ISE_STORE_BF16, uses_shift(h), ch, grid, lds, st, rp);
            else launch_range(h, ch, grid, lds, st, rp);
            HIP_TRY(hipGetLastError());
        } else {
            hipLaunchKernelGGL(range_compact_kernel, dim3((unsigned)((rp.nseg + 3) / 4), (unsigned)m), dim3(256), 0,
                               st, ws.cnt.p, ws.sD.p, ws.sI.p, ws.lims.p, ws.segoff.p, rp.nseg, rp.cap, ws.D.p, ws.I.p);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(ws.D_pin.p, ws.D.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ws.I_pin.p, ws.I.p, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        r->D.insert(r->D.end(), ws.D_pin.p, ws.D_pin.p + total);
        r->I.insert(r->I.end(), ws.I_pin.p, ws.I_pin.p + total);
    }
    const int64_t base = r->lims.back();
    for (long long i = 1; i <= m; i++) r->lims.push_back(base + ws.lims_pin.p[i]);
    if (sel) h->sel_range_batches++;
    else h->range_batches++;
    if (overflow) h->range_overflows++;
    return ISE_OK;
}

static int range_search_host(ise_index_t* h, const float* q, int64_t nq, float radius, const ise_selector* sel,
                             ise_range_result_t** out) {
    if (!h) return fail(ISE_E_INVALID, "handle is NULL");
    if (!out) return fail(ISE_E_INVALID, "output pointer is NULL");
    *out = nullptr;
    if (nq < 0 || (nq > 0 && !q)) return fail(ISE_E_INVALID, "bad query argument");
    std::unique_ptr<ise_range_result> r(new (std::nothrow) ise_range_result);
    if (!r) return fail(ISE_E_NOMEM, "range result");
    try {
        r->lims.reserve((size_t)nq + 1);
        r->lims.push_back(0);
        if (nq > 0 && h->n > 0) {
            DeviceGuard gd(h->device);
            CtxLease lease(h);
            int rc = lease.stream();
            if (rc) return rc;
            std::lock_guard<std::mutex> lk(h->rg_mu);
            for (long long i0 = 0; i0 < nq && !rc; i0 += RANGE_NQ_CHUNK)
                rc = range_batch(h, lease.c->stream, q + (size_t)i0 * h->d, std::min<long long>(RANGE_NQ_CHUNK, nq - i0), radius, sel,
                                 r.get());
            if (rc) return rc;
        }
        r->lims.resize((size_t)nq + 1, r->lims.back());  // an empty index: every list is empty
    } catch (const std::bad_alloc&) {
        return fail(ISE_E_NOMEM, "range result: host allocation failed");
    }
    *out = r.release();
    return ISE_OK;
}

extern "C" int ise_index_range_search_host(ise_index_t* h, const float* q, int64_t nq, float radius,
                                           ise_range_result_t** out) {
    return range_search_host(h, q, nq, radius, nullptr, out);
}

extern "C" int ise_index_range_search_sel_host(ise_index_t* h, const float* q, int64_t nq, float radius,
                                               const ise_selector_t* sel, ise_range_result_t** out) {
    if (out) *out = nullptr;
    if (!h) return fail(ISE_E_INVALID, "handle is NULL");
    if (!sel) return fail(ISE_E_INVALID, "selector is NULL");
    {
        std::lock_guard<std::mutex> lk(h->mu_);
        const int rc = selector_check_locked(h, sel);  // also when the index is empty or nq == 0
        if (rc) return rc;
    }
    return range_search_host(h, q, nq, radius, sel, out);
}

extern "C" int ise_range_result_get(const ise_range_result_t* r, int64_t* nq, const int64_t** lims, const float** D,
                                    const int64_t** I) {
    if (!r) return fail(ISE_E_INVALID, "result is NULL");
    if (nq) *nq = (int64_t)r->lims.size() - 1;
    if (lims) *lims = r->lims.data();
    if (D) *D = r->D.data();
    if (I) *I = r->I.data();
    return ISE_OK;
}

extern "C" int ise_range_result_destroy(ise_range_result_t* r) {
    delete r;
    return ISE_OK;
}

extern "C" int ise_index_range_stats(ise_index_t* h, uint64_t* out2) {
    if (!h || !out2) return fail(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->rg_mu);
    out2[0] = h->range_batches;
    out2[1] = h->range_overflows;
    return ISE_OK;
}
