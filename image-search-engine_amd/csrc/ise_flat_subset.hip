// ise_flat_subset.hip -- the float index's subset scoring (ise_subset.hpp; ise_flat.hpp: the handle).
#include "ise_flat.hpp"
#include "ise_pass_host.hpp"
#include "ise_sel_scan.hpp"
#include "ise_subset.hpp"

// ---- subset scoring (ise_subset.hpp): exact scores of per-query candidate lists, and their k best
#define SUBSET_NQ_CHUNK 4096 /* queries per pair of launches (grid.y) and per staging round of the host forms */

static int check_subset_args(const ise_index* h, const void* q, long long nq, const void* cand, int kc) {
    if (!h) return fail(ISE_E_INVALID, "handle is NULL");
    if (h->storage != ISE_STORE_F32) return fail(ISE_E_INVALID, "subset scoring needs float32 rows (this index keeps bf16)");
    if (nq < 0 || nq > (1ll << 20)) return fail(ISE_E_INVALID, "nq must be in [0, 2^20]");
    if (kc < 1 || kc > ISE_MAX_K) return fail(ISE_E_INVALID, "kc (candidates per query) must be in [1, 2048]");
    if (nq > 0 && (!q || !cand)) return fail(ISE_E_INVALID, "query or candidate pointer is NULL");
    return ISE_OK;
}

// mu_ held.  Enqueues only (it waits on the host only where the key workspace has to grow, and once for the counter's
// allocation).  D_dev / I_dev ([nq][k]) and / or dist_dev ([nq][kc])
static int subset_enqueue(ise_index* h, const float* q_dev, long long nq, int k, const long long* cand_dev, int kc,
                          float* D_dev, long long* I_dev, float* dist_dev, hipStream_t st) {
    auto& sb = h->sub;
    const int ip = h->metric == ISE_METRIC_INNER_PRODUCT;
    if (!sb.order.ev) HIP_TRY(sb.order.create());
    int rc = sb.order.wait(st);
    if (rc) return rc;
    if (h->n == 0) {  // nothing to score: padding, no score launch
        sb.batches++;
        if (D_dev) {
            knn_fill_launch(D_dev, I_dev, nq * k, h->metric != ISE_METRIC_L2, st);
        }
        if (dist_dev) {
            const long long tot = nq * kc;
            hipLaunchKernelGGL(subset_fill_dist_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, dist_dev, tot, ip);
        }
    } else {
        const int n2 = rerank_pow2(kc);
        const long long chunk = std::min<long long>(nq, SUBSET_NQ_CHUNK);
        if (D_dev && (rc = grow_drained_exact(sb.keys, (size_t)chunk * n2))) return rc;
        if (!sb.valid.p) {
            if ((rc = buf_realloc(sb.valid, 1))) return rc;
            // on the call's stream: a plain hipMemset of device memory may return before it has run, and this stream
            // does not wait for the null stream
            HIP_TRY(hipMemsetAsync(sb.valid.p, 0, sizeof(unsigned long long), st));
        }
        sb.batches++;  // counted once the batch is certain to be enqueued
        SubsetParams sp{};
        sp.xb = static_cast<const float*>(h->xb);
        sp.n = h->n; sp.d = h->d; sp.dp = h->dp; sp.kc = kc; sp.n2 = n2; sp.ip = ip;
        sp.valid = sb.valid.p;
        const unsigned gx = (unsigned)((n2 + SUB_CPB - 1) / SUB_CPB);
        const size_t lds = (size_t)h->dp * sizeof(float);  // at most 8 KiB + padding for d <= 2048; far below the default limit
        const int sort_threads = std::min(SUB_SORT_MAX_THREADS, std::max(64, n2 / 2));
        for (long long i0 = 0; i0 < nq; i0 += SUBSET_NQ_CHUNK) {
            const long long m = std::min<long long>(SUBSET_NQ_CHUNK, nq - i0);
            sp.q = q_dev + (size_t)i0 * h->d;
            sp.cand = cand_dev + (size_t)i0 * kc;
            sp.keys = D_dev ? sb.keys.p : nullptr;
            sp.dist = dist_dev ? dist_dev + (size_t)i0 * kc : nullptr;
            const dim3 grid(gx, (unsigned)m);
            if (ip) hipLaunchKernelGGL(subset_score_ip_kernel, grid, dim3(64), lds, st, sp);
            else hipLaunchKernelGGL(subset_score_l2_kernel, grid, dim3(SUB_W * 64), lds, st, sp);
            sb.launches++;
            if (D_dev)
                hipLaunchKernelGGL(subset_select_kernel, dim3((unsigned)m), dim3(sort_threads), subset_select_lds_bytes(n2), st,
                                   (const u64*)sb.keys.p, n2, k, ip, D_dev + (size_t)i0 * k, I_dev + (size_t)i0 * k);
        }
    }
    HIP_TRY(hipGetLastError());
    return sb.order.mark(st);
}

extern "C" int ise_index_search_subset_device(ise_index_t* h, const float* q_dev, int64_t nq, int k, const int64_t* cand_dev,
                                              int kc, float* D_dev, int64_t* I_dev, void* stream) {
    int rc = check_subset_args(h, q_dev, nq, cand_dev, kc);
    if (rc) return rc;
    if (k < 1 || k > ISE_MAX_K) return fail(ISE_E_INVALID, "k must be in [1, 2048]");
    if (nq > 0 && (!D_dev || !I_dev)) return fail(ISE_E_INVALID, "output pointer is NULL");
    if (nq == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    return subset_enqueue(h, q_dev, nq, k, (const long long*)cand_dev, kc, D_dev, (long long*)I_dev, nullptr,
                          (hipStream_t)stream);
}

extern "C" int ise_index_distance_subset_device(ise_index_t* h, const float* q_dev, int64_t nq, const int64_t* cand_dev, int kc,
                                                float* dist_dev, void* stream) {
    int rc = check_subset_args(h, q_dev, nq, cand_dev, kc);
    if (rc) return rc;
    if (nq > 0 && !dist_dev) return fail(ISE_E_INVALID, "output pointer is NULL");
    if (nq == 0) return ISE_OK;
    std::lock_guard<std::mutex> lk(h->mu_);
    DeviceGuard gd(h->device);
    return subset_enqueue(h, q_dev, nq, 0, (const long long*)cand_dev, kc, nullptr, nullptr, dist_dev, (hipStream_t)stream);
}

// the host forms: SUBSET_NQ_CHUNK queries at a time are copied in, enqueued under mu_, copied out and waited for.
// k == 0: the scores (dist [nq][kc]); else D / I [nq][k]
static int subset_host(ise_index* h, const float* q, long long nq, int k, const long long* cand, int kc, float* D,
                       long long* I, float* dist) {
    std::lock_guard<std::mutex> lk(h->sub.mu);
    DeviceGuard gd(h->device);
    auto& sb = h->sub;
    hipStream_t st = h->stream;
    const long long batch = std::min<long long>(nq, SUBSET_NQ_CHUNK);
    const int width = dist ? kc : k;
    int rc = grow_drained_exact(sb.q, (size_t)batch * h->d);
    if (!rc) rc = grow_drained_exact(sb.cand, (size_t)batch * kc);
    if (!rc) rc = grow_drained_exact(sb.out, (size_t)batch * width);
    if (!rc && !dist) rc = grow_drained_exact(sb.I, (size_t)batch * k);
    if (rc) return rc;
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        HIP_TRY(hipMemcpyAsync(sb.q.p, q + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sb.cand.p, cand + (size_t)i0 * kc, (size_t)m * kc * sizeof(long long), hipMemcpyHostToDevice, st));
        {
            std::lock_guard<std::mutex> lk2(h->mu_);
            rc = subset_enqueue(h, sb.q.p, m, k, sb.cand.p, kc, dist ? nullptr : sb.out.p, dist ? nullptr : sb.I.p,
                                dist ? sb.out.p : nullptr, st);
        }
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync((dist ? dist : D) + (size_t)i0 * width, sb.out.p, (size_t)m * width * sizeof(float),
                               hipMemcpyDeviceToHost, st));
        if (!dist)
            HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, sb.I.p, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_index_search_subset_host(ise_index_t* h, const float* q, int64_t nq, int k, const int64_t* cand, int kc,
                                            float* D, int64_t* I) {
    int rc = check_subset_args(h, q, nq, cand, kc);
    if (rc) return rc;
    if (k < 1 || k > ISE_MAX_K) return fail(ISE_E_INVALID, "k must be in [1, 2048]");
    if (nq > 0 && (!D || !I)) return fail(ISE_E_INVALID, "output pointer is NULL");
    if (nq == 0) return ISE_OK;
    return subset_host(h, q, nq, k, (const long long*)cand, kc, D, (long long*)I, nullptr);
}

extern "C" int ise_index_distance_subset_host(ise_index_t* h, const float* q, int64_t nq, const int64_t* cand, int kc,
                                              float* dist) {
    int rc = check_subset_args(h, q, nq, cand, kc);
    if (rc) return rc;
    if (nq > 0 && !dist) return fail(ISE_E_INVALID, "output pointer is NULL");
    if (nq == 0) return ISE_OK;
    return subset_host(h, q, nq, 0, (const long long*)cand, kc, nullptr, nullptr, dist);
}

extern "C" int ise_index_subset_stats(ise_index_t* h, uint64_t* out3) {
    if (!h || !out3) return fail(ISE_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu_);
    out3[0] = h->sub.batches;
    out3[1] = h->sub.launches;
    out3[2] = 0;
    if (h->sub.valid.p) {  // counted on the device: wait for the passes in flight
        DeviceGuard gd(h->device);
        HIP_TRY(hipDeviceSynchronize());
        unsigned long long v = 0;
        HIP_TRY(hipMemcpy(&v, h->sub.valid.p, sizeof(v), hipMemcpyDeviceToHost));
        out3[2] = v;
    }
    return ISE_OK;
}
