// rerank_harness.hip -- test-only launchers around the exact re-rank of csrc/ise_exact.hpp: rerank_kernel (candidates
// in memory, 4 waves) and merge_kernel<true> (candidates merged from lists, 8 waves), so that tests/test_rerank_gpu.py
// can hand them crafted rows, queries and candidate keys.  Built by csrc/Makefile into libise_rerank_check.so; never
// linked into libise_knn.so.  The headers are included as they are: whatever is wrong here is wrong in the product.
//
// Every launcher takes device pointers, launches on the null stream and returns hipGetLastError() as an int.  The
// callers validate the sizes and that every candidate id names a row (tests/test_rerank_gpu.py); the kernels trust them.
#include "ise_common.hpp"
#include "ise_exact.hpp"
#include "ise_merge.hpp"

#define HARNESS_BAD_ARGS ((int)hipErrorInvalidValue)

static bool fill_params(ExactParams& xp, const float* xb, const float* q, long long n, int d, int dp, int nq, int k, int kc,
                        unsigned id_base, float* D, long long* I, u64* keys_out, u64* fl_state, int* fl_list, unsigned seq,
                        const float* tau_bound, int force_fail) {
    if (n < 0 || d <= 0 || dp < d || dp % 4 != 0 || nq <= 0 || k <= 0 || k > kc || kc > 1024 || seq == 0) return false;
    xp = ExactParams();
    xp.xb = xb; xp.q = q; xp.n = n; xp.d = d; xp.dp = dp; xp.nq = nq; xp.k = k; xp.kc = kc; xp.id_base = id_base;
    xp.D = D; xp.I = I; xp.keys_out = keys_out; xp.fl_state = fl_state; xp.fl_list = fl_list; xp.seq = seq;
    xp.stats = nullptr; xp.force_fail = force_fail; xp.tau_bound = tau_bound;
    return true;
}

// rerank_kernel: keys_in [nq][kc] ascending lower-bound keys, KEY_PAD behind
extern "C" int chk_rerank(const float* xb, const float* q, long long n, int d, int dp, int nq, int k, int kc,
                          unsigned id_base, const u64* keys_in, float* D, long long* I, u64* keys_out, u64* fl_state,
                          int* fl_list, unsigned seq, const float* tau_bound, int force_fail) {
    ExactParams xp;
    if (!fill_params(xp, xb, q, n, d, dp, nq, k, kc, id_base, D, I, keys_out, fl_state, fl_list, seq, tau_bound, force_fail))
        return HARNESS_BAD_ARGS;
    hipLaunchKernelGGL(rerank_kernel, dim3((unsigned)nq), dim3(256), rerank_lds_bytes(dp, kc), 0, xp, keys_in);
    return (int)hipGetLastError();
}

// merge_kernel<true>: lists [n_lists][nq][kc] (one query tile of nq queries), each ascending, KEY_PAD behind
extern "C" int chk_merge_rerank(const float* xb, const float* q, long long n, int d, int dp, int nq, int k, int kc,
                                unsigned id_base, const u64* lists, int n_lists, float* D, long long* I, u64* keys_out,
                                u64* fl_state, int* fl_list, unsigned seq, const float* tau_bound, int force_fail) {
    ExactParams xp;
    if (!fill_params(xp, xb, q, n, d, dp, nq, k, kc, id_base, D, I, keys_out, fl_state, fl_list, seq, tau_bound, force_fail))
        return HARNESS_BAD_ARGS;
    if (n_lists <= 0 || n_lists > MERGE_LISTS_MAX) return HARNESS_BAD_ARGS;
    MergeParams mp{};
    mp.lists = lists;
    mp.stride_list = (long long)nq * kc;
    mp.stride_qtile = 0;
    mp.qt = nq;
    mp.n_lists = n_lists;
    mp.nq = nq;
    mp.k = kc;
    mp.metric = ISE_METRIC_L2;
    hipLaunchKernelGGL((merge_kernel<true>), dim3((unsigned)nq), dim3(MERGE_THREADS), rerank_lds_bytes(dp, kc), 0, mp, xp);
    return (int)hipGetLastError();
}
