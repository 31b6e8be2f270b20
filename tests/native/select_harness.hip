// select_harness.hip -- test-only launchers around the selection and merge primitives of csrc/ (ise_select.hpp,
// ise_merge.hpp, ise_cand.hpp), so that tests/test_select_gpu.py can hand them crafted key sets and know which lane,
// register, wave and list every key sits in.  Built by csrc/Makefile into libise_select_check.so; never linked into
// libise_knn.so.  The headers are included as they are: whatever is wrong here is wrong in the product.
//
// Every launcher takes device pointers, launches on the null stream and returns hipGetLastError() as an int.  One
// block (or wave) serves one CASE, blockIdx.x = case: a few hundred cases cost one launch.  The callers validate the
// sizes (tests/test_select_gpu.py, the wrappers at its top); the kernels trust them.
#include "ise_common.hpp"
#include "ise_select.hpp"
#include "ise_merge.hpp"
#include "ise_cand.hpp"
#include "ise_pq.hpp"
#include "ise_sq.hpp"
// last: its CAP macro (a scan wave's private list) is also the name of a template parameter of CandBuf
#include "ise_scan_params.hpp"

#define HARNESS_BAD_VARIANT ((int)hipErrorInvalidValue)

// ---------------------------------------------------------------- wave_select / wave_cut: one wave per case
// in [case][64 KPL], dst [case][64 KPL + 8]; dst, nw, kth / cnt, cut arrive filled with the caller's sentinel
template <int KPL>
__global__ __launch_bounds__(64) void sel_kernel(const u64* in, const int* n, const int* k, u64* dst, int* nw, u64* kth) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int nn = __builtin_amdgcn_readfirstlane(n[c]), kv = __builtin_amdgcn_readfirstlane(k[c]);
    u64 kk[KPL];
#pragma unroll
    for (int e = 0; e < KPL; e++) kk[e] = 64 * e < nn ? in[(size_t)c * 64 * KPL + lane + 64 * e] : KEY_PAD;
    const int w = wave_select<KPL>(kk, nn, kv, dst + (size_t)c * (64 * KPL + 8), kth + c);
    if (lane == 0) nw[c] = w;
}

template <int KPL>
__global__ __launch_bounds__(64) void cut_kernel(const u64* in, const int* n, const int* kmin, const int* kmax, u64* dst,
                                                 int* cnt, u64* cut) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int nn = __builtin_amdgcn_readfirstlane(n[c]);
    const int lo = __builtin_amdgcn_readfirstlane(kmin[c]), hi = __builtin_amdgcn_readfirstlane(kmax[c]);
    u64 kk[KPL];
#pragma unroll
    for (int e = 0; e < KPL; e++) kk[e] = 64 * e < nn ? in[(size_t)c * 64 * KPL + lane + 64 * e] : KEY_PAD;
    const int w = wave_cut<KPL>(kk, nn, lo, hi, dst + (size_t)c * (64 * KPL + 8), cut + c);
    if (lane == 0) cnt[c] = w;
}

extern "C" int chk_sel(int kpl, int ncases, const u64* in, const int* n, const int* k, u64* dst, int* nw, u64* kth) {
    if (ncases <= 0) return HARNESS_BAD_VARIANT;
#define GO(K) hipLaunchKernelGGL(sel_kernel<K>, dim3(ncases), dim3(64), 0, 0, in, n, k, dst, nw, kth)
    switch (kpl) {
        case 1: GO(1); break;
        case 2: GO(2); break;
        case 4: GO(4); break;
        case 5: GO(5); break;
        case 8: GO(8); break;
        case 16: GO(16); break;
        default: return HARNESS_BAD_VARIANT;
    }
#undef GO
    return (int)hipGetLastError();
}

extern "C" int chk_cut(int kpl, int ncases, const u64* in, const int* n, const int* kmin, const int* kmax, u64* dst,
                       int* cnt, u64* cut) {
    if (ncases <= 0) return HARNESS_BAD_VARIANT;
#define GO(K) hipLaunchKernelGGL(cut_kernel<K>, dim3(ncases), dim3(64), 0, 0, in, n, kmin, kmax, dst, cnt, cut)
    switch (kpl) {
        case 1: GO(1); break;
        case 2: GO(2); break;
        case 4: GO(4); break;
        default: return HARNESS_BAD_VARIANT;
    }
#undef GO
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- block_topk_u64: 256 threads per case
// in [case][in_stride] (n[case] <= in_stride <= 4096 keys read), out [case][64]: out[0 .. k) written
#define TOPK_N_MAX 4096
#define TOPK_K_MAX 64
__global__ __launch_bounds__(256) void topk_kernel(const u64* in, int in_stride, const int* n, const int* k, u64* out) {
    extern __shared__ __align__(16) unsigned char smem_tk[];
    u64* list = reinterpret_cast<u64*>(smem_tk);  // [TOPK_N_MAX]
    u64* stage = list + TOPK_N_MAX;               // [4][TOPK_K_MAX]
    u64* res = stage + 4 * TOPK_K_MAX;            // [TOPK_K_MAX]
    const int c = blockIdx.x, nn = n[c], kv = k[c];
    for (int i = threadIdx.x; i < nn; i += 256) list[i] = in[(size_t)c * in_stride + i];
    __syncthreads();
    block_topk_u64(list, nn, kv, stage, res);
    if ((int)threadIdx.x < kv) out[(size_t)c * TOPK_K_MAX + threadIdx.x] = res[threadIdx.x];
}

extern "C" int chk_topk(int ncases, const u64* in, int in_stride, const int* n, const int* k, u64* out) {
    if (ncases <= 0 || in_stride < 0 || in_stride > TOPK_N_MAX) return HARNESS_BAD_VARIANT;
    const size_t lds = (size_t)(TOPK_N_MAX + 5 * TOPK_K_MAX) * sizeof(u64);
    hipLaunchKernelGGL(topk_kernel, dim3(ncases), dim3(256), lds, 0, in, in_stride, n, k, out);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- merge_waves: MERGE_THREADS per case
// lists [case][n_lists][k] (stride_list = k: a list is read up to its k-th slot), res [case][MERGE_FAST_K]: res[0 .. k)
// written, and the block's need_full flag -- which of merge_waves' two paths ran
__global__ __launch_bounds__(MERGE_THREADS) void mwaves_kernel(const MergeParams p, long long case_stride, u64* res_out,
                                                              int* need_full) {
    __shared__ MergeFastScratch fast;
    __shared__ u64 res[MERGE_FAST_K];
    const int c = blockIdx.x;
    merge_waves(p, p.lists + (size_t)c * case_stride, fast, res);
    const int t = threadIdx.x;
    if (t < p.k) res_out[(size_t)c * MERGE_FAST_K + t] = res[t];
    if (t == 0) need_full[c] = fast.need_full;
}

extern "C" int chk_mwaves(int ncases, const u64* lists, int n_lists, int k, u64* res, int* need_full) {
    if (ncases <= 0 || n_lists <= 0 || n_lists > MERGE_LISTS_MAX || k <= 0 || k > MERGE_FAST_K) return HARNESS_BAD_VARIANT;
    MergeParams mp{};
    mp.lists = lists;
    mp.stride_list = k;
    mp.qt = 1;
    mp.n_lists = n_lists;
    mp.nq = ncases;
    mp.k = k;
    hipLaunchKernelGGL(mwaves_kernel, dim3(ncases), dim3(MERGE_THREADS), 0, 0, mp, (long long)n_lists * k, res, need_full);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- pass_merge_kernel<float | int> itself
// lists [n_lists][qt][kpass], as a coded scan's blocks leave them; D, I [nqt][k], lo [nqt]
template <class T>
static int pass_merge_go(const u64* lists, int qt, int kpass, int n_lists, int nqt, int kp, T* D, long long* I, u64* lo,
                         int k, int off, int ip) {
    if (n_lists <= 0 || n_lists > MERGE_LISTS_MAX || nqt <= 0 || nqt > qt || kp <= 0 || kp > kpass || kp > MERGE_FAST_K ||
        off < 0 || off + kp > k)
        return HARNESS_BAD_VARIANT;
    MergeParams mp{};
    mp.lists = lists;
    mp.stride_list = (long long)qt * kpass;
    mp.stride_qtile = 0;
    mp.stride_query = kpass;
    mp.qt = qt;
    mp.n_lists = n_lists;
    mp.nq = nqt;
    mp.k = kp;
    const PassOut<T> mo{D, I, lo, k, off, ip};
    hipLaunchKernelGGL(pass_merge_kernel<T>, dim3((unsigned)nqt), dim3(MERGE_THREADS), 0, 0, mp, mo);
    return (int)hipGetLastError();
}
extern "C" int chk_pass_merge_f32(const u64* lists, int qt, int kpass, int n_lists, int nqt, int kp, float* D, long long* I,
                                  u64* lo, int k, int off, int ip) {
    return pass_merge_go<float>(lists, qt, kpass, n_lists, nqt, kp, D, I, lo, k, off, ip);
}
extern "C" int chk_pass_merge_i32(const u64* lists, int qt, int kpass, int n_lists, int nqt, int kp, int* D, long long* I,
                                  u64* lo, int k, int off, int ip) {
    return pass_merge_go<int>(lists, qt, kpass, n_lists, nqt, kp, D, I, lo, k, off, ip);
}

// ---------------------------------------------------------------- merge_kernel<false> with the caller's layout
// query lq reads list l at lists + (lq / qt) stride_qtile + (lq % qt) k + l stride_list; keys_out, D, I [nq][k]
extern "C" int chk_merge(const u64* lists, long long stride_list, long long stride_qtile, int qt, int n_lists, int nq, int k,
                         int metric, u64* keys_out, float* D, long long* I) {
    if (n_lists <= 0 || n_lists > MERGE_LISTS_MAX || nq <= 0 || k <= 0 || qt <= 0) return HARNESS_BAD_VARIANT;
    MergeParams mp{};
    mp.lists = lists;
    mp.stride_list = stride_list;
    mp.stride_qtile = stride_qtile;
    mp.qt = qt;
    mp.n_lists = n_lists;
    mp.nq = nq;
    mp.k = k;
    mp.metric = metric;
    mp.D = D;
    mp.I = I;
    mp.keys_out = keys_out;
    hipLaunchKernelGGL((merge_kernel<false>), dim3((unsigned)nq), dim3(MERGE_THREADS), 0, 0, mp, ExactParams());
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- CandBuf: one 4-wave block per case
// keys [case][nqt][ntiles * 64]: wave w streams tiles w, w + 4, ..; lane i of a tile offers key [q][64 t + i] to query
// q, KEY_PAD = the lane is invalid (a partial tile).  lo [case][QT], lists [case][QT][KPASS].
// The append loop is the harness's own, copied from pq_scan_kernel (key >= lo && key < thr, ballot-prefix slot, the
// count kept in the lanes of the query's column).  What is under test is cut, make_room, fold and the buffer contract:
// a tile's appends fit behind the kept keys, and lane q carries query q whether col is the lane (PqCand) or lane & 15
// (SqCand, COL16).
template <class Cand, int QT, int KPASS, bool COL16>
__global__ __launch_bounds__(PQ_WAVES * 64) void cand_kernel(const u64* keys, int ntiles, int nqt, int kp, const u64* lo,
                                                             u64* lists) {
    extern __shared__ __align__(16) unsigned char smem_cd[];
    u64* buf = reinterpret_cast<u64*>(smem_cd);  // [WAVES][QT][CAP]
    const int cs = blockIdx.x;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    Cand cand(buf, w, COL16 ? (lane & 15) : lane, kp);
    const u64 lo_v = lane < nqt ? lo[(size_t)cs * QT + lane] : KEY_PAD;
    const u64 lt_mask = (1ull << lane) - 1ull;
    const u64* src = keys + (size_t)cs * nqt * ntiles * 64;
    for (int t = w; t < ntiles; t += PQ_WAVES) {
#pragma unroll
        for (int q = 0; q < QT; q++) {
            if (q < nqt) {
                const u64 key = src[((size_t)q * ntiles + t) * 64 + lane];
                const bool c = key != KEY_PAD && key >= readlane_u64(lo_v, q) && key < readlane_u64(cand.thr, q);
                const u64 mk = __ballot(c);
                if (mk) {
                    const int cnt = __builtin_amdgcn_readlane(cand.cnt, q);
                    if (c) cand.keys(q)[cnt + __popcll(mk & lt_mask)] = key;
                    if (cand.col == q) cand.cnt += __popcll(mk);
                }
            }
        }
        cand.make_room();
    }
    cand.fold(nqt, lists + (size_t)cs * QT * KPASS);
}

static_assert(PQ_WAVES == SQ_WAVES && PQ_CAP == SQ_CAP, "one block shape serves both kinds' buffers");

// which: 0 = PqCand<16>, 1 = PqCand<2>, 2 = SqCand<16>, 3 = SqCand<8>
extern "C" int chk_cand(int which, int ncases, const u64* keys, int ntiles, int nqt, int kp, const u64* lo, u64* lists) {
    static LdsAttrOnce attr[4];
    if (ncases <= 0 || ntiles < 0 || nqt <= 0 || kp <= 0) return HARNESS_BAD_VARIANT;
    auto go = [&](auto kern, LdsAttrOnce& a, int qt, int kpass) -> int {
        if (nqt > qt || kp > kpass) return HARNESS_BAD_VARIANT;
        a.ensure(reinterpret_cast<const void*>(kern), LDS_LIMIT);
        const size_t lds = (size_t)PQ_WAVES * qt * PQ_CAP * sizeof(u64);
        hipLaunchKernelGGL(kern, dim3(ncases), dim3(PQ_WAVES * 64), lds, 0, keys, ntiles, nqt, kp, lo, lists);
        return (int)hipGetLastError();
    };
    switch (which) {
        case 0: return go(cand_kernel<PqCand<16>, 16, PQ_KPASS, false>, attr[0], 16, PQ_KPASS);
        case 1: return go(cand_kernel<PqCand<2>, 2, PQ_KPASS, false>, attr[1], 2, PQ_KPASS);
        case 2: return go(cand_kernel<SqCand<16>, 16, SQ_KPASS, true>, attr[2], 16, SQ_KPASS);
        case 3: return go(cand_kernel<SqCand<8>, 8, SQ_KPASS, true>, attr[3], 8, SQ_KPASS);
        default: return HARNESS_BAD_VARIANT;
    }
}
