// ise_pass_host.hpp -- host side of what the coded index kinds share (binary, product-quantised, scalar-quantised and the
// inverted lists over 8-bit rows): the growth of the code storage, the grid rule of a pass, and the two launches of a
// search that do not depend on the codec -- the merge half of a k-pass and the fill of an index with nothing to rank.
// Host code only; the handle's mutex is held.
#pragma once
#include "ise_host.hpp"
#include "ise_merge.hpp"

// Room for `need` rows in *rows ([*cap][rb] bytes, n of them in use) and, where the kind has one, in a second per-row
// array *side ([*cap] elements of sb bytes): geometric growth on re-add, *cap a multiple of `round` rows, the rows
// behind n zero.  Blocks when it grows: searches in flight still read the old storage.
template <class T, class S = unsigned char>
int reserve_code_rows(T** rows, size_t rb, long long n, long long* cap, long long need, long long round, hipStream_t st,
                      S** side = nullptr, size_t sb = 0) {
    if (need <= *cap) return ISE_OK;
    long long want = need;
    if (*cap > 0 && want < *cap + *cap / 2) want = *cap + *cap / 2;  // geometric growth on re-add
    want = (want + round - 1) / round * round;
    char *nx = nullptr, *ns = nullptr;  // typed locals, handed back below: no caller's pointer is written through void**
    HIP_TRY(hipMalloc((void**)&nx, (size_t)want * rb));
    hipError_t e = side ? hipMalloc((void**)&ns, (size_t)want * sb) : hipSuccess;
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(nx, *rows, (size_t)n * rb, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && n > 0 && side) e = hipMemcpyAsync(ns, *side, (size_t)n * sb, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(nx + (size_t)n * rb, 0, (size_t)(want - n) * rb, st);
    if (e == hipSuccess && side) e = hipMemsetAsync(ns + (size_t)n * sb, 0, (size_t)(want - n) * sb, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && *rows) e = hipDeviceSynchronize();  // searches in flight still read the old storage
    if (e != hipSuccess) {
        (void)hipFree(nx);
        if (ns) (void)hipFree(ns);
        return ise_fail_(e == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP,
                         std::string("growing the code storage: ") + hipGetErrorString(e));
    }
    if (*rows) (void)hipFree(*rows);
    if (side && *side) (void)hipFree(*side);
    *rows = reinterpret_cast<T*>(nx);
    if (side) *side = reinterpret_cast<S*>(ns);
    *cap = want;
    return ISE_OK;
}

// blocks of a pass over `tiles` wave tiles: about tiles_per_wave per wave on a short index, at most what the CUs hold at
// once (blocks_per_cu: the kernel's LDS or a cap of the kind's own) and the merge's list count
inline unsigned coded_grid(long long tiles, int tiles_per_wave, int waves, long long blocks_per_cu, int num_cu) {
    const long long per_block = (long long)tiles_per_wave * waves;
    long long g = (tiles + per_block - 1) / per_block;
    g = std::min<long long>(g, std::min<long long>(blocks_per_cu * num_cu, MERGE_LISTS_MAX));
    return (unsigned)std::max<long long>(g, 1);
}

// the merge half of a k-pass: the `grid` blocks' lists ([grid][qt][kpass]) of nqt queries -> positions [off, off + kp) of
// their k results at D, I and the floor keys of the next pass at lo
template <class T>
void pass_merge_launch(u64* lists, int qt, int kpass, unsigned grid, int nqt, int kp, T* D, long long* I, u64* lo, int k, int off,
                       int ip, hipStream_t st) {
    MergeParams mp{};
    mp.lists = lists;
    mp.stride_list = (long long)qt * kpass;
    mp.stride_qtile = 0;
    mp.stride_query = kpass;
    mp.qt = qt;
    mp.n_lists = (int)grid;
    mp.nq = nqt;
    mp.k = kp;
    const PassOut<T> mo{D, I, lo, k, off, ip};
    hipLaunchKernelGGL(pass_merge_kernel<T>, dim3((unsigned)nqt), dim3(MERGE_THREADS), 0, st, mp, mo);
}

// cnt unfilled results at D, I (knn_fill_kernel reads D, I and ip of its PassOut only)
template <class T>
void knn_fill_launch(T* D, long long* I, long long cnt, int ip, hipStream_t st) {
    const PassOut<T> o{D, I, nullptr, 0, 0, ip};
    hipLaunchKernelGGL(knn_fill_kernel<T>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, o, cnt);
}
