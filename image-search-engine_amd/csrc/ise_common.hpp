// ise_common.hpp -- types and device utilities shared by the kernels of libise_knn.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/ise_knn.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

#define KEY_PAD (~0ull)
#define TAU0 ((u64)0xFF7FFFFFu << 32) /* ord(FLT_MAX) << 32: strict gate score < FLT_MAX */

// ---------------------------------------------------------------- device utils
__device__ __forceinline__ uint32_t ord_f32(float f) {
    uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t o) {
    uint32_t u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
    return __uint_as_float(u);
}
// float32 L2 with non-finite inputs (Faiss's gate: an L2 score enters only if it is < FLT_MAX).
// nonfinite_mark(x) is 0 for a finite x and NaN for +-inf or NaN.  Added to a partial squared norm (never -0,
// so a finite sum keeps its bits) it makes the shifted norm of a row or query with a non-finite entry NaN:
// every L2 score of such a row is inf or NaN, and a NaN norm keeps its lower bound NaN, so it never becomes a
// candidate.  A non-finite bound from a norm that is not NaN is then an OVERFLOW of finite entries (|y - mu|^2,
// |x - mu|^2 or their sum above FLT_MAX): it bounds nothing, and such a row may still be at a finite direct
// distance, so l2_lower_bound keys it -FLT_MAX -- always a candidate, decided by the direct re-rank (or, when
// every row is keyed so, by the certificate's fallback to the exact scan; ise_exact.hpp).
__device__ __forceinline__ float nonfinite_mark(float x) { return x - x; }
__device__ __forceinline__ float nonfinite_mark(f32x4 x) {
    const f32x4 z = x - x;
    return (z[0] + z[1]) + (z[2] + z[3]);
}
__device__ __forceinline__ float l2_lower_bound(float beta, float tt, float sc) {
    const float lo = fmaf(-beta, tt, sc);
    return (fabsf(lo) <= FLT_MAX || tt != tt) ? lo : -FLT_MAX;
}
// The fp16 shadow-row filter's key (ise_scan.hpp, HALF).  tt = |u~|^2 + |v~|^2 and dot = u~.v~ as
// the kernel has them (dot already scaled back by 2^-(s_r + sh)); e = e_r + e_q.  beta covers every rounding
// between the exact |u~ - v~|^2 and tt - 2 dot relative to tt, 2^-140 the underflow of the scaled terms;
// sqrt(.) (1 - 2^-21) - E is then <= |u~ - v~| - e_r - e_q <= |(x - mu) - (y - mu)|, and shrink takes the
// square below the float32 direct-difference value the verifier computes.  NaN norms (a non-finite entry)
// stay NaN: never a candidate; a bound that overflowed (tt = +inf: |u~|^2 or |v~|^2 beyond FLT_MAX, or a lo that
// did) is keyed -FLT_MAX, as l2_lower_bound does.
__device__ __forceinline__ float half_lower_bound(float beta, float shrink, float tt, float dot, float e) {
    const float dd = fmaf(-beta, tt, tt - 2.f * dot) - 0x1p-140f;
    const float E = fmaf(e, 1.f + 0x1p-20f, 0x1p-126f);
    const float r = sqrtf(fmaxf(dd, 0.f)) * (1.f - 0x1p-21f) - E;
    const float lo = r > 0.f ? fmaxf(r * r * shrink - 0x1p-126f, 0.f) : 0.f;
    if (tt != tt) return tt;
    return (tt <= FLT_MAX && lo <= FLT_MAX) ? lo : -FLT_MAX;
}
// The byte shadow-row filter's key (ise_scan.hpp, BYTE), the expanded form
//   lo = |v|^2 + |y - mu|^2 - 2 v~.u~ - 2 (|v| e_r + |y - mu| e_q + e_r e_q) - beta tt,
// v = x - mu, u~ = c_r q the row's int8 image, v~ the query's two int8 limbs: |v.(y - mu) - v~.u~| <= |v| e_r +
// |u~| e_q and |u~| <= |y - mu| + e_r.  xn, yn are |v|^2 and the row's float32 norm, tt = xn + yn, dot = v~.u~ as
// the kernel has it (scaled back), rv and ry the square roots of xn and yn (raised by 2^-60 against their
// underflow).  beta covers the roundings of xn, yn, dot and of the expression relative to tt, 1 + 2^-10 those of the
// cross terms, 2^-140 the underflow of the scaled terms; shrink takes a positive bound below the float32
// direct-difference value the verifier computes.  Non-finite values as half_lower_bound: a NaN norm stays NaN
// (never a candidate), an overflow (tt or the bound) is keyed -FLT_MAX.
__device__ __forceinline__ float byte_lower_bound(float beta, float shrink, float xn, float yn, float dot, float rv,
                                                  float ry, float er, float eq) {
    const float tt = xn + yn;
    const float E = fmaf(fmaf(rv, er, fmaf(ry, eq, er * eq)), 1.f + 0x1p-10f, 0x1p-126f);
    const float dd = fmaf(-beta, tt, (tt - 2.f * dot) - 2.f * E) - 0x1p-140f;
    const float lo = dd > 0.f ? fmaxf(dd * shrink - 0x1p-126f, 0.f) : dd;
    if (tt != tt) return tt;
    return (tt <= FLT_MAX && fabsf(lo) <= FLT_MAX) ? lo : -FLT_MAX;
}
__device__ __forceinline__ u64 readlane_u64(u64 v, int src) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = (uint32_t)__builtin_amdgcn_readlane((int)lo, src);
    hi = (uint32_t)__builtin_amdgcn_readlane((int)hi, src);
    return ((u64)hi << 32) | lo;
}
template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ u64 min_u64(u64 a, u64 b) { return a < b ? a : b; }
// min over each aligned group of 16 lanes (all lanes of the group get it)
__device__ __forceinline__ u64 row_min_u64(u64 v) {
    v = min_u64(v, dpp_u64<0xB1>(v));   // quad_perm [1,0,3,2]
    v = min_u64(v, dpp_u64<0x4E>(v));   // quad_perm [2,3,0,1]
    v = min_u64(v, dpp_u64<0x141>(v));  // row_half_mirror
    v = min_u64(v, dpp_u64<0x140>(v));  // row_mirror
    return v;
}
// min over the whole wave (all lanes get it)
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
    v = row_min_u64(v);
    const u64 r0 = readlane_u64(v, 0), r1 = readlane_u64(v, 16), r2 = readlane_u64(v, 32),
              r3 = readlane_u64(v, 48);
    return min_u64(min_u64(r0, r1), min_u64(r2, r3));
}
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// makes `dev` the current device for a scope of host code
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set once per (kernel, device),
// race-free (one static LdsAttrOnce per launcher; the launch that follows is ordered behind the set by the mutex)
struct LdsAttrOnce {
    std::atomic<unsigned long long> done{0};  // bit i: set on device i (< 64 devices per process)
    std::mutex mu;
    void ensure(const void* kernel, int bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        const unsigned long long bit = 1ull << dev;
        if (done.load(std::memory_order_acquire) & bit) return;
        std::lock_guard<std::mutex> lk(mu);
        if (done.load(std::memory_order_relaxed) & bit) return;
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
            (void)hipGetLastError();  // a launch that needs the attribute then fails with its own error
        done.fetch_or(bit, std::memory_order_release);
    }
};

// dev builds (-DISE_ABLATE): block 0 / lane 0 stamps the 100 MHz real-time clock into a debug buffer
#ifdef ISE_ABLATE
#define DBG_STAMP(buf, i)                                                                   \
    do {                                                                                    \
        if ((buf) && blockIdx.x == 0 && threadIdx.x == 0) (buf)[(i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define DBG_STAMP(buf, i) do {} while (0)
#endif
