// ise_stage.hpp -- query staging of the shadow-row filters (HALF and BYTE of ise_scan.hpp): one float32 query row
// x becomes the LDS image the MFMAs read (hi | lo limbs of 2^sh (x - mu)) plus |v|^2, e_q and sh.
//
// TPR threads stage one query row.  Two paths, the same per-element arithmetic (shadow_split):
//   vector  (d % 4 == 0, 16-byte aligned queries, the padded row P a multiple of 4 * TPR elements and at most
//           2 * 4 * TPR * SHADOW_QV of them): the caller REQUESTS the first 4 * TPR * SHADOW_QV elements of the row
//           and of mu with 16-byte loads (stage_request_row) before anything else waits on memory; thread t owns the 4
//           adjacent elements of the slots t, t + TPR, ... and everything -- x - mu, max |v|, the TwoSum remainder, the
//           limbs, |v|^2, e_q -- is computed from those registers: rows of up to 512 floats (TPR = 32) are read once.
//           A longer row goes through the same registers in two halves and is read twice (max |v| of half 0, then of
//           half 1; then half 1 again for its limbs, then half 0): 64 VGPRs for a whole row of 1024 would put the
//           one-tile scan kernels over their 128.  The limbs leave as packed 4- or 8-byte LDS stores.
//   scalar  (every other shape): two passes over the row, one element per thread and iteration.
// Summation order of |v|^2 and of e_q's sum of squares: a thread's own elements as one fmaf chain (vector: ascending
// within a half, the upper half first; scalar: ascending), then an xor butterfly over the TPR threads.  Both paths
// run P / TPR fmaf steps per thread: the budgets of beta_8 and beta_h count steps, not their order.
#pragma once
#include "ise_common.hpp"

constexpr int SHADOW_QV = 4;  // 16-byte pieces per staging thread, query row and half (vector path)

// vector path?  P: padded row length in elements (BYTE: dpb, HALF: dph)
__device__ __forceinline__ bool shadow_vec_ok(int d, int P, const float* q, int tpr) {
    return (d & 3) == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0 && P % (4 * tpr) == 0 && P <= 8 * tpr * SHADOW_QV;
}

// request the 16-byte slots j0, j0 + tpr, ... of one row; no wait here, and no branch: every load is issued (a slot
// behind the row's dslots >= 1 re-reads its last one) and the users skip what lies behind the row, so nothing between
// two loads needs a register that one of them fills
template <int QV>
__device__ __forceinline__ void stage_request_row(f32x4 (&v)[QV], const float* src, int j0, int tpr, int dslots) {
#pragma unroll
    for (int i = 0; i < QV; i++) v[i] = *reinterpret_cast<const f32x4*>(src + 4 * min(j0 + i * tpr, dslots - 1));
}

// v = y - m exactly as the float pair (vh, vl) (TwoSum)
__device__ __forceinline__ void shadow_diff(float y, float m, float& vh, float& vl) {
    vh = y - m;
    const float bb = vh - y;
    vl = (y - (vh - bb)) + (-m - bb);
}

// one element: the limbs of 2^sh (vh + vl) as the bits that go to LDS, |v|^2 and the residual's square accumulated.
//   HALF: fp16 hi | lo halves (16 bits each); |v~|^2 is taken of hi + lo
//   BYTE: int8 limbs hi = rint(V / 256), lo = rint(V - 256 hi + 2^sh vl) (8 bits each); |v|^2 is taken of fl(x - mu)
template <bool BYTE>
__device__ __forceinline__ void shadow_split(float vh, float vl, int sh, uint32_t& hbits, uint32_t& lbits, float& sn,
                                             float& e2) {
    const float V = ldexpf(vh, sh), VL = ldexpf(vl, sh);
    if constexpr (BYTE) {
        float h1 = rintf(V * (1.f / 256.f));  // |h1| <= 64
        const float r1 = fmaf(-256.f, h1, V);  // exact
        float l1 = rintf(r1 + VL);              // |l1| <= 128
        const float res = (r1 - l1) + VL;       // r1 - l1 exact
        if (l1 > 127.f) { h1 += 1.f; l1 -= 256.f; }  // the same 256 hi + lo, lo in int8
        hbits = (uint32_t)(int)h1 & 0xFFu;
        lbits = (uint32_t)(int)l1 & 0xFFu;
        sn = fmaf(V, V, sn);
        e2 = fmaf(res, res, e2);
    } else {
        const _Float16 h1 = (_Float16)V;
        const float r1 = V - (float)h1;  // exact
        const _Float16 h2 = (_Float16)(r1 + VL);
        const float res = (r1 - (float)h2) + VL;
        hbits = __builtin_bit_cast(unsigned short, h1);
        lbits = __builtin_bit_cast(unsigned short, h2);
        const float wv = (float)h1 + (float)h2;
        sn = fmaf(wv, wv, sn);
        e2 = fmaf(res, res, e2);
    }
}

// the query's scale exponent: max |V| lands in [2^14, 2^15) (HALF) or [2^13, 2^14) (BYTE)
template <bool BYTE>
__device__ __forceinline__ int shadow_scale_exp(float amax, bool ovf) {
    return (amax > 0.f && !ovf) ? (BYTE ? 13 : 14) - ilogbf(amax) : 0;
}

// butterfly of the two sums over the TPR threads of a row, then thread 0 writes e_q, sh and |v|^2
template <int TPR>
__device__ __forceinline__ void shadow_finish(float sn, float e2, float mark, bool ovf, int sh, int t, float* xn_cc,
                                              float* xe_cc, int* xsh_cc) {
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) {
        sn += __shfl_xor(sn, o);
        e2 += __shfl_xor(e2, o);
    }
    if (t == 0) {
        // scaled units: |V - V~| <= sqrt(e2) up to the rounding of e2 (the margins) and 2^-44 |V| (res)
        const float es = sqrtf(e2 * (1.f + 0x1p-9f)) * (1.f + 0x1p-20f) + 0x1p-44f * sqrtf(sn);
        *xe_cc = ldexpf(es, -sh);
        *xsh_cc = sh;
        // |v|^2: NaN for a non-finite entry (never enters), +inf when x - mu overflowed (keyed -FLT_MAX)
        *xn_cc = mark != 0.f ? mark : (ovf ? INFINITY : ldexpf(sn, -2 * sh));
    }
}

// vector path, first part: max |x - mu| and the non-finite mark of the row, butterflied over its TPR threads.  qv holds
// the slots t, t + TPR, ... of the first half of the query row src (stage_request_row; dslots = d / 4), muv those of mu
// unless mu_stale (a two-half row before this one left other slots there); P4 = P / 4.
template <int TPR>
__device__ __forceinline__ void stage_shadow_vec_scale(f32x4 (&qv)[SHADOW_QV], f32x4 (&muv)[SHADOW_QV], const float* src,
                                                       const float* mu, int dslots, bool rowok, int t, int P4,
                                                       bool mu_stale, float& amax, float& mark) {
    constexpr int H4 = TPR * SHADOW_QV;  // slots per half
    amax = 0.f;
    mark = 0.f;
    auto max_pass = [&](int h) {
#pragma unroll
        for (int i = 0; i < SHADOW_QV; i++)
            if (rowok && h * H4 + t + i * TPR < dslots) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float y = qv[i][e];
                    amax = fmaxf(amax, fabsf(y - muv[i][e]));
                    mark += y - y;  // NaN for a non-finite entry (ise_common.hpp, nonfinite_mark)
                }
            }
    };
    if (P4 > H4) {
        if (mu_stale) stage_request_row(muv, mu, t, TPR, dslots);
        max_pass(0);
        stage_request_row(muv, mu, H4 + t, TPR, dslots);
        stage_request_row(qv, src, H4 + t, TPR, dslots);
        max_pass(1);
    } else {
        max_pass(0);
    }
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o));
        mark += __shfl_xor(mark, o);
    }
}

// vector path, second part: the limbs into LDS (hi and lo point at the row's images, P elements each), then |v|^2, e_q
// and sh.  A one-half row is still in qv / muv; a two-half row is requested again, the upper half first.
template <bool BYTE, int TPR>
__device__ __forceinline__ void stage_shadow_vec_limbs(f32x4 (&qv)[SHADOW_QV], f32x4 (&muv)[SHADOW_QV], const float* src,
                                                       const float* mu, int dslots, bool rowok, int t, int P4, float amax,
                                                       float mark, unsigned char* hi, unsigned char* lo, float* xn_cc,
                                                       float* xe_cc, int* xsh_cc) {
    constexpr int H4 = TPR * SHADOW_QV;
    const bool ovf = !(amax <= FLT_MAX);  // x - mu overflowed: no bound (keyed -FLT_MAX)
    const bool skip = ovf || mark != 0.f;
    const int sh = shadow_scale_exp<BYTE>(amax, ovf);
    float sn = 0.f, e2 = 0.f;
    auto split_pass = [&](int h) {
#pragma unroll
        for (int i = 0; i < SHADOW_QV; i++) {
            const int j4 = h * H4 + t + i * TPR;
            if (j4 < P4) {
                const bool on = rowok && !skip && j4 < dslots;  // zeros behind the row, up to P
                uint32_t hb[4], lb[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float vh, vl;
                    shadow_diff(qv[i][e], muv[i][e], vh, vl);
                    shadow_split<BYTE>(on ? vh : 0.f, on ? vl : 0.f, sh, hb[e], lb[e], sn, e2);
                }
                if constexpr (BYTE) {
                    reinterpret_cast<uint32_t*>(hi)[j4] = hb[0] | (hb[1] << 8) | (hb[2] << 16) | (hb[3] << 24);
                    reinterpret_cast<uint32_t*>(lo)[j4] = lb[0] | (lb[1] << 8) | (lb[2] << 16) | (lb[3] << 24);
                } else {
                    reinterpret_cast<uint2*>(hi)[j4] = make_uint2(hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16));
                    reinterpret_cast<uint2*>(lo)[j4] = make_uint2(lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16));
                }
            }
        }
    };
    if (P4 > H4) {
        stage_request_row(muv, mu, H4 + t, TPR, dslots);
        stage_request_row(qv, src, H4 + t, TPR, dslots);
        split_pass(1);
        stage_request_row(muv, mu, t, TPR, dslots);
        stage_request_row(qv, src, t, TPR, dslots);
        split_pass(0);
    } else {
        split_pass(0);  // no memory wait on this path
    }
    shadow_finish<TPR>(sn, e2, mark, ovf, sh, t, xn_cc, xe_cc, xsh_cc);
}

// scalar path: two passes over the query row (the scale needs max |v| first), one element per thread and iteration
template <bool BYTE, int TPR>
__device__ __forceinline__ void stage_shadow_scalar(const float* src, const float* mu, int d, int P, bool rowok, int t,
                                                    unsigned char* hi, unsigned char* lo, float* xn_cc, float* xe_cc,
                                                    int* xsh_cc) {
    float amax = 0.f, mark = 0.f;
    if (rowok)
        for (int j = t; j < d; j += TPR) {
            const float y = src[j];
            amax = fmaxf(amax, fabsf(y - mu[j]));
            mark += y - y;  // NaN for a non-finite entry (ise_common.hpp, nonfinite_mark)
        }
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o));
        mark += __shfl_xor(mark, o);
    }
    const bool ovf = !(amax <= FLT_MAX);  // x - mu overflowed: no bound (keyed -FLT_MAX)
    const bool skip = ovf || mark != 0.f;
    const int sh = shadow_scale_exp<BYTE>(amax, ovf);
    float sn = 0.f, e2 = 0.f;
    for (int j = t; j < P; j += TPR) {
        float vh = 0.f, vl = 0.f;
        if (rowok && j < d && !skip) shadow_diff(src[j], mu[j], vh, vl);
        uint32_t hb, lb;
        shadow_split<BYTE>(vh, vl, sh, hb, lb, sn, e2);
        if constexpr (BYTE) {
            hi[j] = (unsigned char)hb;
            lo[j] = (unsigned char)lb;
        } else {
            reinterpret_cast<unsigned short*>(hi)[j] = (unsigned short)hb;
            reinterpret_cast<unsigned short*>(lo)[j] = (unsigned short)lb;
        }
    }
    shadow_finish<TPR>(sn, e2, mark, ovf, sh, t, xn_cc, xe_cc, xsh_cc);
}

// One query row through the staging on its own (ise_index_stage_query_debug; tests only): one block of 32 threads.
// out_limbs: hi then lo, P elements each (1 byte: int8, 2 bytes: fp16 bits); out_f: |v|^2, e_q; out_i: sh, vector path?
template <bool BYTE>
__global__ __launch_bounds__(32) void stage_debug_kernel(const float* q, const float* mu, int d, int P,
                                                          unsigned char* out_limbs, float* out_f, int* out_i) {
    constexpr int TPR = 32, ES = BYTE ? 1 : 2;
    __shared__ __align__(16) unsigned char img[2 * 1024 * ES];
    __shared__ float xn1, xe1;
    __shared__ int xsh1;
    const int t = threadIdx.x;
    const bool vec = shadow_vec_ok(d, P, q, TPR);
    if (vec) {
        f32x4 qv[SHADOW_QV], muv[SHADOW_QV];
        stage_request_row(muv, mu, t, TPR, d >> 2);
        stage_request_row(qv, q, t, TPR, d >> 2);
        float amax, mark;
        stage_shadow_vec_scale<TPR>(qv, muv, q, mu, d >> 2, true, t, P >> 2, false, amax, mark);
        stage_shadow_vec_limbs<BYTE, TPR>(qv, muv, q, mu, d >> 2, true, t, P >> 2, amax, mark, img, img + P * ES, &xn1, &xe1, &xsh1);
    } else {
        stage_shadow_scalar<BYTE, TPR>(q, mu, d, P, true, t, img, img + P * ES, &xn1, &xe1, &xsh1);
    }
    __syncthreads();
    for (int i = t; i < 2 * P * ES; i += TPR) out_limbs[i] = img[i];
    if (t == 0) {
        out_f[0] = xn1;
        out_f[1] = xe1;
        out_i[0] = xsh1;
        out_i[1] = vec ? 1 : 0;
    }
}
