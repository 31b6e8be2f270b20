// ise_linear.hpp -- kernels of the linear transform y = A x + b (ise_linear_*): PCA, OPQ and rotation
// matrices in front of an index.  Two launch shapes with ONE arithmetic (include/ise_knn.h): k in segments of LIN_KSEG,
// each segment a k-ascending fmaf chain from +0 -- 64 v_mfma_f32_16x16x4_f32 in a row on one accumulator, which is
// bit for bit that chain -- and the segments added to the bias in ascending order by float32 adds.  The matrix is read
// from the panels of ise_linear_plan.hpp: one coalesced 256-byte load per MFMA, no LDS.  The rows are the other
// operand: lane (c = l & 15, g = l >> 4) supplies x[row c][4 t + g] to k step t.
//   few rows (n <= ISE_LINEAR_FEW_ROWS): a block owns 16 outputs, each of its waves one segment (rows straight from
//     global memory), and the block adds the segments in order through LDS.  At 2048 -> 256: 16 blocks x 8 waves.
//   many rows: a block owns 64 rows x up to 128 outputs; a segment of its rows is staged in LDS (16-byte loads where
//     the pointer and d_in allow, 4-byte loads otherwise), each of its 4 waves runs 4 row tiles x 2 output tiles = 8
//     independent chains, and folds them into the output registers at the segment's end: one add per accumulator.
// No atomics, no scratch in global memory, no order between blocks.
#pragma once
#include "ise_common.hpp"
#include "ise_linear_plan.hpp"

#define LIN_ROWS 64       /* rows of a tiled block, and the most rows of a few-row launch: 4 row tiles */
#define LIN_XT 4          /* row tiles of a block */
#define LIN_OT 2          /* output tiles of a wave of the tiled kernel */
#define LIN_WAVES 4       /* waves of a tiled block */
#define LIN_XS (LIN_KSEG + 4) /* LDS row stride in floats: lanes (c, g) of one read fall into 64 different banks */
#define LIN_TILED_LDS (LIN_ROWS * LIN_XS * (int)sizeof(float))

struct LinearParams {
    const float* x;      // [n][d_in], rows 4-byte aligned
    const float* panel;  // ise_linear_plan.hpp
    const float* bias;   // [jtiles * 16], zeros without a bias
    float* y;            // [n][d_out]
    long long n;
    int d_in, d_out, nseg, ksteps, jtiles;
};

// grid: jtiles blocks of nseg waves; NT = ceil(n / 16) row tiles, LDS: nseg * NT * 256 floats
template <int NT>
__global__ __launch_bounds__(1024) void linear_few_kernel(const LinearParams p) {
    extern __shared__ __align__(16) float part[];  // [nseg][NT][4 regs][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63, s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int jt = blockIdx.x;
    const float* pb = p.panel + ((size_t)jt * p.ksteps + (size_t)s * (LIN_KSEG / LIN_KSTEP)) * 64 + lane;
    f32x4 acc[NT];
    const float* xr[NT];
    bool rok[NT];
#pragma unroll
    for (int xt = 0; xt < NT; xt++) {
        acc[xt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const long long r = xt * 16 + c;
        rok[xt] = r < p.n;
        xr[xt] = p.x + (size_t)(rok[xt] ? r : 0) * p.d_in;
    }
    const int k0 = s * LIN_KSEG + g;
#pragma unroll 8
    for (int t = 0; t < LIN_KSEG / LIN_KSTEP; t++) {
        const float b = pb[(size_t)t * 64];
        const int k = k0 + LIN_KSTEP * t;
#pragma unroll
        for (int xt = 0; xt < NT; xt++) {
            const float a = (rok[xt] && k < p.d_in) ? xr[xt][k] : 0.f;
            acc[xt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[xt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int xt = 0; xt < NT; xt++)
#pragma unroll
        for (int j = 0; j < 4; j++) part[((s * NT + xt) * 4 + j) * 64 + lane] = acc[xt][j];
    __syncthreads();
    // the segments in ascending order behind the bias; accumulator register j of lane l is row 4 (l >> 4) + j, column l & 15
    for (int i = tid; i < NT * 256; i += blockDim.x) {
        const int xt = i >> 8, j = (i >> 6) & 3, l = i & 63;
        const int col = jt * 16 + (l & 15);
        const long long row = xt * 16 + 4 * (l >> 4) + j;
        float out = p.bias[col];
        for (int ss = 0; ss < p.nseg; ss++) out = out + part[((ss * NT + xt) * 4 + j) * 64 + l];
        if (row < p.n && col < p.d_out) p.y[(size_t)row * p.d_out + col] = out;
    }
}

// grid: ceil(n / 64) * ceil(jtiles / 8) blocks of 4 waves, the output blocks of one row block next to each other;
// LDS: LIN_TILED_LDS.  VEC: x is 16-byte aligned and d_in a multiple of 4
template <bool VEC>
__global__ __launch_bounds__(LIN_WAVES * 64) void linear_tiled_kernel(const LinearParams p) {
    extern __shared__ __align__(16) float xs[];  // [LIN_ROWS][LIN_XS]
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int nob = (p.jtiles + LIN_WAVES * LIN_OT - 1) / (LIN_WAVES * LIN_OT);
    const long long rb = blockIdx.x / nob;
    const int ob = (int)(blockIdx.x - rb * nob);
    const long long r0 = rb * LIN_ROWS;
    int jt[LIN_OT];
    bool live[LIN_OT];
    const float* pb[LIN_OT];
    f32x4 out[LIN_XT][LIN_OT], acc[LIN_XT][LIN_OT];
#pragma unroll
    for (int ot = 0; ot < LIN_OT; ot++) {
        const int t = (ob * LIN_OT + ot) * LIN_WAVES + w;  // waves interleaved: a short d_out still feeds every wave
        live[ot] = t < p.jtiles;
        jt[ot] = live[ot] ? t : p.jtiles - 1;  // a dead tile reads a live one's panel and stores nothing
        pb[ot] = p.panel + (size_t)jt[ot] * p.ksteps * 64 + lane;
        const float b = p.bias[jt[ot] * 16 + c];
#pragma unroll
        for (int xt = 0; xt < LIN_XT; xt++) out[xt][ot] = (f32x4){b, b, b, b};
    }
    for (int s = 0; s < p.nseg; s++) {
        __syncthreads();  // everyone is done with the previous segment's rows
        const int k0 = s * LIN_KSEG;
        if (VEC) {
            const int k = k0 + 4 * lane;
            for (int r = w; r < LIN_ROWS; r += LIN_WAVES) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (r0 + r < p.n && k < p.d_in) v = *reinterpret_cast<const f32x4*>(p.x + (size_t)(r0 + r) * p.d_in + k);
                *reinterpret_cast<f32x4*>(xs + r * LIN_XS + 4 * lane) = v;
            }
        } else {
            const int k = k0 + tid;
            for (int r = 0; r < LIN_ROWS; r++)
                xs[r * LIN_XS + tid] = (r0 + r < p.n && k < p.d_in) ? p.x[(size_t)(r0 + r) * p.d_in + k] : 0.f;
        }
        __syncthreads();
        if (!live[0]) continue;  // wave-uniform; the barriers above are met by every wave
#pragma unroll
        for (int xt = 0; xt < LIN_XT; xt++)
#pragma unroll
            for (int ot = 0; ot < LIN_OT; ot++) acc[xt][ot] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* xa = xs + c * LIN_XS + g;
        const size_t t0 = (size_t)s * (LIN_KSEG / LIN_KSTEP);
#pragma unroll 8
        for (int t = 0; t < LIN_KSEG / LIN_KSTEP; t++) {
            float b[LIN_OT], a[LIN_XT];
#pragma unroll
            for (int ot = 0; ot < LIN_OT; ot++) b[ot] = pb[ot][(t0 + t) * 64];
#pragma unroll
            for (int xt = 0; xt < LIN_XT; xt++) a[xt] = xa[xt * 16 * LIN_XS + LIN_KSTEP * t];
#pragma unroll
            for (int xt = 0; xt < LIN_XT; xt++)
#pragma unroll
                for (int ot = 0; ot < LIN_OT; ot++)
                    acc[xt][ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[xt], b[ot], acc[xt][ot], 0, 0, 0);
        }
#pragma unroll
        for (int xt = 0; xt < LIN_XT; xt++)
#pragma unroll
            for (int ot = 0; ot < LIN_OT; ot++) out[xt][ot] = out[xt][ot] + acc[xt][ot];  // the segment, in order
    }
#pragma unroll
    for (int ot = 0; ot < LIN_OT; ot++) {
        const int col = jt[ot] * 16 + c;
        if (!live[ot] || col >= p.d_out) continue;
#pragma unroll
        for (int xt = 0; xt < LIN_XT; xt++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const long long row = r0 + xt * 16 + 4 * g + j;
                if (row < p.n) p.y[(size_t)row * p.d_out + col] = out[xt][ot][j];
            }
    }
}
