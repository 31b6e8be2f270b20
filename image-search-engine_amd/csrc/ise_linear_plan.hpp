// ise_linear_plan.hpp -- the panel layout of a linear transform's matrix (ise_linear_*).  Host-only and
// pure: no HIP, so tests/native/linear_plan_check.cpp builds it with a host compiler under the sanitizers.
//
// The kernels multiply with v_mfma_f32_16x16x4_f32, whose matrix operand is one float per lane: lane l supplies
// B[k = l >> 4][j = l & 15] of a 4 x 16 slice.  A, [d_out][d_in] row-major, is therefore stored as the lanes read it:
//   panel[(jt * ksteps + t) * 64 + l] = A[16 jt + (l & 15)][4 t + (l >> 4)]     (0 where either index is out of range)
// for output tile jt < ceil(d_out / 16) and k step t < ksteps = 64 * ceil(d_in / 256): one k step is one MFMA, one
// coalesced 256-byte load per wave, and k steps [64 s, 64 s + 64) are segment s of the arithmetic contract.  The zero
// padding of a ragged last segment and of a ragged last tile is exact (a chain that starts from +0 never holds -0).
#pragma once
#include <cstddef>
#include <cstdint>

#define LIN_KSEG 256  // k entries of one fmaf chain: the same constant in every launch shape
#define LIN_KSTEP 4   // k entries of one MFMA
#define LIN_TILE 16   // outputs of one MFMA

struct LinearPlan {
    int d_in, d_out;
    int nseg;    // ceil(d_in / LIN_KSEG)
    int ksteps;  // nseg * LIN_KSEG / LIN_KSTEP
    int jtiles;  // ceil(d_out / LIN_TILE)
    size_t panel_floats() const { return (size_t)jtiles * (size_t)ksteps * 64; }
};

inline LinearPlan linear_plan(int d_in, int d_out) {
    LinearPlan p;
    p.d_in = d_in;
    p.d_out = d_out;
    p.nseg = (d_in + LIN_KSEG - 1) / LIN_KSEG;
    p.ksteps = p.nseg * (LIN_KSEG / LIN_KSTEP);
    p.jtiles = (d_out + LIN_TILE - 1) / LIN_TILE;
    return p;
}

// where entry (j, k) of A lies in the panels
inline size_t linear_panel_index(const LinearPlan& p, int j, int k) {
    const int jt = j / LIN_TILE, t = k / LIN_KSTEP, lane = (k % LIN_KSTEP) * 16 + (j % LIN_TILE);
    return ((size_t)jt * (size_t)p.ksteps + (size_t)t) * 64 + (size_t)lane;
}

// panel: panel_floats() floats, every one written
inline void linear_pack(const LinearPlan& p, const float* A, float* panel) {
    for (int jt = 0; jt < p.jtiles; jt++)
        for (int t = 0; t < p.ksteps; t++) {
            float* dst = panel + ((size_t)jt * (size_t)p.ksteps + (size_t)t) * 64;
            for (int l = 0; l < 64; l++) {
                const int j = jt * LIN_TILE + (l & 15), k = t * LIN_KSTEP + (l >> 4);
                dst[l] = (j < p.d_out && k < p.d_in) ? A[(size_t)j * (size_t)p.d_in + (size_t)k] : 0.f;
            }
        }
}
