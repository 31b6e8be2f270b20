// ise_geometry.hpp -- the row geometry and the bound width every host side shares (ise_knn.hip, ise_ivf.hip): one
// definition, so that an index type cannot drift from the flat index whose tile functions and lower bound it uses.
#pragma once
#include "../../include/ise_knn.h"

// rows are padded to whole k-steps of 64 bytes (16 floats / 32 bf16); rows longer than
// 4 steps to a multiple of 4 steps so that wider register chunks divide them
static inline int elem_size(int storage) { return storage == ISE_STORE_BF16 ? 2 : 4; }
static inline int pad_dim(int d, int storage) {
    const int per_step = 64 / elem_size(storage);
    const int steps = (d + per_step - 1) / per_step;
    return (steps > 4 ? (steps + 3) / 4 * 4 : steps) * per_step;
}
// k-steps per register chunk of a row of rb bytes
static inline int chunk_steps_rb(size_t rb) {
    const int steps = (int)(rb / 64);
    for (int ch = 8; ch > 1; ch >>= 1)
        if (steps % ch == 0) return ch;
    return 1;
}
// LDS query row stride in 4-byte units: (stride/4) % 16 == 2 makes the 16 rows x 4 k-groups
// ds_read_b128 pattern bank-conflict-free
static inline int qs_stride_units(int units) {
    const int pad = ((2 - (units / 4)) % 16 + 16) % 16 * 4;
    return units + pad;
}
// relative width of the float32 L2 lower bound for rows padded to dp (ise_exact.hpp)
static inline float exact_beta_dp(int dp) { return (0.5625f * dp + 256.f) * 5.9604645e-8f * 1.02f; }
// the range / masked passes' query staging (ise_range.hpp, range_stage_queries) for an index whose one-tile streaming
// plan has `waves` waves: threads per query row, and the vector path where the rows allow it
static inline void range_staging_rule(int waves, bool bf16, int d, int qs_stride, int* tpr, int* vec_q) {
    *tpr = waves >= 8 ? 32 : 16;
    *vec_q = (d & (bf16 ? 7 : 3)) == 0 && (qs_stride >> 2) <= *tpr * (bf16 ? 4 : 8);
}
