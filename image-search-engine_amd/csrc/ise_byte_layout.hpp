// ise_byte_layout.hpp -- where a 16-byte unit of a byte shadow row lives in xq8 (ise_knn.hip).  ONE map for the
// builder (ise_rows.hpp), the scan (ise_scan.hpp, load_chunk), the growth copy, the mover and the debug read.
//
// xq8 is tile-blocked: [cap / 16 tiles][dpb / 64 k-steps s][4 k-groups g][16 rows r][16 B].  Unit u of a row holds its
// columns 16u .. 16u + 15 and is (s, g) = (u / 4, u % 4); lane l = 16g + r of a wave scoring tile t reads
// tile_base + s * 1024 + 16 l: the 64 units of one (tile, k-step) are 1 KB contiguous in lane order, whole cache
// lines, and a lane's 16 bytes are the A operand of v_mfma_i32_16x16x64_i8 for row r, k-group g.  A tile occupies the
// same 16 * dpb bytes it would occupy row-major, so sizes, whole-tile copies and the zero fill of whole tiles do not
// depend on the layout.  Plain C++: tests compile this header on the host.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISE_BYTE_HD __host__ __device__
#else
#define ISE_BYTE_HD
#endif

constexpr int BYTE_TILE_ROWS = 16;

// index, in 16-byte units from the start of xq8, of unit u (0 <= u < upr) of row `row`; upr = dpb / 16, a multiple of 4
ISE_BYTE_HD inline size_t byte_unit_index(long long row, int u, int upr) {
    const size_t tile = (size_t)(row >> 4);
    const int r = (int)(row & 15);
    return tile * 16 * (size_t)upr + (size_t)(u >> 2) * 64 + (size_t)(u & 3) * 16 + (size_t)r;
}
