// scan_kernel family: float32 L2 filtered through the byte shadow rows (BYTE).  Own translation unit so the
// families compile in parallel.
#include "ise_scan_launch.hpp"

void ise_launch_scan_i8_shadow(int ch, int waves, int T, dim3 grid, size_t lds, hipStream_t st, const ScanParams& sp) {
    launch_scan_v<false, true, ROWS_I8>(ch, waves, T, grid, lds, st, sp);
}
