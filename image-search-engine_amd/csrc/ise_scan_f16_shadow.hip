// scan_kernel family: float32 L2 filtered through the fp16 shadow rows (HALF).  Own translation unit so the
// families compile in parallel.
#include "ise_scan_launch.hpp"

void ise_launch_scan_f16_shadow(int ch, int waves, int T, dim3 grid, size_t lds, hipStream_t st, const ScanParams& sp) {
    launch_scan_v<false, true, ROWS_F16>(ch, waves, T, grid, lds, st, sp);
}
