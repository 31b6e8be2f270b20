// sel_scan_kernel family and the masked range pass (ise_sel_scan.hpp).  Own translation unit so the families
// compile in parallel.
#include "ise_scan_params.hpp"
#include "ise_sel_scan.hpp"

template <bool BF16, bool SHIFT>
static void launch_sel_v(int ch, dim3 grid, size_t lds, hipStream_t st, const SelScanParams& sp) {
    static LdsAttrOnce attr[3];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), LDS_LIMIT);
        hipLaunchKernelGGL(kern, grid, dim3(SEL_W * 64), lds, st, sp);
    };
    if (ch >= 4) go(sel_scan_kernel<4, BF16, SHIFT>, attr[0]);
    else if (ch == 2) go(sel_scan_kernel<2, BF16, SHIFT>, attr[1]);
    else go(sel_scan_kernel<1, BF16, SHIFT>, attr[2]);
}

void ise_launch_sel_scan(int storage_bf16, int shift, int ch, dim3 grid, size_t lds, hipStream_t st, const SelScanParams& sp) {
    if (storage_bf16) launch_sel_v<true, false>(ch, grid, lds, st, sp);
    else if (shift) launch_sel_v<false, true>(ch, grid, lds, st, sp);
    else launch_sel_v<false, false>(ch, grid, lds, st, sp);
}

template <bool BF16, bool SHIFT>
static void launch_range_masked_v(int ch, dim3 grid, size_t lds, hipStream_t st, const RangeParams& rp) {
    static LdsAttrOnce attr[3];
    auto go = [&](auto kern, LdsAttrOnce& a) {
        a.ensure(reinterpret_cast<const void*>(kern), LDS_LIMIT);
        hipLaunchKernelGGL(kern, grid, dim3(RANGE_W * 64), lds, st, rp);
    };
    if (ch >= 4) go(range_scan_kernel<4, BF16, SHIFT, true>, attr[0]);
    else if (ch == 2) go(range_scan_kernel<2, BF16, SHIFT, true>, attr[1]);
    else go(range_scan_kernel<1, BF16, SHIFT, true>, attr[2]);
}

void ise_launch_range_masked(int storage_bf16, int shift, int ch, dim3 grid, size_t lds, hipStream_t st, const RangeParams& rp) {
    if (storage_bf16) launch_range_masked_v<true, false>(ch, grid, lds, st, rp);
    else if (shift) launch_range_masked_v<false, true>(ch, grid, lds, st, rp);
    else launch_range_masked_v<false, false>(ch, grid, lds, st, rp);
}
