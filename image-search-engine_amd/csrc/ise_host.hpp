// ise_host.hpp -- host plumbing every translation unit of libise_knn.so shares: the error path into
// ise_last_error(), the lazily grown device buffer, and the one knob another translation unit reads.  No kernels.
#pragma once
#include "ise_common.hpp"

// ise_knn.hip: stores msg as the calling thread's ise_last_error() and returns code
int ise_fail_(int code, const std::string& msg);
// ise_knn.hip: $ISE_REMOVE_SLAB_ROWS as last refreshed (ise_refresh_env_knobs)
int ise_remove_slab_rows_();

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ise_fail_(e_ == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP,                  \
                             std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

// A buffer grown lazily, contents not kept.  What has to be waited for before the old one is freed differs per
// index kind, so each has its own grow function (range_grow, bin_grow, the inverted lists' grow).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
};
