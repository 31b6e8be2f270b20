// ise_linear.hip -- host side and C ABI of the linear transform (include/ise_knn.h, ise_linear_*; kernels in
// ise_linear.hpp, the panel layout in ise_linear_plan.hpp).
//
// A handle is immutable once created: the panels and the bias never change and the device form uses no scratch memory,
// so ise_linear_apply_device takes no lock and calls on different streams need no order between them.  The host form
// stages through two grown buffers of its own, one call at a time (a mutex), on the handle's stream.
#include "ise_host.hpp"
#include "ise_linear.hpp"

struct ise_linear {
    LinearPlan plan{};
    int have_bias = 0, device = 0;
    float* panel = nullptr;  // plan.panel_floats()
    float* bias = nullptr;   // [jtiles * 16], zeros without a bias and beyond d_out
    hipStream_t stream = nullptr;
    std::mutex mu;              // the host form
    DevBuf<float> xraw, yraw;   // the host form's pieces
    std::atomic<uint64_t> st_calls{0}, st_few{0}, st_tiled{0};
};

namespace {
int check_handle(const ise_linear* h) { return h ? ISE_OK : ise_fail_(ISE_E_INVALID, "linear transform handle is NULL"); }

template <int NT>
void launch_few(const LinearParams& lp, hipStream_t st) {
    static LdsAttrOnce attr;
    attr.ensure(reinterpret_cast<const void*>(linear_few_kernel<NT>), 64 * 1024);
    hipLaunchKernelGGL(linear_few_kernel<NT>, dim3(lp.jtiles), dim3(lp.nseg * 64), (size_t)lp.nseg * NT * 256 * sizeof(float), st, lp);
}

template <bool VEC>
void launch_tiled(const LinearParams& lp, hipStream_t st) {
    static LdsAttrOnce attr;
    attr.ensure(reinterpret_cast<const void*>(linear_tiled_kernel<VEC>), LIN_TILED_LDS);
    const long long nob = (lp.jtiles + LIN_WAVES * LIN_OT - 1) / (LIN_WAVES * LIN_OT);
    const long long nrb = (lp.n + LIN_ROWS - 1) / LIN_ROWS;
    hipLaunchKernelGGL(linear_tiled_kernel<VEC>, dim3((unsigned)(nrb * nob)), dim3(LIN_WAVES * 64), LIN_TILED_LDS, st, lp);
}

// n >= 1 rows at x_dev -> y_dev, on st; the current device is the handle's
int apply_enqueue(ise_linear* h, const float* x_dev, long long n, float* y_dev, hipStream_t st) {
    LinearParams lp{};
    lp.x = x_dev;
    lp.panel = h->panel;
    lp.bias = h->bias;
    lp.y = y_dev;
    lp.n = n;
    lp.d_in = h->plan.d_in;
    lp.d_out = h->plan.d_out;
    lp.nseg = h->plan.nseg;
    lp.ksteps = h->plan.ksteps;
    lp.jtiles = h->plan.jtiles;
    h->st_calls++;
    if (n <= ISE_LINEAR_FEW_ROWS) {
        h->st_few++;
        switch ((int)((n + 15) / 16)) {
            case 1: launch_few<1>(lp, st); break;
            case 2: launch_few<2>(lp, st); break;
            case 3: launch_few<3>(lp, st); break;
            default: launch_few<4>(lp, st); break;
        }
    } else {
        h->st_tiled++;
        const bool vec = (reinterpret_cast<uintptr_t>(x_dev) & 15) == 0 && (lp.d_in & 3) == 0;
        if (vec) launch_tiled<true>(lp, st);
        else launch_tiled<false>(lp, st);
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

void free_all(ise_linear* h) {
    if (h->panel) (void)hipFree(h->panel);
    if (h->bias) (void)hipFree(h->bias);
    buf_free(h->xraw, h->yraw);
    if (h->stream) (void)hipStreamDestroy(h->stream);
}
}  // namespace

extern "C" int ise_linear_create(ise_linear_t** out, int d_in, int d_out, const float* A, const float* b, int device) {
    if (!out) return ise_fail_(ISE_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d_in <= 0 || d_out <= 0) return ise_fail_(ISE_E_INVALID, "d_in and d_out must be positive");
    if (d_in > ISE_LINEAR_MAX_D || d_out > ISE_LINEAR_MAX_D)
        return ise_fail_(ISE_E_INVALID, "d_in and d_out must be at most ISE_LINEAR_MAX_D");
    if (!A) return ise_fail_(ISE_E_INVALID, "matrix pointer is NULL");
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    ise_linear* h = new (std::nothrow) ise_linear();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    h->plan = linear_plan(d_in, d_out);
    h->have_bias = b ? 1 : 0;
    h->device = device;
    const size_t np = h->plan.panel_floats(), nb = (size_t)h->plan.jtiles * LIN_TILE;
    std::vector<float> panel, bias;
    try {
        panel.resize(np);
        bias.assign(nb, 0.f);
    } catch (const std::bad_alloc&) {
        delete h;
        return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    }
    linear_pack(h->plan, A, panel.data());
    if (b) std::copy(b, b + d_out, bias.begin());
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->panel, np * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->bias, nb * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->panel, panel.data(), np * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->bias, bias.data(), nb * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_all(h);
        delete h;
        return ise_fail_(e == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP, std::string("linear transform setup: ") + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

extern "C" int ise_linear_destroy(ise_linear_t* h) {
    if (!h) return ISE_OK;
    {
        DeviceGuard gd(h->device);
        (void)hipDeviceSynchronize();
        free_all(h);
    }
    delete h;
    return ISE_OK;
}

extern "C" int ise_linear_info(const ise_linear_t* h, int* d_in, int* d_out, int* have_bias, int* device) {
    if (check_handle(h)) return ISE_E_INVALID;
    if (d_in) *d_in = h->plan.d_in;
    if (d_out) *d_out = h->plan.d_out;
    if (have_bias) *have_bias = h->have_bias;
    if (device) *device = h->device;
    return ISE_OK;
}

extern "C" int ise_linear_apply_device(ise_linear_t* h, const float* x_dev, int64_t n, float* y_dev, void* stream) {
    if (n <= 0) return ise_fail_(ISE_E_INVALID, "n must be positive");
    if (!x_dev || !y_dev) return ise_fail_(ISE_E_INVALID, "rows or output pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    if (n >= (1ll << 36)) return ise_fail_(ISE_E_INVALID, "n is too large");
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x_dev), y0 = reinterpret_cast<uintptr_t>(y_dev);
    const uintptr_t x1 = x0 + (uintptr_t)n * h->plan.d_in * sizeof(float), y1 = y0 + (uintptr_t)n * h->plan.d_out * sizeof(float);
    if (x0 < y1 && y0 < x1) return ise_fail_(ISE_E_INVALID, "the output overlaps the rows: the transform is not in place");
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    return apply_enqueue(h, x_dev, n, y_dev, (hipStream_t)stream);
}

extern "C" int ise_linear_apply_host(ise_linear_t* h, const float* x, int64_t n, float* y) {
    if (n <= 0) return ise_fail_(ISE_E_INVALID, "n must be positive");
    if (!x || !y) return ise_fail_(ISE_E_INVALID, "rows or output pointer is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    const int di = h->plan.d_in, dn = h->plan.d_out;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
    if (x0 < y0 + (uintptr_t)n * dn * sizeof(float) && y0 < x0 + (uintptr_t)n * di * sizeof(float))
        return ise_fail_(ISE_E_INVALID, "the output overlaps the rows: the transform is not in place");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard gd(h->device);
    if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
    hipStream_t st = h->stream;
    const long long step = upload_step((size_t)std::max(di, dn) * sizeof(float));  // 256 MiB at most either way
    int rc;
    for (long long i0 = 0; i0 < n; i0 += step) {
        const long long m = std::min<long long>(step, n - i0);
        if ((rc = grow_owned(h->xraw, (size_t)m * di))) return rc;  // the stream is drained between pieces
        if ((rc = grow_owned(h->yraw, (size_t)m * dn))) return rc;
        HIP_TRY(hipMemcpyAsync(h->xraw.p, x + (size_t)i0 * di, (size_t)m * di * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = apply_enqueue(h, h->xraw.p, m, h->yraw.p, st))) return rc;
        HIP_TRY(hipMemcpyAsync(y + (size_t)i0 * dn, h->yraw.p, (size_t)m * dn * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}

extern "C" int ise_linear_stats(ise_linear_t* h, uint64_t* out3) {
    if (!out3) return ise_fail_(ISE_E_INVALID, "out3 is NULL");
    if (check_handle(h)) return ISE_E_INVALID;
    out3[0] = h->st_calls.load();
    out3[1] = h->st_few.load();
    out3[2] = h->st_tiled.load();
    return ISE_OK;
}
