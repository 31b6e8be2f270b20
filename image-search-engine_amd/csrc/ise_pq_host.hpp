// ise_pq_host.hpp -- the host state of the product-quantiser codec (kernels and arithmetic: ise_pq.hpp), held once each
// by the flat index (ise_pq.hip) and the inverted lists over its codes (ise_ivfpq.hip), with the launches that do not
// depend on where the rows lie: encode, decode, the queries' tables, and a scan kernel's launch with its LDS attribute
// (the merge half of a k-pass is ise_pass_host.hpp's).  Host code only; the handle's mutex is held.
#pragma once
#include <cmath>

#include "ise_pass_host.hpp"
#include "ise_pq.hpp"

struct PqCodec {
    int d = 0, M = 0, dsub = 0, stride = 0, qt = 0;  // stride: M rounded up to 16; qt: queries per pass
    bool trained = false;
    float* cb = nullptr;  // [M][256][dsub]
    BadFlag bad;          // set by an encode that met a NaN or inf entry
    size_t cb_count() const { return (size_t)M * PQ_KSUB * dsub; }
    size_t tab_floats() const { return (size_t)M * PQ_KSUB; }  // of one query's tables
    size_t lds_bytes() const { return pq_lds_bytes(M, qt); }
    // blocks of a pass one CU holds at once (their LDS)
    long long blocks_per_cu() const { return std::max<long long>(1, (long long)PQ_LDS_LIMIT / (long long)lds_bytes()); }

    hipError_t create(int d_, int M_) {
        d = d_;
        M = M_;
        dsub = d / M;
        stride = (M + 15) / 16 * 16;
        qt = pq_qt(M);
        const hipError_t e = hipMalloc((void**)&cb, cb_count() * sizeof(float));
        return e == hipSuccess ? bad.create() : e;
    }
    void destroy() {
        if (cb) (void)hipFree(cb);
        if (bad.p) (void)hipFree(bad.p);
        cb = nullptr;
        bad.p = nullptr;
    }
    int check_trained() const {
        return trained ? ISE_OK : ise_fail_(ISE_E_INVALID, "the index is not trained: set the centroids first");
    }

    // c: [M][256][dsub] floats, finite; the index holds no rows
    int set_centroids(const float* c, int device) {
        const size_t cnt = cb_count();
        for (size_t i = 0; i < cnt; i++)
            if (!(std::fabs(c[i]) <= FLT_MAX)) return ise_fail_(ISE_E_INVALID, "a centroid has a NaN or inf entry");
        DeviceGuard gd(device);
        if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
        HIP_TRY(hipDeviceSynchronize());  // an encode or a table build in flight still reads the old centroids
        HIP_TRY(hipMemcpy(cb, c, cnt * sizeof(float), hipMemcpyHostToDevice));
        trained = true;
        return ISE_OK;
    }
    int get_centroids(float* c, int device) const {
        if (check_trained()) return ISE_E_INVALID;
        DeviceGuard gd(device);
        if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
        HIP_TRY(hipMemcpy(c, cb, cb_count() * sizeof(float), hipMemcpyDeviceToHost));
        return ISE_OK;
    }

    // byte m of rows [0, n) of dst (row stride `stride_`) <- the code of x's rows; sets the bad flag on a non-finite entry
    void encode_launch(const float* x_dev, long long n, uint8_t* dst, int stride_, hipStream_t st) const {
        static LdsAttrOnce attr;
        const dim3 grid((unsigned)((n + PQ_ENC_ROWS - 1) / PQ_ENC_ROWS), (unsigned)M);
        if (dsub <= PQ_ENC_LDS_DSUB) {
            attr.ensure(reinterpret_cast<const void*>(pq_encode_kernel<true>), PQ_ENC_LDS_DSUB * PQ_KSUB * 4);
            hipLaunchKernelGGL(pq_encode_kernel<true>, grid, dim3(PQ_WAVES * 64), (size_t)dsub * PQ_KSUB * 4, st, x_dev, n, d, M,
                               (const float*)cb, dst, stride_, bad.p);
        } else {
            hipLaunchKernelGGL(pq_encode_kernel<false>, grid, dim3(PQ_WAVES * 64), 0, st, x_dev, n, d, M, (const float*)cb, dst,
                               stride_, bad.p);
        }
    }
    void decode_launch(const uint8_t* codes, int stride_, long long n, float* x_dev, hipStream_t st) const {
        const long long tot = n * d;
        hipLaunchKernelGGL(pq_decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, codes, stride_, n, d, M,
                           (const float*)cb, x_dev);
    }
    // tab <- the tables of q's mc <= PQ_TAB_CHUNK queries, [group][m][256][qt]
    void table_launch(const float* q_dev, int mc, int ip, float* tab, hipStream_t st) const {
        const int groups = (mc + qt - 1) / qt;
        hipLaunchKernelGGL(pq_table_kernel, dim3((unsigned)M, (unsigned)groups), dim3(PQ_KSUB), 0, st, q_dev, mc, d, M, qt, ip,
                           (const float*)cb, tab);
    }
};

// one scan kernel family's launch: kern[i] for QT = 16, 8, 4, 2, each with the LDS attribute set once per device.  One
// static instance per family (ise_pq.hip: pq_scan_kernel; ise_ivfpq.hip: ivfpq_scan_kernel)
template <class P>
struct PqScanLaunch {
    void (*kern[4])(P);
    LdsAttrOnce attr[4];
    void operator()(int qt, unsigned grid, size_t lds, hipStream_t st, const P& sp) {
        const int i = qt == 16 ? 0 : qt == 8 ? 1 : qt == 4 ? 2 : 3;
        attr[i].ensure(reinterpret_cast<const void*>(kern[i]), PQ_LDS_LIMIT);
        hipLaunchKernelGGL(kern[i], dim3(grid), dim3(PQ_WAVES * 64), lds, st, sp);
    }
};
