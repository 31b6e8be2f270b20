// ise_sq_host.hpp -- the host state of the scalar-quantiser codec (kernels and arithmetic: ise_sq.hpp), held once each by
// the flat index (ise_sq.hip) and the inverted lists over 8-bit rows (ise_ivfsq.hip), with the launch of a search that
// does not depend on where the rows lie: the queries' staging (the merge half of a k-pass is ise_pass_host.hpp's).  Host
// code only; the handle's mutex is held.
#pragma once
#include <cmath>

#include "ise_pass_host.hpp"
#include "ise_sq.hpp"

struct SqCodec {
    int d = 0, qtype = ISE_SQ_8BIT;
    bool trained = false;
    float* par = nullptr;             // [3][d]: vmin | s | o = vmin + s / 2
    std::vector<float> trained_host;  // Faiss's layout: [vmin.., vdiff..] (2 d) or [vmin, vdiff] (uniform)
    BadFlag bad;                      // set by an encode that met a NaN or inf entry
    const float* vmin() const { return par; }
    const float* step() const { return par + d; }
    const float* off() const { return par + 2 * (size_t)d; }
    bool uniform() const { return qtype == ISE_SQ_8BIT_UNIFORM; }
    size_t trained_count() const { return uniform() ? 2 : 2 * (size_t)d; }

    hipError_t create(int d_, int qtype_) {
        d = d_;
        qtype = qtype_;
        const hipError_t e = hipMalloc((void**)&par, 3 * (size_t)d * sizeof(float));
        return e == hipSuccess ? bad.create() : e;
    }
    void destroy() {
        if (par) (void)hipFree(par);
        if (bad.p) (void)hipFree(bad.p);
        par = nullptr;
        bad.p = nullptr;
    }
    int check_trained() const {
        return trained ? ISE_OK : ise_fail_(ISE_E_INVALID, "the index is not trained: set the trained state first");
    }

    // t: trained_count() floats; the index holds no rows.  The step and offset taken here decide the code bits and the
    // decoded values: this is the one place that does
    int set_trained(const float* t, int device) {
        const size_t cnt = trained_count(), half = cnt / 2;
        for (size_t i = 0; i < cnt; i++)
            if (!(std::fabs(t[i]) <= FLT_MAX)) return ise_fail_(ISE_E_INVALID, "the trained state has a NaN or inf entry");
        for (size_t i = half; i < cnt; i++)
            if (t[i] < 0.f) return ise_fail_(ISE_E_INVALID, "the trained state has a negative vdiff");
        const size_t dd = (size_t)d;
        std::vector<float> host(3 * dd);
        for (size_t j = 0; j < dd; j++) {
            const float vmin = t[uniform() ? 0 : j], vdiff = t[uniform() ? 1 : dd + j];
            const float s = vdiff / 255.0f;
            host[j] = vmin;
            host[dd + j] = s;
            host[2 * dd + j] = std::fmaf(0.5f, s, vmin);
        }
        DeviceGuard gd(device);
        if (!gd.ok) return ise_fail_(ISE_E_HIP, "hipSetDevice failed");
        HIP_TRY(hipDeviceSynchronize());  // an encode or a scan in flight still reads the old state
        HIP_TRY(hipMemcpy(par, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        trained_host.assign(t, t + cnt);
        trained = true;
        return ISE_OK;
    }
    int get_trained(float* t) const {
        if (check_trained()) return ISE_E_INVALID;
        std::copy(trained_host.begin(), trained_host.end(), t);
        return ISE_OK;
    }

    // rows [0, n) of dst (row stride `stride`) <- the codes of x's rows, rterm (may be null) <- their row terms; sets
    // the bad flag on a non-finite entry
    void encode_launch(const float* x_dev, long long n, uint8_t* dst, int stride, double* rterm, hipStream_t st) const {
        hipLaunchKernelGGL(sq_encode_kernel, dim3((unsigned)((n + SQ_ENC_ROWS - 1) / SQ_ENC_ROWS)), dim3(SQ_WAVES * 64), 0, st, x_dev,
                           n, d, vmin(), step(), dst, stride, rterm, bad.p);
    }
    // rterm [0, n) <- the row terms of codes that came in as codes
    void rowterm_launch(const uint8_t* codes, int stride, long long n, double* rterm, hipStream_t st) const {
        hipLaunchKernelGGL(sq_rowterm_kernel, dim3((unsigned)((n + SQ_ENC_ROWS - 1) / SQ_ENC_ROWS)), dim3(SQ_WAVES * 64), 0, st, codes,
                           stride, n, d, step(), rterm);
    }
    void decode_launch(const uint8_t* codes, int stride, long long n, float* x_dev, hipStream_t st) const {
        const long long tot = n * d;
        hipLaunchKernelGGL(sq_decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, codes, stride, n, d, vmin(), step(),
                           x_dev);
    }
    // rec <- the staged records of q's nq <= SQ_STAGE_CHUNK queries
    void stage_launch(const float* q, int nq, int ip, uint8_t* rec, hipStream_t st) const {
        SqStageParams gp{};
        gp.q = q;
        gp.nq = nq;
        gp.d = d;
        gp.ip = ip;
        gp.step = step();
        gp.off = off();
        gp.rec = rec;
        hipLaunchKernelGGL(sq_stage_kernel, dim3((unsigned)nq), dim3(64), 0, st, gp);
    }
};
