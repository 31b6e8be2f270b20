// ise_rows.hpp -- wave-per-row helper kernels: norms, padding / conversion, normalize_L2, shift vector.
#pragma once
#include "ise_common.hpp"
#include "ise_byte_layout.hpp"

// ---------------------------------------------------------------- row helpers
// |y|^2 per row, wave per row, fixed summation order (lanes stride float4, then
// an xor butterfly): deterministic for a given dp.  Shifted (float32 L2): NaN for a row with a
// NaN or inf entry, even where |y - mu|^2 would be inf (ise_common.hpp, nonfinite_mark).
__global__ __launch_bounds__(256) void norms_kernel(const float* __restrict__ x, long long row0,
                                                    long long n, int dp, const float* __restrict__ mu,
                                                    float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = row0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= row0 + n) return;
    const float* xr = x + (size_t)r * dp;
    float s = 0.f;
    for (int j = lane * 4; j < dp; j += 256) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(xr + j);
        f32x4 v = x;
        if (mu) v = v - *reinterpret_cast<const f32x4*>(mu + j);  // |y - mu|^2 (padding columns: 0 - 0)
        s = fmaf(v[0], v[0], s);
        s = fmaf(v[1], v[1], s);
        s = fmaf(v[2], v[2], s);
        s = fmaf(v[3], v[3], s);
        if (mu) s += nonfinite_mark(x);  // a non-finite entry: |y - mu|^2 = NaN (ise_common.hpp)
    }
    s = wave_sum_f32(s);
    if (lane == 0) out[r] = s;
}

// fp16 shadow rows of a float32 L2 index (the scan's filter reads them; ise_scan.hpp HALF), wave per
// row, in float64 from the exact a = y - mu:  s_r puts max |a| in [2^14, 2^15) (no fp16 overflow), the row holds
// fp16(2^s_r a) (zero padded to dph), and hn = |u~|^2, he = e_r >= |a - u~| (rounded up; a margin for a - mu not
// being exact in float64 when the exponents are far apart), hs = s_r, with u~ = 2^-s_r fp16(2^s_r a).  A row
// with a NaN or inf entry gets hn = NaN and a zero shadow (never a candidate, as its norm does).
__global__ __launch_bounds__(256) void shadow_rows_kernel(const float* __restrict__ x, long long row0, long long n,
                                                          int d, int dp, const float* __restrict__ mu,
                                                          _Float16* __restrict__ xh, int dph, float* __restrict__ hn,
                                                          float* __restrict__ he, float* __restrict__ hs) {
    const int lane = threadIdx.x & 63;
    const long long r = row0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= row0 + n) return;
    const float* xr = x + (size_t)r * dp;
    double amax = 0.0;
    float mark = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float v = xr[j];
        mark += v - v;
        amax = fmax(amax, fabs((double)v - (double)mu[j]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        amax = fmax(amax, __shfl_xor(amax, o));
        mark += __shfl_xor(mark, o);
    }
    const bool bad = mark != 0.f;
    const int s = (amax > 0.0 && !bad) ? 14 - ilogb(amax) : 0;
    _Float16* hr = xh + (size_t)r * dph;
    double nu = 0.0, e2 = 0.0;
    for (int j = lane; j < dph; j += 64) {
        const double a = (j < d && !bad) ? (double)xr[j] - (double)mu[j] : 0.0;
        const _Float16 u = (_Float16)(float)ldexp(a, s);
        hr[j] = u;
        const double ut = ldexp((double)(float)u, -s);
        nu = fma(ut, ut, nu);
        e2 = fma(a - ut, a - ut, e2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nu += __shfl_xor(nu, o);
        e2 += __shfl_xor(e2, o);
    }
    if (lane == 0) {
        const double e = sqrt(e2) * (1.0 + 0x1p-40) + sqrt(nu) * 0x1p-49;
        float ef = (float)e;
        if ((double)ef < e) ef = nextafterf(ef, INFINITY);
        hn[r] = bad ? __int_as_float(0x7fc00000) : (float)nu;
        he[r] = ef;
        hs[r] = (float)s;
    }
}

// byte shadow rows of a float32 L2 index (ise_scan.hpp BYTE), wave per row, in float64 from the
// exact a = y - mu:  c_r = max |a| / 127 rounded UP to bf16, the row holds q = rint(a / c_r) in [-127, 127] (zero
// padded to dpb), and bm packs c_r (bf16, low half) with e_r / c_r (fp16, rounded up, high half), where
// e_r >= |a - c_r q| (rounded up; the margins of shadow_rows_kernel).  Their product (8 x 11 significant bits) is
// exact in float32, so the scan recovers e_r with one multiply and a tile's c_r, e_r are one 16-byte load per lane.
// A row with a NaN or inf entry gets a zero shadow and c_r = 0 (its float32 norm is NaN: never a candidate).
__global__ __launch_bounds__(256) void byte_rows_kernel(const float* __restrict__ x, long long row0, long long n,
                                                        int d, int dp, const float* __restrict__ mu,
                                                        int8_t* __restrict__ xq, int dpb, uint32_t* __restrict__ bm) {
    const int lane = threadIdx.x & 63;
    const long long r = row0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= row0 + n) return;
    const float* xr = x + (size_t)r * dp;
    double amax = 0.0;
    float mark = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float v = xr[j];
        mark += v - v;
        amax = fmax(amax, fabs((double)v - (double)mu[j]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        amax = fmax(amax, __shfl_xor(amax, o));
        mark += __shfl_xor(mark, o);
    }
    const bool bad = mark != 0.f;
    const double c = bad ? 0.0 : amax / 127.0;
    float cf = (float)c;
    if ((double)cf < c) cf = nextafterf(cf, INFINITY);
    uint32_t cb = __float_as_uint(cf);
    if (cb & 0xFFFFu) cb = (cb + 0x10000u) & 0xFFFF0000u;  // bf16, rounded up: |a| / c_r <= 127
    const double cr = (double)__uint_as_float(cb);
    const int upr = dpb >> 4;  // 16-byte units per row; dpb is a multiple of 64, so every pass has all 64 lanes
    double nu = 0.0, e2 = 0.0;
    for (int j = lane; j < dpb; j += 64) {
        const double a = (j < d && !bad) ? (double)xr[j] - (double)mu[j] : 0.0;
        const double q = cr > 0.0 ? fmin(fmax(rint(a / cr), -127.0), 127.0) : 0.0;
        // the 16 codes of lanes 16g .. 16g + 15 are unit j / 16 of the row: gathered into lane 16g (bytes, then
        // dwords) and stored as one 16-byte unit where ise_byte_layout.hpp puts it
        const uint32_t b = (uint32_t)(uint8_t)(int8_t)q;
        const uint32_t w4 = b | (__shfl_down(b, 1) << 8) | (__shfl_down(b, 2) << 16) | (__shfl_down(b, 3) << 24);
        u32x4 unit;
        unit[0] = w4;
        unit[1] = __shfl_down(w4, 4);
        unit[2] = __shfl_down(w4, 8);
        unit[3] = __shfl_down(w4, 12);
        if ((lane & 15) == 0)
            *reinterpret_cast<u32x4*>(xq + (byte_unit_index(r, j >> 4, upr) << 4)) = unit;
        const double res = a - cr * q;  // cr q is exact (8 + 7 significant bits)
        nu = fma(a, a, nu);
        e2 = fma(res, res, e2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nu += __shfl_xor(nu, o);
        e2 += __shfl_xor(e2, o);
    }
    if (lane == 0) {
        const double e = sqrt(e2) * (1.0 + 0x1p-40) + sqrt(nu) * 0x1p-49;
        const double eps = cr > 0.0 ? e / cr * (1.0 + 0x1p-40) : 0.0;
        float ef = (float)eps;
        if ((double)ef < eps) ef = nextafterf(ef, INFINITY);
        unsigned short hb = __builtin_bit_cast(unsigned short, (_Float16)ef);
        if ((float)__builtin_bit_cast(_Float16, hb) < ef) hb++;  // fp16, rounded up (eps <= sqrt(d) / 2 + margins)
        bm[r] = (cb >> 16) | ((uint32_t)hb << 16);
    }
}

// Rows [row0, row1) of the tile-blocked byte rows read zero again (remove_ids: the rows of a last, partial tile that
// are no longer rows; whole tiles behind it are cleared with a memset).  One thread per (row, unit).
__global__ __launch_bounds__(256) void byte_rows_zero_kernel(int8_t* __restrict__ xq, long long row0, long long row1,
                                                             int upr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = row0 + i / upr;
    if (row >= row1) return;
    const u32x4 z = {0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(xq + (byte_unit_index(row, (int)(i % upr), upr) << 4)) = z;
}

// Debug read (ise_index_byte_row_codes): the upr units of one row, gathered into out[upr] in column order.
__global__ __launch_bounds__(64) void byte_row_read_kernel(const int8_t* __restrict__ xq, long long row, int upr,
                                                           u32x4* __restrict__ out) {
    for (int u = threadIdx.x; u < upr; u += 64)
        out[u] = *reinterpret_cast<const u32x4*>(xq + (byte_unit_index(row, u, upr) << 4));
}

// The byte route's index statistic (ise_knn.hip, byte_rel_ok): mean e_r / |y - mu| over the rows with a finite,
// positive norm.  One block, a fixed summation order: deterministic for given rows.
__global__ __launch_bounds__(1024) void byte_rel_kernel(const float* __restrict__ norms, const uint32_t* __restrict__ bm,
                                                        long long n, double* __restrict__ out) {
    __shared__ double ss[1024], sc[1024];
    double s = 0.0, cnt = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        const float nn = norms[i];
        if (nn > 0.f && nn <= FLT_MAX) {  // NaN (a non-finite row), 0 and overflowed norms are left out
            const uint32_t m = bm[i];
            const float er = __uint_as_float(m << 16) * (float)__builtin_bit_cast(_Float16, (unsigned short)(m >> 16));
            s += (double)er / sqrt((double)nn);
            cnt += 1.0;
        }
    }
    ss[threadIdx.x] = s;
    sc[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ss[threadIdx.x] += ss[threadIdx.x + o];
            sc[threadIdx.x] += sc[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sc[0] > 0.0 ? ss[0] / sc[0] : 0.0;
}

// ... and its neighbourhood statistic: squared distances between m sample rows (rows i * stride, float32, fixed order),
// out[i * m + j], +inf on the diagonal; rho_kernel then takes mean_i min_j d_ij / mean_{i != j} d_ij (one block, m <=
// 1024, non-finite distances left out).  Small on clustered rows, whose neighbours sit far closer than typical pairs.
__global__ __launch_bounds__(256) void sample_dist_kernel(const float* __restrict__ x, int dp, int d, long long stride, int m,
                                                          float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)m * m) return;
    const int i = (int)(t / m), j = (int)(t % m);
    const float* a = x + (size_t)i * stride * dp;
    const float* b = x + (size_t)j * stride * dp;
    float s = 0.f;
    for (int c = 0; c < d; c++) s = fmaf(a[c] - b[c], a[c] - b[c], s);
    out[t] = i == j ? INFINITY : s;
}
__global__ __launch_bounds__(1024) void rho_kernel(const float* __restrict__ dist, int m, double* __restrict__ out) {
    __shared__ double sn[1024], sp[1024], cn[1024], cp[1024];
    const int i = threadIdx.x;
    double mn = INFINITY, sum = 0.0, cnt = 0.0;
    if (i < m)
        for (int j = 0; j < m; j++) {
            const float v = dist[(size_t)i * m + j];
            if (v <= FLT_MAX) {  // finite (the diagonal and non-finite rows are left out)
                mn = fmin(mn, (double)v);
                sum += v;
                cnt += 1.0;
            }
        }
    const bool ok = mn <= 1e300;
    sn[i] = ok ? mn : 0.0;
    cn[i] = ok ? 1.0 : 0.0;
    sp[i] = sum;
    cp[i] = cnt;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (i < o) {
            sn[i] += sn[i + o];
            cn[i] += cn[i + o];
            sp[i] += sp[i + o];
            cp[i] += cp[i + o];
        }
        __syncthreads();
    }
    if (i == 0) out[0] = (cn[0] > 0.0 && sp[0] > 0.0) ? (sn[0] / cn[0]) / (sp[0] / cp[0]) : 0.0;
}

// column mean of `rows` rows (d columns of a padded row).  Two levels, both in a fixed order
// (`groups` row groups summed in row order, then the groups in group order): deterministic for a
// given row count.  NaN / inf entries are skipped (they must not poison every distance).
#define COLMEAN_GROUPS_MAX 1024
__global__ __launch_bounds__(256) void col_sum_kernel(const float* __restrict__ x, long long rows, int d, int dp,
                                                      int groups, float* __restrict__ partial /* [groups][dp] */) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int gidx = blockIdx.y;
    if (j >= dp) return;
    const long long per = (rows + groups - 1) / groups;
    const long long r0 = gidx * per, r1 = min(rows, r0 + per);
    float s = 0.f;
    if (j < d)
        for (long long r = r0; r < r1; r++) {
            const float v = x[(size_t)r * dp + j];
            if (fabsf(v) <= FLT_MAX) s += v;
        }
    partial[(size_t)gidx * dp + j] = s;
}
__global__ __launch_bounds__(256) void col_mean_kernel(const float* __restrict__ partial, long long rows, int d, int dp,
                                                       int groups, float* __restrict__ mu) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dp) return;
    float s = 0.f;
    for (int gi = 0; gi < groups; gi++) s += partial[(size_t)gi * dp + j];
    const float m = s / (float)rows;
    mu[j] = (j < d && fabsf(m) <= FLT_MAX) ? m : 0.f;
}

// |y|^2 of bf16 rows (the values the bf16 scan multiplies), fp32 accumulation
__global__ __launch_bounds__(256) void norms_bf16_kernel(const __bf16* __restrict__ x, long long row0, long long n,
                                                         int dp, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = row0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= row0 + n) return;
    const __bf16* xr = x + (size_t)r * dp;
    float s = 0.f;
    for (int j = lane * 8; j < dp; j += 512) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + j);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float f = (float)v[e];
            s = fmaf(f, f, s);
        }
    }
    s = wave_sum_f32(s);
    if (lane == 0) out[r] = s;
}

// float32 rows (unpadded) -> padded bf16 index rows (round to nearest even)
__global__ __launch_bounds__(256) void pad_rows_bf16_kernel(const float* __restrict__ src, long long n, int d,
                                                            __bf16* __restrict__ dst, int dp) {
    const long long total = n * dp;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / dp;
        const int j = (int)(i - r * dp);
        dst[i] = (__bf16)(j < d ? src[(size_t)r * d + j] : 0.f);
    }
}

// padded bf16 rows -> float32 rows of d (reconstruct / write_index)
__global__ __launch_bounds__(256) void unpack_rows_bf16_kernel(const __bf16* __restrict__ src, long long n, int d,
                                                               int dp, float* __restrict__ dst) {
    const long long total = n * d;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / d;
        const int j = (int)(i - r * d);
        dst[i] = (float)src[(size_t)r * dp + j];
    }
}

// copy n rows of d floats (unpadded, src) into the padded index layout
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ src, long long n, int d,
                                                       float* __restrict__ dst, int dp) {
    const long long total = n * dp;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / dp;
        const int j = (int)(i - r * dp);
        dst[i] = j < d ? src[(size_t)r * d + j] : 0.f;
    }
}

// faiss.normalize_L2 [upstream-faiss fvec_renorm_L2]: nr = |x|^2 (float32);
// if nr > 0: x *= (float)(1.0 / sqrtf(nr)).  Wave per row.
__global__ __launch_bounds__(256) void normalize_kernel(float* __restrict__ x, long long n, int d) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float* xr = x + (size_t)r * d;
    constexpr int VMAX = 8;  // up to 8 float4 per lane: rows of <= 2048 floats stay in registers
    const bool vec = (d & 3) == 0 && d <= 64 * 4 * VMAX && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
    if (vec) {  // one read, one write
        f32x4 v[VMAX];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VMAX; i++) {
            const int j = (lane + 64 * i) * 4;
            v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (j < d) v[i] = *reinterpret_cast<const f32x4*>(xr + j);
            s = fmaf(v[i][0], v[i][0], s);
            s = fmaf(v[i][1], v[i][1], s);
            s = fmaf(v[i][2], v[i][2], s);
            s = fmaf(v[i][3], v[i][3], s);
        }
        s = wave_sum_f32(s);
        if (s > 0.f) {
            const float inv = (float)(1.0 / (double)sqrtf(s));
#pragma unroll
            for (int i = 0; i < VMAX; i++) {
                const int j = (lane + 64 * i) * 4;
                if (j < d) *reinterpret_cast<f32x4*>(xr + j) = v[i] * inv;
            }
        }
        return;
    }
    float s = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float v = xr[j];
        s = fmaf(v, v, s);
    }
    s = wave_sum_f32(s);
    if (s > 0.f) {
        const float inv = (float)(1.0 / (double)sqrtf(s));
        for (int j = lane; j < d; j += 64) xr[j] *= inv;
    }
}

// ---------------------------------------------------------------- visual-word histograms
// One block per image: np.histogram(labels_of_image, bins=K) exactly as the reference's BoVW loop
// calls it (backend/bag_of_visual_words.py:98-106) -- K equal-width bins between the image's OWN
// smallest and largest label (no range argument), not a bincount over [0, K).  The float64
// arithmetic follows numpy's uniform-bin path operation for operation (numpy/lib/_histograms_impl.py:
// scale, truncate, then the two one-ulp corrections against linspace edges j*step + first), with
// contraction off so that no multiply-add pair is fused.  Counts accumulate in LDS.
#define HIST_K_MAX 16384
__global__ __launch_bounds__(256) void bovw_histogram_kernel(const long long* __restrict__ labels,
                                                             const long long* __restrict__ offsets, int K,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
    extern __shared__ unsigned int hist[];  // [K]
    __shared__ long long red_lo[4], red_hi[4];
    const long long img = blockIdx.x;
    const long long b = offsets[img], e = offsets[img + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int j = tid; j < K; j += 256) hist[j] = 0u;
    long long lo = 0x7fffffffffffffffll, hi = -0x7fffffffffffffffll - 1;
    for (long long i = b + tid; i < e; i += 256) {
        const long long a = labels[i];
        lo = a < lo ? a : lo;
        hi = a > hi ? a : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long lo2 = __shfl_xor(lo, off), hi2 = __shfl_xor(hi, off);
        lo = lo2 < lo ? lo2 : lo;
        hi = hi2 > hi ? hi2 : hi;
    }
    if (lane == 0) { red_lo[w] = lo; red_hi[w] = hi; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        lo = red_lo[i] < lo ? red_lo[i] : lo;
        hi = red_hi[i] > hi ? red_hi[i] : hi;
    }
    if (e > b) {
        double first = (double)lo, last = (double)hi, denom;
        if (lo == hi) {  // numpy widens an empty range by half a unit on both sides
            first = first - 0.5;
            last = last + 0.5;
            denom = last - first;
        } else {
            denom = (double)(unsigned long long)(hi - lo);
        }
        const double step = (last - first) / (double)K;  // np.linspace(first, last, K + 1)
        auto edge = [&](long long j) -> double {
            if (j == K) return last;
            const double t = (double)j * step;
            return t + first;
        };
        for (long long i = b + tid; i < e; i += 256) {
            const double a = (double)labels[i];
            const double f = ((a - first) / denom) * (double)K;
            long long idx = (long long)f;
            if (idx == K) idx -= 1;
            if (a < edge(idx)) idx -= 1;
            if (a >= edge(idx + 1) && idx != K - 1) idx += 1;
            atomicAdd(&hist[idx], 1u);
        }
    }
    __syncthreads();
    double* o = out + (size_t)img * K;
    for (int j = tid; j < K; j += 256) o[j] = (double)hist[j];
}
