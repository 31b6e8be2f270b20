// ise_sq.hpp -- kernels of the scalar-quantised index (include/ise_knn.h, ise_sq_*): faiss.IndexScalarQuantizer with
// the 8-bit types.  DESIGN.md 4.15.  Host side: ise_sq.hip.
//
// Codec (float32 throughout): s_j = vdiff_j / 255 (taken once, on the host, when the trained state is set);
//   code   c_j = 0 if s_j == 0, else min(255, max(0, floor((x_j - vmin_j) / s_j)))
//   decode y_j = fmaf(c_j + 0.5, s_j, vmin_j)
// The uniform type is the same kernels with constant vmin / s vectors.
//
// Storage: [n][stride] bytes, stride = d rounded up to a multiple of 64 (a whole number of the scan's steps, so its
// loads need no guard), the bytes past d zero; beside it one float64
// per row, R_i = sum_j (s_j c_j)^2 (sq_row_term: lane l sums j = l, l + 64, ... as one fma chain, then an xor
// butterfly -- the encoder and the add_codes path share it, so a re-read index searches to the same bits).
//
// Score: with o_j = vmin_j + s_j / 2 the decoded row is y_j = o_j + s_j c_j, so with the weights w_j = s_j (x_j - o_j)
// (L2) or s_j x_j (inner product) and the centred code c'_j = c_j - 128
//   L2:  |x - y|^2 = [ |x - o|^2 - 256 sum_j w_j ] + R_i - 2 sum_j w_j c'_j      (clamped at +0)
//   IP:  <x, y>    = [ <x, o>    + 128 sum_j w_j ]       +   sum_j w_j c'_j
// The last sum runs on the matrix cores (sq_scan_kernel): 16 code rows x 16 queries x 32 entries per
// mfma_f32_16x16x32_f16.  A centred code byte is exact in fp16 (1024 + c by a byte permute into 0x64cc, one packed
// subtract of 1152); the weights are staged in LDS, scaled by the query's own power of two 2^sh (max |w| 2^sh in
// [2^14, 2^15)), as fp16 hi + lo limbs w~ (22 bits of a weight); hi and lo feed two float32 accumulator chains.
// Centring halves what the float32 accumulators hold: partial sums of w_j c'_j, up to 128 sum_j |w_j|.  Where a query
// sits near the middle of the trained range the w_j change sign and that is the size of the score itself; where rows and
// queries sit together near one end of a range that an outlier stretched, w_j and c'_j keep one sign over all j and
// the accumulators hold orders of magnitude more than an L2 distance -- its error is bounded by 128 sum_j |w_j|
// (2^-22 of the limbs, 2^-24 per accumulation), not by the score (DESIGN.md 4.15 has the bound and what was measured).
// The large terms that cancel outside the sum --
// the bracket (per query, of the limbs w~ themselves, so the identity is exact; sq_stage_kernel builds it and the limb
// images once per call, the scan's blocks copy them in), R_i and the assembly -- are float64,
// and the result is rounded to float32 once.  On integer data every term is an integer and the result exact.
// A query with a NaN or inf entry (or whose weights overflow) scores NaN everywhere and gets padding.
//
// Selection is the k-pass of ise_cand.hpp (CandBuf; pass_merge_kernel<float>), a pass repeated with a floor key for
// k > SQ_KPASS.  A wave's tile is 64 rows (SQ_RT MFMA row tiles), so a lane ends a tile with 16 scores of ONE query
// (column = lane & 15): the per-query state is kept replicated in the four lanes of that column, and a tile's keys are
// appended at per-column popcount positions.
//
// LDS per pass: QT x (two limb images of 2 dpad + 16 bytes, dpad = d rounded up to 64; the 16 bytes stagger the
// queries over the banks) + QT x 4 KiB of selection buffers + QT x 16 bytes; QT = 16 while that fits 160 KiB
// (d <= 1472), else 8 (sq_qt).
//
// The scan's body (sq_scan_body) also serves the inverted lists over these rows (ise_ivfsq.hpp), which
// walk a work list of tiles instead of the whole array; this file's kernels do not depend on that one.
#pragma once
#include "ise_cand.hpp"

#define SQ_WAVES 4    /* waves per block */
#define SQ_RT 4       /* MFMA row tiles (16 rows) of a wave's tile */
#define SQ_TILE (16 * SQ_RT) /* rows of a wave's tile */
#define SQ_RING 4     /* steps (64 entries of the tile's rows: 4 KiB per wave) in flight or in use per wave */
#define SQ_KPASS 32   /* results per query and pass */
#define SQ_CAP 128    /* keys of a wave's buffer per query: two registers per lane in wave_cut */
#define SQ_CUT_MAX 48 /* most keys a cut in the stream keeps (at least kp) */
#define SQ_QT_MAX 16  /* most queries per pass: the MFMA's columns */
#define SQ_STAGE_CHUNK 64 /* queries staged per sq_stage_kernel launch: a multiple of every QT */
#define SQ_LDS_LIMIT (160 * 1024)
#define SQ_BLOCK_TILES 2 /* wave tiles per wave a short index's grid is sized for: 2 * SQ_WAVES * SQ_TILE rows per block */

static_assert(SQ_TILE == 64, "a tile adds at most 64 keys per query; the row-term loads are 16-byte aligned");
template <int QT>
using SqCand = CandBuf<QT, SQ_WAVES, SQ_CAP, SQ_TILE, SQ_CUT_MAX, SQ_KPASS>;

constexpr int sq_dpad(int d) { return (d + 63) / 64 * 64; }
constexpr int sq_stride(int d) { return sq_dpad(d); }
constexpr size_t sq_qrow_bytes(int d) { return (size_t)2 * sq_dpad(d) + 16; }
constexpr size_t sq_lds_bytes(int d, int qt) { return (size_t)qt * (2 * sq_qrow_bytes(d) + SQ_WAVES * SQ_CAP * 8 + 16); }
// queries per pass
constexpr int sq_qt(int d) { return sq_lds_bytes(d, 16) <= SQ_LDS_LIMIT ? 16 : 8; }
static_assert(sq_qt(1472) == 16 && sq_qt(1473) == 8 && sq_lds_bytes(ISE_SQ_MAX_D, 8) <= SQ_LDS_LIMIT,
              "every QT(d) fits the CU's LDS");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- the row term R = sum_j (s_j c_j)^2 of the wave's row; code(j) gives byte j.  Every lane returns it
template <class Code>
__device__ __forceinline__ double sq_row_term(Code code, const float* __restrict__ step, int d, int lane) {
    double acc = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double t = (double)step[j] * (double)code(j);  // exact
        acc = fma(t, t, acc);
    }
    return wave_sum_f64(acc);
}

// ---- encoding.  A wave owns a row at a time, SQ_ENC_ROWS rows per block.  codes: row stride `stride` (bytes at or
// past d are not written); rterm (may be null): one double per row.  A NaN or inf entry sets *bad (the caller then
// drops the whole call); its byte is whatever the arithmetic gives.
#define SQ_ENC_ROWS 64
static __global__ __launch_bounds__(SQ_WAVES * 64) void sq_encode_kernel(const float* __restrict__ x, long long n, int d,
                                                                         const float* __restrict__ vmin,
                                                                         const float* __restrict__ step,
                                                                         uint8_t* __restrict__ codes, int stride,
                                                                         double* __restrict__ rterm,
                                                                         unsigned int* __restrict__ bad) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long r0 = (long long)blockIdx.x * SQ_ENC_ROWS;
    for (int i = w; i < SQ_ENC_ROWS; i += SQ_WAVES) {
        const long long row = r0 + i;  // wave-uniform
        if (row >= n) break;
        const float* xs = x + (size_t)row * d;
        uint8_t* cs = codes + (size_t)row * stride;
        float mark = 0.f;
        double acc = 0.0;
        for (int j = lane; j < d; j += 64) {
            const float xv = xs[j], s = step[j];
            mark += nonfinite_mark(xv);
            float t = floorf((xv - vmin[j]) / s);
            t = t >= 255.f ? 255.f : (t > 0.f ? t : 0.f);  // NaN -> 0
            if (s == 0.f) t = 0.f;
            cs[j] = (uint8_t)(int)t;
            const double sc = (double)s * (double)t;
            acc = fma(sc, sc, acc);  // sq_row_term's chain: the same j, the same order
        }
        acc = wave_sum_f64(acc);
        mark = wave_sum_f32(mark);
        if (lane == 0) {
            if (rterm) rterm[row] = acc;
            if (mark != mark) atomicOr(bad, 1u);
        }
    }
}

// the row terms of codes that arrived ready-made (add_codes)
static __global__ __launch_bounds__(SQ_WAVES * 64) void sq_rowterm_kernel(const uint8_t* __restrict__ codes, int stride,
                                                                          long long n, int d,
                                                                          const float* __restrict__ step,
                                                                          double* __restrict__ rterm) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long r0 = (long long)blockIdx.x * SQ_ENC_ROWS;
    for (int i = w; i < SQ_ENC_ROWS; i += SQ_WAVES) {
        const long long row = r0 + i;
        if (row >= n) break;
        const uint8_t* cs = codes + (size_t)row * stride;
        const double r = sq_row_term([&](int j) { return cs[j]; }, step, d, lane);
        if (lane == 0) rterm[row] = r;
    }
}

// ---- decoding: x[i][j] = fmaf(code[i][j] + 0.5, s_j, vmin_j)
static __global__ void sq_decode_kernel(const uint8_t* __restrict__ codes, int stride, long long n, int d,
                                        const float* __restrict__ vmin, const float* __restrict__ step,
                                        float* __restrict__ x) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * d) return;
    const long long r = i / d;
    const int j = (int)(i % d);
    x[i] = fmaf((float)codes[(size_t)r * stride + j] + 0.5f, step[j], vmin[j]);
}

// ---- scan
struct SqScanParams {
    const uint8_t* codes;  // [cap][stride]
    const double* rterm;   // [cap], cap a multiple of SQ_TILE
    int d, stride;
    long long n;
    const unsigned char* qrec;  // the pass's first query's staged record (sq_stage_kernel), nqt of them
    int nqt, kp;        // queries of the pass (<= QT), results of this pass (<= SQ_KPASS)
    int ip;             // inner product: the key is taken of -score
    const u64* lo;      // [nqt] smallest key admitted (KEY_PAD: the query is finished); null in the first pass: 0
    u64* lists;         // [grid][QT][SQ_KPASS]: one sorted list per block and query, KEY_PAD behind the last
};

// bytes (b0 b1 b2 b3 | b4 .. b7) -> eight fp16 of the values less 128: 0x64cc is 1024 + cc
__device__ __forceinline__ f16x8 sq_bytes_to_f16(uint32_t w0, uint32_t w1) {
    u32x4 v;
    v[0] = __builtin_amdgcn_perm(0x64646464u, w0, 0x04010400u);
    v[1] = __builtin_amdgcn_perm(0x64646464u, w0, 0x04030402u);
    v[2] = __builtin_amdgcn_perm(0x64646464u, w1, 0x04010400u);
    v[3] = __builtin_amdgcn_perm(0x64646464u, w1, 0x04030402u);
    const _Float16 k = (_Float16)1152.f;
    return __builtin_bit_cast(f16x8, v) - (f16x8){k, k, k, k, k, k, k, k};
}

// ---- query staging: one wave per query of the call's chunk.  A query's record is what the scan keeps of it in LDS:
// [hi limb image, qrow bytes][lo limb image, qrow bytes][float64 bracket][int32 sh][4 bytes unused], qrow = 2 dpad + 16
// (fp16 limbs of 2^sh w_j, zeros behind d).  The sums run lane l over j = l, l + 64, ... as one fma chain, then an xor
// butterfly: they do not depend on where in a batch the query stands.
constexpr size_t sq_rec_bytes(int d) { return 2 * sq_qrow_bytes(d) + 16; }
struct SqStageParams {
    const float* q;  // [nq][d]
    int nq, d, ip;
    const float* step;  // [d] s_j
    const float* off;   // [d] o_j = vmin_j + s_j / 2
    unsigned char* rec;  // [nq][sq_rec_bytes(d)]
};
static __global__ __launch_bounds__(64) void sq_stage_kernel(const SqStageParams p) {
    const int lane = threadIdx.x, q = blockIdx.x;
    const int dpad = sq_dpad(p.d), qrow = 2 * dpad + 16;
    const float* x = p.q + (size_t)q * p.d;
    unsigned char* rec = p.rec + (size_t)q * (2 * qrow + 16);
    float amax = 0.f, mark = 0.f;
    double cst = 0.0, wsum = 0.0;
#pragma unroll 8
    for (int j = lane; j < p.d; j += 64) {
        const float xv = x[j], o = p.off[j];
        const float base = p.ip ? xv : xv - o;
        const float wv = p.step[j] * base;
        amax = fmaxf(amax, fabsf(wv));
        mark += nonfinite_mark(xv) + nonfinite_mark(wv);
        cst = p.ip ? fma((double)xv, (double)o, cst) : fma((double)base, (double)base, cst);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    mark = wave_sum_f32(mark);
    cst = wave_sum_f64(cst);
    const bool skip = mark != 0.f || !(amax <= FLT_MAX);
    const int sh = (amax > 0.f && !skip) ? 14 - ilogbf(amax) : 0;
    _Float16* hi = reinterpret_cast<_Float16*>(rec);
    _Float16* lo = reinterpret_cast<_Float16*>(rec + qrow);
#pragma unroll 8
    for (int j = lane; j < dpad + 8; j += 64) {  // the 16 stagger bytes too: nothing of a record is left unwritten
        float V = 0.f;
        if (!skip && j < p.d) V = ldexpf(p.step[j] * (p.ip ? x[j] : x[j] - p.off[j]), sh);
        const _Float16 h1 = (_Float16)V;
        const float r1 = V - (float)h1;  // exact
        const _Float16 h2 = (_Float16)r1;
        hi[j] = h1;
        lo[j] = h2;
        wsum += (double)h1 + (double)h2;
    }
    wsum = ldexp(wave_sum_f64(wsum), -sh);  // sum_j w~_j
    if (lane == 0) {
        *reinterpret_cast<double*>(rec + 2 * qrow) = skip ? (double)__builtin_nanf("") : (p.ip ? cst + 128.0 * wsum : cst - 256.0 * wsum);
        *reinterpret_cast<int*>(rec + 2 * qrow + 8) = sh;
        *reinterpret_cast<int*>(rec + 2 * qrow + 12) = 0;
    }
}

// The scan of one pass, for both layouts (IVF false: the flat index's rows [0, n), sq_scan_kernel; IVF true: the work
// list of an inverted-list pass, P = SqIvfScanParams, ise_ivfsq.hpp).  What differs stands under `if constexpr (IVF)`:
// which tile a wave's next unit names, the row mask (row < n | position < valid rows and the query's mask bit) and the
// key's low word (row | ids[slot]).  The record copy-in, the byte -> fp16 MFMA step, the float64 assembly, the cuts and
// the block's final selection exist once.
template <int QT, bool IVF, class P>
__device__ __forceinline__ void sq_scan_body(const P& p) {
    extern __shared__ __align__(16) unsigned char smem_sq[];
    const int dpad = sq_dpad(p.d);
    const int qrow = 2 * dpad + 16;  // bytes of one limb image
    const int rec = 2 * qrow + 16;   // bytes of one query's record
    u64* buf = reinterpret_cast<u64*>(smem_sq + QT * rec);  // [SQ_WAVES][QT][SQ_CAP]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    long long nent = 0;  // IVF: entries of the group's work list
    if constexpr (IVF) {
        nent = (long long)__builtin_amdgcn_readfirstlane((int)*p.count);
        if (blockIdx.x == 0 && threadIdx.x == 0 && nent) atomicAdd(p.tiles_loaded, (unsigned long long)nent);
        if ((long long)blockIdx.x * SQ_WAVES >= nent) {  // no entry for this block: its lists are padding
            for (int i = threadIdx.x; i < p.nqt * SQ_KPASS; i += SQ_WAVES * 64)
                p.lists[(size_t)blockIdx.x * QT * SQ_KPASS + i] = KEY_PAD;
            return;
        }
    }
    {  // the pass's records, zeros behind the last: every 16-byte load is independent
        const u32x4* src = reinterpret_cast<const u32x4*>(p.qrec);
        u32x4* dst = reinterpret_cast<u32x4*>(smem_sq);
        const int have = p.nqt * rec / 16, units = QT * rec / 16;
        for (int i = threadIdx.x; i < units; i += SQ_WAVES * 64) dst[i] = i < have ? src[i] : u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();

    const int g = lane >> 4, c16 = lane & 15;
    const int qsrc = c16 & (QT - 1);  // QT = 8: columns 8 .. 15 repeat 0 .. 7 and are never selected from
    // per-query state of the wave, query q in the four lanes of column q: keys held, threshold, floor
    SqCand<QT> cand(buf, w, c16, p.kp);
    const u64 lo_v = c16 < p.nqt ? (p.lo ? p.lo[c16] : 0ull) : KEY_PAD;
    const u64 below_mask = (1ull << (16 * g)) - 1ull;  // the lower lanes of my column
    const double cq = *reinterpret_cast<const double*>(smem_sq + qsrc * rec + 2 * qrow);
    const int shq = *reinterpret_cast<const int*>(smem_sq + qsrc * rec + 2 * qrow + 8);

    long long ntiles;  // units of the pass: the index's tiles | the work list's entries
    if constexpr (IVF) ntiles = nent;
    else ntiles = (p.n + SQ_TILE - 1) / SQ_TILE;
    const long long tstep = (long long)gridDim.x * SQ_WAVES;
    const int nsteps = dpad >> 6;  // 64 entries per step: lane group g takes bytes [64 S + 16 g, + 16) of its row
    const unsigned char* bh = smem_sq + qsrc * rec + 32 * g;
    const unsigned char* bl = bh + qrow;
    // the 16 bytes of step S of the lane's rows in tile t (a row at or beyond n reads the last row and is masked).  No
    // branch: every load is issued, so nothing between two loads waits for one of them
    auto load_step = [&](u32x4(&a)[SQ_RT], long long t, int S) {
        const int kb = 64 * S + 16 * g;
#pragma unroll
        for (int rt = 0; rt < SQ_RT; rt++) {
            long long r = t * SQ_TILE + rt * 16 + c16;
            if constexpr (!IVF) r = r < p.n ? r : p.n - 1;  // (the lists' slots are whole tiles)
            a[rt] = *reinterpret_cast<const u32x4*>(p.codes + (size_t)r * p.stride + kb);
        }
    };
    // the lane holds query c16 against rows t * 64 + 16 rt + 4 g + reg: score, gate, append; then the cuts
    // IVF: valid = rows of the tile that belong to its list, qm = the list's query mask, idv = the lane's rows' ids
    auto epilogue = [&](long long t, const f32x4(&acc0)[SQ_RT], const f32x4(&acc1)[SQ_RT], const double2(&rr)[SQ_RT][2], int valid,
                        uint32_t qm, const u32x4(&idv)[SQ_RT]) {
        const bool probes = (qm >> c16) & 1u;
#pragma unroll
        for (int rt = 0; rt < SQ_RT; rt++) {
            const long long rbase = t * SQ_TILE + rt * 16 + 4 * g;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const long long row = rbase + reg;
                const double dot = ldexp((double)acc0[rt][reg] + (double)acc1[rt][reg], -shq);
                const double rterm = (reg & 1) ? rr[rt][reg >> 1].y : rr[rt][reg >> 1].x;
                float sc = (float)(p.ip ? cq + dot : (cq + rterm) - 2.0 * dot);
                if (!p.ip) sc = sc < 0.f ? 0.f : sc;  // NaN stays NaN
                sc += 0.f;                            // a zero is +0
                const float s = p.ip ? -sc : sc;
                u64 key;
                bool c;
                if constexpr (IVF) {
                    key = ((u64)ord_f32(s) << 32) | idv[rt][reg];
                    c = rt * 16 + 4 * g + reg < valid && probes && s < FLT_MAX && key >= lo_v && key < cand.thr;
                } else {
                    key = ((u64)ord_f32(s) << 32) | (uint32_t)row;
                    c = row < p.n && s < FLT_MAX && key >= lo_v && key < cand.thr;
                }
                const u64 mk = __ballot(c);
                if (mk) {
                    const u64 col = (mk >> c16) & 0x0001000100010001ull;  // my column's four lanes
                    if (c) cand.keys(c16)[cand.cnt + __popcll(col & below_mask)] = key;
                    cand.cnt += __popcll(col);
                }
            }
        }
        cand.make_room();
    };

    // ---- main loop: the wave's (tile, step) sequence through a ring of SQ_RING steps' bytes, requested SQ_RING - 1
    // steps (across tile ends too) ahead of the MFMAs that consume them
    const long long t0 = (long long)blockIdx.x * SQ_WAVES + w;
    long long lt = t0, ct = t0;  // the tile being requested | computed
    int lS = 0, cS = 0;          // and the step in it
    // IVF: lt / ct count ENTRIES; an entry is (tile, valid rows, query mask, 0).  The entry behind the one in use is
    // fetched a tile ahead on either side (wave-uniform loads), so no code-byte request waits for the entry it has just
    // asked for.  Behind the wave's last entry: the list's last entry again -- a valid tile, unused
    [[maybe_unused]] auto entry_at = [&](long long e) {
        if constexpr (IVF) return p.work[e < nent ? e : nent - 1];
        else return u32x4{0u, 0u, 0u, 0u};
    };
    [[maybe_unused]] uint32_t ltile = 0, lnext = 0;
    [[maybe_unused]] u32x4 cent = {0u, 0u, 0u, 0u}, cnext = {0u, 0u, 0u, 0u};
    if constexpr (IVF) {
        ltile = entry_at(lt)[0];
        lnext = entry_at(lt + tstep)[0];
        cent = entry_at(ct);
        cnext = entry_at(ct + tstep);
    }
    auto request = [&](u32x4(&a)[SQ_RT]) {
        if constexpr (IVF) load_step(a, (long long)ltile, lS);
        else load_step(a, lt < ntiles ? lt : ntiles - 1, lS);  // behind the wave's last tile: the index's last tile again, unused
        if (++lS == nsteps) {
            lS = 0;
            lt += tstep;
            if constexpr (IVF) {
                ltile = lnext;
                lnext = entry_at(lt + tstep)[0];
            }
        }
    };
    u32x4 ring[SQ_RING][SQ_RT];
#pragma unroll
    for (int j = 0; j < SQ_RING - 1; j++) request(ring[j]);
    f32x4 acc0[SQ_RT], acc1[SQ_RT];
#pragma unroll
    for (int rt = 0; rt < SQ_RT; rt++) acc0[rt] = acc1[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    double2 rr[SQ_RT][2];  // the row terms of the tile being computed (the inner product never uses them)
    [[maybe_unused]] u32x4 idv[SQ_RT] = {};  // IVF: and the ids in its slots
    bool done = ct >= ntiles;
    while (!done) {
#pragma unroll
        for (int j = 0; j < SQ_RING; j++) {
            if (!done) {
                // the tile's row terms are requested ahead of the younger code bytes: the epilogue's wait for them
                // does not drain the ring
                if (cS == 0) {
                    long long tile = ct;
                    if constexpr (IVF) tile = (long long)cent[0];
#pragma unroll
                    for (int rt = 0; rt < SQ_RT; rt++)
#pragma unroll
                        for (int h2 = 0; h2 < 2; h2++)
                            rr[rt][h2] = *reinterpret_cast<const double2*>(p.rterm + tile * SQ_TILE + rt * 16 + 4 * g + 2 * h2);
                    if constexpr (IVF) {
#pragma unroll
                        for (int rt = 0; rt < SQ_RT; rt++)
                            idv[rt] = *reinterpret_cast<const u32x4*>(p.ids + tile * SQ_TILE + rt * 16 + 4 * g);
                    }
                }
                request(ring[(j + SQ_RING - 1) % SQ_RING]);
                const f16x8 bh0 = *reinterpret_cast<const f16x8*>(bh + 128 * cS);
                const f16x8 bh1 = *reinterpret_cast<const f16x8*>(bh + 128 * cS + 16);
                const f16x8 bl0 = *reinterpret_cast<const f16x8*>(bl + 128 * cS);
                const f16x8 bl1 = *reinterpret_cast<const f16x8*>(bl + 128 * cS + 16);
#pragma unroll
                for (int rt = 0; rt < SQ_RT; rt++) {
                    const f16x8 a0 = sq_bytes_to_f16(ring[j][rt][0], ring[j][rt][1]);
                    const f16x8 a1 = sq_bytes_to_f16(ring[j][rt][2], ring[j][rt][3]);
                    acc0[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bh0, acc0[rt], 0, 0, 0);
                    acc1[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bl0, acc1[rt], 0, 0, 0);
                    acc0[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bh1, acc0[rt], 0, 0, 0);
                    acc1[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bl1, acc1[rt], 0, 0, 0);
                }
                if (++cS == nsteps) {
                    if constexpr (IVF) epilogue((long long)cent[0], acc0, acc1, rr, (int)cent[1], cent[2], idv);
                    else epilogue(ct, acc0, acc1, rr, 0, 0u, idv);
#pragma unroll
                    for (int rt = 0; rt < SQ_RT; rt++) acc0[rt] = acc1[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    cS = 0;
                    ct += tstep;
                    done = ct >= ntiles;
                    if constexpr (IVF) {
                        cent = cnext;
                        cnext = entry_at(ct + tstep);
                    }
                }
            }
        }
    }
    cand.fold(p.nqt, p.lists + (size_t)blockIdx.x * QT * SQ_KPASS);
}

template <int QT>
__global__ __launch_bounds__(SQ_WAVES * 64) void sq_scan_kernel(const SqScanParams p) {
    sq_scan_body<QT, false>(p);
}
