// ise_scan.hpp -- the streaming distance + top-k kernel (see ise_knn.hip for the overview).
#pragma once
#include "ise_common.hpp"
#include "ise_scan_params.hpp"
#include "ise_byte_layout.hpp"
#include "ise_select.hpp"
#include "ise_stage.hpp"

// build-time switch of the filtered final phase of the exchange kernels (on in every shipped build; a dev build
// with -DISE_FINAL_FILTER=0 is what an A/B of it runs against)
#ifndef ISE_FINAL_FILTER
#define ISE_FINAL_FILTER 1
#endif

#ifdef ISE_ABLATE
#define ABL(bit) (p.ablate & (bit))
#define STAMP(i)                                                                                   \
    do {                                                                                           \
        if (p.stamps && lane == 0)                                                                 \
            p.stamps[((size_t)blockIdx.x * W + w) * 16 + (i)] = __builtin_amdgcn_s_memrealtime();  \
    } while (0)
#define CSTAMP(i)                                                                                  \
    do {                                                                                           \
        if (p.stamps && lane == 0)                                                                 \
            p.stamps[((size_t)blockIdx.x * W + w) * 16 + (i)] = __builtin_amdgcn_s_memtime();      \
    } while (0)
#else
#define ABL(bit) 0
#define STAMP(i) do {} while (0)
#define CSTAMP(i) do {} while (0)
#endif

// CH : k-steps (16 floats each) per register chunk; dp/16 is a multiple of CH
// W  : waves per block
// T  : query tiles of 16 per pass: the index stream is read once for 16*T queries
//      (one MFMA column block and two accumulator chains per tile)
//
// Top-k bookkeeping (all off the streaming path, per query):
//   boot   every wave scores its first row tile and dumps all 16x16 keys; two block
//          barriers later the query has a block list bootw of between k and kb of
//          the best of those W*16 rows (windowed cut) and a threshold tauS = the cut.
//          SEEDED boot (byte shadow rows, T = 1, W = 8; blocks whose every wave reads the exchange): no cut.  A
//          wave's first TWO row tiles are the boot window; their 2 x 16 x 16 keys go unfiltered to an LDS home.  The
//          block's best first-tile key per query is folded with LDS atomics and published by the last wave to
//          arrive; behind the second tile (one barrier) the query's owner wave reads the exchange and seeds bootw
//          with the home keys at or below the bound, tauS = the bound; a second barrier, then steady state.  Without
//          a bound, or with more than kb home keys under it, the owner cuts the 256 home keys as above.
//   steady a lane holds 4 scores per row tile for one query per query tile and
//          compares them with its copy of the threshold; survivors (a few per wave
//          over the whole kernel) are appended to the wave's private list; at
//          MERGE_TRIG entries the wave takes the query's LDS lock, folds its list
//          into bootw (exact top-k of the union, sorted) and publishes the new k-th
//          key, so tauS tracks the block's running k-th best.
//   final  one wave selects the exact sorted top-k of bootw + what is left in the W
//          private lists and writes the block's list to HBM.  In the exchange kernels a wave that
//          obtained the grid-wide bound of a query first drops every key above it: of the ~k keys a
//          block holds (k of its first W*16 rows seeded the list) one or two lie below a bound as
//          tight as the k-th best of a 65k-row sample, and only they are ranked and written, KEY_PAD
//          behind them (the merge reads short lists).  No dropped key can be among the k smallest of
//          the launch (see the final phase), so the merged keys are unchanged.
//   exchange (8-wave kernels with T >= 2, once per block): at boot a block publishes, per query, the score of its best boot
//          row (one 8-byte store: launch seq << 32 | ord(score)).  After its first row tile a
//          wave reads the entries of all blocks for its queries: the k-th smallest of those scores
//          is the k-th best of nblocks DISTINCT rows, hence an upper bound of the final k-th
//          distance -- as tight as the k-th best of a W*16*nblocks-row sample (32k-64k rows)
//          instead of the block's own W*16.  It lowers tauS, and the wave keeps it for the final
//          phase of its queries (xbound); entries not yet written (or of an older launch: seq
//          mismatch) just count as absent.  No polling, no ordering needed.  The seeded-boot kernel reads after
//          its second tile, requests a lane's entries four at a time and selects among the 64 per-lane minima
//          (still k distinct rows: a valid bound); its thresholds obey the two invariants stated at seed_phase.
//
// SHIFT (fp32 L2 only): distances are translation invariant, and the expanded form
// |x|^2 + |y|^2 - 2 x.y loses digits when the rows share a large common component
// (CNN embeddings: |y|^2 ~ 1e5, neighbour distances ~ 1e-1).  The index keeps a shift
// vector mu (the column mean of its rows); norms are |y - mu|^2, queries are staged as
// x - mu and the row fragments are shifted in registers before the MFMAs (4 VALU subs per
// k-step), so every term is as small as the data's spread, not its offset.  Rows stay
// stored unshifted (reconstruct / write_index are exact).  What the expanded form still
// loses is bounded rigorously (beta) and the rows are keyed by that lower bound: this
// kernel is the FILTER of the exact search, ise_exact.hpp holds the verifier.
//
// HALF (with SHIFT; long float32 L2 indexes): the same filter read through the index's fp16 SHADOW rows
// u~ = 2^-s_r fp16(2^s_r (y - mu)) instead of the float32 rows -- half the bytes, 16x16x32 f16 MFMAs.  The
// query v = x - mu is staged exactly as fp16 hi + lo halves scaled by 2^sh (two MFMAs per k-step, one per
// accumulator chain), and a row is keyed by lo = (max(0, sqrt(max(0, d~ - beta tt)) - e_r - e_q))^2
// with d~ = |u~|^2 + |v~|^2 - 2 u~.v~, tt = |u~|^2 + |v~|^2: a rigorous lower bound of the float32
// direct-difference distance the verifier computes (tests/half_filter_ref.py restates it).
//
// BYTE (with SHIFT; long float32 L2 indexes, k <= 10): the same filter read through the BYTE shadow rows
// q = rint((y - mu) / c_r) in [-127, 127], u~ = c_r q -- a quarter of the float32 bytes, 16x16x64 i8 MFMAs.  The
// query v = x - mu is staged as two int8 limbs of V = 2^sh v (V ~ 256 hi + lo, one exact i32 accumulator chain
// per limb), and a row is keyed by the expanded-form bound byte_lower_bound (ise_common.hpp), which uses the
// float32 norm |y - mu|^2 and bounds only the cross terms by e_r and e_q (tests/byte_filter_ref.py).
template <int CH, int W, int T, bool BF16, bool SHIFT, int RM = ROWS_OWN>
__global__ __launch_bounds__(W * 64, T == 1 ? W / 2 : (W / 4 > 0 ? W / 4 : 1)) void scan_kernel(const ScanParams p) {
    constexpr bool HALF = RM == ROWS_F16, BYTE = RM == ROWS_I8 || RM == ROWS_I8_ONE, SHADOW = HALF || BYTE;
    static_assert(!(BF16 && SHIFT), "the shift is applied to fp32 rows only");
    static_assert(!SHADOW || SHIFT, "shadow rows belong to float32 L2 indexes");
    constexpr bool F32S = SHIFT && !SHADOW;  // float32 rows shifted in registers
    if (p.gate && *p.gate == 0u) return;  // a queued rerun that is not needed
    constexpr int BLOCK_THREADS = W * 64;
    // threshold exchange: compiled into the 8-wave kernels with two or more query tiles, where the candidate
    // bookkeeping is what it saves (nq = 48: 560 -> 508 us; nq = 32: 399 (16 waves) -> 383 us).  Not into the
    // 16-wave two-tile kernel (the read costs more than it saves there: 399 -> 406 us; the host picks it
    // for short indexes, where the exchange would not run anyway) nor at T = 1 (neutral).
    // The byte shadow kernel takes it at T = 1 as well: its kc = 32 lists over ~2000-row blocks admit twice the
    // candidates of the k + 4 lists, and a grid-wide threshold after the first tile cuts that bookkeeping.
    constexpr bool XCHG = T >= 3 || (T == 2 && W == 8) || (BYTE && T == 1 && W == 8);
    constexpr bool FFILT = XCHG && ISE_FINAL_FILTER;    // final phase filtered by the exchange bound (below)
    // boot without the cut (the byte shadow one-tile kernel): a two-tile boot window seeded from the exchange bound
    constexpr bool NBOOT = scan_seeded_boot(BYTE, W, T);
    static_assert(!NBOOT || XCHG, "the seeded boot reads the exchange");
    constexpr int NQ = 16 * T;                        // queries per block pass
    // threads staging one query row (per tile).  16-wave blocks stage with their first 8 waves: |x|^2 then has the
    // summation order of the 8-wave kernels (and of short_scan_kernel), and the bf16 L2 distances, which carry it,
    // come out the same bits whichever kernel scans (4-wave blocks exist for rows no other kernel takes)
    constexpr int TPR = W >= 16 ? 32 : BLOCK_THREADS / 16;
    constexpr int KPLB = (W * 16 + 63) / 64;          // boot: keys per lane
    constexpr int KPLF = (KB_MAX + W * CAP + 63) / 64;  // final: keys per lane (worst case)
    static_assert(KB_MAX + CAP <= 64 && MERGE_TRIG + 4 <= CAP, "list sizes");
    extern __shared__ __align__(16) unsigned char smem[];
    const int S = p.qs_stride;
    const int kb = p.kb;
    float* mus = reinterpret_cast<float*>(smem);                // [S] shift vector (SHIFT only)
    float* qs = mus + S;                                        // [NQ][S]
    float* xn = qs + NQ * S;                                    // [NQ]
    float* xe = xn + NQ;                                        // [NQ] SHADOW: e_q
    int* xsh = reinterpret_cast<int*>(xe + NQ);                 // [NQ] SHADOW: the query's scale exponent sh
    u64* tauS = reinterpret_cast<u64*>(xn + (SHADOW ? 3 : 1) * NQ);  // [NQ]
    int* bwc = reinterpret_cast<int*>(tauS + NQ);               // [NQ]
    int* lockS = bwc + NQ;                                      // [NQ]
    int* cntS = lockS + NQ;                                     // [W][NQ]
    u64* bootw = reinterpret_cast<u64*>(cntS + W * NQ);         // [NQ][kb]
    u64* cand = bootw + NQ * kb;                                // [W][NQ][CAP]
    u64* boot = cand;                                           // [NQ][W*16], dead before cand is used
    u64* home2 = cand + (size_t)W * NQ * CAP;                   // NBOOT: [NQ][W*16] keys of the window's second tile
    u64* bminS = home2 + (size_t)NQ * W * 16;                   // NBOOT: [NQ] smallest first-tile key of the block
    int* arrS = reinterpret_cast<int*>(bminS + NQ);             // NBOOT: waves whose first tile is folded into bminS

    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: a scalar
    const int c = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.y * NQ;
    const int nqt = min(NQ, p.nq - q0);  // valid queries of this pass
    const int k = p.k;
    const int nsteps = p.row_slots >> 2;  // one k-step = 64 bytes of a row: 16 floats or 32 bf16
    const int t0 = blockIdx.x * p.tiles_per_block;
    const int t1 = min(t0 + p.tiles_per_block, p.tiles_total);
    const bool l2 = p.metric == ISE_METRIC_L2;
    STAMP(0);

    auto load_chunk = [&](f32x4(&a)[CH], int tile, int s0) {
        // byte shadow rows are tile-blocked (ise_byte_layout.hpp): lane (c, g) wants unit 4 s + g of row 16 tile + c,
        // byte_unit_index(16 tile + c, 4 s + g, row_slots) = tile * 16 * row_slots + s * 64 + lane -- the
        // wave-uniform part is inlined here, a k-step is 1 KB contiguous per wave instruction
        // Loads: fp16 and float32 rows are row-major, a wave load covers 16 rows x 64 B, half lines whose other half
        // the next load wants from L2, and non-temporal loads lose with that shape (float32: 369 vs 343 us; byte rows
        // row-major: step 107.6 vs 91.4 us) -- plain loads.  Blocked byte rows, whole lines: the scan that runs alone
        // (ROWS_I8) is faster non-temporal (isolated 96.6 vs 105.9 us), the one-request kernel of the deep plan
        // (ROWS_I8_ONE), which always shares the device with its neighbour's scan, is faster plain (step 88.9 vs
        // 89.9 us) -- DESIGN.md 5.0g.  Compile-time: the one-tile kernels have no register to spare for a branch.
        constexpr bool BLOCKED = BYTE;
        constexpr bool NT = RM == ROWS_I8;
        constexpr int STEP = BLOCKED ? 1024 : 64;  // bytes from one k-step of a lane to the next
        const char* base = static_cast<const char*>(p.xb) +
                           (BLOCKED ? (((size_t)tile * 16 * p.row_slots + (size_t)s0 * 64 + lane) << 4)
                                    : ((((size_t)tile * 16 + c) * p.row_slots + 4 * s0 + g) << 4));
        if (ABL(32)) base = static_cast<const char*>(p.xb) + (((size_t)c * p.row_slots + g) << 4);  // dev: L1-hot
        if (ABL(128)) return;  // dev: no index loads at all (registers keep whatever they hold)
#pragma unroll
        for (int s = 0; s < CH; s++) {
            const f32x4* src = reinterpret_cast<const f32x4*>(base + STEP * s);
            a[s] = NT ? __builtin_nontemporal_load(src) : *src;
        }
    };
    auto load_norms = [&](int tile) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(p.norms + (size_t)tile * 16 + 4 * g);
    };
    auto load_meta = [&](const void* m, int tile) -> f32x4 {  // HALF: e_r or s_r, BYTE: packed c_r | e_r / c_r
        if constexpr (!SHADOW) return (f32x4){0.f, 0.f, 0.f, 0.f};
        return *reinterpret_cast<const f32x4*>(static_cast<const float*>(m) + (size_t)tile * 16 + 4 * g);
    };

    // ---- query staging, step 1: REQUEST the query tiles first (small, L2-resident after
    // the first block): issued behind the index prefetch they would queue for microseconds.
    // TPR threads per query row, QV 16-byte pieces per thread and tile.
    // A thread handles 16-byte LDS slots j4 = t, t + TPR, ...: 4 floats (f32 store) or 8
    // bf16 converted from 8 floats (bf16 store), i.e. FPS float4 loads per slot.
    constexpr int FPS = BF16 ? 2 : 1;
    constexpr int QV = 8;              // float4 registers per thread and tile
    constexpr int QVS = QV / FPS;      // slots per thread and tile
    const int S4 = S >> 2;             // 16-byte slots per LDS query row
    const int dslots = BF16 ? (p.d >> 3) : (p.d >> 2);  // slots that carry data (vector path only)
    const bool vec_q = !SHADOW && (p.d & (BF16 ? 7 : 3)) == 0 && ((reinterpret_cast<uintptr_t>(p.q) & 15) == 0) &&
                       S4 <= TPR * QVS;
    f32x4 qv[T][QV];
    f32x4 muv[F32S ? QVS : 1];
    const bool stager = tid < 16 * TPR;  // whole waves
    if (F32S && vec_q && stager) {
#pragma unroll
        for (int i = 0; i < QVS; i++) {
            const int j4 = tid % TPR + i * TPR;
            muv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (j4 < dslots) muv[i] = *reinterpret_cast<const f32x4*>(p.mu + 4 * j4);
        }
    }
    if (vec_q && stager) {
#pragma unroll
        for (int tq = 0; tq < T; tq++) {
            const int cc = tq * 16 + tid / TPR, t = tid % TPR;
            const bool rowok = cc < nqt && !ABL(1);
            const float* src = p.q + (size_t)(q0 + (rowok ? cc : 0)) * p.d;
#pragma unroll
            for (int i = 0; i < QVS; i++) {
                const int j4 = t + i * TPR;
#pragma unroll
                for (int f = 0; f < FPS; f++) {
                    qv[tq][i * FPS + f] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (rowok && j4 < dslots)
                        qv[tq][i * FPS + f] = *reinterpret_cast<const f32x4*>(src + 4 * (j4 * FPS + f));
                }
            }
        }
    }
    // shadow rows: the same request, through ise_stage.hpp (mu once, then the rows of every query tile)
    const int PS = p.row_slots * (BYTE ? 16 : 8);  // SHADOW: padded row length in elements (dpb / dph)
    // (not in 16-wave blocks: at their 128 VGPRs two tiles' rows would spill, and the plan sends shadow rows to them
    // only when the threshold exchange is switched off)
    const bool vec_s = SHADOW && W < 16 && shadow_vec_ok(p.d, PS, p.q, TPR);
    f32x4 sqv[SHADOW ? T : 1][SHADOW_QV], smuv[SHADOW_QV];
    auto shadow_src = [&](int tq) -> const float* {
        const int cc = tq * 16 + tid / TPR;
        return p.q + (size_t)(q0 + ((cc < nqt && !ABL(1)) ? cc : 0)) * p.d;
    };
    if constexpr (SHADOW) {
        if (vec_s && stager) {
            stage_request_row(smuv, p.mu, tid % TPR, TPR, p.d >> 2);
#pragma unroll
            for (int tq = 0; tq < T; tq++) stage_request_row(sqv[tq], shadow_src(tq), tid % TPR, TPR, p.d >> 2);
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- register ring of R index chunks (CH k-steps x 16 rows each).  Chunk positions
    // run tile-major over this wave's row tiles (t0 + w, + W, ...).  The first R - 1
    // chunks are requested now: their HBM latency overlaps the rest of the staging.
    constexpr int R = (T == 1 || W >= 16) ? 2 : (T == 2 ? 4 : (T == 3 ? 3 : 2));
    const bool has_work = (t0 + w) < t1 && !ABL(16);
    f32x4 A[R][CH];
    int ltile = t0 + w, ls0 = 0;  // position of the next chunk to LOAD (clamped at the end)
    auto advance_load = [&]() {
        int ns = ls0 + CH, nt = ltile;
        if (ns >= nsteps) { ns = 0; nt = ltile + W; }
        if (nt < t1) { ltile = nt; ls0 = ns; }  // past the end: keep re-reading the last chunk
    };
    if (has_work) {
#pragma unroll
        for (int j = 0; j < R - 1; j++) {
            load_chunk(A[j], ltile, ls0);
            advance_load();
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- query staging, step 2: into LDS (zero padded to NQ x S units) with |x|^2.  With bf16
    // storage the queries are rounded to bf16 as well and |x|^2 is taken of the rounded values.
    auto to_bf16_pair = [](float lo, float hi) -> uint32_t {
        const __bf16 a = (__bf16)lo, b = (__bf16)hi;
        return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
    };
    auto bf16_round = [](float v) -> float { return (float)(__bf16)v; };
#pragma unroll
    for (int tq = 0; tq < T; tq++) {
        if (!stager) continue;
        const int cc = tq * 16 + tid / TPR, t = tid % TPR;
        float sn = 0.f;
        if (vec_q) {
#pragma unroll
            for (int i = 0; i < QVS; i++) {
                const int j4 = t + i * TPR;
                if (j4 < S4) {
                    if (BF16) {
                        const f32x4 v0 = qv[tq][i * FPS], v1 = qv[tq][i * FPS + FPS - 1];
                        u32x4 o;
                        o[0] = to_bf16_pair(v0[0], v0[1]);
                        o[1] = to_bf16_pair(v0[2], v0[3]);
                        o[2] = to_bf16_pair(v1[0], v1[1]);
                        o[3] = to_bf16_pair(v1[2], v1[3]);
                        *reinterpret_cast<u32x4*>(qs + cc * S + 4 * j4) = o;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float r0 = bf16_round(v0[e]), r1 = bf16_round(v1[e]);
                            sn = fmaf(r0, r0, sn);
                            sn = fmaf(r1, r1, sn);
                        }
                    } else {
                        f32x4 v = qv[tq][i];
                        if (F32S) {
                            if (cc < nqt) v = v - muv[i];  // padding rows stay zero
                            if (cc == 0) *reinterpret_cast<f32x4*>(mus + 4 * j4) = muv[i];
                        }
                        *reinterpret_cast<f32x4*>(qs + cc * S + 4 * j4) = v;
                        sn = fmaf(v[0], v[0], sn);
                        sn = fmaf(v[1], v[1], sn);
                        sn = fmaf(v[2], v[2], sn);
                        sn = fmaf(v[3], v[3], sn);
                        if (F32S) sn += nonfinite_mark(qv[tq][i]);  // a non-finite entry: |x - mu|^2 = NaN
                    }
                }
            }
        } else if (SHADOW) {
            // shadow rows (ise_stage.hpp): v = x - mu exactly as a float pair, scaled by 2^sh, split into fp16 hi | lo
            // halves (HALF) or int8 limbs (BYTE); e_q bounds what the split misses.  From the registers requested in
            // step 1 when the shape allows, else two scalar passes over the query.
            if constexpr (SHADOW) {
                const bool rowok = cc < nqt && !ABL(1);
                unsigned char* hi = reinterpret_cast<unsigned char*>(qs + cc * S);
                unsigned char* lo = hi + 16 * p.row_slots;
                if (vec_s) {
                    float amax, mark;
                    stage_shadow_vec_scale<TPR>(sqv[tq], smuv, shadow_src(tq), p.mu, p.d >> 2, rowok, t, PS >> 2, tq > 0,
                                                amax, mark);
                    stage_shadow_vec_limbs<BYTE, TPR>(sqv[tq], smuv, shadow_src(tq), p.mu, p.d >> 2, rowok, t, PS >> 2,
                                                      amax, mark, hi, lo, xn + cc, xe + cc, xsh + cc);
                } else {
                    stage_shadow_scalar<BYTE, TPR>(shadow_src(tq), p.mu, p.d, PS, rowok, t, hi, lo, xn + cc, xe + cc,
                                                   xsh + cc);
                }
            }
        } else {  // odd d, unaligned queries or very long rows: scalar path, one 4-byte unit at a time
            // (the loads of SB units are requested together, then consumed in the same ascending order as a
            // plain loop would: |x|^2 keeps its summation order, the staging of a 2048-float row its round trips
            // cut by SB -- 8.7 -> see DESIGN.md 4.1)
            const bool rowok = cc < nqt && !ABL(1);
            const float* src = p.q + (size_t)(q0 + (rowok ? cc : 0)) * p.d;
            constexpr int SB = 8;
            for (int j0 = t; j0 < S; j0 += SB * TPR) {
                float lo[SB], hi[SB], m[SB];
#pragma unroll
                for (int b = 0; b < SB; b++) {
                    const int j = j0 + b * TPR;
                    lo[b] = hi[b] = m[b] = 0.f;
                    if (BF16) {
                        if (rowok && j < S && 2 * j < p.d) lo[b] = src[2 * j];
                        if (rowok && j < S && 2 * j + 1 < p.d) hi[b] = src[2 * j + 1];
                    } else {
                        if (SHIFT && j < S && j < p.d) m[b] = p.mu[j];
                        if (rowok && j < S && j < p.d) lo[b] = src[j];
                    }
                }
#pragma unroll
                for (int b = 0; b < SB; b++) {
                    const int j = j0 + b * TPR;
                    if (j < S) {
                        if (BF16) {
                            reinterpret_cast<uint32_t*>(qs)[cc * S + j] = to_bf16_pair(lo[b], hi[b]);
                            const float r0 = bf16_round(lo[b]), r1 = bf16_round(hi[b]);
                            sn = fmaf(r0, r0, sn);
                            sn = fmaf(r1, r1, sn);
                        } else {
                            const float v = (rowok && j < p.d) ? lo[b] - m[b] : 0.f;
                            qs[cc * S + j] = v;
                            if (SHIFT && cc == 0) mus[j] = m[b];
                            sn = fmaf(v, v, sn);
                            if (SHIFT) sn += nonfinite_mark(lo[b]);
                        }
                    }
                }
            }
        }
        if (!SHADOW) {
#pragma unroll
            for (int o = TPR / 2; o > 0; o >>= 1) sn += __shfl_xor(sn, o);
            if (t == 0) xn[cc] = sn;
        }
    }
    for (int i = tid; i < NQ; i += BLOCK_THREADS) {
        tauS[i] = TAU0;
        bwc[i] = 0;
        lockS[i] = 0;
        if constexpr (NBOOT) {
            bminS[i] = KEY_PAD;
            if (i == 0) *arrS = 0;
        }
    }
    __syncthreads();
    STAMP(1);
    CSTAMP(8);

    const float* qrow = qs + c * S + 4 * g;
    const bool use_floor = p.floor_keys != nullptr;

    float xq_n[T], xq_e[T], xq_r[T];
    int xq_sh[T];
    u64 tau[T];
    int cnt[T];
    f32x4 acc0[T], acc1[T];  // BYTE: i32 accumulators (bit casts)
#pragma unroll
    for (int t = 0; t < T; t++) {
        xq_n[t] = xn[t * 16 + c];
        xq_e[t] = SHADOW ? xe[t * 16 + c] : 0.f;
        xq_sh[t] = SHADOW ? xsh[t * 16 + c] : 0;
        xq_r[t] = BYTE ? sqrtf(xq_n[t]) + 0x1p-60f : 0.f;
        tau[t] = TAU0;
        cnt[t] = 0;
        acc0[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    u64 xbound = KEY_PAD;  // FFILT: lane i keeps the exchange bound of the wave's i-th query (w + i W), KEY_PAD = none
    bool booted = false;
    // NBOOT: the seeded boot is taken by a block whose EVERY wave has, behind its two window tiles, the 4 W row tiles
    // that make the exchange read pay (block-uniform: the seeding needs every owner wave at the read).  Other blocks
    // -- short ones, the exchange switched off, floor keys of a multi-pass k -- boot with the cut, as every other kernel.
    const bool nboot = NBOOT && p.xchg != nullptr && !use_floor && !ABL(8 | 16 | 256 | 16384) &&
                       (int)gridDim.x <= 512 /* what the folded read of seed_phase covers */ &&
                       t1 - (t0 + (W - 1) + 2 * W) >= 4 * W;

    // fold the wave's private list of query qq = 16 t + cq into the block list bootw[qq]
    // (exact sorted top-k of their union) under the query's LDS lock; publish the k-th key
    auto merge_out = [&](int t, int cq) {
        const int qq = t * 16 + cq;
        const int n_ = __builtin_amdgcn_readlane(cnt[t], cq);
        const u64* buf = cand + (size_t)(w * NQ + qq) * CAP;
        if (lane == 0)
            while (atomicCAS(&lockS[qq], 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
        wave_lds_fence();
        const int nb = bwc[qq];
        u64 kk[1];
        kk[0] = lane < nb ? bootw[qq * kb + lane] : (lane - nb < n_ ? buf[lane - nb] : KEY_PAD);
        wave_lds_fence();
        u64 ktau = KEY_PAD;
        const int nw = wave_select<1>(kk, nb + n_, k, bootw + qq * kb, &ktau);  // nb + n_ <= kb + CAP <= 64
        if (lane == 0) {
            bwc[qq] = nw;
            if (nw == k) tauS[qq] = min_u64(tauS[qq], ktau);  // the exchange may have set it lower
        }
        wave_lds_fence();
        if (lane == 0) atomicExch(&lockS[qq], 0);
        if (c == cq) {
            cnt[t] = 0;
            if (nw == k) tau[t] = min_u64(tau[t], ktau);
        }
    };

    // boot: all W*16 first-tile keys of a query -> block list + block threshold
    auto boot_phase = [&](const u64(&key)[T][4]) {
        STAMP(2);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) boot[(size_t)(t * 16 + c) * (W * 16) + w * 16 + 4 * g + j] = key[t][j];
        __syncthreads();
        STAMP(7);
        for (int qq = w; qq < NQ; qq += W) {
            u64 kk[KPLB];
#pragma unroll
            for (int e = 0; e < KPLB; e++)
                kk[e] = (lane + 64 * e) < W * 16 ? boot[(size_t)qq * (W * 16) + lane + 64 * e] : KEY_PAD;
            u64 ktau = TAU0;
            const int nw = wave_cut<KPLB>(kk, W * 16, k, kb, bootw + qq * kb, &ktau);
            u64 best = kk[0];
#pragma unroll
            for (int e = 1; e < KPLB; e++) best = min_u64(best, kk[e]);
            best = wave_min_u64(best);
            if (lane == 0) {
                bwc[qq] = nw;
                tauS[qq] = ktau;  // TAU0 when fewer than k real keys were seen
                if (XCHG && p.xchg)
                    __hip_atomic_store(p.xchg + ((size_t)blockIdx.y * NQ + qq) * gridDim.x + blockIdx.x,
                                       ((u64)p.xchg_seq << 32) | (best >> 32), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < T; t++) tau[t] = tauS[t * 16 + c];
        booted = true;
        STAMP(3);
    };

    // NBOOT, blocks all of whose waves will read the exchange (nboot): no cut.  A wave's first TWO row tiles are its
    // boot window: their keys go to the home unfiltered (first tile: the boot staging; second: home2), so no
    // threshold is needed before the exchange bound exists.  The block's smallest first-tile key per query is folded
    // with LDS atomics, and the last wave to arrive publishes the entries -- no barrier: a wave goes straight on to
    // its second tile, and that tile's streaming is the distance between the publish and the read (seed_phase).
    int wtiles = 0;  // window tiles this wave has stored (wave-uniform)
    auto boot_window = [&](const u64(&key)[T][4]) {
        u64* dst = (wtiles == 0 ? boot : home2) + (size_t)c * (W * 16) + w * 16 + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; j++) dst[j] = key[0][j];
        if (wtiles == 0) {
            STAMP(2);
            u64 m = min_u64(min_u64(key[0][0], key[0][1]), min_u64(key[0][2], key[0][3]));
            m = min_u64(m, __shfl_xor(m, 16));
            m = min_u64(m, __shfl_xor(m, 32));
            if (g == 0 && m != KEY_PAD) atomicMin(reinterpret_cast<unsigned long long*>(bminS + c), (unsigned long long)m);
            wave_lds_fence();
            int arrived = 0;
            if (lane == 0) arrived = __hip_atomic_fetch_add(arrS, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            arrived = __builtin_amdgcn_readfirstlane(arrived);
            wave_lds_fence();
            if (arrived == W - 1 && lane < NQ)  // the score of one real row of this block, or 0xFFFFFFFF
                __hip_atomic_store(p.xchg + ((size_t)blockIdx.y * NQ + lane) * gridDim.x + blockIdx.x,
                                   ((u64)p.xchg_seq << 32) | (bminS[lane] >> 32), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            STAMP(7);
        }
        wtiles++;
    };

    // score of (query tile t, row slot j) exactly as it is keyed.
    //   float32 rows, L2 (SHIFT): a rigorous LOWER BOUND of the direct-difference distance,
    //       lo = (|x-mu|^2 + |y-mu|^2 - 2 (x-mu).(y-mu)) - beta (|x-mu|^2 + |y-mu|^2),
    //     beta covering every rounding between the stored floats and this value.
    //     The scan selects the K' = k + extra rows of smallest lo; the merge stage re-evaluates
    //     them as sum (x-y)^2 and proves (or sends to the exact fallback scan) that no other
    //     row can enter the top k (ise_exact.hpp).  Not clamped: the order is what matters.
    //     Non-finite inputs (ise_common.hpp, l2_lower_bound): a row or query with a NaN or inf entry
    //     has a NaN norm, so lo = NaN and it never enters; finite entries whose shifted norms overflow
    //     give no bound and are keyed -FLT_MAX, so they stay candidates for the direct re-rank.
    //   bf16 rows, L2: the expanded form clamped at 0 (NaN kept), approximate by construction.
    //   inner product: minus the dot product.
    auto score = [&](int t, float dotj, float ynj, float yej, float ysj) -> float {
        if constexpr (HALF) return half_lower_bound(p.beta, p.lo_shrink, xq_n[t] + ynj,
                                                    ldexpf(dotj, -((int)ysj + xq_sh[t])), yej + xq_e[t]);
        if constexpr (BYTE) {  // dotj = 256 A_hi + A_lo; yej the packed c_r | e_r / c_r
            const uint32_t m = __float_as_uint(yej);
            const float cr = __uint_as_float(m << 16);
            const float er = cr * (float)__builtin_bit_cast(_Float16, (unsigned short)(m >> 16));  // exact
            return byte_lower_bound(p.beta, p.lo_shrink, xq_n[t], ynj, ldexpf(dotj * cr, -xq_sh[t]), xq_r[t],
                                    sqrtf(ynj) + 0x1p-60f, er, xq_e[t]);
        }
        if (l2) {
            const float tt = xq_n[t] + ynj;
            const float sc = tt - 2.f * dotj;
            if (SHIFT) return l2_lower_bound(p.beta, tt, sc);
            return sc < 0.f ? 0.f : sc;  // keeps NaN (Faiss: if (dis < 0) dis = 0)
        }
        return -dotj;
    };
    auto make_keys = [&](int etile, const f32x4(&sc)[T], u64(&key)[T][4]) {
        const long long row0 = (long long)etile * 16 + 4 * g;
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bool ok = (row0 + j < p.n) && (sc[t][j] < FLT_MAX) && (t * 16 + c < nqt);
                const u64 kj = ((u64)ord_f32(sc[t][j]) << 32) | (uint32_t)((uint32_t)(row0 + j) + p.id_base);
                if (use_floor) ok = ok && (kj > p.floor_keys[q0 + min(t * 16 + c, nqt - 1)]);  // multi-pass k only
                key[t][j] = ok ? kj : KEY_PAD;
            }
    };

    float tau_sc[T];  // float image of tau's score part: a conservative pre-filter
#pragma unroll
    for (int t = 0; t < T; t++) tau_sc[t] = FLT_MAX;

    auto epilogue = [&](int etile, f32x4 yn, f32x4 ye, f32x4 ys) {
        f32x4 sc[T];
#pragma unroll
        for (int t = 0; t < T; t++) {
            f32x4 dot = acc0[t] + acc1[t];
            if constexpr (BYTE) {  // the exact integer dot products of the hi and lo limbs (|A| < 2^24 for dpb <= 1024)
                const i32x4 ah = __builtin_bit_cast(i32x4, acc0[t]), al = __builtin_bit_cast(i32x4, acc1[t]);
#pragma unroll
                for (int j = 0; j < 4; j++) dot[j] = fmaf(256.f, (float)ah[j], (float)al[j]);
            }
            acc0[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; j++) sc[t][j] = score(t, dot[j], yn[j], ye[j], ys[j]);
        }
        if (!booted) {
            u64 key[T][4];
            make_keys(etile, sc, key);
            if constexpr (NBOOT) {
                if (nboot) {
                    boot_window(key);
                    return;
                }
            }
            boot_phase(key);
#pragma unroll
            for (int t = 0; t < T; t++) tau_sc[t] = unord_f32((uint32_t)(tau[t] >> 32));
            return;
        }
        // fast path: a row can only enter if its score does not exceed the threshold's score
        // (ties on the score are settled by the exact key compare below).  One ballot per
        // (query tile, row slot); keys are built only for the slots some lane may fill.
#pragma unroll
        for (int t = 0; t < T; t++) {
            tau[t] = min_u64(tau[t], tauS[t * 16 + c]);  // other waves' merges tighten it
            tau_sc[t] = unord_f32((uint32_t)(tau[t] >> 32));
        }
        u64 hit[T][4];
        u64 any_hit = 0;
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                hit[t][j] = __ballot(sc[t][j] <= tau_sc[t]);
                any_hit |= hit[t][j];
            }
        if (any_hit && !ABL(2)) {
            const long long row0 = (long long)etile * 16 + 4 * g;
            const u64 qmask = 0x0001000100010001ull << c;  // lanes holding the same query
            const u64 lt_mask = (1ull << lane) - 1ull;
#pragma unroll
            for (int t = 0; t < T; t++) {
                u64* mybuf = cand + (size_t)(w * NQ + t * 16 + c) * CAP;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (hit[t][j]) {  // wave-uniform
                        const float s_ = sc[t][j];
                        bool ok = (row0 + j < p.n) && (s_ < FLT_MAX) && (t * 16 + c < nqt);
                        const u64 kj = ((u64)ord_f32(s_) << 32) | (uint32_t)((uint32_t)(row0 + j) + p.id_base);
                        if (use_floor) ok = ok && (kj > p.floor_keys[q0 + min(t * 16 + c, nqt - 1)]);  // multi-pass k only
                        const bool v = ok && kj < tau[t];
                        const u64 m = __ballot(v);
                        if (m) {
                            const u64 mq = m & qmask;
                            if (v) mybuf[cnt[t] + __popcll(mq & lt_mask)] = kj;
                            cnt[t] += __popcll(mq);
                            u64 nm = __ballot(cnt[t] >= MERGE_TRIG) & 0xFFFFull;
                            while (nm) {
                                const int cq = __ffsll((long long)nm) - 1;
                                nm &= nm - 1;
                                merge_out(t, cq);
                            }
                        }
                    }
                }
                tau_sc[t] = unord_f32((uint32_t)(tau[t] >> 32));
            }
        }
    };

    // one-shot threshold exchange (see the header comment): queries w, w + W, ... of this wave.
    // 256 slots (4 per lane) cover the grid, a slot folding G entries by their minimum; the k-th
    // smallest slot value is found bit by bit with ballot counts (absent entries = 0xFFFFFFFF).
    auto xchg_prefix = [&](int qq) -> uint32_t {  // the k-th smallest published score of query qq, 0xFFFFFFFF = none
        const int nb = (int)gridDim.x;
        const int G = (nb + 255) >> 8;
        const u64* src = p.xchg + ((size_t)blockIdx.y * NQ + qq) * nb;
        auto slot_value = [&](int slot) -> uint32_t {
            uint32_t best = 0xFFFFFFFFu;
            for (int j = 0; j < G; j++) {
                const int i = slot * G + j;
                if (i < nb) {
                    const u64 v = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((uint32_t)(v >> 32) == p.xchg_seq) best = min(best, (uint32_t)v);
                }
            }
            return best;
        };
        const uint32_t v0 = slot_value(lane), v1 = slot_value(lane + 64), v2 = slot_value(lane + 128),
                       v3 = slot_value(lane + 192);
        uint32_t prefix = 0;
        int rank = k;  // 1-based rank of the wanted value among those matching the prefix
        for (int b = 31; b >= 0; b--) {
            const uint32_t hm = b == 31 ? 0u : 0xFFFFFFFFu << (b + 1);
            auto zero_here = [&](uint32_t v) { return ((v ^ prefix) & hm) == 0u && ((v >> b) & 1u) == 0u; };
            const int c0 = __popcll(__ballot(zero_here(v0))) + __popcll(__ballot(zero_here(v1))) +
                           __popcll(__ballot(zero_here(v2))) + __popcll(__ballot(zero_here(v3)));
            if (rank > c0) {
                rank -= c0;
                prefix |= 1u << b;
            }
        }
        return prefix;
    };
    // XFOLD (the seeded-boot kernel): the same bound from ONE value per lane.  Stamped, the read above cost 6.5 us per
    // query -- eight dependent agent-scope loads per lane, each behind the ring's prefetch, then 32 rounds of four
    // ballots.  Here the eight entries of a lane (grids of up to 512 blocks; a larger
    // grid boots with the cut and reads as above) are requested four at a time, clamped instead of branched around, and folded to their minimum: 64 values, each the score of one real row, all of different
    // blocks, so their k-th smallest (one ballot per bit, k <= KB_MAX < 64) is still the k-th best of k distinct rows
    // -- a valid bound, at k = 32 about 1.4 times as far out in the distribution as the k-th of all entries.
    constexpr bool XFOLD = NBOOT;
    // ROWS_I8_ONE, the kernel the launcher picks for a grid of at most 64 XE = 256 blocks (the deep plan of the host's
    // make_plan): a lane has at most XE entries, lane + 64 i, all in ONE request (half 0; there is no half 1), so no
    // round trip is left behind the barrier.  The bound is still the k-th smallest of 64 values of distinct blocks.
    // (A compile-time split, not a branch on gridDim.x: the branch cost the one-tile kernel its last registers.)
    constexpr int XE = 4;  // entries per lane in flight at once (8 would spill the one-tile kernel): two halves per query
    constexpr int XGRID = 512;  // blocks the folded read covers (64 lanes x 2 halves x XE); larger grids: nboot is off
    constexpr bool XREQ1 = RM == ROWS_I8_ONE;
    auto xchg_request = [&](int qq, int half, u64(&e)[XE]) {  // gridDim.x <= XGRID
        const int nb = (int)gridDim.x;
        const int G = XREQ1 ? 1 : (nb + 255) >> 8;
        const u64* src = p.xchg + ((size_t)blockIdx.y * NQ + qq) * nb;
#pragma unroll
        for (int i = 0; i < XE; i++) {
            const int idx = XREQ1 ? lane + 64 * i : (lane + 64 * (2 * half + (i >> 1))) * G + (i & 1);
            e[i] = __hip_atomic_load(src + (((XREQ1 || (i & 1) < G) && idx < nb) ? idx : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    auto xchg_fold = [&](int half, const u64(&e)[XE], uint32_t best) -> uint32_t {
        const int nb = (int)gridDim.x;
        const int G = XREQ1 ? 1 : (nb + 255) >> 8;
#pragma unroll
        for (int i = 0; i < XE; i++) {
            const int idx = XREQ1 ? lane + 64 * i : (lane + 64 * (2 * half + (i >> 1))) * G + (i & 1);
            if ((XREQ1 || (i & 1) < G) && idx < nb && (uint32_t)(e[i] >> 32) == p.xchg_seq) best = min(best, (uint32_t)e[i]);
        }
        return best;
    };
    auto lanes_kth = [&](uint32_t v) -> uint32_t {  // the k-th smallest of the lanes' values, 0xFFFFFFFF = fewer than k
        uint32_t prefix = 0;
        int rank = k;
        for (int b = 31; b >= 0; b--) {
            const uint32_t hm = b == 31 ? 0u : 0xFFFFFFFFu << (b + 1);
            const int c0 = __popcll(__ballot(((v ^ prefix) & hm) == 0u && ((v >> b) & 1u) == 0u));
            if (rank > c0) {
                rank -= c0;
                prefix |= 1u << b;
            }
        }
        return prefix;
    };
    // dev bit 32768 (ROWS_I8_ONE): the k-th smallest of ALL the grid's entries, four ballots per bit as in xchg_prefix,
    // instead of the k-th of the lanes' folded minima -- a tighter bound for four times the ballot work
    auto lanes_kth4 = [&](const u64(&e)[XE]) -> uint32_t {
        const int nb = (int)gridDim.x;
        uint32_t v[XE];
#pragma unroll
        for (int i = 0; i < XE; i++)
            v[i] = (lane + 64 * i < nb && (uint32_t)(e[i] >> 32) == p.xchg_seq) ? (uint32_t)e[i] : 0xFFFFFFFFu;
        uint32_t prefix = 0;
        int rank = k;
        for (int b = 31; b >= 0; b--) {
            const uint32_t hm = b == 31 ? 0u : 0xFFFFFFFFu << (b + 1);
            int c0 = 0;
#pragma unroll
            for (int i = 0; i < XE; i++) c0 += __popcll(__ballot(((v[i] ^ prefix) & hm) == 0u && ((v[i] >> b) & 1u) == 0u));
            if (rank > c0) {
                rank -= c0;
                prefix |= 1u << b;
            }
        }
        return prefix;
    };
    auto exchange = [&]() {
        STAMP(12);
        for (int qq = w; qq < NQ; qq += W) {
            uint32_t prefix;
            // (a larger grid than the folded read covers -- none on a 256-CU device -- keeps the read above; so does
            // dev bit 16384, which with the cut boot it selects is the path of every other exchange kernel)
            if (XFOLD && (int)gridDim.x <= XGRID && !ABL(16384)) {
                u64 e[XE];
                xchg_request(qq, 0, e);
                uint32_t folded = xchg_fold(0, e, 0xFFFFFFFFu);
                if constexpr (!XREQ1) {
                    xchg_request(qq, 1, e);
                    folded = xchg_fold(1, e, folded);
                }
                prefix = lanes_kth(folded);
            } else {
                prefix = xchg_prefix(qq);
            }
            if (prefix != 0xFFFFFFFFu) {  // at least k entries of this launch were there
                const u64 bound = ((u64)prefix << 32) | 0xFFFFFFFFull;  // every id at that score stays admissible
                if (FFILT && lane == (qq - w) / W) xbound = bound;  // for the final phase of this query, below
                if (lane == 0) {
                    while (atomicCAS(&lockS[qq], 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
                }
                wave_lds_fence();
                if (lane == 0 && bound < tauS[qq]) tauS[qq] = bound;
                wave_lds_fence();
                if (lane == 0) atomicExch(&lockS[qq], 0);
            }
        }
        STAMP(13);
    };

    // NBOOT: the end of the seeded boot, once per block and with every wave in it, after the wave's second window
    // tile.  The owner wave of a query reads the exchange and seeds the query's block list with the home keys <= bound.
    // Invariants (with the cut of boot_phase and merge_out they hold in every kernel):
    //   (a) tauS[q], whenever it is below TAU0, is at or above the launch's final k-th key of q: it is either the
    //       block's own k-th smallest key so far (cut, merge_out) or an exchange bound of this launch -- the k-th
    //       smallest score of k DISTINCT published rows, with id part 0xFFFFFFFF;
    //   (b) every key of the block that is <= that final k-th key is in bootw or a private list, hence in the list
    //       the block writes: a key is dropped only for being above some tauS value (here: above the bound; steady
    //       state: not below tau; merge_out: above the union's k-th), or above xbound in the final phase.
    // Fallback to the exact path -- wave_cut over the home keys, kmin = k, kmax = kb as in boot_phase -- when no bound
    // arrived (fewer than k entries of this launch visible) or more than kb home keys lie under it (many equal rows in
    // the window).  Nothing here needs lockS: bootw, bwc and tauS of a query are written by its owner alone, between
    // two block barriers, and no merge_out runs before the second (a wave's private lists are empty until then).
    auto seed_phase = [&]() {
        STAMP(10);
        // the entries of the wave's first query are requested ahead of the barrier, those of its second ahead of the
        // first one's seeding: the round trips overlap the wait and the LDS work
        u64 xe_[XE];
        xchg_request(w, 0, xe_);
        __syncthreads();  // every wave's window keys are in the home
        STAMP(11);
        const u64 lt_mask = (1ull << lane) - 1ull;
        for (int qq = w; qq < NQ; qq += W) {
            u64 kk[4];
#pragma unroll
            for (int e = 0; e < 4; e++)
                kk[e] = ((e < 2 ? boot : home2) + (size_t)qq * (W * 16))[lane + 64 * (e & 1)];
            uint32_t folded = xchg_fold(0, xe_, 0xFFFFFFFFu);
            if constexpr (!XREQ1) {  // (ROWS_I8_ONE: all the entries were in the first request)
                xchg_request(qq, 1, xe_);
                folded = xchg_fold(1, xe_, folded);
            }
            const uint32_t all4 = (XREQ1 && ABL(32768)) ? lanes_kth4(xe_) : 0u;
            if (qq + W < NQ) xchg_request(qq + W, 0, xe_);
            const uint32_t prefix = (XREQ1 && ABL(32768)) ? all4 : lanes_kth(folded);
            if (qq == w) STAMP(12);
            const u64 bound = ((u64)prefix << 32) | 0xFFFFFFFFull;  // KEY_PAD when no bound arrived
            if (FFILT && prefix != 0xFFFFFFFFu && lane == (qq - w) / W) xbound = bound;
            u64 keep[4];
            int n_in = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                keep[e] = __ballot(kk[e] <= bound && kk[e] != KEY_PAD);
                n_in += __popcll(keep[e]);
            }
            if (prefix != 0xFFFFFFFFu && n_in <= kb) {
                int off = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if ((keep[e] >> lane) & 1ull) bootw[qq * kb + off + __popcll(keep[e] & lt_mask)] = kk[e];
                    off += __popcll(keep[e]);
                }
                if (lane == 0) {
                    bwc[qq] = n_in;
                    tauS[qq] = bound;
                }
            } else {
                u64 ktau = TAU0;
                const int nw = wave_cut<4>(kk, 4 * 64, k, kb, bootw + qq * kb, &ktau);
                if (lane == 0) {
                    bwc[qq] = nw;
                    tauS[qq] = min_u64(ktau, bound);  // TAU0 when fewer than k real keys were seen and no bound arrived
                }
            }
            if (qq == w) STAMP(13);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < T; t++) {
            tau[t] = tauS[t * 16 + c];
            tau_sc[t] = unord_f32((uint32_t)(tau[t] >> 32));
        }
        booted = true;
        STAMP(3);
    };

    // B operand (queries, from LDS) is software-pipelined one k-step ahead of the MFMAs
    // that consume it, across chunk boundaries too: bcur holds the B fragments of the
    // next step to be computed.
    // SHADOW: bcur_lo the lo limbs of the same step (4 row_slots floats behind the hi limbs of a query row)
    f32x4 bcur[T], bcur_lo[SHADOW ? T : 1];
    auto load_b = [&](f32x4(&b)[T], f32x4(&blo)[SHADOW ? T : 1], int step) {
        if (ABL(512)) return;  // dev: no LDS reads of the query operand (registers keep whatever they hold)
#pragma unroll
        for (int t = 0; t < T; t++) {
            b[t] = *reinterpret_cast<const f32x4*>(qrow + (size_t)t * 16 * S + 16 * step);
            if constexpr (SHADOW) blo[t] = *reinterpret_cast<const f32x4*>(qrow + (size_t)t * 16 * S + 4 * p.row_slots + 16 * step);
        }
    };
    auto compute_chunk = [&](const f32x4(&a)[CH], int s0, int next_first_step) {
#pragma unroll
        for (int s = 0; s < CH; s++) {
            f32x4 bnext[T], bnext_lo[SHADOW ? T : 1];
            if (ABL(64)) {  // dev: no LDS reads, no MFMA -- the loaded data is only summed
#pragma unroll
                for (int t = 0; t < T; t++) acc0[t] += a[s];
                continue;
            }
            load_b(bnext, bnext_lo, s + 1 < CH ? s0 + s + 1 : next_first_step);
            f32x4 as = a[s];
            if (F32S && !ABL(1024)) as = as - *reinterpret_cast<const f32x4*>(mus + 4 * g + 16 * (s0 + s));
#pragma unroll
            for (int t = 0; t < T; t++) {
                if (BYTE) {  // two 16x16x64 i8 MFMAs per k-step: the query's hi limbs, then its lo limbs
                    const i32x4 av = __builtin_bit_cast(i32x4, a[s]);
                    acc0[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(
                                                            av, __builtin_bit_cast(i32x4, bcur[t]),
                                                            __builtin_bit_cast(i32x4, acc0[t]), 0, 0, 0));
                    acc1[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(
                                                            av, __builtin_bit_cast(i32x4, bcur_lo[t]),
                                                            __builtin_bit_cast(i32x4, acc1[t]), 0, 0, 0));
                } else if (HALF) {  // two 16x16x32 f16 MFMAs per k-step: the query's hi halves, then its lo halves
                    const f16x8 av = __builtin_bit_cast(f16x8, a[s]);
                    acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, __builtin_bit_cast(f16x8, bcur[t]), acc0[t], 0, 0, 0);
                    acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, __builtin_bit_cast(f16x8, bcur_lo[t]), acc1[t], 0, 0, 0);
                } else if (BF16) {  // one 16x16x32 bf16 MFMA per k-step (8 bf16 per lane and operand)
                    const bf16x8 av = __builtin_bit_cast(bf16x8, a[s]), bv = __builtin_bit_cast(bf16x8, bcur[t]);
                    if (s & 1) acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc1[t], 0, 0, 0);
                    else acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc0[t], 0, 0, 0);
                } else {     // four 16x16x4 fp32 MFMAs per k-step (exact fp32 fmaf chains)
                    acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[0], bcur[t][0], acc0[t], 0, 0, 0);
                    acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[1], bcur[t][1], acc1[t], 0, 0, 0);
                    acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[2], bcur[t][2], acc0[t], 0, 0, 0);
                    acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[3], bcur[t][3], acc1[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < T; t++) {
                bcur[t] = bnext[t];
                if constexpr (SHADOW) bcur_lo[t] = bnext_lo[t];
            }
        }
    };

    // ---- main loop.  Each step: request the chunk R - 1 positions ahead (unconditionally:
    // no control-flow join between a load and its use, so hipcc emits counted vmcnt waits
    // and the ring stays in flight), then run the MFMAs of the oldest chunk.  The row
    // norms of the tile being computed are requested first, so the epilogue's wait on them
    // never drains the younger index loads.
    if (has_work) {
        int tile = t0 + w, s0 = 0;  // position of the chunk being COMPUTED
        int tiles_done = 0;
        bool exchanged = !XCHG || p.xchg == nullptr || ABL(256);
        load_b(bcur, bcur_lo, 0);
        bool done = false;
        while (!done) {
#pragma unroll
            for (int j = 0; j < R; j++) {
                if (!done) {
                    const f32x4 yn = load_norms(tile);
                    const f32x4 ye = load_meta(BYTE ? (const void*)p.bmeta : p.herr, tile);
                    const f32x4 ys = HALF ? load_meta(p.hexp, tile) : (f32x4){0.f, 0.f, 0.f, 0.f};
                    load_chunk(A[(j + R - 1) % R], ltile, ls0);
                    advance_load();
                    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMAs
                    int ns0 = s0 + CH, ntile = tile;
                    if (ns0 >= nsteps) { ns0 = 0; ntile = tile + W; }
                    compute_chunk(A[j], s0, ns0);
                    if (ns0 == 0 && !ABL(8) && !(ABL(2048) && booted)) epilogue(tile, yn, ye, ys);  // 2048: boot only
                    if (ns0 == 0) tiles_done++;
                    done = ntile >= t1;
                    tile = ntile; s0 = ns0;
                }
            }
            // outside the unrolled ring steps (one copy of the code): after the wave's second row tile
            // -- and only when enough row tiles remain for the tighter threshold to pay for the read
            if constexpr (XCHG) {
                if (!exchanged && tiles_done >= (nboot ? 2 : 1)) {
                    if constexpr (NBOOT) {
                        if (nboot) seed_phase();
                    }
                    if (!nboot && t1 - tile >= 4 * W) exchange();
                    exchanged = true;
                }
            }
        }
    }
    if (!booted) {  // a wave without a row tile still takes part in the two boot barriers
        u64 none[T][4];
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) none[t][j] = KEY_PAD;
        boot_phase(none);
    }

    // ---- final: per query, exact sorted top-k of bootw + the W private lists
    STAMP(4);
    CSTAMP(9);
#pragma unroll
    for (int t = 0; t < T; t++)
        if (g == 0) cntS[w * NQ + t * 16 + c] = cnt[t];
    __syncthreads();
    STAMP(5);
    for (int qq = w; qq < NQ && !ABL(4); qq += W) {
        int P[W + 2];
        P[0] = 0;
        P[1] = bwc[qq];
#pragma unroll
        for (int i = 0; i < W; i++) P[i + 2] = P[i + 1] + cntS[i * NQ + qq];
        const int n = P[W + 1];
        // FFILT: where this wave obtained the exchange bound of the query, every key above it is dropped BEFORE the
        // selection.  The bound is the k-th smallest score of k DISTINCT rows of this launch (one per block), so the
        // final k-th key over all blocks is <= xbound = (that score << 32) | 0xFFFFFFFF and no dropped key can be among the k
        // smallest: the merged list is unchanged, and of the block's ~k keys the one or two survivors are all that is
        // ranked.  No bound (too few published entries, a block too short to read the exchange, ISE_NO_XCHG, or the
        // floor keys of a multi-pass k): xbound is KEY_PAD and nothing is dropped.
        u64 bnd = KEY_PAD;
        if constexpr (FFILT) {
            if (!use_floor && !ABL(8192)) bnd = readlane_u64(xbound, (qq - w) / W);
        }
        u64 kk[KPLF];
#pragma unroll
        for (int e = 0; e < KPLF; e++) {
            kk[e] = KEY_PAD;
            const int idx = lane + 64 * e;
            if (64 * e < n) {
                if (idx < P[1]) kk[e] = bootw[qq * kb + idx];
#pragma unroll
                for (int i = 0; i < W; i++)
                    if (idx >= P[i + 1] && idx < P[i + 2])
                        kk[e] = cand[(size_t)(i * NQ + qq) * CAP + idx - P[i + 1]];
                if (FFILT && kk[e] > bnd) kk[e] = KEY_PAD;
            }
        }
        u64* out = p.part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NQ + qq) * k;
        u64 kth_unused;
        const int nw = wave_select<KPLF>(kk, n, k, out, &kth_unused);
        if (lane >= nw && lane < k) out[lane] = KEY_PAD;  // k <= KB_MAX <= 64
    }
    STAMP(6);
}
