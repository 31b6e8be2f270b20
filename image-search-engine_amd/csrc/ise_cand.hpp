// ise_cand.hpp -- the candidate buffers of a coded scan's k-pass: what the product-quantised and scalar-quantised scans
// (ise_pq.hpp and ise_sq.hpp, and through them ise_ivfpq.hpp and ise_ivfsq.hpp) share once a tile's keys exist.  DESIGN.md 4.10 describes the
// scheme.  The binary scan (ise_binary_scan.hpp), where it began, keeps its own body with counts in LDS: measured, this
// one was slower there on one masked row (profiles/cands).
//
// A pass serves up to QT queries and kp <= KPASS results each.  A wave streams tiles of at most TILE rows; per query it
// keeps a threshold key (KEY_PAD until a cut has held kp keys) and a buffer of CAP keys in LDS.  The kernel appends
// the tile's keys that lie below the threshold (and at or above the pass's floor) behind the `cnt` held ones -- that
// part is bound to its lane layout and stays with it.  Then:
//   make_room  every query whose buffer may not take another tile (more than CAP - TILE keys) is cut: wave_cut keeps
//              between kp and kp + kp / 2 + 4 (at most CUT_MAX) of its keys, unsorted, and the cut key becomes the
//              threshold -- a window close to kp, so that the threshold is tight and a wave rarely cuts twice.
//   fold       at the end of the stream the slots behind each buffer are emptied, and after a block barrier wave w takes
//              queries w, w + WAVES, ..: the waves' buffers of a query (WAVES * CAP = 512 keys, eight registers per
//              lane) go through one wave_select into the block's list of the query, SORTED, KEY_PAD behind the last.
// pass_merge_kernel (ise_merge.hpp) walks the blocks' lists; a k above KPASS repeats the pass with a floor key.
//
// Keys are unique and lie strictly between 0 and KEY_PAD (ise_select.hpp): wave_cut keeps a key 0 but does not count
// it, so a kind whose best key could be 0 shifts it (bin_key, ise_binary_scan.hpp).
#pragma once
#include "ise_common.hpp"
#include "ise_merge.hpp"
#include "ise_select.hpp"

// The wave's state.  `col` is the query whose count and threshold this lane carries: the lane number where query q
// lives in lane q, lane & 15 where a lane ends a tile with scores of one query (the MFMA's column).  Either way lane q
// carries query q for every q < QT, which is where cut and fold read them.
template <int QT, int WAVES, int CAP, int TILE, int CUT_MAX, int KPASS>
struct CandBuf {
    static_assert(TILE <= 64 && CUT_MAX + TILE <= CAP && KPASS <= CUT_MAX, "a tile's keys fit behind the kept ones");
    static_assert(CAP == 128, "a wave's buffer is two registers per lane in wave_cut");
    static_assert(WAVES * CAP == 512, "the block's selection holds the waves' buffers in eight registers per lane");
    static_assert(KPASS <= MERGE_FAST_K, "merge_waves serves every pass");
    static_assert(QT <= 16, "a query's state sits in lane q of the first 16");

    u64* buf;   // the block's buffers, [WAVES][QT][CAP]
    u64* mine;  // this wave's, [QT][CAP]
    int lane, w, col, kp, kmax;
    int cnt = 0;        // keys held by query `col`
    u64 thr = KEY_PAD;  // a new key must be below it

    __device__ __forceinline__ CandBuf(u64* base, int wave, int column, int kp_)
        : buf(base), mine(base + wave * QT * CAP), lane(threadIdx.x & 63), w(wave), col(column), kp(kp_),
          kmax(kp_ + kp_ / 2 + 4 < CUT_MAX ? kp_ + kp_ / 2 + 4 : CUT_MAX) {}

    // query q's buffer in this wave
    __device__ __forceinline__ u64* keys(int q) const { return mine + q * CAP; }

    // query q (wave-uniform) keeps between kp and kmax of its keys, unsorted; everything kept is <= the cut key, which
    // becomes the threshold
    __device__ __forceinline__ void cut(int q) {
        const int held = __builtin_amdgcn_readlane(cnt, q);
        u64 kk[2];
#pragma unroll
        for (int e = 0; e < 2; e++) kk[e] = lane + 64 * e < held ? keys(q)[lane + 64 * e] : KEY_PAD;
        u64 ckey = KEY_PAD;
        const int nw = wave_cut<2>(kk, CAP, kp, kmax, keys(q), &ckey);
        wave_lds_fence();
        if (col == q) {
            cnt = nw;
            thr = ckey;
        }
    }

    // behind a tile's appends: the next tile may not fit
    __device__ __forceinline__ void make_room() {
        wave_lds_fence();
        u64 need = __ballot(cnt > CAP - TILE) & ((1ull << QT) - 1ull);
        while (need) {
            const int q = __ffsll((long long)need) - 1;
            need &= need - 1;
            cut(q);
        }
    }

    // End of the stream, every wave of the block: lists = the block's [QT][KPASS].  The slots behind a buffer's keys are
    // made to read as empty, so the block's selection needs no counts and the kernel no further LDS.  Only the pass's
    // queries are selected from: a pass of one query pads one buffer per wave, not QT.
    __device__ __forceinline__ void fold(int nqt, u64* lists) {
#pragma unroll
        for (int q = 0; q < QT; q++) {
            if (q < nqt) {
                const int held = __builtin_amdgcn_readlane(cnt, q);
#pragma unroll
                for (int e = 0; e < 2; e++)
                    if (lane + 64 * e >= held) keys(q)[lane + 64 * e] = KEY_PAD;
            }
        }
        __syncthreads();
        // wave w takes queries w, w + WAVES, ..: the waves' buffers of a query -> the block's sorted list
        for (int q = w; q < nqt; q += WAVES) {
            u64 kk[2 * WAVES];
#pragma unroll
            for (int e = 0; e < 2 * WAVES; e++) kk[e] = buf[((e >> 1) * QT + q) * CAP + lane + 64 * (e & 1)];
            u64* dst = lists + q * KPASS;
            u64 kth_unused = 0;
            const int nw = wave_select<2 * WAVES>(kk, WAVES * CAP, kp, dst, &kth_unused);
            for (int i = nw + lane; i < kp; i += 64) dst[i] = KEY_PAD;
        }
    }
};
