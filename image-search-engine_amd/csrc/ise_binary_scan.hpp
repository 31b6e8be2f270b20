// ise_binary_scan.hpp -- kernels of the binary flat index (include/ise_knn.h, ise_binary_index_*): exact Hamming
// kNN and range search over bit codes, faiss.IndexBinaryFlat.  DESIGN.md 4.10.
//
// Storage: a row is `ws` 64-bit words (ws = 1, or ceil(code_size / 8) rounded up to an even count so that every row
// starts on 16 bytes); the bytes past code_size are zero in the rows AND in the staged queries, so they add nothing to
// any distance.  Rows at or beyond n are masked by row number.
//
// Scan: a lane owns a row, a wave a tile of 64 consecutive rows, 16 queries per pass.  ws = 1: one coalesced 8-byte
// load per lane, ws >= 2: 16-byte loads (a loop over 16-byte chunks for ws > 2).  The tile's queries are wave-uniform:
// ws <= 2 holds them in scalar registers, loaded once per wave before the tile loop (BinQueries), larger rows stage
// them once per block in LDS.  Distance = xor + popcount, accumulated in int.
//
// Selection: key = (u64)(dist + 1) << 32 | row (bin_key: the + 1 keeps every real key above 0) -- ascending key is
// ascending (distance, id), so the "ties by ascending id" rule is key order.  Per wave and query: a threshold key (KEY_PAD until kp keys are held), lanes under it are
// ballot-appended to an LDS buffer of BIN_CAP keys; when fewer than 64 slots are free, wave_cut (a windowed cut: a few
// rounds, no sort) keeps between kp and kp + kp / 2 + 4 (at most BIN_CUT_MAX) of them and its cut key becomes the
// threshold -- a window close to kp, so that the threshold is tight and a wave rarely cuts twice.  At the end the
// block selects once per query: a wave takes every fourth query, gathers the four waves' buffers (at most 512 keys)
// and wave_select writes the kp smallest, SORTED, as the block's list.  pass_merge_kernel<int> walks the blocks' lists
// (merge_waves, ise_merge.hpp) and writes int32 D / int64 I.  A pass yields at most BIN_KPASS results per query; a
// larger k repeats the pass with lo = (last key found) + 1 as the smallest key admitted.
// The same scheme serves the other coded kinds as CandBuf (ise_cand.hpp); this kernel keeps its own body, with the waves'
// final counts in LDS (cnts) where CandBuf pads the buffers' tails: measured, the shared body was 0.1 to 0.3 us slower on
// the masked scan at 16 queries over a 1 % random selection (profiles/cands).
//
// Selectors: binary_scan_masked_kernel / binary_range_masked_kernel are the same passes over the tiles
// of a selector's row window, skipping every 64-row tile whose mask word is zero (BinMask); the unmasked kernels are
// the same body with the mask compiled out.  binary_sel_census_kernel counts a bitmap's rows, window and non-empty
// 64-row tiles.
//
// remove_ids: the stable in-place compaction of ise_remove.hpp (source map, ascending slabs, gather into a bounce
// buffer, copy back, ordered by one stream).  Rows of ws >= 2 words are whole 16-byte units and move with
// remove_rows_kernel (upr = ws / 2); the 8-byte rows of ws == 1 move with binary_remove_words_kernel below.  The tail
// [n_new, n_old) is NOT zeroed: rows at or beyond n are masked by row number in every kernel here, and an add
// overwrites whole padded rows.
#pragma once
#include <climits>

#include "ise_common.hpp"
#include "ise_merge.hpp"
#include "ise_select.hpp"

#define BIN_QT 16     /* queries per pass */
#define BIN_WAVES 4   /* waves per block */
#define BIN_KPASS 32  /* results per query and pass */
#define BIN_CAP 128   /* keys of a wave's buffer per query: two registers per lane in wave_cut */
#define BIN_CUT_MAX 48 /* most keys a cut in the stream keeps (at least kp) */
#define BIN_BUF_BYTES (BIN_WAVES * BIN_QT * BIN_CAP * 8)
#define BIN_CNT_BYTES (BIN_WAVES * BIN_QT * 4)
#define BIN_CHUNK_UNROLL 4 /* 16-byte chunks of a long row in flight per lane */
#define BIN_MAX_WS 128 /* ISE_BINARY_MAX_BITS / 64 */
#define BIN_LDS_MAX (BIN_BUF_BYTES + BIN_CNT_BYTES + BIN_QT * BIN_MAX_WS * 8)

static_assert(BIN_CUT_MAX + 64 <= BIN_CAP && BIN_KPASS <= BIN_CUT_MAX, "a tile's 64 keys fit behind the kept ones");
static_assert(BIN_WAVES * BIN_CAP == 512, "the block's selection holds the waves' buffers in eight registers per lane");
static_assert(BIN_KPASS <= MERGE_FAST_K, "merge_waves serves every pass");

// The tile's 16 queries as a wave reads them.  WT = 1, 2 (a row is one or two words): 16 or 32 words held in SCALAR
// registers, loaded once per wave before the tile loop from wave-uniform addresses (qpad: 16 padded queries readable;
// the words of queries the tile does not have are never used).  WT = 0: the block's LDS copy, [16][ws], staged once
// per block, rows of queries the tile does not have zero; init ends with a block barrier.
template <int WT>
struct BinQueries {
    u64 w[WT == 0 ? 1 : BIN_QT * WT];
    const u64* lds;
    __device__ __forceinline__ void init(u64* qs, const u64* __restrict__ qpad, int ws, int nqt) {
        lds = qs;
        if constexpr (WT == 0) {
            for (int i = threadIdx.x; i < BIN_QT * ws; i += BIN_WAVES * 64) qs[i] = i < nqt * ws ? qpad[i] : 0ull;
            __syncthreads();
        } else {
#pragma unroll
            for (int i = 0; i < BIN_QT * WT; i++) w[i] = readlane_u64(qpad[i], 0);  // every lane is active here
        }
    }
};

// Hamming distance of one row (this lane's) to the 16 queries of the tile.
template <int WT>
__device__ __forceinline__ void hamming16(const u64* __restrict__ codes, int ws, long long row, bool valid,
                                          const BinQueries<WT>& qr, int (&acc)[BIN_QT]) {
    if constexpr (WT == 1) {
        const u64 r = valid ? codes[row] : 0ull;
#pragma unroll
        for (int q = 0; q < BIN_QT; q++) acc[q] = __popcll(r ^ qr.w[q]);
    } else if constexpr (WT == 2) {
        ulonglong2 r = make_ulonglong2(0ull, 0ull);
        if (valid) r = *reinterpret_cast<const ulonglong2*>(codes + row * 2);
#pragma unroll
        for (int q = 0; q < BIN_QT; q++) acc[q] = __popcll(r.x ^ qr.w[2 * q]) + __popcll(r.y ^ qr.w[2 * q + 1]);
    } else {
#pragma unroll
        for (int q = 0; q < BIN_QT; q++) acc[q] = 0;
        const int nch = ws >> 1;
        const ulonglong2* rp = reinterpret_cast<const ulonglong2*>(codes + (valid ? row : 0ll) * ws);
        const ulonglong2* qp = reinterpret_cast<const ulonglong2*>(qr.lds);
#pragma unroll BIN_CHUNK_UNROLL
        for (int c = 0; c < nch; c++) {
            const ulonglong2 r = rp[c];
#pragma unroll
            for (int q = 0; q < BIN_QT; q++) {
                const ulonglong2 v = qp[q * nch + c];
                acc[q] += __popcll(r.x ^ v.x) + __popcll(r.y ^ v.y);
            }
        }
    }
}

// The candidate key: ascending key = ascending (distance, row).  The distance is stored + 1 so that every real key
// lies strictly between 0 and KEY_PAD -- what wave_cut and wave_select (ise_select.hpp) require: (distance 0, row 0),
// a query that is the index's first row, would otherwise be key 0, which wave_cut keeps but does not count.
// PassOut<int> (ise_merge.hpp) takes the 1 off again.
__device__ __forceinline__ u64 bin_key(int dist, long long row) { return ((u64)((uint32_t)dist + 1u) << 32) | (uint32_t)row; }

struct BinScanParams {
    const u64* codes;  // [n][ws]
    int ws;
    long long n;
    const u64* qpad;  // the tile's queries, [16][ws] readable
    int nqt, kp;      // queries of the tile (<= 16), results of this pass (<= BIN_KPASS)
    const u64* lo;    // [nqt] smallest key admitted (KEY_PAD: the query is finished); null in the first pass: 0
    u64* lists;       // [grid][16][BIN_KPASS]: one sorted list per block and query, KEY_PAD behind the last
};

// A selector's device side (ise_binary_selector, ise_binary_scan.hip): the bitmap read as one 8-byte word per 64-row
// tile -- bit r & 63 of word r >> 6, which is bit r & 31 of uint32 word r >> 5 -- and the tiles [tile0, tile1) of
// the window from the first to the last selected row.  The allocation holds a whole word for every tile below
// ceil(ntotal / 64); bits at or beyond ntotal are zero.
struct BinMask {
    const u64* words;
    long long tile0, tile1;
};

// MASK: the pass runs over the window's tiles only; a wave reads the tile's mask word (wave-uniform, before any row
// load is issued) and skips a tile without a selected row -- no load, no append, no cut check.  Behind `valid`
// nothing differs from the unmasked pass, and all 64 lanes stay active at every readlane / ballot.
template <int WT, bool MASK>
__device__ __forceinline__ void binary_scan_body(const BinScanParams p, const BinMask mk) {
    extern __shared__ __align__(16) unsigned char smem_bin[];
    u64* buf = reinterpret_cast<u64*>(smem_bin);  // [BIN_WAVES][16][BIN_CAP]
    int* cnts = reinterpret_cast<int*>(buf + BIN_WAVES * BIN_QT * BIN_CAP);  // [BIN_WAVES][16] keys held at the end
    u64* qs = buf + BIN_WAVES * BIN_QT * BIN_CAP + BIN_CNT_BYTES / 8;  // WT == 0: [16][ws]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    BinQueries<WT> qr;
    qr.init(qs, p.qpad, p.ws, p.nqt);
    u64* mybuf = buf + w * BIN_QT * BIN_CAP;
    const int kp = p.kp;
    // per-query state of the wave, query q in lane q: keys held, threshold (a new key must be below it), floor
    int cnt_v = 0;
    u64 thr_v = KEY_PAD;
    const u64 lo_v = lane < p.nqt ? (p.lo ? p.lo[lane] : 0ull) : KEY_PAD;
    const u64 lt_mask = (1ull << lane) - 1ull;

    // query q's buffer is nearly full (more than BIN_CAP - 64 >= BIN_CUT_MAX keys): keep between kp and kmax of them,
    // unsorted; everything kept is <= the cut key, which becomes the threshold
    const int kmax = kp + kp / 2 + 4 < BIN_CUT_MAX ? kp + kp / 2 + 4 : BIN_CUT_MAX;
    auto cut = [&](int q) {
        const int cnt = __builtin_amdgcn_readlane(cnt_v, q);
        u64 kk[2];
#pragma unroll
        for (int e = 0; e < 2; e++) kk[e] = lane + 64 * e < cnt ? mybuf[q * BIN_CAP + lane + 64 * e] : KEY_PAD;
        u64 ckey = KEY_PAD;
        const int nw = wave_cut<2>(kk, BIN_CAP, kp, kmax, mybuf + q * BIN_CAP, &ckey);
        wave_lds_fence();
        if (lane == q) {
            cnt_v = nw;
            thr_v = ckey;
        }
    };

    const long long ntiles = MASK ? mk.tile1 : (p.n + 63) >> 6;
    for (long long t = (MASK ? mk.tile0 : 0ll) + (long long)blockIdx.x * BIN_WAVES + w; t < ntiles;
         t += (long long)gridDim.x * BIN_WAVES) {
        const long long row = t * 64 + lane;
        u64 mw = ~0ull;
        if constexpr (MASK) {
            mw = readlane_u64(mk.words[t], 0);  // t is wave-uniform: one scalar 8-byte load
            if (mw == 0ull) continue;
        }
        const bool valid = MASK ? (row < p.n && ((mw >> lane) & 1ull)) : row < p.n;
        int acc[BIN_QT];
        hamming16<WT>(p.codes, p.ws, row, valid, qr, acc);
#pragma unroll
        for (int q = 0; q < BIN_QT; q++) {
            if (q < p.nqt) {
                const u64 key = bin_key(acc[q], row);
                const bool c = valid && key >= readlane_u64(lo_v, q) && key < readlane_u64(thr_v, q);
                const u64 m = __ballot(c);
                if (m) {
                    const int cnt = __builtin_amdgcn_readlane(cnt_v, q);
                    if (c) mybuf[q * BIN_CAP + cnt + __popcll(m & lt_mask)] = key;
                    if (lane == q) cnt_v += __popcll(m);
                }
            }
        }
        wave_lds_fence();
        u64 need = __ballot(cnt_v > BIN_CAP - 64);  // the next tile may not fit
        while (need) {
            const int q = __ffsll((long long)need) - 1;
            need &= need - 1;
            cut(q);
        }
    }
    if (lane < BIN_QT) cnts[w * BIN_QT + lane] = cnt_v;
    __syncthreads();
    // the waves' buffers -> the block's sorted list
    for (int q = w; q < p.nqt; q += BIN_WAVES) {
        u64 kk[2 * BIN_WAVES];
#pragma unroll
        for (int e = 0; e < 2 * BIN_WAVES; e++) {
            const int sw = e >> 1, i = lane + 64 * (e & 1);
            kk[e] = i < cnts[sw * BIN_QT + q] ? buf[(sw * BIN_QT + q) * BIN_CAP + i] : KEY_PAD;
        }
        u64* dst = p.lists + ((size_t)blockIdx.x * BIN_QT + q) * BIN_KPASS;
        u64 kth_unused = 0;
        const int nw = wave_select<2 * BIN_WAVES>(kk, BIN_WAVES * BIN_CAP, kp, dst, &kth_unused);
        for (int i = nw + lane; i < kp; i += 64) dst[i] = KEY_PAD;
    }
}

template <int WT>
__global__ __launch_bounds__(BIN_WAVES * 64) void binary_scan_kernel(const BinScanParams p) {
    binary_scan_body<WT, false>(p, BinMask{});
}

template <int WT>
__global__ __launch_bounds__(BIN_WAVES * 64) void binary_scan_masked_kernel(const BinScanParams p, const BinMask mk) {
    binary_scan_body<WT, true>(p, mk);
}

// ---- range search: every row with dist < radius, per query in ascending row order.  The rows are cut into S
// consecutive SEGMENTS of seg_rows (a multiple of 64), one per wave, segment s = 4 * block + wave: the count pass
// leaves counts[q][s], an exclusive scan over (q, s) gives every segment's first output slot, and the fill pass
// writes a segment's matches tile by tile at ballot-prefix positions -- ascending id by construction, no sort.
// The scan is two small kernels: binary_offsets_kernel, one block per query, scans the query's S counts;
// binary_lims_kernel scans the queries' totals into lims.
struct BinRangeParams {
    const u64* codes;
    int ws;
    long long n;
    const u64* qpad;  // the tile's queries
    int nqt, radius;
    long long seg_rows;
    int S;
    int* counts;            // count pass: the tile's first query, [nqt][S]
    const long long* offs;  // fill pass: the same shape, first output slot of (q, s) within query q's results
    const long long* lims;  // fill pass: the tile's first query, [nqt] first output slot of the query
    int* D;                 // fill pass: the batch's results
    long long* I;
};

// MASK: the segments cut the selector's window instead of [0, n): segment s starts at mk.tile0 * 64 + s * seg_rows --
// a multiple of 64 in absolute row numbers, so a tile's mask word is still index row >> 6 -- and the last one ends
// at mk.tile1 * 64 or n; a tile without a selected row is skipped before its loads, as in the scan.
template <int WT, bool FILL, bool MASK>
__device__ __forceinline__ void binary_range_body(const BinRangeParams p, const BinMask mk) {
    extern __shared__ __align__(16) unsigned char smem_bin[];
    u64* qs = reinterpret_cast<u64*>(smem_bin);  // WT == 0: [16][ws]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    BinQueries<WT> qr;
    qr.init(qs, p.qpad, p.ws, p.nqt);
    const int s = blockIdx.x * BIN_WAVES + w;
    const long long r0 = (MASK ? mk.tile0 * 64 : 0ll) + (long long)s * p.seg_rows;
    const long long rend = MASK && mk.tile1 * 64 < p.n ? mk.tile1 * 64 : p.n;
    const long long r1 = r0 + p.seg_rows < rend ? r0 + p.seg_rows : rend;
    const u64 lt_mask = (1ull << lane) - 1ull;
    int cnt_v = 0;  // query q in lane q
    u64 base_v = 0;
    if (FILL && lane < p.nqt) base_v = (u64)(p.lims[lane] + p.offs[(size_t)lane * p.S + s]);
    for (long long rb = r0; rb < r1; rb += 64) {
        const long long row = rb + lane;
        u64 mw = ~0ull;
        if constexpr (MASK) {
            mw = readlane_u64(mk.words[rb >> 6], 0);  // rb is wave-uniform
            if (mw == 0ull) continue;
        }
        const bool valid = MASK ? (row < r1 && ((mw >> lane) & 1ull)) : row < r1;
        int acc[BIN_QT];
        hamming16<WT>(p.codes, p.ws, row, valid, qr, acc);
#pragma unroll
        for (int q = 0; q < BIN_QT; q++) {
            if (q < p.nqt) {
                const bool c = valid && acc[q] < p.radius;
                const u64 m = __ballot(c);
                if (m) {
                    if (FILL) {
                        const u64 at = readlane_u64(base_v, q) + (u64)__popcll(m & lt_mask);
                        if (c) {
                            p.D[at] = acc[q];
                            p.I[at] = row;
                        }
                        if (lane == q) base_v += (u64)__popcll(m);
                    } else if (lane == q) {
                        cnt_v += __popcll(m);
                    }
                }
            }
        }
    }
    if (!FILL && lane < p.nqt) p.counts[(size_t)lane * p.S + s] = cnt_v;
}

template <int WT, bool FILL>
__global__ __launch_bounds__(BIN_WAVES * 64) void binary_range_kernel(const BinRangeParams p) {
    binary_range_body<WT, FILL, false>(p, BinMask{});
}

template <int WT, bool FILL>
__global__ __launch_bounds__(BIN_WAVES * 64) void binary_range_masked_kernel(const BinRangeParams p, const BinMask mk) {
    binary_range_body<WT, FILL, true>(p, mk);
}

// inclusive scan over the block's threads (NT a multiple of 64, at most 1024); wsum: NT / 64 entries of LDS
template <int NT>
__device__ __forceinline__ long long block_inclusive_scan(long long v, long long* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    long long before = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) before += i < w ? wsum[i] : 0;
    return v + before;
}

// block q: offs[q][s] = counts[q][0] + .. + counts[q][s - 1], totals[q] = the sum of the row.  S <= 4096.
#define BIN_SCAN_THREADS 1024
static_assert(MERGE_LISTS_MAX * BIN_WAVES <= 4 * BIN_SCAN_THREADS, "four segments per thread cover the largest grid");
static __global__ __launch_bounds__(BIN_SCAN_THREADS) void binary_offsets_kernel(const int* __restrict__ counts, int S,
                                                                                 long long* __restrict__ offs,
                                                                                 long long* __restrict__ totals) {
    __shared__ long long wsum[BIN_SCAN_THREADS / 64];
    const int t = threadIdx.x;
    const int* c = counts + (size_t)blockIdx.x * S;
    long long* o = offs + (size_t)blockIdx.x * S;
    int v[4];
    long long sum = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        v[e] = 4 * t + e < S ? c[4 * t + e] : 0;
        sum += v[e];
    }
    long long run = block_inclusive_scan<BIN_SCAN_THREADS>(sum, wsum) - sum;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (4 * t + e < S) o[4 * t + e] = run;
        run += v[e];
    }
    if (t == BIN_SCAN_THREADS - 1) totals[blockIdx.x] = run;
}

// lims[q] = totals[0] + .. + totals[q - 1] for q <= nq; nq <= 256, one block
static __global__ __launch_bounds__(256) void binary_lims_kernel(const long long* __restrict__ totals, int nq,
                                                                 long long* __restrict__ lims) {
    __shared__ long long wsum[4];
    const int t = threadIdx.x;
    const long long v = t < nq ? totals[t] : 0;
    const long long incl = block_inclusive_scan<256>(v, wsum);
    if (t < nq) lims[t + 1] = incl;
    if (t == 0) lims[0] = 0;
}

// n rows of code_size bytes -> n rows of ws words, the bytes past code_size zero (queries and device-side adds)
static __global__ void binary_pad_kernel(const uint8_t* __restrict__ src, int code_size, u64* __restrict__ dst, int ws,
                                         long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * ws) return;
    const long long r = i / ws;
    const int wd = (int)(i % ws);
    const uint8_t* s = src + r * code_size;
    u64 v = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const int j = wd * 8 + b;
        if (j < code_size) v |= (u64)s[j] << (8 * b);
    }
    dst[i] = v;
}

// ---- selectors: the census of a bitmap, read as one 8-byte word per 64-row tile.  Bits at or beyond n are cleared
// (a user's bitmap); out[0] selected rows, out[1] non-empty 64-row tiles, out[2] first selected row (init: ~0),
// out[3] last selected row + 1 (init: 0)
static __global__ __launch_bounds__(256) void binary_sel_census_kernel(u64* words, long long nwords, long long n,
                                                                       unsigned long long* out) {
    const long long wd = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cnt = 0, tiles = 0, lo = ~0ull, hi = 0;
    if (wd < nwords) {
        u64 v = words[wd];
        const long long left = n - wd * 64;
        if (left < 64) {
            const u64 keep = left <= 0 ? 0ull : ((1ull << left) - 1ull);
            if (v & ~keep) words[wd] = v & keep;
            v &= keep;
        }
        if (v) {
            cnt = (unsigned long long)__popcll(v);
            tiles = 1;
            lo = (unsigned long long)(wd * 64 + (__ffsll((long long)v) - 1));
            hi = (unsigned long long)(wd * 64 + (64 - __clzll((long long)v)));
        }
    }
    // one atomic per wave and field
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        tiles += __shfl_xor(tiles, o);
        const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(out + 0, cnt);
        atomicAdd(out + 1, tiles);
        atomicMin(out + 2, lo);
        atomicMax(out + 3, hi);
    }
}

// ---- remove_ids, ws == 1: rows of 8 bytes, half a 16-byte unit, which remove_rows_kernel (ise_remove.hpp) cannot
// gather.  The same shape: dst[i] <- src[GATHER ? idx[i] : i], i < total, dealt to the waves grid-stride in pieces of
// BIN_REMOVE_UNROLL wave-loads; a wave issues all of a piece's loads before its first store.
#define BIN_REMOVE_UNROLL 8 /* independent 8-byte loads per lane in flight (4 KiB per wave and piece) */
template <bool GATHER>
__global__ __launch_bounds__(256) void binary_remove_words_kernel(const u64* __restrict__ src, const uint32_t* __restrict__ idx,
                                                                  u64* __restrict__ dst, uint32_t total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const uint32_t piece = 64 * BIN_REMOVE_UNROLL;
    const uint32_t npieces = (total + piece - 1) / piece;
    for (uint32_t p = wave; p < npieces; p += nwaves) {
        const uint32_t base = p * piece + lane;
        // a piece's tail past `total` re-reads the last row (no branch between the loads) and is not stored
        size_t s[BIN_REMOVE_UNROLL];
#pragma unroll
        for (int t = 0; t < BIN_REMOVE_UNROLL; t++) {
            const uint32_t i = min(base + 64 * t, total - 1);
            s[t] = GATHER ? (size_t)idx[i] : (size_t)i;
        }
        u64 v[BIN_REMOVE_UNROLL];
#pragma unroll
        for (int t = 0; t < BIN_REMOVE_UNROLL; t++) v[t] = __builtin_nontemporal_load(src + s[t]);
#pragma unroll
        for (int t = 0; t < BIN_REMOVE_UNROLL; t++) {
            const uint32_t i = base + 64 * t;
            if (i < total) dst[i] = v[t];
        }
    }
}
