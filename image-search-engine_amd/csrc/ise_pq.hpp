// ise_pq.hpp -- kernels of the product-quantised index (include/ise_knn.h, ise_pq_*): faiss.IndexPQ with 8-bit
// sub-quantisers.  DESIGN.md 4.13.  The table and scan code lives here, apart from the host side (ise_pq.hip): the
// inverted lists over these codes (ise_ivfpq.hpp) include it, and their pass is pq_scan_body too.
//
// Codec: a row of d floats is M sub-vectors of dsub = d / M; byte m of its code is the number j of the centroid
// C[m][j] (codebook [M][256][dsub], float32) nearest to sub-vector m in squared L2, the lowest j among equals.
//
// Storage: [n][stride] bytes, stride = M rounded up to a multiple of 16, the bytes past M zero; a lane loads its row
// in 16-byte pieces and never looks a pad byte up.  Rows at or beyond n are masked by row number.
//
// Search is asymmetric distance computation: score(query x, row i) = sum_m T[m][code[i][m]], T[m][j] =
// |x_m - C[m][j]|^2 (L2, the direct difference) or <x_m, C[m][j]> (inner product), accumulated in ascending m from
// +0.0f (so a sum of signed zeros is +0).  pq_table_kernel builds the tables of up to PQ_TAB_CHUNK queries, laid out
// per pass: [group][m][256][QT], the pass's QT queries innermost, so that ONE LDS read per (row, m) serves 4 queries
// (QT >= 4: ds_read_b128; QT = 2: ds_read_b64).
//
// Scan (pq_scan_kernel<QT>): the shape of the binary scan (ise_binary_scan.hpp) -- a lane owns a row, a wave a tile of
// 64 consecutive rows, QT queries per pass, the tile's keys ballot-appended per query -- and the k-pass of ise_cand.hpp
// behind it (CandBuf, query q's state in lane q; pass_merge_kernel<float>), a pass repeated with a floor key for
// k > PQ_KPASS.  What is new: the pass's tables sit in LDS ([m][256][QT], copied in by the whole block), and the lane
// walks the bytes of its code and gathers.  Key = ord_f32(score) << 32 | row (inner product: of -score): ascending key
// is (best score, ascending id); a score enters only if it is < FLT_MAX (NaN never), so every key lies strictly between
// 0 and KEY_PAD.
//
// LDS: QT * (M KiB of tables + 4 KiB of selection buffers: PQ_WAVES * PQ_CAP keys per query), nothing else, against
// 160 KiB per CU:
//   QT(M) = 16 for M <= 5, 8 for M <= 15, 4 for M <= 35, 2 for M <= ISE_PQ_MAX_M = 64   (pq_qt)
// i.e. the largest power of two with QT * (M + 4) KiB <= 160 KiB; M = 16 takes 80 KiB, two blocks per CU.
#pragma once
#include "ise_cand.hpp"

#define PQ_KSUB 256     /* centroids per sub-quantiser (8 bits) */
#define PQ_WAVES 4      /* waves per block */
#define PQ_KPASS 32     /* results per query and pass */
#define PQ_CAP 128      /* keys of a wave's buffer per query: two registers per lane in wave_cut */
#define PQ_CUT_MAX 48   /* most keys a cut in the stream keeps (at least kp) */
#define PQ_QT_MAX 16    /* most queries per pass */
#define PQ_TAB_CHUNK 64 /* queries whose tables one pq_table_kernel launch builds: a multiple of every QT */
#define PQ_COPY_UNROLL 8 /* 16-byte loads in flight per thread while the tables are copied into LDS */
#define PQ_LDS_LIMIT (160 * 1024)

template <int QT>
using PqCand = CandBuf<QT, PQ_WAVES, PQ_CAP, 64, PQ_CUT_MAX, PQ_KPASS>;

// queries per pass for M sub-quantisers, and the pass's LDS
constexpr int pq_qt(int M) { return M <= 5 ? 16 : M <= 15 ? 8 : M <= 35 ? 4 : 2; }
constexpr size_t pq_lds_bytes(int M, int qt) { return (size_t)qt * ((size_t)M * PQ_KSUB * 4 + PQ_WAVES * PQ_CAP * 8); }
static_assert(pq_lds_bytes(5, 16) <= PQ_LDS_LIMIT && pq_lds_bytes(15, 8) <= PQ_LDS_LIMIT &&
                  pq_lds_bytes(35, 4) <= PQ_LDS_LIMIT && pq_lds_bytes(ISE_PQ_MAX_M, 2) <= PQ_LDS_LIMIT,
              "every QT(M) fits the CU's LDS");
static_assert(PQ_TAB_CHUNK % PQ_QT_MAX == 0, "a chunk is whole groups");

// ---- tables.  Block (m, g): sub-quantiser m, group g of the launch (QT queries from q0 = g * QT); thread j owns
// centroid j.  tab[g][m][j][qi]; queries at or beyond nq give zero entries (never read as results).  The query's
// sub-vector is read at wave-uniform addresses.  On integer inputs every entry is the exact integer (a sum of exact
// squares / products, each partial sum an integer below 2^24).
static __global__ __launch_bounds__(PQ_KSUB) void pq_table_kernel(const float* __restrict__ q, int nq, int d, int M, int qt,
                                                                  int ip, const float* __restrict__ cb,
                                                                  float* __restrict__ tab) {
    const int m = blockIdx.x, g = blockIdx.y, j = threadIdx.x;
    const int dsub = d / M;
    const float* c = cb + ((size_t)m * PQ_KSUB + j) * dsub;
    float* out = tab + (((size_t)g * M + m) * PQ_KSUB + j) * qt;
    for (int qi = 0; qi < qt; qi++) {
        const int qq = g * qt + qi;
        float acc = 0.f;
        if (qq < nq) {
            const float* x = q + (size_t)qq * d + (size_t)m * dsub;
            if (ip) {
                for (int t = 0; t < dsub; t++) acc = fmaf(x[t], c[t], acc);
            } else {
                for (int t = 0; t < dsub; t++) {
                    const float df = x[t] - c[t];
                    acc = fmaf(df, df, acc);
                }
            }
        }
        out[qi] = acc;
    }
}

// ---- scan
struct PqScanParams {
    const uint8_t* codes;  // [n][stride]
    int M, stride;
    long long n;
    const float* tab;  // the pass's tables, [M][256][QT]
    int nqt, kp;       // queries of the pass (<= QT), results of this pass (<= PQ_KPASS)
    int ip;            // inner product: the key is taken of -score
    const u64* lo;     // [nqt] smallest key admitted (KEY_PAD: the query is finished); null in the first pass: 0
    u64* lists;        // [grid][QT][PQ_KPASS]: one sorted list per block and query, KEY_PAD behind the last
};

// acc[0 .. QT) += T[m][j][0 .. QT): one ds_read_b128 per four queries, one ds_read_b64 for QT = 2
template <int QT>
__device__ __forceinline__ void pq_gather(const float* __restrict__ tabs, int m, uint32_t j, float (&acc)[QT]) {
    const float* e = tabs + ((size_t)m * PQ_KSUB + j) * QT;
    if constexpr (QT == 2) {
        const float2 v = *reinterpret_cast<const float2*>(e);
        acc[0] += v.x;
        acc[1] += v.y;
    } else {
#pragma unroll
        for (int c = 0; c < QT / 4; c++) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(e + 4 * c);
#pragma unroll
            for (int i = 0; i < 4; i++) acc[4 * c + i] += v[i];
        }
    }
}

// The scan of one pass, for both layouts (IVF false: the flat index's rows [0, n), pq_scan_kernel; IVF true: the work
// list of an inverted-list pass, P = PqIvfScanParams, ise_ivfpq.hpp).  What differs stands under `if constexpr (IVF)`:
// which tile a wave's next unit names, the row mask (row < n | position < valid rows and the query's mask bit) and the
// key's low word (row | ids[slot]).  The table copy into LDS, the gathers, the selection buffers and the block's fold
// exist once.
template <int QT, bool IVF, class P>
__device__ __forceinline__ void pq_scan_body(const P& p) {
    extern __shared__ __align__(16) unsigned char smem_pq[];
    float* tabs = reinterpret_cast<float*>(smem_pq);                                 // [M][256][QT]
    u64* buf = reinterpret_cast<u64*>(smem_pq + (size_t)p.M * PQ_KSUB * QT * 4);  // [PQ_WAVES][QT][PQ_CAP]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    [[maybe_unused]] long long nent = 0;  // IVF: entries of the group's work list
    if constexpr (IVF) {
        nent = (long long)__builtin_amdgcn_readfirstlane((int)*p.count);
        if (blockIdx.x == 0 && threadIdx.x == 0 && nent) atomicAdd(p.tiles_loaded, (unsigned long long)nent);
        if ((long long)blockIdx.x * PQ_WAVES >= nent) {  // no entry for this block: its lists are padding, no table is copied
            for (int i = threadIdx.x; i < p.nqt * PQ_KPASS; i += PQ_WAVES * 64)
                p.lists[(size_t)blockIdx.x * QT * PQ_KPASS + i] = KEY_PAD;
            return;
        }
    }
    {  // the pass's tables, PQ_COPY_UNROLL loads in flight per thread
        const f32x4* src = reinterpret_cast<const f32x4*>(p.tab);
        f32x4* dst = reinterpret_cast<f32x4*>(tabs);
        const int units = p.M * PQ_KSUB * QT / 4;
        int i = threadIdx.x;
        for (; i + (PQ_COPY_UNROLL - 1) * PQ_WAVES * 64 < units; i += PQ_COPY_UNROLL * PQ_WAVES * 64) {
            f32x4 v[PQ_COPY_UNROLL];
#pragma unroll
            for (int u = 0; u < PQ_COPY_UNROLL; u++) v[u] = src[i + u * PQ_WAVES * 64];
#pragma unroll
            for (int u = 0; u < PQ_COPY_UNROLL; u++) dst[i + u * PQ_WAVES * 64] = v[u];
        }
        for (; i < units; i += PQ_WAVES * 64) dst[i] = src[i];
    }
    __syncthreads();
    // per-query state of the wave, query q in lane q: keys held, threshold (a new key must be below it), floor
    PqCand<QT> cand(buf, w, lane, p.kp);
    const u64 lo_v = lane < p.nqt ? (p.lo ? p.lo[lane] : 0ull) : KEY_PAD;
    const u64 lt_mask = (1ull << lane) - 1ull;
    const uint32_t flip = p.ip ? 0x80000000u : 0u;

    long long ntiles;  // units of the pass: the index's tiles | the work list's entries
    if constexpr (IVF) ntiles = nent;
    else ntiles = (p.n + 63) >> 6;
    const int pieces = p.stride >> 4;
    const long long tstep = (long long)gridDim.x * PQ_WAVES;
    // one tile: the lane's row starts at rp, its first piece is cv (loaded a tile ahead); the lane takes part if `valid`
    // (IVF: and query q if bit q of qmask is set), the key's low word is `low`
    auto scan_tile = [&](const u32x4* rp, u32x4 cv, bool valid, [[maybe_unused]] uint32_t qmask, uint32_t low) {
        float acc[QT];
#pragma unroll
        for (int q = 0; q < QT; q++) acc[q] = 0.f;
        for (int c = 0; c < pieces; c++) {
            const u32x4 cn = c + 1 < pieces ? rp[c + 1] : cv;  // the row's next piece, requested before this one is used
            const int m0 = 16 * c;
#pragma unroll
            for (int b = 0; b < 16; b++) {
                if (m0 + b < p.M) pq_gather<QT>(tabs, m0 + b, (cv[b >> 2] >> (8 * (b & 3))) & 0xFFu, acc);  // wave-uniform
            }
            cv = cn;
        }
#pragma unroll
        for (int q = 0; q < QT; q++) {
            if (q < p.nqt) {
                const float s = __uint_as_float(__float_as_uint(acc[q]) ^ flip);
                const u64 key = ((u64)ord_f32(s) << 32) | low;
                bool c = valid && s < FLT_MAX && key >= readlane_u64(lo_v, q) && key < readlane_u64(cand.thr, q);
                if constexpr (IVF) c = c && ((qmask >> q) & 1u);
                const u64 mk = __ballot(c);
                if (mk) {
                    const int cnt = __builtin_amdgcn_readlane(cand.cnt, q);
                    if (c) cand.keys(q)[cnt + __popcll(mk & lt_mask)] = key;
                    if (lane == q) cand.cnt += __popcll(mk);
                }
            }
        }
        cand.make_room();
    };
    long long t = (long long)blockIdx.x * PQ_WAVES + w;
    if constexpr (IVF) {
        // t counts ENTRIES; an entry is (tile, valid rows, query mask, 0), the lane owns slot tile * 64 + lane.  The entry
        // two steps on, and the first piece and the id of the next entry's slot, are requested before this tile's
        // gathers, so no code-byte request waits for the entry it has just asked for.  Behind the wave's last entry: the
        // list's last entry again -- a valid tile, unused
        auto entry_at = [&](long long e) { return p.work[e < nent ? e : nent - 1]; };
        auto slot_of = [&](uint32_t tile) { return (size_t)tile * 64 + lane; };
        auto slot_piece = [&](uint32_t tile) { return reinterpret_cast<const u32x4*>(p.codes + slot_of(tile) * p.stride); };
        u32x4 cent = entry_at(t), cnext = entry_at(t + tstep);
        u32x4 ahead = *slot_piece(cent[0]);
        uint32_t aid = p.ids[slot_of(cent[0])];
        for (; t < ntiles; t += tstep) {
            const u32x4* rp = slot_piece(cent[0]);
            const u32x4 cv = ahead;
            const uint32_t id = aid;
            const u32x4 cafter = entry_at(t + 2 * tstep);
            ahead = *slot_piece(cnext[0]);
            aid = p.ids[slot_of(cnext[0])];
            scan_tile(rp, cv, lane < (int)cent[1], cent[2], id);
            cent = cnext;
            cnext = cafter;
        }
    } else {
        // the first 16 bytes of the lane's row in tile t (a lane beyond n reads row 0 and is masked)
        auto row_piece = [&](long long tt) {
            const long long r = tt * 64 + lane;
            return reinterpret_cast<const u32x4*>(p.codes + (r < p.n ? r : 0ll) * p.stride);
        };
        u32x4 ahead = t < ntiles ? *row_piece(t) : u32x4{0u, 0u, 0u, 0u};
        for (; t < ntiles; t += tstep) {
            const long long row = t * 64 + lane;
            const u32x4* rp = row_piece(t);
            const u32x4 cv = ahead;
            if (t + tstep < ntiles) ahead = *row_piece(t + tstep);  // the next tile's load flies under this tile's gathers
            scan_tile(rp, cv, row < p.n, 0u, (uint32_t)row);
        }
    }
    cand.fold(p.nqt, p.lists + (size_t)blockIdx.x * QT * PQ_KPASS);
}

template <int QT>
__global__ __launch_bounds__(PQ_WAVES * 64) void pq_scan_kernel(const PqScanParams p) {
    pq_scan_body<QT, false>(p);
}

// ---- encoding (build side).  A wave owns a row at a time, block (rows, m) sub-quantiser m = blockIdx.y: lane l holds
// centroids l, l + 64, l + 128, l + 192 and the row's sub-vector is read at wave-uniform addresses; the distance is the
// direct difference, the winner the smallest (distance, j) key over the wave -- the lowest j among equals.  LDSC: the
// sub-quantiser's centroids staged once per block, transposed [t][256] (conflict-free: lane l reads word t * 256 + l
// + 64 e); otherwise (dsub too long for LDS) they are read from the codebook in place.  A row with a NaN or inf entry
// sets *bad (the caller then drops the whole call); its byte is whatever the arithmetic gives.
#define PQ_ENC_ROWS 64      /* rows per block: 16 per wave */
#define PQ_ENC_LDS_DSUB 128 /* longest sub-vector whose 256 centroids are staged in LDS (128 KiB) */
template <bool LDSC>
__global__ __launch_bounds__(PQ_WAVES * 64) void pq_encode_kernel(const float* __restrict__ x, long long n, int d, int M,
                                                                   const float* __restrict__ cb, uint8_t* __restrict__ codes,
                                                                   int stride, unsigned int* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem_pq[];
    float* ct = reinterpret_cast<float*>(smem_pq);  // LDSC: [dsub][256]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int m = blockIdx.y, dsub = d / M;
    const float* c = cb + (size_t)m * PQ_KSUB * dsub;  // [256][dsub]
    if constexpr (LDSC) {
        for (int i = threadIdx.x; i < PQ_KSUB * dsub; i += PQ_WAVES * 64) ct[(i % dsub) * PQ_KSUB + i / dsub] = c[i];
        __syncthreads();
    }
    const long long r0 = (long long)blockIdx.x * PQ_ENC_ROWS;
    for (int i = w; i < PQ_ENC_ROWS; i += PQ_WAVES) {
        const long long row = r0 + i;  // wave-uniform
        if (row >= n) break;
        const float* xs = x + (size_t)row * d + (size_t)m * dsub;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float mark = 0.f;
        for (int t = 0; t < dsub; t++) {
            const float xv = xs[t];
            mark += nonfinite_mark(xv);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float cv = LDSC ? ct[t * PQ_KSUB + lane + 64 * e] : c[(size_t)(lane + 64 * e) * dsub + t];
                const float df = xv - cv;
                acc[e] = fmaf(df, df, acc[e]);
            }
        }
        u64 best = KEY_PAD;
#pragma unroll
        for (int e = 0; e < 4; e++) best = min_u64(best, ((u64)ord_f32(acc[e]) << 32) | (uint32_t)(lane + 64 * e));
        best = wave_min_u64(best);
        if (lane == 0) {
            codes[(size_t)row * stride + m] = (uint8_t)(best & 0xFFu);
            if (mark != mark) atomicOr(bad, 1u);
        }
    }
}

// ---- decoding: x[i][m * dsub + t] = C[m][code[i][m]][t]
static __global__ void pq_decode_kernel(const uint8_t* __restrict__ codes, int stride, long long n, int d, int M,
                                        const float* __restrict__ cb, float* __restrict__ x) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * d) return;
    const long long r = i / d;
    const int col = (int)(i % d), dsub = d / M, m = col / dsub;
    x[i] = cb[((size_t)m * PQ_KSUB + codes[(size_t)r * stride + m]) * dsub + (col - m * dsub)];
}
