// ise_flat.hpp -- the float index as its translation units share it: ise_knn.hip (the core: rows, shift and shadows,
// plans, the search paths) and one unit per feature, ise_flat_range.hip, ise_flat_sel.hip, ise_flat_subset.hip.  The
// handle with its workspaces, the row geometry, the host-context lease with the staged host search, and -- at the end
// -- what a feature may call in another unit.  Host code only; no kernels.
#pragma once
#include "ise_host.hpp"
#include "ise_geometry.hpp"

inline int fail(int code, const std::string& msg) { return ise_fail_(code, msg); }

struct ise_index {
    int d = 0, dp = 0, metric = ISE_METRIC_L2, device = 0;
    int storage = ISE_STORE_F32;  // element type of xb
    long long n = 0, cap = 0;
    void* xb = nullptr;
    float* norms = nullptr;
    // float32 L2 indexes: shift vector mu [dp] = column mean of the rows, (re)computed lazily at the
    // first search after the index has grown by a quarter since the last time (or pinned by
    // ise_index_set_shift); norms [0, norms_rows) are |y - mu|^2 for the current mu.  mu only
    // decides how tight the scan's lower bounds are -- results are exact for any mu (ise_exact.hpp)
    float* mu = nullptr;
    bool shift_pinned = false;
    long long mu_rows = 0;     // rows mu was computed from (0 = not yet)
    long long norms_rows = 0;  // rows whose norm is valid
    // fp16 shadow of the centred rows (float32 L2 indexes of more than SHADOW_MIN_ROWS rows): the scan's filter
    // streams it instead of xb (ise_scan.hpp HALF).  Built at the first search past the threshold, then kept
    // with the norms: valid for rows [0, norms_rows) whenever xh is set (launch_norms writes both)
    void* xh = nullptr;        // [cap][dph] fp16
    float* hmeta = nullptr;    // [3][cap]: |u~|^2, e_r, s_r
    int dph = 0;               // padded shadow row length (whole 64-byte k-steps)
    bool shadow_off = false;   // its allocation failed: the float32 filter serves (no retry until reset)
    // ... and its byte image (ise_scan.hpp BYTE), kept with the fp16 shadow: set only while xh is
    void* xq8 = nullptr;       // [cap][dpb] int8, tile-blocked (ise_byte_layout.hpp)
    uint32_t* bmeta = nullptr; // [cap]: c_r | e_r / c_r
    int dpb = 0;               // padded byte row length (whole 64-byte k-steps)
    bool byte_off = false;     // its allocation failed: the fp16 shadow serves (no retry until reset)
    double byte_rel = 0.0;     // mean e_r / |y - mu| when the byte shadow was last built over all rows (byte_rel_ok)
    double byte_rho = 1.0;     // ... and the sample rows' mean nearest-neighbour over mean pair distance (byte_rel_ok)
    unsigned long long half_batches = 0;  // batches whose filter read shadow rows, fp16 or byte (under mu_)
    unsigned long long byte_batches = 0;  // ... of them, those that read the byte shadow rows (under mu_)
    unsigned long long byte_deep_batches = 0;  // ... of those, the ones scanned with a deep plan (make_plan, depth > 1)
    // the stream of the index's previous search (search_enqueue, under mu_): a batch on another one is pipelined
    hipStream_t prev_stream = nullptr;
    bool prev_search = false;
    // [32]: 0 reranked queries, 1 exact-scan queries, 2 queries the large-batch path's plain select found incomplete
    // (ISE_STAT_GEMM_LOST), 8..23 the merge stage's debug stamps
    unsigned long long* stats_dev = nullptr;
    unsigned long long mu_updates = 0;
    unsigned long long gemm_chunks = 0;  // query chunks that took the large-batch path
    // workspaces (grown lazily, guarded by mu): NWS slots, so searches on different streams
    // may be in flight together.  A stream keeps the slot it used last (stream order is all
    // the ordering that needs); a stream without one takes a fresh slot, or the least
    // recently taken one behind an event wait.  Six slots on purpose: a server that issues
    // batches round-robin on more streams than that (bench.py: 16) gets at most six scans in
    // flight, chained slot to slot on the GPU, with the next ones already queued -- measured
    // best at 1M x 512 (303 us per batch against 328 with 4 streams and 319 with 16 slots)
    // With the byte route's deep plan (make_plan, depth 2) a scan fills half the block slots, so two of
    // the six slots' scans are resident together and the other four are the queue behind them.
    struct WorkSlot {
        DevBuf<u64> part;
        DevBuf<u64> keys_tmp;     // multi-pass k scratch
        DevBuf<u64> xchg;         // threshold-exchange entries of the scan kernel, tagged by xchg_seq
        uint32_t xchg_seq = 0;    // bumped per scan launch: entries of older launches never match
        // large-batch path (ise_gemm_scan.hpp): one allocation holding qprep | xn | tau | ccnt | sample keys | cand
        DevBuf<char> gemm;
        DevBuf<u64> fl_state;     // exact path: launch seq << 32 | number of queries on the fallback list
        DevBuf<int> fl_list;      // the listed queries
        uint32_t fl_seq = 0;      // bumped per rerank launch, never reset while fl_state lives
        CallOrder order;          // its event is made by ensure_workspace
        void release() {
            buf_free(part, keys_tmp, xchg, gemm, fl_state, fl_list);
            order.destroy();
            *this = WorkSlot();
        }
    };
    static constexpr int NWS = 6;
    WorkSlot ws[NWS];
    unsigned ws_next = 0;
    hipStream_t stream = nullptr;  // add / reconstruct / shift maintenance
    // host-API search contexts: a caller owns one for the duration of its call (CtxLease)
    struct HostCtx {
        hipStream_t stream = nullptr;
        DevBuf<float> q_dev, D_dev;
        DevBuf<long long> I_dev;
        // page-locked staging of a combined batch (queries in, results out; the results as the device addresses them)
        DevBuf<float, MEM_PINNED> q_pin;
        DevBuf<float, MEM_MAPPED> D_pin;
        DevBuf<long long, MEM_MAPPED> I_pin;
        bool busy = false;
        // the device staging: room for qe query floats and oe results
        int stage(size_t qe, size_t oe) {
            int rc = grow_owned(q_dev, qe);
            if (!rc) rc = grow_owned(D_dev, oe);
            if (!rc) rc = grow_owned(I_dev, oe);
            return rc;
        }
        void release() {
            buf_free(q_dev, D_dev, I_dev, q_pin, D_pin, I_pin);
            if (stream) (void)hipStreamDestroy(stream);
            *this = HostCtx();
        }
    };
    static constexpr int NHC = 4;
    HostCtx hc[NHC];
    std::mutex hc_mu;
    std::condition_variable hc_cv;
    // combining of concurrent host searches (ise_index_search_host): callers queue their request; one
    // of them -- at most CQ_LEADERS at a time -- takes the requests at the head of the queue that ask
    // for the same k, runs them as ONE batch and hands the results out
    struct HostReq {
        const float* q; long long nq; int k; float* D; long long* I;
        int rc = 0; std::string err; bool done = false;
        std::condition_variable cv;
    };
    static constexpr int CQ_LEADERS = 2;
    std::mutex cq_mu;
    std::deque<HostReq*> cq;
    int cq_leaders = 0;
    unsigned long long cq_batches = 0, cq_requests = 0;
    unsigned long long direct_queries = 0;  // queries answered by the direct small-batch scan (under mu_)
    unsigned long long short_batches = 0;   // batches whose scan was the short-index kernel (under mu_)
    int num_cu = 256;
    std::mutex mu_;
    // range search (ise_range.hpp): a workspace of its own, grown lazily and held by one call at a time (rg_mu,
    // taken before mu_); the WorkSlot rotation of search is never touched
    struct RangeWs {
        DevBuf<float> q;                        // [m][dp] padded queries
        DevBuf<unsigned> cnt;                   // [m][nseg] hits per segment
        DevBuf<long long> segoff;               // [m][nseg] offset of a segment within its query
        DevBuf<float> sD;                       // [m][nseg][cap] staged distances
        DevBuf<uint32_t> sI;                    // [m][nseg][cap] staged row ids
        DevBuf<long long> tot, lims;            // [m], [m + 1]
        DevBuf<unsigned> flag;                  // overflow flag
        DevBuf<float> D;                        // [total]
        DevBuf<long long> I;                    // [total]
        DevBuf<float, MEM_PINNED> q_pin;        // page-locked staging
        DevBuf<long long, MEM_PINNED> lims_pin; // [m + 1] lims, then the overflow flag
        DevBuf<float, MEM_PINNED> D_pin;
        DevBuf<long long, MEM_PINNED> I_pin;
        void release() { buf_free(q, cnt, segoff, sD, sI, tot, lims, flag, D, I, q_pin, lims_pin, D_pin, I_pin); }
    };
    RangeWs rg;
    std::mutex rg_mu;
    unsigned long long range_batches = 0, range_overflows = 0;  // under rg_mu
    // remove_ids (ise_remove.hpp): calls that removed something, rows removed, rows moved (under mu_); and the last
    // such call's slab launches as HIP events timed them, with the bytes they moved (each counted once)
    unsigned long long remove_calls = 0, remove_rows = 0, remove_moved = 0;
    float remove_last_ms = 0.f;
    unsigned long long remove_last_bytes = 0;
    // selectors (ise_sel_scan.hpp).  row_epoch: bumped by whatever removes rows (reset, remove_ids, remove_range), never
    // by add; a selector made at another epoch or ntotal is refused (under mu_).  The masked pass has a slot scheme
    // of its own, NSS slots handed out like the WorkSlots (a stream keeps its slot; another stream takes a fresh one,
    // or the least recently taken one behind an event wait), so filtered searches of several threads and streams
    // run beside unfiltered ones and beside each other
    unsigned long long row_epoch = 0;
    struct SelSlot {
        DevBuf<float> q;      // [chunk][dp] padded queries
        DevBuf<u64> part;     // [groups][blocks][16][kpass]
        DevBuf<u64> keys;     // [chunk][32] one pass's merged keys (k > 32) | [chunk] floors
        CallOrder order;      // its event is made by search_sel_enqueue
        void release() {
            buf_free(q, part, keys);
            order.destroy();
            *this = SelSlot();
        }
    };
    static constexpr int NSS = 4;
    SelSlot ss[NSS];
    unsigned ss_next = 0;
    unsigned long long sel_batches = 0, sel_passes = 0;  // under mu_
    unsigned long long sel_range_batches = 0;            // under rg_mu
    // subset scoring (ise_subset.hpp): ONE key workspace per handle (under mu_).  A call on another stream than the
    // previous subset call's waits for that call through `order`; a workspace that has to grow is replaced only after
    // the device has drained.  The host forms stage through buffers of their own, held by one call at a time (mu,
    // taken before mu_)
    struct SubsetWs {
        DevBuf<u64> keys;                 // [chunk][n2]
        DevBuf<unsigned long long> valid; // [1] device counter: candidate entries inside [0, ntotal)
        CallOrder order;
        unsigned long long batches = 0, launches = 0;
        std::mutex mu;
        DevBuf<float> q, out;             // host forms: [chunk][d] queries | [chunk][k] D or [chunk][kc] scores
        DevBuf<long long> cand, I;        // host forms: [chunk][kc] | [chunk][k]
        void release() {
            buf_free(keys, valid, q, out, cand, I);
            order.destroy();
            order = CallOrder();
        }
    };
    SubsetWs sub;
};

static inline size_t row_bytes(const ise_index* h) { return (size_t)h->dp * elem_size(h->storage); }
static inline size_t shadow_row_bytes(const ise_index* h) { return (size_t)h->dph * 2; }
static inline size_t byte_row_bytes(const ise_index* h) { return (size_t)h->dpb; }
static inline int chunk_steps(const ise_index* h) { return chunk_steps_rb(row_bytes(h)); }
static inline int qs_stride_for(const ise_index* h) { return qs_stride_units((int)(row_bytes(h) / 4)); }
// the shadow-row kernel's query row: fp16 hi halves | lo halves, dph each
static inline int qs_stride_half(const ise_index* h) { return qs_stride_units(h->dph); }
// the byte shadow-row kernel's query row: int8 hi limbs | lo limbs, dpb each
static inline int qs_stride_byte(const ise_index* h) { return qs_stride_units(h->dpb / 2); }
static inline bool uses_shift(const ise_index* h) { return h->storage == ISE_STORE_F32 && h->metric == ISE_METRIC_L2; }
// relative width of the scan's lower bound: every rounding between the stored floats and the keyed
// value, in units of u = 2^-24 times (|x-mu|^2 + |y-mu|^2) (derivation: DESIGN.md section 4.1)
static inline float exact_beta(const ise_index* h) { return exact_beta_dp(h->dp); }
#define KPASS_MAX 36 /* most keys per query one scan pass selects: k = 32 with the exact path's 4 spare candidates still is
                        ONE pass (k = 29..32 took two: 730 us instead of 355 at 1M x 512); more: floor-keyed passes */
#define XPASS_MAX 32 /* most results per query of one exact-scan pass, of the direct scan and of the large-batch paths */

// Test / rehearsal knobs that may change while the process runs: read from the environment when the library
// is first used and again whenever ise_refresh_env_knobs() is called (the tests call it after changing the
// environment) -- never inside a search, where another thread's setenv would race with getenv.
struct EnvKnobs {
    std::atomic<int> force_exact{0};    // ISE_FORCE_EXACT=1: fail every certificate (exercises the exact scan)
    std::atomic<int> no_direct{0};      // ISE_NO_DIRECT=1: one-query batches take the filtered path as well
    std::atomic<int> no_short{0};       // ISE_NO_SHORT=1: short indexes take the streaming kernel + merge launches
    std::atomic<int> short_tpb_max{0};  // ISE_SHORT_TPB_MAX: most row tiles per block the short-index kernel takes
    std::atomic<int> direct_short_max_tiles{0};  // ISE_DIRECT_SHORT_MAX_TILES: longest SHORT index (16-row tiles) whose one-query batches take the direct scan
    std::atomic<int> range_stage_cap{0};  // ISE_RANGE_STAGE_CAP: staging entries per range-search segment (tests: force the overflow pass)
    std::atomic<int> no_half{0};        // ISE_NO_HALF_FILTER=1: long float32 L2 indexes keep the float32 filter (A/B, tests)
    std::atomic<int> no_byte{0};        // ISE_NO_BYTE_FILTER=1: ... filter through the fp16 shadow, never the byte one
    std::atomic<int> fail_byte_alloc{0};  // ISE_FAIL_BYTE_ALLOC=1: the byte shadow's allocation fails as out of memory (tests)
    std::atomic<int> remove_slab_rows{0};  // ISE_REMOVE_SLAB_ROWS: destination rows per slab of a removal (tests: cross many slabs)
    std::atomic<int> scan_depth{0};     // ISE_SCAN_DEPTH: 0 = by the stream rule of search_enqueue, 1 = isolated plan, N >= 2 = depth N
    void refresh() {
        auto flag = [](const char* name) { const char* e = getenv(name); return (e && e[0] == '1') ? 1 : 0; };
        auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; };
        force_exact.store(flag("ISE_FORCE_EXACT"));
        no_direct.store(flag("ISE_NO_DIRECT"));
        no_short.store(flag("ISE_NO_SHORT"));
        short_tpb_max.store(num("ISE_SHORT_TPB_MAX"));
        direct_short_max_tiles.store(num("ISE_DIRECT_SHORT_MAX_TILES"));
        range_stage_cap.store(num("ISE_RANGE_STAGE_CAP"));
        no_half.store(flag("ISE_NO_HALF_FILTER"));
        no_byte.store(flag("ISE_NO_BYTE_FILTER"));
        fail_byte_alloc.store(flag("ISE_FAIL_BYTE_ALLOC"));
        remove_slab_rows.store(num("ISE_REMOVE_SLAB_ROWS"));
        scan_depth.store(std::max(0, num("ISE_SCAN_DEPTH")));
    }
};

// Host-API searches run on a small pool of contexts (stream + staging buffers), and hold the handle
// lock only while their kernels are enqueued: concurrent callers (Flask request threads,
// backend/engine.py:137; joblib threads, backend/descriptors.py:125) overlap their copies and
// their scans instead of queueing behind one stream.  A lease is one context for a scope's duration: taken (it blocks
// while all NHC are out) and given back on every path; stream() makes the context's stream at its first use
struct CtxLease {
    ise_index* h;
    ise_index::HostCtx* c = nullptr;
    explicit CtxLease(ise_index* h_) : h(h_) {
        std::unique_lock<std::mutex> lk(h->hc_mu);
        while (!c) {
            for (auto& x : h->hc)
                if (!x.busy) { x.busy = true; c = &x; break; }
            if (!c) h->hc_cv.wait(lk);
        }
    }
    ~CtxLease() {
        { std::lock_guard<std::mutex> lk(h->hc_mu); c->busy = false; }
        h->hc_cv.notify_one();
    }
    int stream() {
        if (!c->stream) HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        return ISE_OK;
    }
};

// The staging loop of the plain and the filtered host search, on one of the host contexts: `batch` queries at a time
// (bounds the workspace; larger calls loop) are copied in, enqueued by enqueue(c, m) under mu_, copied out, waited for
template <class Enqueue>
static int search_host_staged(ise_index* h, const float* q, long long nq, int k, long long batch, float* D, long long* I,
                              Enqueue enqueue) {
    DeviceGuard gd(h->device);
    CtxLease lease(h);
    ise_index::HostCtx* c = lease.c;
    int rc = lease.stream();
    if (!rc) rc = c->stage((size_t)std::min<long long>(nq, batch) * h->d, (size_t)std::min<long long>(nq, batch) * k);
    if (rc) return rc;
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        HIP_TRY(hipMemcpyAsync(c->q_dev.p, q + (size_t)i0 * h->d, (size_t)m * h->d * sizeof(float), hipMemcpyHostToDevice,
                               c->stream));
        {
            std::lock_guard<std::mutex> lk(h->mu_);
            rc = enqueue(c, m);
        }
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(D + (size_t)i0 * k, c->D_dev.p, (size_t)m * k * sizeof(float), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, c->I_dev.p, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return ISE_OK;
}

// ---- the interface between the units: everything a unit calls in another one.  No lock is taken by any of them
struct ise_selector;  // ise_selector.hpp
// ise_knn.hip: the knobs as last refreshed; no lock
EnvKnobs& knobs();
// ise_knn.hip: mu and the norms (and the shadows) brought up to date with the rows before a pass reads them; mu_ held
int prepare_shift_locked(ise_index* h, hipStream_t st);
// ise_knn.hip: the arguments of a search, host or device form; no lock
int check_search_args(const ise_index* h, const void* q, long long nq, int k);
// ise_knn.hip: the streaming kernel's query staging for this index, from its one-tile plan (make_plan); mu_ held
int range_staging(const ise_index* h, int qs_stride, int* tpr, int* vec_q);
// ise_flat_sel.hip: a selector is good for the handle it was made from while ntotal and the row epoch stand; mu_ held
int selector_check_locked(const ise_index* h, const ise_selector* sel);
