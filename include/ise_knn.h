/*
 * include/ise_knn.h -- C ABI of the MI355X (gfx950) brute-force kNN library.
 *
 * This is the drop-in boundary for the one hot path of
 * ManuelZ/image-search-engine: the arithmetic the reference delegates to the
 * Faiss IndexFlat objects.  The reference has no FFI of its own (pure Python
 * over the Faiss SWIG module), so every entry point names the
 * reference call site whose native work it replaces.  Plain pointers and
 * sizes only; no C++ or torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (ISE_E_*); nothing
 *     throws across the ABI; ise_last_error() returns a thread-local message.
 *   - the caller owns every buffer it passes; the index owns a private copy of
 *     added rows (reference contract of index.add, backend/utils.py:327).
 *   - "device" pointers are HIP device pointers on the index's device;
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     *_device entry points only enqueue work; *_host entry points block.
 *   - distances follow Faiss: METRIC_L2 = SQUARED L2, ascending;
 *     METRIC_INNER_PRODUCT = inner product, descending; ties by ascending id;
 *     a row enters a result only if strictly better than +-FLT_MAX, so
 *     unfilled slots come back as id -1 / distance +-FLT_MAX.
 *   - ids are row numbers in insertion order (+ id_base); a (sharded) index
 *     holds fewer than 2^32 rows.
 *   - concurrent *_host calls on one handle are safe and overlap on the GPU (each runs on one of
 *     a few internal contexts; the handle is locked only while kernels are enqueued);
 *     *_device calls on one handle may target different streams (the handle
 *     rotates through a few workspaces and orders their reuse with events, so
 *     independent batches on different streams overlap on the GPU); results of
 *     a call are ordered after it on its own stream only.
 */
#ifndef ISE_KNN_H
#define ISE_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISE_METRIC_INNER_PRODUCT 0 /* faiss.METRIC_INNER_PRODUCT */
#define ISE_METRIC_L2 1            /* faiss.METRIC_L2 */

#define ISE_STORE_F32 0  /* index rows kept as float32: exact results */
#define ISE_STORE_BF16 1 /* index rows (and queries) rounded to bf16, fp32 accumulation: approximate,
                            half the HBM traffic (BASELINE config 5: cosine over normalised rows) */

#define ISE_OK 0
#define ISE_E_INVALID -1  /* bad argument (shape, k, NULL) */
#define ISE_E_HIP -2      /* HIP runtime error (message has the hipError string) */
#define ISE_E_NOMEM -3    /* host or device allocation failed */
#define ISE_E_NODEVICE -4 /* no usable gfx950 device */

#define ISE_MAX_K 2048 /* largest k accepted by the search entry points */
#define ISE_SQ_MAX_D 2048 /* longest row of a scalar-quantised index (ise_sq_*): what its scan's LDS holds of 8 queries */
#define ISE_PQ_MAX_M 64 /* most sub-quantisers of a product-quantised index (ise_pq_*): what its scan's LDS holds */
#define ISE_LINEAR_MAX_D 4096 /* largest d_in and d_out of a linear transform (ise_linear_*): 16 segments of 256, one
                                 wave each in the few-row launch shape */
#define ISE_LINEAR_FEW_ROWS 64 /* ise_linear_apply_*: n <= this takes the few-row launch shape, more the tiled one */

typedef struct ise_index ise_index_t;

/* library / device ------------------------------------------------------- */
int ise_version(void);
const char* ise_last_error(void);
int ise_device_count(int* count);
/* name of device `device` into buf (NUL-terminated), e.g. "gfx950:sramecc+:xnack-" */
int ise_device_arch(int device, char* buf, int buflen);

/* index lifetime: replaces faiss.IndexFlatL2(d) / faiss.IndexFlatIP(d)
 * (backend/utils.py:302,306; backend/siamese/siamese_pt/create_index.py:40). */
int ise_index_create(ise_index_t** out, int d, int metric, int device);
/* same with an explicit row storage type (ISE_STORE_*); not a Faiss IndexFlat feature */
int ise_index_create_ex(ise_index_t** out, int d, int metric, int device, int storage);
int ise_index_destroy(ise_index_t* h);
int ise_index_reset(ise_index_t* h); /* drop all rows, keep d/metric */
int ise_index_info(const ise_index_t* h, int* d, int* metric, int64_t* ntotal, int* device);

/* index.add(x) (backend/utils.py:327): append n rows of d float32, copied.
 * Also computes the per-row squared norms the L2 search uses. */
int ise_index_add_host(ise_index_t* h, const float* x, int64_t n);
int ise_index_add_device(ise_index_t* h, const float* x_dev, int64_t n, void* stream);

/* Float32 L2 indexes are searched EXACTLY: the streaming scan evaluates the expanded form
 * |x-mu|^2 + |y-mu|^2 - 2 (x-mu).(y-mu) around a shift vector mu (the column mean of the rows,
 * refreshed at the first search after the index has grown by a quarter) only as a filter keyed by
 * a rigorous lower bound; the candidates are re-evaluated as sum (x_i - y_i)^2 -- what Faiss's
 * IndexFlatL2 computes for the reference's one-query searches (backend/engine.py:55) -- and a
 * query the filter cannot certify is recomputed by a direct-difference scan of the whole index
 * (csrc/ise_exact.hpp).  Ids and distances therefore do not depend on mu; it only decides how
 * often the slower path runs.  set_shift pins mu (no automatic refresh) -- e.g. to give the shards
 * of one logical index the same one; get_shift returns the current one.  mu: d float32 on the
 * host.  No-ops for inner-product and bf16 indexes. */
int ise_index_set_shift(ise_index_t* h, const float* mu_host);
int ise_index_get_shift(ise_index_t* h, float* mu_host);

/* Counters of the exact float32 L2 path since the index was created:
 *   out4[0] queries re-ranked, out4[1] queries whose certificate failed and that were recomputed by
 *   the exact scan, out4[2] refreshes of the shift vector, out4[3] query chunks (<= 1024 queries) that
 *   took the large-batch GEMM-shaped path (nq >= 64).  Blocks. */
int ise_index_stats(ise_index_t* h, uint64_t* out4);
/* The large-batch path alone: out2[0] = out4[3] above; out2[1] = queries of the flavours without a re-rank (float32
 * inner product, bf16 rows) whose candidates the pass left incomplete (a candidate buffer overflowed), so that the
 * streaming passes queued behind the chunk rewrote it: same results, at the streaming passes' cost.  A float32 L2
 * query in that state goes to the exact scan and counts in out4[1].  Blocks. */
int ise_index_gemm_stats(ise_index_t* h, uint64_t* out2);

/* Short indexes (a batch of <= 16 queries, k + spare candidates <= 32, at most 32 row tiles of 16 rows per
 * block of the grid: <= 262k rows on an MI355X) are scanned by short_scan_kernel (csrc/ise_short_scan.hpp: the
 * rows' scores are dumped to LDS and selected once per block, no boot and no thresholds in the stream): the
 * reference's own regime, ~1 k images and one query per request (backend/utils.py:309-310,
 * backend/engine.py:50-55).  out1[0] = batches scanned that way ($ISE_NO_SHORT=1: none; same bits). */
int ise_index_short_stats(ise_index_t* h, uint64_t* out1);

/* Long float32 L2 indexes (more than 262144 rows, d <= 1024) keep an fp16 SHADOW of their centred rows,
 * u~ = 2^-s_r fp16(2^s_r (y - mu)) (+2 bytes per element), and a BYTE shadow beside it, q = rint((y - mu) / c_r)
 * in [-127, 127] (+1 byte per element).  The streaming scan's filter reads the byte shadow for batches with k <= 10
 * and nq <= 16, and the fp16 one for the other batches with k <= 12, instead of the float32 rows; the re-rank, the certificate and the exact scan
 * still read the float32 rows, so results do not change ($ISE_NO_BYTE_FILTER=1 keeps the fp16 shadow for k <= 10,
 * $ISE_NO_HALF_FILTER=1 the float32 filter for every batch).  ise_index_half_stats: out1[0] = batches whose filter
 * read shadow rows of either kind.  ise_index_byte_stats: out2[0] = those of them that read the byte shadow, out2[1] = 1
 * when the index's byte route is open (the byte shadow exists and its build-time statistics admit it).
 * ise_index_shadow_row: out3 = (|u~|^2, e_r, s_r) of fp16 shadow row i, e_r >= |(y - mu) - u~|.
 * ise_index_byte_row: out2 = (c_r, e_r) of byte shadow row i, e_r >= |(y - mu) - c_r q|.
 * ise_index_byte_row_codes (debug): the codes q of byte shadow row i in column order, out_dpb[0 .. dpb), dpb = d rounded
 * up to whole 64-column k-steps, and to a multiple of four of them beyond four (pad columns read zero); the rows are stored tile-blocked and this read goes through the same
 * address map as the scan.  i may also name an allocated row at or beyond n (below the capacity): it reads zero.  All three
 * ISE_E_INVALID when the index has no such shadow. */
int ise_index_half_stats(ise_index_t* h, uint64_t* out1);
int ise_index_byte_stats(ise_index_t* h, uint64_t* out2);
/* The byte-shadow scan has two plans.  A batch enqueued on another stream than the index's previous search has
 * other batches in flight beside it and is scanned by half as many blocks of twice the rows (depth 2), so that two
 * consecutive batches are resident together and a block's fixed phases are paid once per twice the rows; a caller
 * that stays on one stream, and the first search, keep the isolated plan (depth 1), which has the lower latency.
 * Same bits either way.  $ISE_SCAN_DEPTH (read by ise_refresh_env_knobs): 0 / unset = that rule, 1 = always the
 * isolated plan, N >= 2 = depth N wherever the plan allows it.  out2[0] = byte-shadow batches scanned at depth 1,
 * out2[1] = at depth > 1 (their sum is ise_index_byte_stats' out2[0]). */
int ise_index_depth_stats(ise_index_t* h, uint64_t* out2);
int ise_index_shadow_row(ise_index_t* h, int64_t i, float* out3);
int ise_index_byte_row(ise_index_t* h, int64_t i, float* out2);
int ise_index_byte_row_codes(ise_index_t* h, int64_t i, int8_t* out_dpb);

/* Tests only (nothing on the search path calls it): one float32 query (device pointer, d floats) through the query
 * staging of a shadow filter (csrc/ise_stage.hpp, the device functions the scan kernel runs) in a one-block kernel.
 * route: 0 = fp16 shadow, 1 = byte shadow; ISE_E_INVALID when the index has no such shadow.  limbs (host,
 * limbs_bytes >= 2 * P * element size): the hi limbs of the padded row (P elements: int8, or fp16 bits), then the
 * lo limbs.  out2 = (|v|^2, e_q) as the kernel keeps them, info3 = (sh, 1 if the vector path ran, P). */
int ise_index_stage_query_debug(ise_index_t* h, const void* q_dev, int route, void* limbs, int64_t limbs_bytes,
                                float* out2, int32_t* info3);

/* Test / rehearsal knobs ($ISE_FORCE_EXACT, $ISE_NO_DIRECT, $ISE_NO_SHORT, $ISE_SHORT_TPB_MAX,
 * $ISE_DIRECT_SHORT_MAX_TILES, $ISE_RANGE_STAGE_CAP, $ISE_NO_HALF_FILTER, $ISE_NO_BYTE_FILTER, $ISE_FAIL_BYTE_ALLOC, $ISE_REMOVE_SLAB_ROWS) are read from the environment when the library is first used and again when
 * this is called -- never inside a search. */
int ise_refresh_env_knobs(void);

/* Size every internal workspace for batches of nq queries and k results now (device allocations,
 * fills and the shift refresh otherwise happen inside the first search of that shape), so that a
 * serving loop is allocation-free from its first batch on.  Blocks. */
int ise_index_reserve_workspaces(ise_index_t* h, int64_t nq, int k);

/* copy rows [i0, i0+n) back to host as n x d float32 (used by write_index,
 * backend/indexer.py:59). */
int ise_index_reconstruct_host(ise_index_t* h, int64_t i0, int64_t n, float* out);

/* index.search(x, k) -> (D, I) (backend/engine.py:55,
 * backend/siamese/test_index.py:54, backend/kmeans_faiss.py:49).
 * q: nq x d float32; D: nq x k float32; I: nq x k int64. */
int ise_index_search_host(ise_index_t* h, const float* q, int64_t nq, int k,
                          float* D, int64_t* I);
/* Thread-safe, and concurrent small calls SHARE a pass over the index: calls with nq <= 16 and
 * k <= 32 that arrive while others are waiting or running are run together as one batch of up to
 * $ISE_HOST_COMBINE_MAX (default 64; 0 = never) queries of the same k, each caller getting exactly
 * the rows it would have got alone.  This is the reference's serving pattern -- one query per HTTP
 * request on a threaded Flask (backend/engine.py:55,137) -- where a scan costs the same for 1 or 16
 * queries.  ise_index_host_stats: out3[0] = batches run that way, out3[1] = calls they served,
 * out3[2] = queries (of any entry point) answered by the direct small-batch scan: float32 L2 batches of
 * up to 4 queries with k <= 32 run Faiss's nq < 20 algorithm as it stands -- one direct-difference scan with
 * a k-best list, no filter in front ($ISE_NO_DIRECT=1 sends them through the filtered path; same bits). */
int ise_index_host_stats(ise_index_t* h, uint64_t* out3);

/* index.range_search(x, radius) -> (lims, D, I) (Faiss IndexFlat; not called by the reference, whose DHASH
 * method returns every image with the query's hash, backend/engine.py:82-91: this is that request on the
 * descriptors).  q: nq x d float32 on the host.  Every row with D < radius (L2) or D > radius (inner
 * product) -- plain float comparisons: a NaN distance or radius keeps nothing, no +-FLT_MAX gate -- with D
 * the bits ise_index_search_host reports for the same (query, row) pair on the streaming path.  Query i's
 * results are [lims[i], lims[i+1]) in ascending id order; lims has nq + 1 entries, lims[0] = 0; no cap on
 * the count.  One pass over the index per 16 queries (csrc/ise_range.hpp), a second one only when a wave's
 * staging segment overflowed; one host synchronisation per 256 queries.  Thread-safe (range calls on one
 * handle run one at a time; searches run beside them).  *out is NULL on error. */
typedef struct ise_range_result ise_range_result_t;
int ise_index_range_search_host(ise_index_t* h, const float* q, int64_t nq, float radius, ise_range_result_t** out);
/* pointers valid until ise_range_result_destroy; any output pointer may be NULL */
int ise_range_result_get(const ise_range_result_t* r, int64_t* nq, const int64_t** lims, const float** D,
                         const int64_t** I);
int ise_range_result_destroy(ise_range_result_t* r); /* NULL is a no-op */
/* out2[0] = range batches (<= 256 queries of a call against a non-empty index), out2[1] = batches that needed
 * the overflow pass ($ISE_RANGE_STAGE_CAP: staging entries per segment, default 16; tests set it small) */
int ise_index_range_stats(ise_index_t* h, uint64_t* out2);

/* index.remove_ids(faiss.IDSelectorBatch(ids)) (Faiss IndexFlatCodes::remove_ids; the reference never removes rows:
 * it rebuilds its index file with backend/indexer.py).  Every existing row named in ids (host, n_ids int64, in any
 * order; duplicates and values outside [0, ntotal) are ignored) is removed once; the other rows keep their order and
 * are renumbered densely, so ids handed out earlier shift (IndexIDMap in faiss_compat.py keeps external ids).  The
 * rows, their norms and, where the index has them, both shadows and their metadata are compacted IN PLACE on the
 * device (csrc/ise_remove.hpp): capacity is kept, the extra memory is one bounce buffer of at most 256 MiB
 * ($ISE_REMOVE_SLAB_ROWS: destination rows per slab; tests set it small), nothing is re-uploaded or rebuilt.
 * The shift vector stays (results never depend on it); an unpinned index that has shrunk below three quarters of
 * the rows it was taken from refreshes it at the next search, and an index at or below 262144 rows drops its shadows.
 * *n_removed (may be NULL) = rows removed.  Blocks; searches and range searches of other threads run entirely
 * before or entirely after it.  A call that removes nothing returns at once. */
int ise_index_remove_ids_host(ise_index_t* h, const int64_t* ids, int64_t n_ids, int64_t* n_removed);
/* index.remove_ids(faiss.IDSelectorRange(i0, i1)): rows [i0, i1), clipped to [0, ntotal); as above (the
 * reference never removes rows). */
int ise_index_remove_range(ise_index_t* h, int64_t i0, int64_t i1, int64_t* n_removed);
/* Counters of the two calls above since the index was created (Faiss keeps none; the reference never removes
 * rows): out3[0] = calls that removed something, out3[1] = rows removed, out3[2] = rows moved to a new position. */
int ise_index_remove_stats(ise_index_t* h, uint64_t* out3);
/* measurement hook for scripts/remove_probe.py (Faiss has no counterpart; the reference never removes rows): the
 * slab launches of the last call that removed something, as HIP events on the index's stream timed them
 * (milliseconds), and the bytes they moved, each counted once (they are read twice and written twice). */
int ise_index_remove_last_timing(ise_index_t* h, float* ms, uint64_t* bytes);
int ise_index_search_device(ise_index_t* h, const float* q_dev, int64_t nq, int k,
                            float* D_dev, int64_t* I_dev, void* stream);

/* Selector-filtered search: index.search(x, k, params=faiss.SearchParameters(sel=sel)) and the same for
 * range_search (Faiss IndexFlat with an IDSelector; the reference never filters: "similar images, but not the one I
 * uploaded" or "only within this album" it would answer by oversampling and dropping on the host).
 *
 * ise_selector_t is a selector that lives on the index's device, so a serving loop that filters by the same category
 * pays for it once: a bitmap of uint32 words, one bit per row (bit r & 31 of word r >> 5; a 16-row tile is one
 * half-word), zero padded past ntotal like the pad rows of the index; with it the row WINDOW [r0, r1) from the first
 * to the last selected row, the selected count and the number of non-empty 16-row tiles, all taken on the device at
 * creation.  The constructors block:
 *   ise_selector_create_range   rows [i0, i1) clipped to [0, ntotal); nothing is uploaded, the bitmap is filled on
 *                               the device
 *   ise_selector_create_ids     ids in any order; duplicates and ids outside [0, ntotal) are ignored, as in
 *                               ise_index_remove_ids_host; invert != 0 selects every OTHER row.  The ids travel, not a
 *                               bitmap: a device fill, then a scatter kernel
 *   ise_selector_create_bitmap  the general form: n_words must be ceil(ntotal / 32); bits at or beyond ntotal are
 *                               cleared
 *   ise_selector_info           out5 = ntotal, selected count, r0, r1, non-empty tiles
 *   ise_selector_destroy        NULL is a no-op
 * A selector is valid only for the handle it was made from, and only while that handle's ntotal and ROW EPOCH are
 * unchanged: the epoch is a per-handle counter that ise_index_reset, ise_index_remove_ids_host and
 * ise_index_remove_range bump when they remove something (an add changes ntotal instead).  The filtered entry points
 * return ISE_E_INVALID otherwise, with a message that says which of the two changed; they never read a stale bitmap.
 *
 * ise_index_search_sel_device / _host: the k best rows among the selected ones, D and I as ise_index_search_* report
 * them (the same bits for the same (query, row) pair on the streaming path; ties by ascending id; unfilled slots
 * -1 / +-FLT_MAX).  One masked pass per 16 queries over the tiles of the window, tiles without a selected row are not
 * read (csrc/ise_sel_scan.hpp); float32 L2 results are exact by construction (every row whose lower bound does not
 * prove it out is re-evaluated by direct difference), whatever the shift vector.  k > 32 repeats the pass per 32
 * results.  An empty selection costs no pass.  The device form only enqueues; the host form blocks, is thread-safe
 * and is never combined with other callers' requests.  sel == NULL, a foreign or stale selector, k out of range and
 * NULL buffers return ISE_E_INVALID.
 * ise_index_range_search_sel_host: ise_index_range_search_host restricted to the window and the mask.
 * ise_index_sel_stats: out3[0] = filtered search batches, out3[1] = masked passes launched, out3[2] = filtered range
 * batches. */
typedef struct ise_selector ise_selector_t;
int ise_selector_create_range(ise_index_t* h, int64_t i0, int64_t i1, ise_selector_t** out);
int ise_selector_create_ids(ise_index_t* h, const int64_t* ids_host, int64_t n_ids, int invert, ise_selector_t** out);
int ise_selector_create_bitmap(ise_index_t* h, const uint32_t* words_host, int64_t n_words, ise_selector_t** out);
int ise_selector_info(const ise_selector_t* sel, int64_t* out5);
int ise_selector_destroy(ise_selector_t* sel);
int ise_index_search_sel_device(ise_index_t* h, const float* q_dev, int64_t nq, int k, const ise_selector_t* sel,
                                float* D_dev, int64_t* I_dev, void* stream);
int ise_index_search_sel_host(ise_index_t* h, const float* q, int64_t nq, int k, const ise_selector_t* sel, float* D,
                              int64_t* I);
int ise_index_range_search_sel_host(ise_index_t* h, const float* q, int64_t nq, float radius, const ise_selector_t* sel,
                                    ise_range_result_t** out);
int ise_index_sel_stats(ise_index_t* h, uint64_t* out3);

/* Subset scoring on the flat float32 index (csrc/ise_subset.hpp): the exact scores of a PER-QUERY LIST of row ids and
 * the k best of them -- what faiss.IndexRefineFlat does with the labels of its base index, and Faiss's
 * compute_distance_subset (faiss_compat.IndexRefineFlat; the reference never refines: its "cell-probe" index,
 * backend/utils.py:311-325, returns the product quantiser's order as it is).  All the conventions at the top of this
 * header hold (0 / ISE_E_* returns, *_host blocks, *_device only enqueues on the given stream; it waits on the host only
 * where the key workspace has to be replaced by a larger one).  cand: nq x kc int64 row ids.
 *   candidates       an entry that is -1 or otherwise outside [0, ntotal) is ignored; an id named twice in a row of
 *                    cand delivers its row once
 *   search_subset    the exact k best among the query's candidate rows: D has the bits ise_index_search_* reports for
 *                    the same (query, row) pair -- float32 L2: the direct-difference value of exact_l2_rows
 *                    (csrc/ise_exact.hpp); inner product: the scan's two-chain MFMA dot product (range_tile_dots,
 *                    csrc/ise_range.hpp), the k-steps in the same order, lane (c, g) reading row cand[c] where the scan
 *                    reads row 16 tile + c.  L2 ascending, inner product descending, ties by ascending id; a score
 *                    enters only if it is strictly better than +-FLT_MAX (NaN never); unfilled slots are id -1 with
 *                    +-FLT_MAX.  k in 1 .. ISE_MAX_K and may exceed kc
 *   distance_subset  dist[q][j] = the same value for candidate j, in candidate order: the raw value, so a NaN stays a
 *                    NaN; for an ignored entry +FLT_MAX (L2) / -FLT_MAX (inner product).  Faiss's
 *                    compute_distance_subset, with invalid entries given a defined value
 *   limits           kc in 1 .. ISE_MAX_K; anything else, NULL buffers and a handle with bf16 storage are ISE_E_INVALID
 *   empty cases      nq = 0 returns at once; an empty index fills the padding without a score launch
 *   work             per 4096 queries one score launch spread over the device by candidate (a wave per 4 rows for L2,
 *                    per tile of 16 gathered rows for inner product; keys ord(score) << 32 | id into a
 *                    [nq][pow2(kc)] workspace) and one select launch (a block per query sorts the keys, drops adjacent
 *                    duplicates, writes k); distance_subset makes the score launch only.  One key workspace per handle:
 *                    calls on different streams are ordered one behind the other on the device.  The host forms work
 *                    through 4096 queries at a time
 *   stats            out3[0] = batches (device calls with nq > 0; the host forms: one per 4096 queries), out3[1] =
 *                    score launches, out3[2] = candidate entries inside [0, ntotal) that were scored (counted on the
 *                    device; the call waits for the device) */
int ise_index_search_subset_device(ise_index_t* h, const float* q_dev, int64_t nq, int k, const int64_t* cand_dev, int kc,
                                   float* D_dev, int64_t* I_dev, void* stream);
int ise_index_search_subset_host(ise_index_t* h, const float* q, int64_t nq, int k, const int64_t* cand, int kc, float* D,
                                 int64_t* I);
int ise_index_distance_subset_device(ise_index_t* h, const float* q_dev, int64_t nq, const int64_t* cand_dev, int kc,
                                     float* dist_dev, void* stream);
int ise_index_distance_subset_host(ise_index_t* h, const float* q, int64_t nq, const int64_t* cand, int kc, float* dist);
int ise_index_subset_stats(ise_index_t* h, uint64_t* out3);

/* Binary flat index: faiss.IndexBinaryFlat(d_bits) -- exact brute-force kNN and range search over bit codes under
 * the HAMMING distance (csrc/ise_binary_scan.hpp).  The reference's DHASH method keeps 64-bit difference hashes
 * (backend/indexer.py:39-49) and answers a query with a dict lookup that finds bit-identical hashes only
 * (backend/engine.py:82-91); its hamming(a, b) helper (backend/utils.py:84-88) is never called.  "Every image within
 * r bits of this hash" is ise_binary_index_range_search_host, "the k nearest hashes" ise_binary_index_search_*.
 *
 * A code is d_bits / 8 bytes (d_bits a positive multiple of 8, at most ISE_BINARY_MAX_BITS; anything else is
 * ISE_E_INVALID); rows are copied on add and numbered in insertion order; an index holds fewer than 2^32 rows.  All
 * the conventions at the top of this header hold (0 / ISE_E_* returns, ise_last_error, caller-owned buffers, *_host
 * blocks, *_device only enqueues on the given stream).  Calls on one handle run one at a time; *_device calls on
 * different streams are ordered one behind the other on the device (one set of workspaces per handle).
 *   distance      the Hamming distance (number of differing bits), int32, ascending.  Every score is an integer, so
 *                 results do not depend on the kernel path taken
 *   tie order     ties go by ascending row id, ALWAYS.  This is the project's convention (see the top of this header):
 *                 Faiss's heap promises no order among equal distances
 *   unfilled      k > ntotal, or an empty index: id -1 and distance INT32_MAX (Faiss's CMax<int32_t> neutral, restated
 *                 from memory and unpinned like the rest of the oracle)
 *   k             1 .. ISE_MAX_K; one pass over the codes per 16 queries and per 32 results (k = 70: three passes, the
 *                 later ones admit only keys behind the last result of the one before).  nq = 0 is legal and returns at
 *                 once; an empty index costs no pass
 *   range search  every row with dist < radius (strict, as Faiss's hamming_range_search), per query in ascending id
 *                 order; lims has nq + 1 entries, lims[0] = 0; no cap on the count; radius <= 0 returns nothing without
 *                 a pass.  D is int32, the numbers search reports (Faiss's Python wrapper may hand them out as
 *                 float32).  A count pass and a fill pass over the codes per 16 queries, one host synchronisation per
 *                 256 queries
 *   stats         out3[0] = search batches (calls with nq > 0), out3[1] = scan passes launched, out3[2] = range batches
 *                 (<= 256 queries of a call with radius > 0 against a non-empty index) */
#define ISE_BINARY_MAX_BITS 8192
typedef struct ise_binary_index ise_binary_index_t;
typedef struct ise_binary_range_result ise_binary_range_result_t;
int ise_binary_index_create(ise_binary_index_t** out, int d_bits, int device);
int ise_binary_index_destroy(ise_binary_index_t* h); /* NULL is a no-op */
int ise_binary_index_reset(ise_binary_index_t* h);   /* drop all rows, keep d_bits and the capacity */
int ise_binary_index_info(const ise_binary_index_t* h, int* d_bits, int64_t* ntotal, int* device);
/* append n codes of d_bits / 8 bytes each, copied */
int ise_binary_index_add_host(ise_binary_index_t* h, const uint8_t* codes, int64_t n);
int ise_binary_index_add_device(ise_binary_index_t* h, const uint8_t* codes_dev, int64_t n, void* stream);
/* rows [i0, i0 + n) back to the host as n x d_bits / 8 bytes */
int ise_binary_index_reconstruct_host(ise_binary_index_t* h, int64_t i0, int64_t n, uint8_t* out);
/* q: nq x d_bits / 8 bytes; D: nq x k int32; I: nq x k int64 */
int ise_binary_index_search_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int k, int32_t* D, int64_t* I);
int ise_binary_index_search_device(ise_binary_index_t* h, const uint8_t* q_dev, int64_t nq, int k, int32_t* D_dev,
                                   int64_t* I_dev, void* stream);
/* *out is NULL on error */
int ise_binary_index_range_search_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int32_t radius,
                                       ise_binary_range_result_t** out);
/* pointers valid until ise_binary_range_result_destroy; any output pointer may be NULL */
int ise_binary_range_result_get(const ise_binary_range_result_t* r, int64_t* nq, const int64_t** lims, const int32_t** D,
                                const int64_t** I);
int ise_binary_range_result_destroy(ise_binary_range_result_t* r); /* NULL is a no-op */
int ise_binary_index_stats(ise_binary_index_t* h, uint64_t* out3);

/* remove_ids, selectors and selector-filtered search on the binary index (Faiss: IndexBinaryFlat::remove_ids,
 * SearchParameters(sel=...), IndexBinaryIDMap on top of them in faiss_compat.py).  The semantics are those of the
 * float index, documented at ise_index_remove_ids_host and ise_selector_* above:
 *   removal       duplicate, negative and out-of-range ids are ignored; the rows that stay keep their order and are
 *                 renumbered densely, in place on the device (the capacity is kept; the rows behind the new ntotal are
 *                 not zeroed: every kernel masks them by row number).  A call that removes nothing returns at once and
 *                 counts nothing.  A removal blocks, and other calls on the handle run entirely before or entirely after
 *                 it.  remove_stats: out3[0] = calls that removed something, out3[1] = rows removed, out3[2] = rows that
 *                 moved to a new position (n_new - first removed row, summed)
 *   selectors     a device bitmap over the rows of ONE binary index: bit r & 31 of uint32 word r >> 5, bits at or beyond
 *                 ntotal cleared at creation, the allocation padded to an even word count so that the mask of a 64-row
 *                 tile is one aligned 8-byte word.  create_range: rows [i0, i1) clipped to [0, ntotal); create_ids: the
 *                 ids (host pointer, any order, duplicates and out-of-range values ignored), or with invert != 0 every
 *                 OTHER row; create_bitmap: exactly ceil(ntotal / 32) words.  info: out5 = ntotal, selected rows, first
 *                 selected row, last selected row + 1 (0, 0 for an empty selection), non-empty 64-row tiles
 *   validity      a selector is good only for the handle it was made from and only while that handle's ntotal and ROW
 *                 EPOCH stand: add changes ntotal; reset (of a non-empty index) and every removal that removes something
 *                 bump the epoch, so remove + add back to the old ntotal is caught too.  Every filtered entry point
 *                 checks this first -- also for nq == 0 or an empty index -- and returns ISE_E_INVALID with a message
 *                 naming what changed; a stale bitmap is never read
 *   search        the k best rows AMONG THE SELECTED ONES: int32 distance ascending, ties by ascending id, unfilled slots
 *                 INT32_MAX / -1 (a selection smaller than k); k up to ISE_MAX_K.  One masked pass per 16 queries and per
 *                 32 results over the 64-row tiles from the first to the last selected row; a tile without a selected row
 *                 is not loaded.  An empty selection or an empty index costs a fill and no pass
 *   range search  every selected row with dist < radius, per query in ascending id order; radius <= 0 and an empty
 *                 selection return nothing without a pass
 *   stats         filtered calls count here only (ise_binary_index_stats keeps its meanings): out3[0] = filtered search
 *                 batches, out3[1] = masked passes launched, out3[2] = filtered range batches */
typedef struct ise_binary_selector ise_binary_selector_t;
int ise_binary_index_remove_ids_host(ise_binary_index_t* h, const int64_t* ids, int64_t n_ids, int64_t* n_removed);
int ise_binary_index_remove_range(ise_binary_index_t* h, int64_t i0, int64_t i1, int64_t* n_removed);
int ise_binary_index_remove_stats(ise_binary_index_t* h, uint64_t* out3);
int ise_binary_selector_create_range(ise_binary_index_t* h, int64_t i0, int64_t i1, ise_binary_selector_t** out);
int ise_binary_selector_create_ids(ise_binary_index_t* h, const int64_t* ids_host, int64_t n_ids, int invert,
                                   ise_binary_selector_t** out);
int ise_binary_selector_create_bitmap(ise_binary_index_t* h, const uint32_t* words_host, int64_t n_words,
                                      ise_binary_selector_t** out);
int ise_binary_selector_info(const ise_binary_selector_t* sel, int64_t* out5);
int ise_binary_selector_destroy(ise_binary_selector_t* sel); /* NULL is a no-op */
int ise_binary_index_search_sel_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int k,
                                     const ise_binary_selector_t* sel, int32_t* D, int64_t* I);
int ise_binary_index_search_sel_device(ise_binary_index_t* h, const uint8_t* q_dev, int64_t nq, int k,
                                       const ise_binary_selector_t* sel, int32_t* D_dev, int64_t* I_dev, void* stream);
int ise_binary_index_range_search_sel_host(ise_binary_index_t* h, const uint8_t* q, int64_t nq, int32_t radius,
                                           const ise_binary_selector_t* sel, ise_binary_range_result_t** out);
int ise_binary_index_sel_stats(ise_binary_index_t* h, uint64_t* out3);

/* Inverted lists: faiss.IndexIVFFlat's storage and its search_preassigned (csrc/ise_ivf.hpp; the third, "cell-probe"
 * branch of the reference's create_search_index, backend/utils.py:311-325, without its product quantiser).  An
 * ise_ivf_t holds nlist lists of float32 rows of dimension d on one device and NO centroids: the coarse quantiser is
 * the caller's (faiss_compat.IndexIVFFlat keeps an ordinary flat index for it).  add takes a list number per row,
 * search a table of probed lists per query.  All the conventions at the top of this header hold (0 / ISE_E_* returns,
 * ise_last_error, caller-owned buffers, *_host blocks, *_device only enqueues on the given stream).  Calls on one
 * handle run one at a time; *_device searches on different streams are ordered one behind the other on the device (one
 * set of workspaces per handle).  ise_ivf_search_device waits on the host in two cases only: rows are pending (the
 * rebuild, see add), or a workspace has to be replaced by a larger one (the first call, a larger nq or k than before),
 * which waits for the passes that still use the old one.
 *   create        d <= 0, nlist <= 0, a metric other than the two and a NULL out are ISE_E_INVALID before the device is
 *                 touched; float32 storage only
 *   ids           a row's id is its insertion number (0, 1, 2, ... across all add calls, fewer than 2^32 rows); inside a
 *                 list the rows are in ascending id order whatever the number and size of the add calls
 *   add           list_no: one entry per row in [0, nlist).  An entry outside makes the call ISE_E_INVALID and NOTHING of
 *                 that call is added.  Both forms block (the device form reads the list numbers back to check them).
 *                 The rows wait in insertion order in a pending buffer; the first search or ise_ivf_list_host after an
 *                 add rebuilds the lists (one rebuild moves the whole index, and that call blocks: DESIGN.md 4.12)
 *   lists         list_sizes_host: rows per list, pending ones included.  list_host: the ids (int64) and / or the rows
 *                 (size x d floats, bit-equal to what was added) of one list in list order; either pointer may be NULL
 *   search        probes: nq x nprobe int64 list numbers (nprobe >= 1); an entry that is -1 or otherwise outside
 *                 [0, nlist) is ignored, a list named twice in a row delivers its rows once.  The result is the exact k
 *                 best among the rows of the query's probed lists: D has the bits ise_index_search_* reports for the
 *                 same (query, row) pair (float32 L2: the direct-difference value; inner product: the scan's dot
 *                 product), ties go by ascending id, unfilled slots are id -1 with +-FLT_MAX (fewer than k rows in the
 *                 probed lists, a NaN query).  k in 1 .. ISE_MAX_K: one pass per 16 queries and per 32 results, which
 *                 loads only the 16-row tiles of lists that one of the 16 queries probes (one launch makes the passes
 *                 of up to 64 queries).  k outside the range, nprobe
 *                 < 1 and NULL buffers are ISE_E_INVALID; nq = 0 returns at once; an empty index fills the padding
 *                 without a pass
 *   stats         out3[0] = search batches (calls with nq > 0), out3[1] = scan launches (per 64 queries and 32 results), out3[2] = 16-row tiles
 *                 of list rows the passes loaded (counted on the device; the call waits for the device) */
typedef struct ise_ivf ise_ivf_t;
int ise_ivf_create(ise_ivf_t** out, int d, int metric, int nlist, int device);
int ise_ivf_destroy(ise_ivf_t* h); /* NULL is a no-op */
int ise_ivf_reset(ise_ivf_t* h);   /* drop all rows, keep d / metric / nlist */
int ise_ivf_info(const ise_ivf_t* h, int* d, int* metric, int* nlist, int64_t* ntotal, int* device);
/* append n rows of d floats with their list numbers, copied */
int ise_ivf_add_host(ise_ivf_t* h, const float* x, const int64_t* list_no, int64_t n);
int ise_ivf_add_device(ise_ivf_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream);
int ise_ivf_list_sizes_host(ise_ivf_t* h, int64_t* sizes /* nlist */);
int ise_ivf_list_host(ise_ivf_t* h, int list, int64_t* ids, float* rows); /* either may be NULL */
/* q: nq x d; probes: nq x nprobe; D: nq x k float32; I: nq x k int64 */
int ise_ivf_search_device(ise_ivf_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                          float* D_dev, int64_t* I_dev, void* stream);
int ise_ivf_search_host(ise_ivf_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                        int64_t* I);
int ise_ivf_stats(ise_ivf_t* h, uint64_t* out3);

/* Product quantisation: faiss.IndexPQ with 8-bit sub-quantisers (csrc/ise_pq.hpp; the compression half of the
 * reference's "cell-probe" branch, backend/utils.py:311-325, m = 16 codes of 8 bits; composing it with the inverted
 * lists above is not built).  An ise_pq_t keeps a codebook and, per row, M code bytes -- never the floats.  All the
 * conventions at the top of this header hold.  Calls on one handle run one at a time; *_device calls on different
 * streams are ordered one behind the other on the device (one set of workspaces per handle).
 *   create        d > 0, 1 <= M <= ISE_PQ_MAX_M, d a multiple of M (dsub = d / M), nbits == 8 (256 centroids per
 *                 sub-quantiser, code_size = M bytes), one of the two metrics; anything else, and a NULL out, is
 *                 ISE_E_INVALID before the device is touched.  The index is untrained until the centroids are set
 *   centroids     float32 [M][256][dsub].  set refuses (ISE_E_INVALID) a NaN or inf entry and an index that holds
 *                 rows (their codes belong to the centroids in place: reset first); it marks the index trained.
 *                 Every entry point below except reset / info / stats is ISE_E_INVALID on an untrained index
 *   encode        byte m of a row's code = the j whose centroid C[m][j] is nearest to the row's m-th sub-vector in
 *                 squared L2 (float32, the direct difference), the lowest j among equals -- for both metrics.  A row
 *                 with a NaN or inf entry makes the call ISE_E_INVALID ("NaN or inf" in the message).  Both forms
 *                 block: the flag is read back.  codes: n x M bytes, row-major
 *   decode        row i = the concatenation of C[m][code[i][m]]
 *   add           encode and append; a row with a NaN or inf entry makes the call ISE_E_INVALID and NOTHING of that
 *                 call is added.  Both forms block.  add_codes appends ready-made codes as they are.  A row's id is
 *                 its insertion number; fewer than 2^32 rows
 *   codes /       rows [i0, i0 + n) as row-major n x M bytes / decoded n x d floats (the device keeps a row's M bytes
 *   reconstruct   in a stride of M rounded up to 16)
 *   search        asymmetric distance computation: score(x, i) = sum over m of T[m][code[i][m]] with T[m][j] =
 *                 |x_m - C[m][j]|^2 (L2) or the inner product of x_m and C[m][j], each table entry and the sum over
 *                 ascending m accumulated in float32 from +0 -- the L2 distance / inner product of the query and the
 *                 DECODED row.  L2 ascending, inner product descending, ties by ascending id; a score enters only if
 *                 strictly better than +-FLT_MAX (NaN never); unfilled slots are id -1 with +-FLT_MAX.  k in
 *                 1 .. ISE_MAX_K.  The tables are built per 64 queries; a scan pass serves QT queries and 32 results:
 *                     QT(M) = 16 for M <= 5, 8 for M <= 15, 4 for M <= 35, 2 for M <= 64
 *                 (a pass keeps QT x M KiB of tables and QT x 4 KiB of selection buffers in the CU's 160 KiB of LDS),
 *                 so a call makes ceil(nq / 64) table builds and ceil(nq / QT) x ceil(k / 32) passes; an empty index
 *                 fills the padding without either.  search_device only enqueues (it waits on the host only where a
 *                 workspace has to be replaced by a larger one); search_host works through 4096 queries at a time
 *   stats         out4[0] = search batches (a device call with nq > 0; the host form: one per 4096 queries), out4[1] =
 *                 scan passes, out4[2] = table builds, out4[3] = bytes of code storage allocated on the device */
typedef struct ise_pq ise_pq_t;
int ise_pq_create(ise_pq_t** out, int d, int M, int nbits, int metric, int device);
int ise_pq_destroy(ise_pq_t* h); /* NULL is a no-op */
int ise_pq_reset(ise_pq_t* h);   /* drop all rows, keep the codebook */
int ise_pq_info(const ise_pq_t* h, int* d, int* M, int* nbits, int* metric, int64_t* ntotal, int* is_trained, int* device);
int ise_pq_set_centroids_host(ise_pq_t* h, const float* c /* [M][256][dsub] */);
int ise_pq_get_centroids_host(ise_pq_t* h, float* c);
int ise_pq_encode_host(ise_pq_t* h, const float* x, int64_t n, uint8_t* codes);
int ise_pq_encode_device(ise_pq_t* h, const float* x_dev, int64_t n, uint8_t* codes_dev, void* stream);
int ise_pq_decode_host(ise_pq_t* h, const uint8_t* codes, int64_t n, float* x);
int ise_pq_add_host(ise_pq_t* h, const float* x, int64_t n);
int ise_pq_add_device(ise_pq_t* h, const float* x_dev, int64_t n, void* stream);
int ise_pq_add_codes_host(ise_pq_t* h, const uint8_t* codes, int64_t n);
int ise_pq_codes_host(ise_pq_t* h, int64_t i0, int64_t n, uint8_t* codes);
int ise_pq_reconstruct_host(ise_pq_t* h, int64_t i0, int64_t n, float* x);
/* q: nq x d; D: nq x k float32; I: nq x k int64 */
int ise_pq_search_host(ise_pq_t* h, const float* q, int64_t nq, int k, float* D, int64_t* I);
int ise_pq_search_device(ise_pq_t* h, const float* q_dev, int64_t nq, int k, float* D_dev, int64_t* I_dev, void* stream);
int ise_pq_stats(ise_pq_t* h, uint64_t* out4);

/* Scalar quantisation: faiss.IndexScalarQuantizer with the 8-bit types (csrc/ise_sq.hpp).  An ise_sq_t keeps a
 * per-dimension (ISE_SQ_8BIT) or a single (ISE_SQ_8BIT_UNIFORM) vmin / vdiff and, per row, d code bytes plus one
 * float64 -- never the floats.  All the conventions at the top of this header hold; calls, streams and workspaces as
 * for ise_pq_*.
 *   create        1 <= d <= ISE_SQ_MAX_D, one of the two types (Faiss's enum values), one of the two metrics;
 *                 anything else, and a NULL out, is ISE_E_INVALID before the device is touched.  The index is
 *                 untrained until the trained state is set
 *   trained       float32 in Faiss's layout: [vmin_0 .. vmin_{d-1}, vdiff_0 .. vdiff_{d-1}], or [vmin, vdiff] for the
 *                 uniform type.  set refuses (ISE_E_INVALID) a NaN or inf entry, a negative vdiff and an index that
 *                 holds rows (reset first); it takes the step s_j = vdiff_j / 255.0f (one float32 division) and marks
 *                 the index trained.  Every entry point below except reset / info / stats is ISE_E_INVALID on an
 *                 untrained index
 *   encode        c_j = 0 if s_j == 0, else min(255, max(0, floor((x_j - vmin_j) / s_j))) in float32, for both
 *                 metrics.  A row with a NaN or inf entry makes the call ISE_E_INVALID ("NaN or inf" in the message).
 *                 Both forms block: the flag is read back.  codes: n x d bytes, row-major
 *   decode        y_j = fmaf((float)c_j + 0.5f, s_j, vmin_j)
 *   add           encode and append; a row with a NaN or inf entry makes the call ISE_E_INVALID and NOTHING of that
 *                 call is added.  Both forms block.  add_codes appends ready-made codes as they are.  A row's id is
 *                 its insertion number; fewer than 2^32 rows
 *   codes /       rows [i0, i0 + n) as row-major n x d bytes / decoded n x d floats (the device keeps a row's d bytes
 *   reconstruct   in a stride of d rounded up to 64, and one float64 row term beside it)
 *   search        the squared L2 distance / inner product of the query and the DECODED row in float32, expanded about
 *                 o_j = vmin_j + s_j / 2 with float64 outer terms (csrc/ise_sq.hpp).  The float32 accumulators hold
 *                 sums of size 128 W, W = sum_j |s_j (x_j - o_j)| (L2) or sum_j |s_j x_j| (inner product), so the
 *                 error against the float64 score over the decoded rows is bounded in terms of W, not of the score:
 *                 at most 128 W (3 * 2^-22 + 2 ceil(d / 64) 2^-24 (1 + 2^-9)) for the inner product and twice that
 *                 for L2, plus float32's rounding of the result, of x_j - o_j and of o_j (DESIGN.md 4.15 derives
 *                 every term; tests/sq_ref.py, score_bound).  That is within 1e-4 max(1, |score|) where the data
 *                 fill their trained range, as min/max training on the added rows gives unless outliers stretch it.
 *                 Where a training outlier stretches the range and rows and queries sit together near one end of
 *                 it, W is orders of magnitude above an L2 distance, which then loses its digits from the second
 *                 on (measured: 5e-2 to 1e-1 relative at d = 512 on rows N(900, 1) with one all-zero training row);
 *                 the inner product stays below 1e-6 relative there.  Exact
 *                 where every partial sum is an exactly representable integer, an L2 score never negative, a zero
 *                 +0, and the bits of a (query, row) pair independent of nq, k and the query's place in the batch.
 *                 L2 ascending, inner product descending, ties by ascending id; a score enters only if strictly better
 *                 than +-FLT_MAX (NaN never; a query with a NaN or inf entry gets padding only); unfilled slots are
 *                 id -1 with +-FLT_MAX.  k in 1 .. ISE_MAX_K.  A scan pass serves QT queries and 32 results, QT = 16
 *                 for d <= 1472 and 8 above (the CU's 160 KiB of LDS), so a call makes ceil(nq / QT) x ceil(k / 32)
 *                 passes; an empty index fills the padding without one.  search_device only enqueues (it waits on
 *                 the host only where a workspace has to be replaced by a larger one); search_host works through 4096
 *                 queries at a time
 *   stats         out3[0] = search batches (a device call with nq > 0; the host form: one per 4096 queries), out3[1] =
 *                 scan passes, out3[2] = bytes of code storage allocated on the device */
#define ISE_SQ_8BIT 0
#define ISE_SQ_8BIT_UNIFORM 2
typedef struct ise_sq ise_sq_t;
int ise_sq_create(ise_sq_t** out, int d, int qtype, int metric, int device);
int ise_sq_destroy(ise_sq_t* h); /* NULL is a no-op */
int ise_sq_reset(ise_sq_t* h);   /* drop all rows, keep the trained state */
int ise_sq_info(const ise_sq_t* h, int* d, int* qtype, int* metric, int64_t* ntotal, int* is_trained, int* device);
int ise_sq_set_trained_host(ise_sq_t* h, const float* t /* 2 d floats, or 2 for the uniform type */);
int ise_sq_get_trained_host(ise_sq_t* h, float* t);
int ise_sq_encode_host(ise_sq_t* h, const float* x, int64_t n, uint8_t* codes);
int ise_sq_encode_device(ise_sq_t* h, const float* x_dev, int64_t n, uint8_t* codes_dev, void* stream);
int ise_sq_decode_host(ise_sq_t* h, const uint8_t* codes, int64_t n, float* x);
int ise_sq_add_host(ise_sq_t* h, const float* x, int64_t n);
int ise_sq_add_device(ise_sq_t* h, const float* x_dev, int64_t n, void* stream);
int ise_sq_add_codes_host(ise_sq_t* h, const uint8_t* codes, int64_t n);
int ise_sq_codes_host(ise_sq_t* h, int64_t i0, int64_t n, uint8_t* codes);
int ise_sq_reconstruct_host(ise_sq_t* h, int64_t i0, int64_t n, float* x);
/* q: nq x d; D: nq x k float32; I: nq x k int64 */
int ise_sq_search_host(ise_sq_t* h, const float* q, int64_t nq, int k, float* D, int64_t* I);
int ise_sq_search_device(ise_sq_t* h, const float* q_dev, int64_t nq, int k, float* D_dev, int64_t* I_dev, void* stream);
int ise_sq_stats(ise_sq_t* h, uint64_t* out3);

/* Inverted lists over scalar-quantised rows: faiss.IndexIVFScalarQuantizer with by_residual = false and the two 8-bit
 * types (csrc/ise_ivfsq.hpp).  An ise_ivfsq_t is ise_ivf_t's lists holding ise_sq_t's rows: nlist lists of d code bytes
 * plus one float64 per row, NO centroids (the coarse quantiser is the caller's; rows come with their list numbers,
 * searches with their probe tables, as for ise_ivf_*), and the codec, trained state, code bytes and scores of ise_sq_*
 * for the same trained vector.  Calls, streams and workspaces as for ise_ivf_*.
 *   create        1 <= d <= ISE_SQ_MAX_D, nlist >= 1, one of the two types, one of the two metrics; anything else is
 *                 ISE_E_INVALID before the device is touched.  Untrained until the trained state is set; every entry
 *                 point below except reset / info / list_sizes / stats is then ISE_E_INVALID
 *   trained       as ise_sq_set_trained_host / ise_sq_get_trained_host
 *   add           list_no[i] in [0, nlist) is the list of row i; a number outside makes the call ISE_E_INVALID and
 *                 nothing is added.  The rows are encoded at once into a pending buffer of codes and row terms; a row
 *                 with a NaN or inf entry makes the call ISE_E_INVALID ("NaN or inf" in the message) and NOTHING of that
 *                 call is added.  All forms block.  add_codes takes ready-made codes (n x d bytes).  A row's id is its
 *                 insertion number; fewer than 2^32 rows.  The first search or list_host after an add rebuilds the lists
 *                 (64-row tiles; one rebuild moves the whole index)
 *   list_sizes    rows per list, pending ones included
 *   list          ids (ascending) and codes (m x d bytes) of one list, in list order; either may be NULL
 *   search        probes: nq x nprobe list numbers; -1 and numbers outside [0, nlist) name nothing, a list named twice
 *                 counts once.  The k best among the rows of a query's probed lists, scored as ise_sq_search_* scores
 *                 the same (query, row) pair; ties by ascending id; unfilled slots are id -1 with +-FLT_MAX; a query with
 *                 a NaN or inf entry gets padding only.  A pass serves QT queries and 32 results (QT as for ise_sq_*) and
 *                 reads the 64-row tiles of the lists that at least one of its queries probes, and no others; a call
 *                 makes ceil(nq / QT) x ceil(k / 32) passes, none on an empty index.  search_device only enqueues, unless
 *                 rows are pending or a workspace has to grow; search_host works through 4096 queries at a time
 *   stats         out3[0] = search batches, out3[1] = scan passes, out3[2] = 64-row tiles the passes visited.  Waits
 *                 for the device */
typedef struct ise_ivfsq ise_ivfsq_t;
int ise_ivfsq_create(ise_ivfsq_t** out, int d, int qtype, int metric, int nlist, int device);
int ise_ivfsq_destroy(ise_ivfsq_t* h); /* NULL is a no-op */
int ise_ivfsq_reset(ise_ivfsq_t* h);   /* drop all rows, keep the trained state */
int ise_ivfsq_info(const ise_ivfsq_t* h, int* d, int* qtype, int* metric, int* nlist, int64_t* ntotal, int* is_trained,
                   int* device);
int ise_ivfsq_set_trained_host(ise_ivfsq_t* h, const float* t /* 2 d floats, or 2 for the uniform type */);
int ise_ivfsq_get_trained_host(ise_ivfsq_t* h, float* t);
int ise_ivfsq_add_host(ise_ivfsq_t* h, const float* x, const int64_t* list_no, int64_t n);
int ise_ivfsq_add_device(ise_ivfsq_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream);
int ise_ivfsq_add_codes_host(ise_ivfsq_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n);
int ise_ivfsq_list_sizes_host(ise_ivfsq_t* h, int64_t* sizes /* nlist */);
int ise_ivfsq_list_host(ise_ivfsq_t* h, int list, int64_t* ids, uint8_t* codes);
int ise_ivfsq_search_host(ise_ivfsq_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                          int64_t* I);
int ise_ivfsq_search_device(ise_ivfsq_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                            float* D_dev, int64_t* I_dev, void* stream);
int ise_ivfsq_stats(ise_ivfsq_t* h, uint64_t* out3);

/* Inverted lists over product-quantiser codes: faiss.IndexIVFPQ with by_residual = false and 8-bit sub-quantisers
 * (csrc/ise_ivfpq.hpp).  An ise_ivfpq_t is ise_ivf_t's lists holding ise_pq_t's code rows: nlist lists of M code bytes
 * per row, NO coarse centroids (the coarse quantiser is the caller's; rows come with their list numbers, searches with
 * their probe tables, as for ise_ivf_*), and the codec, codebook, code bytes and scores of ise_pq_* for the same
 * centroids.  Calls, streams and workspaces as for ise_ivf_*.
 *   create        d > 0, 1 <= M <= ISE_PQ_MAX_M, d % M == 0, nbits == 8, nlist >= 1, one of the two metrics; anything
 *                 else is ISE_E_INVALID before the device is touched.  Untrained until the centroids are set; every
 *                 entry point below except reset / info / list_sizes / stats is then ISE_E_INVALID
 *   centroids     as ise_pq_set_centroids_host / ise_pq_get_centroids_host: [M][256][d / M] float32
 *   add           list_no[i] in [0, nlist) is the list of row i; a number outside makes the call ISE_E_INVALID and
 *                 nothing is added.  The rows are encoded at once (ise_pq_*'s encoder) into a pending buffer; a row with
 *                 a NaN or inf entry makes the call ISE_E_INVALID ("NaN or inf" in the message) and NOTHING of that call
 *                 is added.  All forms block.  add_codes takes ready-made codes (n x M bytes).  A row's id is its
 *                 insertion number; fewer than 2^32 rows.  The first search or list_host after an add rebuilds the lists
 *                 (64-row tiles; one rebuild moves the whole index)
 *   list_sizes    rows per list, pending ones included
 *   list          ids (ascending) and codes (m x M bytes) of one list, in list order; either may be NULL
 *   search        probes: nq x nprobe list numbers; -1 and numbers outside [0, nlist) name nothing, a list named twice
 *                 counts once.  The k best among the rows of a query's probed lists, scored as ise_pq_search_* scores
 *                 the same (query, row) pair -- the same tables, summed from +0.0f over ascending m: the same bits --;
 *                 ties by ascending id; unfilled slots are id -1 with +-FLT_MAX; a query with a NaN or inf entry gets
 *                 padding only.  A pass serves QT queries and 32 results (QT as for ise_pq_*) and reads the 64-row tiles
 *                 of the lists that at least one of its queries probes, and no others; a call makes ceil(nq / QT) x
 *                 ceil(k / 32) passes and one table build per 64 queries, none of either on an empty index.
 *                 search_device only enqueues, unless rows are pending or a workspace has to grow; search_host works
 *                 through 4096 queries at a time
 *   stats         out4[0] = search batches, out4[1] = scan passes, out4[2] = 64-row tiles the passes visited, out4[3] =
 *                 table builds.  Waits for the device */
typedef struct ise_ivfpq ise_ivfpq_t;
int ise_ivfpq_create(ise_ivfpq_t** out, int d, int M, int nbits, int metric, int nlist, int device);
int ise_ivfpq_destroy(ise_ivfpq_t* h); /* NULL is a no-op */
int ise_ivfpq_reset(ise_ivfpq_t* h);   /* drop all rows, keep the centroids */
int ise_ivfpq_info(const ise_ivfpq_t* h, int* d, int* M, int* nbits, int* metric, int* nlist, int64_t* ntotal, int* is_trained,
                   int* device);
int ise_ivfpq_set_centroids_host(ise_ivfpq_t* h, const float* c /* M * 256 * (d / M) floats */);
int ise_ivfpq_get_centroids_host(ise_ivfpq_t* h, float* c);
int ise_ivfpq_add_host(ise_ivfpq_t* h, const float* x, const int64_t* list_no, int64_t n);
int ise_ivfpq_add_device(ise_ivfpq_t* h, const float* x_dev, const int64_t* list_no_dev, int64_t n, void* stream);
int ise_ivfpq_add_codes_host(ise_ivfpq_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n);
int ise_ivfpq_list_sizes_host(ise_ivfpq_t* h, int64_t* sizes /* nlist */);
int ise_ivfpq_list_host(ise_ivfpq_t* h, int list, int64_t* ids, uint8_t* codes);
int ise_ivfpq_search_host(ise_ivfpq_t* h, const float* q, int64_t nq, int k, const int64_t* probes, int nprobe, float* D,
                          int64_t* I);
int ise_ivfpq_search_device(ise_ivfpq_t* h, const float* q_dev, int64_t nq, int k, const int64_t* probes_dev, int nprobe,
                            float* D_dev, int64_t* I_dev, void* stream);
int ise_ivfpq_stats(ise_ivfpq_t* h, uint64_t* out4);

/* Inverted lists over bit codes: faiss.IndexBinaryIVF (csrc/ise_binary_ivf.hpp).  An ise_binary_ivf_t is ise_ivfsq_t's
 * lists holding ise_binary_index_t's codes: nlist lists of d_bits / 8 code bytes, NO centroids (the coarse quantiser is
 * the caller's; rows come with their list numbers, searches with their probe tables, as for ise_ivf_*), and the Hamming
 * distances, keys and tie order of ise_binary_index_search_*.  Calls, streams and workspaces as for ise_ivfsq_*.
 *   create        d_bits a positive multiple of 8, at most ISE_BINARY_MAX_BITS, nlist >= 1; anything else is
 *                 ISE_E_INVALID before the device is touched.  There is nothing to train
 *   add           list_no[i] in [0, nlist) is the list of code i (n x d_bits / 8 bytes); a number outside makes the call
 *                 ISE_E_INVALID and nothing is added.  The codes go into a pending buffer; both forms block.  A row's id
 *                 is its insertion number; fewer than 2^32 rows.  The first search or list_host after an add rebuilds the
 *                 lists (64-row tiles; one rebuild moves the whole index)
 *   list_sizes    rows per list, pending ones included
 *   list          ids (ascending) and codes (m x d_bits / 8 bytes) of one list, in list order; either may be NULL
 *   search        probes: nq x nprobe list numbers; -1 and numbers outside [0, nlist) name nothing, a list named twice
 *                 counts once.  The k best among the rows of a query's probed lists: D int32 Hamming distances ascending,
 *                 ties by ascending id, unfilled slots INT32_MAX / -1; k in 1 .. ISE_MAX_K.  A pass serves 16 queries and
 *                 32 results and reads the 64-row tiles of the lists that at least one of its queries probes, and no
 *                 others; a call makes ceil(nq / 16) x ceil(k / 32) passes, none on an empty index.  search_device only
 *                 enqueues, unless rows are pending or a workspace has to grow; search_host works through 4096 queries
 *                 at a time
 *   stats         out3[0] = search batches, out3[1] = scan passes, out3[2] = 64-row tiles the passes visited.  Waits
 *                 for the device */
typedef struct ise_binary_ivf ise_binary_ivf_t;
int ise_binary_ivf_create(ise_binary_ivf_t** out, int d_bits, int nlist, int device);
int ise_binary_ivf_destroy(ise_binary_ivf_t* h); /* NULL is a no-op */
int ise_binary_ivf_reset(ise_binary_ivf_t* h);   /* drop all rows */
int ise_binary_ivf_info(const ise_binary_ivf_t* h, int* d_bits, int* nlist, int64_t* ntotal, int* device);
int ise_binary_ivf_add_host(ise_binary_ivf_t* h, const uint8_t* codes, const int64_t* list_no, int64_t n);
int ise_binary_ivf_add_device(ise_binary_ivf_t* h, const uint8_t* codes_dev, const int64_t* list_no_dev, int64_t n,
                              void* stream);
int ise_binary_ivf_list_sizes_host(ise_binary_ivf_t* h, int64_t* sizes /* nlist */);
int ise_binary_ivf_list_host(ise_binary_ivf_t* h, int list, int64_t* ids, uint8_t* codes);
int ise_binary_ivf_search_host(ise_binary_ivf_t* h, const uint8_t* q, int64_t nq, int k, const int64_t* probes, int nprobe,
                               int32_t* D, int64_t* I);
int ise_binary_ivf_search_device(ise_binary_ivf_t* h, const uint8_t* q_dev, int64_t nq, int k, const int64_t* probes_dev,
                                 int nprobe, int32_t* D_dev, int64_t* I_dev, void* stream);
int ise_binary_ivf_stats(ise_binary_ivf_t* h, uint64_t* out3);

/* Shard-local search for the multi-GPU path: writes nq x k
 * packed candidates, sorted best-first, suitable for one all-gather:
 *   key = (order-preserving uint32 image of the score) << 32 | (row + id_base)
 * with unfilled slots = 0xFFFFFFFFFFFFFFFF.  For inner product the score
 * image is taken of -score so that ascending key order is best-first for
 * both metrics. */
int ise_index_search_keys_device(ise_index_t* h, const float* q_dev, int64_t nq, int k,
                                 uint32_t id_base, uint64_t* keys_dev, void* stream);

/* Merge n_lists sorted candidate lists per query (layout [n_lists][nq][k],
 * e.g. the all-gathered output of ise_index_search_keys_device over ranks)
 * into D (nq x k float32) and I (nq x k int64).  Needs no index handle;
 * `device` selects the GPU the pointers live on. */
int ise_merge_keys_device(const uint64_t* keys_dev, int n_lists, int64_t nq, int k,
                          int metric, float* D_dev, int64_t* I_dev, int device, void* stream);

/* The exchange step of the row-sharded search (the reference itself never shards:
 * one in-RAM IndexFlat, backend/utils.py:327): ONE all-gather of every rank's packed candidates,
 * issued by RCCL on the caller's stream between the shard scans and the merge -- no host
 * synchronisation, no framework in between.
 *   ise_comm_precheck    everything ise_comm_create needs that can be checked WITHOUT the other ranks
 *                        (librccl resolves with every symbol, `device` exists and can be made current):
 *                        the caller agrees on the outcome across ranks BEFORE any rank enters the
 *                        rendezvous of ise_comm_create, where a missing peer would block the others
 *   ise_comm_unique_id   rank 0 draws the 128-byte id of a new communicator; the caller hands it to
 *                        the other ranks (any channel; sharded.py uses one torch.distributed broadcast)
 *   ise_comm_create      every rank, collectively: join as `rank` of `world`, one GPU per rank
 *   ise_comm_allgather_keys  recv[r * count + i] = rank r's send[i] on every rank (count uint64 per
 *                        rank, device pointers); enqueued on `stream`, returns at once
 * librccl is resolved at run time, so the library loads without it; these entry points then
 * return ISE_E_NODEVICE. */
typedef struct ise_comm ise_comm_t;
int ise_comm_precheck(int device);
int ise_comm_unique_id(void* id128);
int ise_comm_create(ise_comm_t** out, const void* id128, int world, int rank, int device);
int ise_comm_allgather_keys(ise_comm_t* c, const uint64_t* send_dev, uint64_t* recv_dev,
                            int64_t count, void* stream);
int ise_comm_destroy(ise_comm_t* c);

/* index.search(X, 1) for MANY rows against a SMALL index: nearest-centroid assignment,
 * FaissKMeans.transform (backend/kmeans_faiss.py:46-50; BASELINE config 4).  X: n x d
 * float32 on the device; I: n int64 (row of the best index entry, -1 if none); D: n
 * float32 or NULL (squared L2 / inner product of the best entry).  MFMA-bound GEMM-shaped
 * kernel; needs a float32 index with d <= 512 (otherwise use ise_index_search_*). */
int ise_index_assign_device(ise_index_t* h, const float* x_dev, int64_t n, float* D_dev,
                            int64_t* I_dev, void* stream);

/* faiss.normalize_L2(x) (backend/utils.py:303, backend/engine.py:53,
 * backend/siamese/test_index.py:53, siamese_pt/create_index.py:57,
 * siamese_tf/create_index.py:54):
 * in-place row L2 normalisation of n x d float32, zero rows untouched. */
int ise_normalize_rows_device(float* x_dev, int64_t n, int d, int device, void* stream);
int ise_normalize_rows_host(float* x, int64_t n, int d, int device);

/* faiss.LinearTransform::apply (PCAMatrix, OPQMatrix, RandomRotationMatrix in front of an index):
 * y = A x + b for n rows, float32.  A handle is immutable: it holds A (host, [d_out][d_in], Faiss's layout), re-packed
 * once into the panels the kernels load, and b (host, d_out floats, or NULL: none).  1 <= d_in, d_out <=
 * ISE_LINEAR_MAX_D.
 *   The arithmetic is a function of d_in only -- not of n, of a row's place in the batch, of the launch shape or of the
 * stream: k is cut into segments of 256; each segment is a k-ascending float32 fmaf chain from +0, s = fmaf(A[j][k],
 * x[k], s); y_j = ((b_j + s_0) + s_1) + ... by float32 adds in ascending segment order (b_j = +0 without a bias).  NaN
 * and inf follow IEEE rules into the outputs of their own row only; subnormals are kept.
 *   apply_device  x_dev: n x d_in on the device (rows 4-byte aligned; 16-byte loads are used where the pointer and
 *                 d_in allow), y_dev: n x d_out, not overlapping x_dev; enqueued on `stream`, nothing is waited for
 *                 and no scratch memory is used, so calls on different streams need no order between them.  n >= 1.
 *                 n <= ISE_LINEAR_FEW_ROWS spreads the matrix over the device (a wave per segment); more rows take an
 *                 LDS-tiled kernel; both give the same bits.
 *   apply_host    the same through the handle's staging buffers, in pieces of 256 MiB at most; one call at a time.
 *   stats         out3: calls of apply_device / apply_host pieces, few-row launches, tiled launches. */
typedef struct ise_linear ise_linear_t;
int ise_linear_create(ise_linear_t** out, int d_in, int d_out, const float* A, const float* b, int device);
int ise_linear_destroy(ise_linear_t* h);
int ise_linear_info(const ise_linear_t* h, int* d_in, int* d_out, int* have_bias, int* device);
int ise_linear_apply_device(ise_linear_t* h, const float* x_dev, int64_t n, float* y_dev, void* stream);
int ise_linear_apply_host(ise_linear_t* h, const float* x, int64_t n, float* y);
int ise_linear_stats(ise_linear_t* h, uint64_t* out3);

/* The visual-word histogram of BOVW.transform (backend/bag_of_visual_words.py:98-106): for
 * every image i, np.histogram(labels[offsets[i] : offsets[i+1]], bins=K) -- K equal-width bins
 * between that image's own smallest and largest label, as numpy computes it when no range is
 * given.  labels: int64 ids from the k = 1 assignment (values in [0, 2^53)); offsets: n_images
 * + 1 non-decreasing int64 row offsets; out: n_images x K float64 counts (the reference's
 * np.zeros((n, K)) array).  An image without rows gives a zero row.  K <= 16384. */
int ise_bovw_histogram_device(const int64_t* labels_dev, const int64_t* offsets_dev,
                              int64_t n_images, int K, double* out_dev, int device, void* stream);

/* measurement hook for bench.py: run one search batch `iters` times on `stream` and return
 * the average duration of the scan kernel (all filter passes when k needs several) and of
 * everything behind it (merge + exact re-rank + the gated exact-scan launches) in milliseconds,
 * measured with hipEvents recorded on that stream around the kernels.  Results land in
 * D_dev / I_dev as for ise_index_search_device. */
int ise_index_search_timed_device(ise_index_t* h, const float* q_dev, int64_t nq, int k,
                                  float* D_dev, int64_t* I_dev, void* stream, int iters,
                                  float* scan_ms_avg, float* merge_ms_avg);

#ifdef __cplusplus
}
#endif
#endif /* ISE_KNN_H */
