// ise_ivf_lists.hpp -- the host side that the four inverted-list kinds share (float32 rows, ise_ivf.hip; 8-bit rows,
// ise_ivfsq.hip; product-quantiser codes, ise_ivfpq.hip; bit codes, ise_binary_ivf.hip; the kernels are ise_ivf_tiles.hpp's): the ids and the
// table of the sorted array beside the host's counts (IvfLists over ise_ivf_plan.hpp), the common part of a handle
// (IvfCore: the sorted rows and their pending buffer as bytes, the call order, the counters, the stream and the mutex)
// with its setup, teardown, reset, stats and rebuild, the search shell of the kinds that scan 64-row tiles from a work
// list, and the staged host form of a search.  What a row IS -- how it is encoded or padded, how a chunk's queries are
// staged, what a pass's kernel is handed -- stays with the index kind.  Host code; the handle's mutex is held.
#pragma once
#include "ise_ivf_tiles.hpp"
#include "ise_pass_host.hpp"

struct IvfLists : IvfBook {
    uint32_t* ids = nullptr;   // [tiles * tile rows] the sorted array's row numbers, ~0 in the pad slots
    uint32_t* meta = nullptr;  // ivf_plan_meta's table
    const uint32_t* list_tile0_dev() const { return meta; }
    const uint32_t* list_size_dev() const { return meta + ivf_meta_size_at((size_t)nlist); }
    const uint32_t* tile_list_dev() const { return meta + ivf_meta_tile_list_at((size_t)nlist); }

    // the device is idle: no rows, sorted or pending
    void free_rows() {
        if (ids) (void)hipFree(ids);
        if (meta) (void)hipFree(meta);
        ids = nullptr;
        meta = nullptr;
        clear();
    }

    // list numbers on the host, checked before anything changes
    int check_lists(const int64_t* list_no, long long m) const {
        if (n + m >= (1ll << 32)) return ise_fail_(ISE_E_INVALID, "an inverted-list index holds fewer than 2^32 rows");
        const long long i = ivf_first_bad_list(list_no, m, nlist);
        if (i >= 0)
            return ise_fail_(ISE_E_INVALID, "list number " + std::to_string((long long)list_no[i]) + " of row " + std::to_string(i) +
                                                " is outside [0, nlist = " + std::to_string(nlist) + "): nothing was added");
        return ISE_OK;
    }

    // the ids and the table of a rebuild, allocated (the caller's guard frees them), the table uploaded on st; *dest:
    // where the pending rows go.  The ids are the caller's to fill, with its rows (pad slots: ~0).  meta_host and pl
    // are pageable host memory on its way: they live until st has drained
    int begin_rebuild(const IvfPlan& pl, int tile_rows, hipStream_t st, std::vector<uint32_t>& meta_host, uint32_t** nids,
                      uint32_t** nmeta, uint32_t** dest) const {
        const size_t slots = (size_t)pl.tile0[(size_t)nlist] * tile_rows;
        meta_host = ivf_plan_meta(pl);
        HIP_TRY(hipMalloc((void**)nids, slots * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)nmeta, meta_host.size() * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)dest, (size_t)pend_n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(*nmeta, meta_host.data(), meta_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(*dest, pl.dest.data(), (size_t)pend_n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        return ISE_OK;
    }
    // st has drained: the new ids and table go in (the old ones are left in *nids, *nmeta for the caller's guard)
    void finish_rebuild(const IvfPlan& pl, uint32_t** nids, uint32_t** nmeta) {
        std::swap(ids, *nids);
        std::swap(meta, *nmeta);
        take_over(pl);
    }

    void list_sizes_host(int64_t* sizes) const {
        for (int l = 0; l < nlist; l++) sizes[l] = size_all[(size_t)l];
    }
    // the ids of `list` (nothing pending) if asked for; *m: its rows, *slot0: its first slot
    int list_ids_host(int list, int tile_rows, int64_t* out, size_t* m, size_t* slot0) const {
        *m = (size_t)size[(size_t)list];
        *slot0 = (size_t)tile0[(size_t)list] * tile_rows;
        if (*m == 0 || !out) return ISE_OK;
        std::vector<uint32_t> tmp(*m);
        HIP_TRY(hipMemcpy(tmp.data(), ids + *slot0, *m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < *m; i++) out[i] = (int64_t)tmp[i];
        return ISE_OK;
    }
};

// ---------------------------------------------------------------- the common part of a handle
// What a kind says of its rows once, at create: tile_rows and unit_bytes pick the rebuild's kernels (ivf_rebuild_launch),
// a row is row_bytes, and with_side every slot carries an 8-byte value beside it.
struct IvfCore {
    int device = 0, num_cu = 256;
    int tile_rows = 0, unit_bytes = 0;
    size_t row_bytes = 0;
    bool with_side = false;
    IvfLists inv;  // the lists' counts, ids and table; the sorted array has [inv.tiles * tile_rows] slots
    char *rows = nullptr, *side = nullptr;  // the sorted array: [slots][row_bytes], [slots][8] (with_side)
    // rows added since the last rebuild, in insertion order (inv.pend_n of them): [pend_cap][row_bytes], [pend_cap][8]
    char *pend = nullptr, *pend_side = nullptr;
    long long pend_cap = 0;
    CallOrder order;
    unsigned long long* stats_dev = nullptr;  // [1] tiles (work-list entries) the passes visited
    unsigned long long batches = 0, passes = 0;
    hipStream_t stream = nullptr;  // add / rebuild from the host entry points / list_host
    std::mutex mu_;

    template <class T> T* rows_as() const { return reinterpret_cast<T*>(rows); }
    template <class T> T* pend_row(long long i) const { return reinterpret_cast<T*>(pend + (size_t)i * row_bytes); }

    void free_pending() {
        if (pend) (void)hipFree(pend);
        if (pend_side) (void)hipFree(pend_side);
        pend = pend_side = nullptr;
        pend_cap = 0;
    }
    // the device is idle: no rows, sorted or pending
    void free_rows() {
        if (rows) (void)hipFree(rows);
        if (side) (void)hipFree(side);
        rows = side = nullptr;
        free_pending();
        inv.free_rows();
    }

    // room for n more pending rows: the buffers at least double (so they are never more than twice their rows), and
    // either both are replaced or neither is
    int reserve_pending(long long n, hipStream_t st) {
        const long long need = inv.pend_n + n;
        if (need <= pend_cap) return ISE_OK;
        const long long cap = std::max(need, 2 * pend_cap);
        char *nx = nullptr, *ns = nullptr;
        DevFreeList<2> fr{{(void**)&nx, (void**)&ns}};
        HIP_TRY(hipMalloc((void**)&nx, (size_t)cap * row_bytes));
        if (with_side) HIP_TRY(hipMalloc((void**)&ns, (size_t)cap * 8));
        if (inv.pend_n > 0) {
            HIP_TRY(hipMemcpyAsync(nx, pend, (size_t)inv.pend_n * row_bytes, hipMemcpyDeviceToDevice, st));
            if (with_side) HIP_TRY(hipMemcpyAsync(ns, pend_side, (size_t)inv.pend_n * 8, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        std::swap(pend, nx);  // the old buffers go with the guard
        std::swap(pend_side, ns);
        pend_cap = cap;
        return ISE_OK;
    }

    // add_device: the rows' list numbers on the host, checked before anything changes
    int download_lists(const int64_t* list_no_dev, long long n, hipStream_t st, std::vector<int64_t>* lists) const {
        lists->resize((size_t)n);
        HIP_TRY(hipMemcpyAsync(lists->data(), list_no_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return inv.check_lists(lists->data(), n);
    }

    // out3: searches, passes, tiles visited.  Waits for the device: the passes enqueued so far have added theirs
    int stats(uint64_t* out3) const {
        unsigned long long loaded = 0;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&loaded, stats_dev, sizeof(loaded), hipMemcpyDeviceToHost));
        out3[0] = batches;
        out3[1] = passes;
        out3[2] = loaded;
        return ISE_OK;
    }
};

// the prologue of an entry point behind its argument checks: the handle's mutex, then its device
struct IvfEntry {
    std::lock_guard<std::mutex> lk;
    DeviceGuard gd;
    explicit IvfEntry(IvfCore& c) : lk(c.mu_), gd(c.device) {}
    int check() const { return gd.ok ? ISE_OK : ise_fail_(ISE_E_HIP, "hipSetDevice failed"); }
};

// everything a handle holds on its device (set, idle); free_own: the kind's own buffers
template <class FreeOwn>
void ivf_free_all(IvfCore& c, FreeOwn free_own) {
    c.free_rows();
    free_own();
    if (c.stats_dev) (void)hipFree(c.stats_dev);
    c.order.destroy();
    if (c.stream) (void)hipStreamDestroy(c.stream);
}

// *_create behind its argument checks.  H: the handle, its IvfCore the member c.  init(h) -> hipError_t fills the
// kind's fields (the core's row shape among them) and allocates what it keeps on the device; free_own(h) frees that
// (on a failed setup too, whatever init got to).  what: the failure message's "... index setup"
template <class H, class Init, class FreeOwn>
int ivf_create(H** out, int nlist, int device, const char* what, Init init, FreeOwn free_own) {
    int num_cu = 0;
    const int rc = device_gate(device, &num_cu);
    if (rc) return rc;
    H* h = new (std::nothrow) H();
    if (!h) return ise_fail_(ISE_E_NOMEM, "host allocation failed");
    IvfCore& c = h->c;
    c.device = device;
    c.num_cu = num_cu;
    c.inv.nlist = nlist;
    c.inv.clear();
    DeviceGuard gd(device);
    hipError_t e = gd.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = c.order.create();
    if (e == hipSuccess) e = hipMalloc((void**)&c.stats_dev, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c.stats_dev, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = init(h);
    if (e != hipSuccess) {
        ivf_free_all(c, [&]() { free_own(h); });
        delete h;
        return ise_fail_(ISE_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    *out = h;
    return ISE_OK;
}

template <class H, class FreeOwn>
int ivf_destroy(H* h, FreeOwn free_own) {
    if (!h) return ISE_OK;
    {
        DeviceGuard gd(h->c.device);
        (void)hipDeviceSynchronize();
        ivf_free_all(h->c, [&]() { free_own(h); });
    }
    delete h;
    return ISE_OK;
}

// drop every row; free_own_rows: what the kind keeps per slot beside the core's arrays
template <class FreeOwnRows>
int ivf_reset(IvfCore& c, FreeOwnRows free_own_rows) {
    IvfEntry en(c);
    if (en.check()) return ISE_E_HIP;
    HIP_TRY(hipDeviceSynchronize());
    c.free_rows();
    free_own_rows();
    c.order.forget();  // the device has drained
    return ISE_OK;
}

// ---------------------------------------------------------------- the rebuild
// the pending rows into the lists (mu_ held).  The host's counting sort says where every pending row goes, a new
// array of exactly the needed tiles is allocated, the old tiles move to where their lists now start and the pending
// rows are scattered behind them (ivf_rebuild_launch); hook(new rows, slots) then enqueues on st what the kind derives
// from the new array.  Blocks: the host's tables are copied from pageable memory and the old arrays are freed behind
// the kernels.  Rows, side values, ids and the table go into fresh buffers that are swapped in together once st has
// drained (a pass still in flight on another stream keeps a consistent set); nothing changes if an allocation fails.
// *rebuilt: the swap happened (the kind swaps in what its hook computed)
inline int ivf_no_hook(char*, size_t) { return ISE_OK; }  // the hook of a kind that derives nothing from its rows
template <class Hook>
int ivf_rebuild_locked(IvfCore& c, hipStream_t st, Hook hook, bool* rebuilt = nullptr) {
    IvfLists& inv = c.inv;
    if (inv.pend_n == 0) return ISE_OK;
    IvfPlan pl;
    if (!inv.plan(&pl, c.tile_rows))
        return ise_fail_(ISE_E_INVALID, "the lists' " + std::to_string(c.tile_rows) + "-row tiles no longer fit 32-bit slot numbers");
    const long long new_tiles = (long long)pl.tile0[(size_t)inv.nlist];
    const size_t slots = (size_t)new_tiles * c.tile_rows;
    char *nx = nullptr, *ns = nullptr;
    uint32_t *nids = nullptr, *nmeta = nullptr, *dest = nullptr;
    DevFreeList<5> fr{{(void**)&nx, (void**)&ns, (void**)&nids, (void**)&nmeta, (void**)&dest}};
    std::vector<uint32_t> meta_host;
    HIP_TRY(hipMalloc((void**)&nx, slots * c.row_bytes));
    if (c.with_side) HIP_TRY(hipMalloc((void**)&ns, slots * 8));
    int rc = inv.begin_rebuild(pl, c.tile_rows, st, meta_host, &nids, &nmeta, &dest);
    if (rc) return rc;
    HIP_TRY(ivf_rebuild_launch(c.tile_rows, c.unit_bytes, c.row_bytes, {c.rows, c.side, inv.ids}, inv.meta, inv.tiles,
                               {c.pend, c.pend_side, nullptr}, inv.pend_n, dest, (uint32_t)(inv.n - inv.pend_n), inv.nlist, nmeta,
                               new_tiles, {nx, ns, nids}, st));
    if ((rc = hook(nx, slots))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::swap(c.rows, nx);  // the old arrays go with the guard (hipFree waits for the passes that still read them)
    std::swap(c.side, ns);
    inv.finish_rebuild(pl, &nids, &nmeta);
    c.free_pending();
    if (rebuilt) *rebuilt = true;
    return ISE_OK;
}

// ---------------------------------------------------------------- the search shell of the kinds that scan 64-row tiles
// A pass serves one group of qt = 1 << qshift queries and kpass results; the work lists of `chunk` queries are built
// per launch; a pass has coded_grid(tiles, tiles_per_wave, waves, blocks_per_cu) blocks (the host does not know how
// many entries a group's work list holds without a wait, so the rule counts the lists' tiles in all).
struct IvfTiledShape {
    int chunk, qt, qshift, kpass;
    int tiles_per_wave, waves;
    long long blocks_per_cu;
    size_t stage_bytes;  // of one call's staged queries
};
// one set of search workspaces
struct IvfTiledWs {
    DevBuf<unsigned char> stage;  // one chunk's staged queries, as the kind lays them out
    DevBuf<u64> lo, lists;        // [qt] floors | [grid][qt][kpass] the blocks' lists
    DevBuf<uint32_t> masks;       // [groups][nlist]
    DevBuf<uint32_t> offs;        // [groups][nlist] | count [groups]
    DevBuf<u32x4> work;           // [groups][tiles]
    void free() { buf_free(stage, lo, lists, masks, offs, work); }
};
// what a kind's pass launch is handed: group g of the chunk with nqt queries, kp results, grid blocks
struct IvfPass {
    int g, nqt, kp;
    unsigned grid;
    const u64* lo;          // [nqt] floors: the merge of the pass before wrote them; null in the first pass
    u64* lists;
    const u32x4* work;      // the group's entries
    const uint32_t* count;  // [1] how many
};

// mu_ held.  Enqueues only, unless rows are pending (the rebuild blocks) or a workspace has to grow.  stage(c0, m)
// -> int enqueues the staging of queries [c0, c0 + m) into w.stage; pass(IvfPass) enqueues one pass's scan.  T: a distance
template <class T, class Stage, class Pass>
int ivf_tiled_search(IvfCore& c, IvfTiledWs& w, const IvfTiledShape& s, long long nq, int k, const long long* probes_dev, int nprobe,
                     T* D_dev, long long* I_dev, int ip, hipStream_t st, Stage stage, Pass pass) {
    c.batches++;
    // a search still in flight on another stream comes first on the device: before the rebuild and before the
    // workspaces are written
    int rc = c.order.wait(st);
    if (rc) return rc;
    if ((rc = ivf_rebuild_locked(c, st, ivf_no_hook))) return rc;
    const IvfLists& inv = c.inv;
    if (inv.tiles == 0) {  // an empty index: padding, no pass
        knn_fill_launch(D_dev, I_dev, nq * k, ip, st);
        HIP_TRY(hipGetLastError());
        return ISE_OK;
    }
    const int qt = s.qt, gmax = s.chunk / qt;
    const unsigned grid = coded_grid(inv.tiles, s.tiles_per_wave, s.waves, s.blocks_per_cu, c.num_cu);
    const size_t nl = (size_t)inv.nlist;
    const hipEvent_t busy = c.order.busy();
    if ((rc = grow_after_event(w.stage, s.stage_bytes, busy))) return rc;
    if ((rc = grow_after_event(w.lo, (size_t)qt, busy))) return rc;
    if ((rc = grow_after_event(w.lists, (size_t)grid * qt * s.kpass, busy))) return rc;
    if ((rc = grow_after_event(w.masks, (size_t)gmax * nl, busy))) return rc;
    if ((rc = grow_after_event(w.offs, (size_t)gmax * nl + gmax, busy))) return rc;
    if ((rc = grow_after_event(w.work, (size_t)gmax * inv.tiles, busy))) return rc;
    CallOrder::Scope release{c.order, st};
    uint32_t* counts = w.offs.p + (size_t)gmax * nl;
    for (long long c0 = 0; c0 < nq; c0 += s.chunk) {
        // the chunk's staged queries, masks and work lists (in stream order behind the passes that read the last chunk's)
        const int m = (int)std::min<long long>(s.chunk, nq - c0);
        const int groups = (m + qt - 1) / qt;
        if ((rc = stage(c0, m))) return rc;
        HIP_TRY(ivf_work_list_launch(probes_dev + (size_t)c0 * nprobe, m, nprobe, inv.nlist, s.qshift, inv.meta, (uint32_t)inv.tiles,
                                     w.masks.p, w.offs.p, counts, w.work.p, st));
        for (int g = 0; g < groups; g++) {
            const long long q0 = c0 + (long long)g * qt;
            const int nqt = (int)std::min<long long>(qt, nq - q0);
            for (int off = 0; off < k; off += s.kpass) {
                const int kp = std::min(s.kpass, k - off);
                pass(IvfPass{g, nqt, kp, grid, off == 0 ? nullptr : w.lo.p, w.lists.p, w.work.p + (size_t)g * inv.tiles, counts + g});
                pass_merge_launch(w.lists.p, qt, s.kpass, grid, nqt, kp, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, w.lo.p, k, off, ip,
                                  st);
                c.passes++;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// the kNN arguments of an inverted-list search: the probe checks on top of the shared ones
inline int check_ivf_knn_args(const void* q, long long nq, int k, const void* probes, int nprobe, const void* D, const void* I) {
    if (nprobe < 1) return ise_fail_(ISE_E_INVALID, "nprobe must be positive");
    if (nq > 0 && (!q || !probes)) return ise_fail_(ISE_E_INVALID, "query or probe pointer is NULL");
    return check_knn_args(q, nq, k, D, I);
}

// the host form of a search: queries and probes go up in batches of 4096 at most, enqueue(q_dev, m, p_dev, D_dev,
// I_dev) ranks a batch on st, the results come back before the next one goes up.  Q: an entry of a query row of d
// entries (float, or the bytes of a bit code), DT: a distance (float, or the int of a Hamming distance)
template <class Q, class DT, class Enqueue>
int ivf_search_staged(int d, hipStream_t st, const Q* q, long long nq, int k, const int64_t* probes, int nprobe, DT* D,
                      int64_t* I, Enqueue enqueue) {
    const long long batch = std::min<long long>(nq, 4096);
    Q* q_dev = nullptr;
    DT* D_dev = nullptr;
    long long *p_dev = nullptr, *I_dev = nullptr;
    DevFreeList<4> fr{{(void**)&q_dev, (void**)&D_dev, (void**)&p_dev, (void**)&I_dev}};
    HIP_TRY(hipMalloc((void**)&q_dev, (size_t)batch * d * sizeof(Q)));
    HIP_TRY(hipMalloc((void**)&p_dev, (size_t)batch * nprobe * sizeof(long long)));
    HIP_TRY(hipMalloc((void**)&D_dev, (size_t)batch * k * sizeof(DT)));
    HIP_TRY(hipMalloc((void**)&I_dev, (size_t)batch * k * sizeof(long long)));
    for (long long i0 = 0; i0 < nq; i0 += batch) {
        const long long m = std::min<long long>(batch, nq - i0);
        HIP_TRY(hipMemcpyAsync(q_dev, q + (size_t)i0 * d, (size_t)m * d * sizeof(Q), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(p_dev, probes + (size_t)i0 * nprobe, (size_t)m * nprobe * sizeof(long long), hipMemcpyHostToDevice, st));
        const int rc = enqueue((const Q*)q_dev, m, (const long long*)p_dev, D_dev, I_dev);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(D + (size_t)i0 * k, D_dev, (size_t)m * k * sizeof(DT), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(I + (size_t)i0 * k, I_dev, (size_t)m * k * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ISE_OK;
}
