// ise_ivf_lists.hpp -- the device side of the inverted lists' bookkeeping, shared by the float32 lists (ise_ivf.hip), the
// 8-bit lists (ise_ivfsq.hip) and the lists over bit codes (ise_binary_ivf.hip): the ids and the table of the sorted
// array beside the host's counts (ise_ivf_plan.hpp), and the staged host form of a search.  What a row IS (float32 rows
// and norms, codes and row terms, or bit codes alone) stays with the index kind: its rebuild allocates and fills the
// payload, this struct's begin_rebuild / finish_rebuild do the ids, the table and the counts around it.  Host code (the
// handle's mutex is held), and the one kernel that reads nothing of a row: the probe table's masks.
#pragma once
#include "ise_host.hpp"
#include "ise_ivf_plan.hpp"

// probes [nq][nprobe] (int64) -> masks [groups of 1 << qshift queries][nlist], bit c: query (group << qshift) + c probes
// the list; the masks are zero on entry.  -1 and out-of-range entries set nothing, a duplicate sets its bit twice
static __global__ __launch_bounds__(256) void ivf_mask_kernel(const long long* probes, long long total, int nprobe, int nlist,
                                                              int qshift, uint32_t* masks) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long l = probes[i];
    if (l < 0 || l >= nlist) return;
    const long long q = i / nprobe;
    atomicOr(masks + (size_t)(q >> qshift) * nlist + l, 1u << (q & ((1 << qshift) - 1)));
}

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
