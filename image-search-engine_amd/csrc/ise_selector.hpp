// ise_selector.hpp -- the selector object of the float and the binary index (ise_flat_sel.hip, ise_binary_scan.hip): a
// device bitmap over the rows of ONE index at ONE (ntotal, row epoch), with its census.  Host code only; the fill and
// scatter kernels are those of ise_sel_scan.hpp, the census kernel is the index kind's own (the word layouts differ)
// and comes in as the launch `census(s, stream, out4)`.  The index's lock is held by every caller that names an index.
#pragma once
#include "ise_host.hpp"
#include "ise_sel_scan.hpp"

struct SelectorBase {
    const void* owner = nullptr;  // the index handle it was made from
    int device = 0;
    uint32_t* bits = nullptr;
    long long nwords = 0;  // allocated uint32 words (the index kind's rule)
    long long ntotal = 0;
    unsigned long long epoch = 0;
    long long count = 0, r0 = 0, r1 = 0, tiles = 0;  // selected rows, window [r0, r1), non-empty tiles
};

// the float index's (ise_flat_range.hip, ise_flat_sel.hip).  bits: ceil(ntotal / 32) words + zero padding (pad rows of
// the last tile and word: zero bits)
struct ise_selector : SelectorBase {};

// the index a selector is made for, as it stands
struct SelectorFor {
    const void* owner;
    int device;
    long long n;
    unsigned long long row_epoch;
    hipStream_t stream;
    long long nwords;
};

struct DevFree {  // a device allocation of the call's duration
    void* p = nullptr;
    ~DevFree() { if (p) (void)hipFree(p); }
};

template <class S>
void selector_free(S* s) {
    if (s->bits) (void)hipFree(s->bits);  // waits for the device: a masked pass in flight is through with the bitmap
    delete s;
}

inline int selector_fill_range(SelectorBase* s, hipStream_t st, long long a, long long b) {
    hipLaunchKernelGGL(sel_fill_range_kernel, dim3((unsigned)((s->nwords + 255) / 256)), dim3(256), 0, st, s->bits,
                       s->nwords, a, std::max(a, b));
    return ISE_OK;
}

// the fill runs on the device: nothing (invert: every row), then the ids are scattered in -- only they travel.
// ids_dev lives until the caller has synchronised (the census does)
inline int selector_scatter_ids(SelectorBase* s, hipStream_t st, const int64_t* ids, long long n_ids, int invert,
                                DevFree* ids_dev) {
    selector_fill_range(s, st, 0ll, invert ? s->ntotal : 0ll);
    if (n_ids > 0) {
        HIP_TRY(hipMalloc(&ids_dev->p, (size_t)n_ids * sizeof(long long)));
        HIP_TRY(hipMemcpyAsync(ids_dev->p, ids, (size_t)n_ids * sizeof(long long), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(sel_scatter_ids_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, st, s->bits,
                           (const long long*)ids_dev->p, n_ids, s->ntotal, invert ? 0 : 1);
    }
    HIP_TRY(hipGetLastError());
    return ISE_OK;
}

// n_words = ceil(ntotal / 32) words from the host, zeros behind them
inline int selector_copy_bitmap(SelectorBase* s, hipStream_t st, const uint32_t* words, long long n_words) {
    HIP_TRY(hipMemsetAsync(s->bits + n_words, 0, (size_t)(s->nwords - n_words) * sizeof(uint32_t), st));
    if (n_words > 0) HIP_TRY(hipMemcpyAsync(s->bits, words, (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    return ISE_OK;
}

// clears bits at or beyond ntotal, then count / window / non-empty tiles on the device (blocks)
template <class Census>
int selector_census(SelectorBase* s, hipStream_t st, Census census) {
    unsigned long long* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, 4 * sizeof(unsigned long long)));
    DevFree fr{dev};
    const unsigned long long init[4] = {0ull, 0ull, ~0ull, 0ull};
    unsigned long long got[4];
    HIP_TRY(hipMemcpyAsync(dev, init, sizeof(init), hipMemcpyHostToDevice, st));
    census(s, st, dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(got, dev, sizeof(got), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s->count = (long long)got[0];
    s->tiles = (long long)got[1];
    s->r0 = got[0] ? (long long)got[2] : 0;
    s->r1 = got[0] ? (long long)got[3] : 0;
    return ISE_OK;
}

// a new selector of type S for ix: allocate, fill(s) -> rc, census; freed again if any step fails
template <class S, class Fill, class Census>
int selector_create(const SelectorFor& ix, Fill fill, Census census, S** out) {
    S* s = new (std::nothrow) S;
    if (!s) return ise_fail_(ISE_E_NOMEM, "selector: host allocation failed");
    s->owner = ix.owner;
    s->device = ix.device;
    s->ntotal = ix.n;
    s->epoch = ix.row_epoch;
    s->nwords = ix.nwords;
    const hipError_t e = hipMalloc((void**)&s->bits, (size_t)s->nwords * sizeof(uint32_t));
    if (e != hipSuccess) {
        delete s;
        return ise_fail_(e == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP, std::string("selector bitmap: ") + hipGetErrorString(e));
    }
    int rc = fill(s);
    if (!rc) rc = selector_census(s, ix.stream, census);
    if (rc) {
        selector_free(s);
        return rc;
    }
    *out = s;
    return ISE_OK;
}

inline int selector_info(const SelectorBase* sel, int64_t* out5) {
    if (!sel || !out5) return ise_fail_(ISE_E_INVALID, "NULL argument");
    out5[0] = sel->ntotal;
    out5[1] = sel->count;
    out5[2] = sel->r0;
    out5[3] = sel->r1;
    out5[4] = sel->tiles;
    return ISE_OK;
}
