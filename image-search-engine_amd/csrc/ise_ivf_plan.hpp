// ise_ivf_plan.hpp -- the host bookkeeping of the inverted lists (ise_ivf.hip, ise_ivfsq.hip, ise_binary_ivf.hip; their device side is
// ise_ivf_lists.hpp): the plan of a rebuild (a stable counting sort of the pending rows' list numbers), the table the
// kernels read built from it, the check of list numbers, and the counts a handle keeps between rebuilds.  Plain C++
// with no device call, so a stand-alone program can run it under a sanitizer.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct IvfPlan {
    std::vector<long long> size;      // [nlist] rows per list after the rebuild
    std::vector<uint32_t> tile0;      // [nlist + 1] first tile of every list, tile0[nlist] = tiles in all
    std::vector<uint32_t> tile_list;  // [tiles] the list of every tile
    std::vector<uint32_t> dest;       // [m] slot of pending row i
};

// old_size [nlist]: rows already in the lists (they keep their positions within their list); pend_list [m]: list of
// pending row i, every entry in [0, nlist).  Pending rows go behind the old rows of their list in the order they
// came (stable), so ids ascend inside every list.  tile_rows: rows of a tile (16: the float32 lists; 64: the byte lists of
// ise_ivfsq.hip).  False if the slots do not fit 32 bits.
inline bool ivf_plan_rebuild(const std::vector<long long>& old_size, const int32_t* pend_list, long long m, IvfPlan* out,
                             int tile_rows = 16) {
    const size_t nlist = old_size.size();
    const unsigned long long tr = (unsigned long long)tile_rows;
    out->size = old_size;
    for (long long i = 0; i < m; i++) out->size[(size_t)pend_list[i]]++;
    out->tile0.assign(nlist + 1, 0u);
    unsigned long long tiles = 0;
    for (size_t l = 0; l < nlist; l++) {
        out->tile0[l] = (uint32_t)tiles;
        tiles += ((unsigned long long)out->size[l] + tr - 1) / tr;
        if (tiles * tr >= (1ull << 32)) return false;
    }
    out->tile0[nlist] = (uint32_t)tiles;
    out->tile_list.resize((size_t)tiles);
    for (size_t l = 0; l < nlist; l++)
        for (uint32_t t = out->tile0[l]; t < out->tile0[l + 1]; t++) out->tile_list[t] = (uint32_t)l;
    std::vector<long long> next(old_size);  // next free position within each list
    out->dest.resize((size_t)m);
    for (long long i = 0; i < m; i++) {
        const size_t l = (size_t)pend_list[i];
        out->dest[(size_t)i] = (uint32_t)((unsigned long long)out->tile0[l] * tr + (unsigned long long)next[l]++);
    }
    return true;
}

// the table the kernels read, the ONE place that knows its layout: list_tile0 [nlist + 1] | list_size [nlist] |
// tile_list [tiles]
inline size_t ivf_meta_size_at(size_t nlist) { return nlist + 1; }
inline size_t ivf_meta_tile_list_at(size_t nlist) { return 2 * nlist + 1; }
inline std::vector<uint32_t> ivf_plan_meta(const IvfPlan& pl) {
    const size_t nlist = pl.size.size();
    std::vector<uint32_t> meta(ivf_meta_tile_list_at(nlist) + pl.tile_list.size());
    std::copy(pl.tile0.begin(), pl.tile0.end(), meta.begin());
    for (size_t l = 0; l < nlist; l++) meta[ivf_meta_size_at(nlist) + l] = (uint32_t)pl.size[l];
    std::copy(pl.tile_list.begin(), pl.tile_list.end(), meta.begin() + ivf_meta_tile_list_at(nlist));
    return meta;
}

// the first row whose list number is not one of the nlist lists, or -1
inline long long ivf_first_bad_list(const int64_t* list_no, long long n, int nlist) {
    for (long long i = 0; i < n; i++)
        if (list_no[i] < 0 || list_no[i] >= nlist) return i;
    return -1;
}

// what a handle knows of its lists on the host (its mutex held)
struct IvfBook {
    int nlist = 0;
    long long n = 0;      // rows in all, the pending ones included
    long long tiles = 0;  // of the sorted array
    std::vector<long long> size;      // [nlist] rows per list in the sorted array
    std::vector<long long> size_all;  // ... with the pending rows
    std::vector<uint32_t> tile0;      // [nlist + 1] first tile of every list in the sorted array
    // rows added since the last rebuild, in insertion order
    long long pend_n = 0;
    std::vector<int32_t> pend_list;

    // no rows, sorted or pending
    void clear() {
        n = tiles = pend_n = 0;
        pend_list.clear();
        size.assign((size_t)nlist, 0);
        size_all.assign((size_t)nlist, 0);
        tile0.assign((size_t)nlist + 1, 0u);
    }
    // m more rows are in the pending buffer (list numbers checked): book them
    void add(const int64_t* list_no, long long m) {
        pend_list.reserve(pend_list.size() + (size_t)m);
        for (long long i = 0; i < m; i++) {
            pend_list.push_back((int32_t)list_no[i]);
            size_all[(size_t)list_no[i]]++;
        }
        pend_n += m;
        n += m;
    }
    bool plan(IvfPlan* pl, int tile_rows) const { return ivf_plan_rebuild(size, pend_list.data(), pend_n, pl, tile_rows); }
    // the arrays of a finished plan are in place: nothing is pending any more
    void take_over(const IvfPlan& pl) {
        pend_n = 0;
        pend_list.clear();
        pend_list.shrink_to_fit();
        tiles = pl.tile0[size.size()];
        size = pl.size;
        tile0 = pl.tile0;
    }
};
