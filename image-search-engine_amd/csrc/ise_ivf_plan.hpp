// ise_ivf_plan.hpp -- the host bookkeeping of an inverted-list rebuild (ise_ivf.hip): a stable counting sort of the
// pending rows' list numbers.  Plain C++ with no device call, so a stand-alone program can run it under a sanitizer.
#pragma once
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
