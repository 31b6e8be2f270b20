// ise_remove_plan.hpp -- the host planning of remove_ids for the float and the binary index (ise_knn.hip,
// ise_binary_scan.hip; kernels in ise_remove.hpp): ids -> runs -> the tables the source-map kernel reads, and the
// slab size.  Plain C++ with no device call, so a stand-alone program can run it under a sanitizer
// (tests/native/remove_plan_check.cpp).  Everything that allocates may throw std::bad_alloc: the callers catch it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct RemoveRun {
    long long start, len;
};

// the ids as passed -> the non-negative ones, sorted, each once (needs no index state: runs before the lock is taken)
inline std::vector<long long> remove_plan_ids(const int64_t* ids, long long n_ids) {
    std::vector<long long> v;
    v.reserve((size_t)n_ids);
    for (long long i = 0; i < n_ids; i++)
        if (ids[i] >= 0) v.push_back(ids[i]);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

// sorted unique ids -> the rows of [0, ntotal) among them as runs: sorted, disjoint, non-adjacent, non-empty.
// Returns the number of rows removed
inline long long remove_plan_runs(const std::vector<long long>& sorted_ids, long long ntotal, std::vector<RemoveRun>* runs) {
    long long removed = 0;
    runs->clear();
    for (long long id : sorted_ids) {
        if (id >= ntotal) break;  // sorted: the rest does not exist either
        if (!runs->empty() && runs->back().start + runs->back().len == id) runs->back().len++;
        else runs->push_back(RemoveRun{id, 1});
        removed++;
    }
    return removed;
}

// runs -> g[t], the destination row at which run t bites, and cend[t], the rows removed up to and including run t:
// destination row j takes source row j + cend[t] for the last t with g[t] <= j (j itself if there is none)
inline void remove_plan_tables(const std::vector<RemoveRun>& runs, std::vector<uint32_t>* g, std::vector<uint32_t>* cend) {
    g->resize(runs.size());
    cend->resize(runs.size());
    long long c = 0;
    for (size_t t = 0; t < runs.size(); t++) {
        (*g)[t] = (uint32_t)(runs[t].start - c);
        c += runs[t].len;
        (*cend)[t] = (uint32_t)c;
    }
}

// rows per slab of the in-place compaction: $ISE_REMOVE_SLAB_ROWS (knob), or 256 MiB of rows when it is <= 0; a
// slab's units (what one kernel index counts: units_per_row each) stay below 2^31 whatever the knob says; never more
// than the moved >= 1 rows there are.  At least 1
inline long long remove_plan_slab_rows(long long knob, long long row_bytes, long long units_per_row, long long moved) {
    long long slab = knob;
    if (slab <= 0) slab = std::max<long long>(1, (256ll << 20) / row_bytes);
    slab = std::min(slab, std::max<long long>(1, (1ll << 31) / units_per_row));
    return std::min(slab, moved);
}
