// The checks of what csrc/ise_ivf_plan.hpp holds beside the plan itself -- the table the kernels read, the check of
// list numbers, the counts a handle keeps -- shared by ivf_plan_check.cpp and ivfsq_plan_check.cpp.  Every expected
// value is written out by hand.  Returns 0, or the number of the check that failed.
#pragma once
#include <cstdio>

#include "../../image-search-engine_amd/csrc/ise_ivf_plan.hpp"

// rows: rows of a tile
static int ivf_book_check_rows(int rows) {
    // ---- the table: nlist = 1
    {
        IvfPlan pl;
        const std::vector<int32_t> pend((size_t)rows + 1, 0);  // one row more than a tile: two tiles
        if (!ivf_plan_rebuild(std::vector<long long>{0}, pend.data(), (long long)pend.size(), &pl, rows)) return 1;
        const std::vector<uint32_t> want = {0, 2, (uint32_t)rows + 1, 0, 0};  // tile0 [2] | size [1] | tile_list [2]
        if (ivf_plan_meta(pl) != want) return 2;
        if (ivf_meta_size_at(1) != 2 || ivf_meta_tile_list_at(1) != 3) return 3;
    }
    // ---- the table: an empty list in the middle, a list of exactly one full tile, a list of one row
    {
        IvfPlan pl;
        std::vector<int32_t> pend((size_t)rows, 0);  // list 0: exactly one tile; list 1: none; list 2: one row
        pend.push_back(2);
        if (!ivf_plan_rebuild(std::vector<long long>{0, 0, 0}, pend.data(), (long long)pend.size(), &pl, rows)) return 4;
        // tile0 [4] | size [3] | tile_list [2]: the empty list starts where the next one does and owns no tile
        const std::vector<uint32_t> want = {0, 1, 1, 2, (uint32_t)rows, 0, 1, 0, 2};
        if (ivf_plan_meta(pl) != want) return 5;
        if (ivf_meta_size_at(3) != 4 || ivf_meta_tile_list_at(3) != 7) return 6;
        if (pl.dest[(size_t)rows] != (uint32_t)rows) return 7;  // list 2's row: the first slot of tile 1
    }
    // ---- the list check: the first offender, for -1 and for nlist
    {
        const int64_t ok[4] = {0, 4, 2, 4}, neg[4] = {0, 4, -1, 5}, big[4] = {0, 5, -1, 2}, last[4] = {0, 1, 2, 5};
        if (ivf_first_bad_list(ok, 4, 5) != -1) return 8;
        if (ivf_first_bad_list(neg, 4, 5) != 2) return 9;    // -1 before the 5 behind it
        if (ivf_first_bad_list(big, 4, 5) != 1) return 10;   // nlist itself is outside
        if (ivf_first_bad_list(last, 4, 5) != 3) return 11;
        if (ivf_first_bad_list(neg, 2, 5) != -1 || ivf_first_bad_list(neg, 0, 5) != -1) return 12;  // only the rows asked for
    }
    // ---- the counts: two adds and a take-over
    {
        IvfBook b;
        b.nlist = 3;
        b.clear();
        if (b.n != 0 || b.tiles != 0 || b.pend_n != 0 || b.size != std::vector<long long>{0, 0, 0} ||
            b.size_all != b.size || b.tile0 != std::vector<uint32_t>{0, 0, 0, 0})
            return 13;
        const int64_t first[3] = {2, 0, 2}, second[2] = {0, 2};
        b.add(first, 3);
        if (b.n != 3 || b.pend_n != 3 || b.size_all != std::vector<long long>{1, 0, 2} || b.size != std::vector<long long>{0, 0, 0})
            return 14;
        b.add(second, 2);
        if (b.n != 5 || b.pend_n != 5 || b.size_all != std::vector<long long>{2, 0, 3} ||
            b.pend_list != std::vector<int32_t>{2, 0, 2, 0, 2} || b.tiles != 0)
            return 15;
        IvfPlan pl;
        if (!b.plan(&pl, rows)) return 16;
        // insertion order inside every list: list 0 gets rows 1, 3; list 2 gets rows 0, 2, 4 in the tile behind
        const uint32_t r = (uint32_t)rows;
        if (pl.dest != std::vector<uint32_t>{r, 0, r + 1, 1, r + 2}) return 17;
        b.take_over(pl);
        if (b.n != 5 || b.pend_n != 0 || !b.pend_list.empty() || b.tiles != 2 || b.size != std::vector<long long>{2, 0, 3} ||
            b.size_all != b.size || b.tile0 != std::vector<uint32_t>{0, 1, 1, 2})
            return 18;
        // a third add lands behind the rows that are now sorted
        const int64_t third[1] = {1};
        b.add(third, 1);
        if (!b.plan(&pl, rows) || pl.dest != std::vector<uint32_t>{r} || pl.tile0 != std::vector<uint32_t>{0, 1, 2, 3} ||
            b.n != 6 || b.size_all != std::vector<long long>{2, 1, 3})
            return 19;
        b.clear();
        if (b.n != 0 || b.nlist != 3 || !b.pend_list.empty() || b.size_all != std::vector<long long>{0, 0, 0}) return 20;
    }
    return 0;
}

// both tile sizes the library uses; prints the failure
static bool ivf_book_check() {
    for (int rows : {16, 64}) {
        const int rc = ivf_book_check_rows(rows);
        if (rc) {
            std::printf("FAIL bookkeeping, %d-row tiles: check %d\n", rows, rc);
            return false;
        }
    }
    return true;
}
