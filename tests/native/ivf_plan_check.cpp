// Stand-alone check of the inverted lists' rebuild bookkeeping (csrc/ise_ivf_plan.hpp): random cases against a
// naive stable grouping, then the table, the list check and the counts against values written out by hand
// (ivf_book_check.hpp).  Built and run by tests/test_ivf.py, with the host sanitizers where the compiler has them.
#include <algorithm>
#include <cstdio>
#include <random>

#include "../../image-search-engine_amd/csrc/ise_ivf_plan.hpp"
#include "ivf_book_check.hpp"

static int check(const std::vector<long long>& old_size, const std::vector<int32_t>& pend) {
    IvfPlan pl;
    if (!ivf_plan_rebuild(old_size, pend.data(), (long long)pend.size(), &pl)) return 1;
    const size_t nlist = old_size.size();
    if (pl.size.size() != nlist || pl.tile0.size() != nlist + 1 || pl.dest.size() != pend.size()) return 2;
    if (pl.tile0[0] != 0) return 3;
    std::vector<long long> next(old_size);
    for (size_t l = 0; l < nlist; l++) {
        long long cnt = old_size[l] + std::count(pend.begin(), pend.end(), (int32_t)l);
        if (pl.size[l] != cnt) return 4;
        if (pl.tile0[l + 1] - pl.tile0[l] != (uint32_t)((cnt + 15) / 16)) return 5;  // every list on a tile boundary
        for (uint32_t t = pl.tile0[l]; t < pl.tile0[l + 1]; t++)
            if (pl.tile_list[t] != l) return 6;
    }
    if (pl.tile_list.size() != pl.tile0[nlist]) return 7;
    std::vector<char> taken((size_t)pl.tile0[nlist] * 16, 0);
    for (size_t i = 0; i < pend.size(); i++) {  // stable: row i sits right behind the earlier rows of its list
        const size_t l = (size_t)pend[i];
        const uint32_t want = pl.tile0[l] * 16 + (uint32_t)next[l]++;
        if (pl.dest[i] != want || want >= taken.size() || taken[want]) return 8;
        taken[want] = 1;
    }
    return 0;
}

int main() {
    std::mt19937 rng(7);
    int cases = 0;
    for (int nlist : {1, 2, 7, 64, 1000})
        for (int m : {0, 1, 15, 16, 17, 600, 5000})
            for (int rep = 0; rep < 3; rep++) {
                std::vector<long long> old_size((size_t)nlist);
                for (auto& s : old_size) s = rep == 0 ? 0 : (long long)(rng() % 40);
                std::vector<int32_t> pend((size_t)m);
                for (auto& l : pend) l = (int32_t)(rng() % (unsigned)std::max(1, rep == 2 ? nlist / 2 : nlist));
                const int rc = check(old_size, pend);
                if (rc) {
                    std::printf("FAIL nlist=%d m=%d rep=%d: check %d\n", nlist, m, rep, rc);
                    return 1;
                }
                cases++;
            }
    // slots that do not fit 32 bits are refused
    IvfPlan pl;
    if (ivf_plan_rebuild(std::vector<long long>{(1ll << 32) - 8}, nullptr, 0, &pl)) {
        std::printf("FAIL: 2^32 slots accepted\n");
        return 1;
    }
    // the table, the list check and the counts (ivf_book_check.hpp)
    if (!ivf_book_check()) return 1;
    cases++;
    std::printf("ok %d cases\n", cases);
    return 0;
}
