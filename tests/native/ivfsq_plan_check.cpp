// Stand-alone check of the rebuild bookkeeping (csrc/ise_ivf_plan.hpp) with the 64-row tiles of the inverted lists
// over 8-bit rows (csrc/ise_ivfsq.hip): the list sizes at a tile's edge, stable order, old rows keeping their
// positions, the 2^32 slot refusal, the default of 16 rows left as it was, and the table, the list check and the counts
// (ivf_book_check.hpp).  Built and run by tests/test_ivfsq.py under the host sanitizers.
#include <algorithm>
#include <cstdio>
#include <random>

#include "../../image-search-engine_amd/csrc/ise_ivf_plan.hpp"
#include "ivf_book_check.hpp"

static const int ROWS = 64;

static int check(const std::vector<long long>& old_size, const std::vector<int32_t>& pend) {
    IvfPlan pl;
    if (!ivf_plan_rebuild(old_size, pend.data(), (long long)pend.size(), &pl, ROWS)) return 1;
    const size_t nlist = old_size.size();
    if (pl.size.size() != nlist || pl.tile0.size() != nlist + 1 || pl.dest.size() != pend.size()) return 2;
    if (pl.tile0[0] != 0) return 3;
    for (size_t l = 0; l < nlist; l++) {
        const long long cnt = old_size[l] + std::count(pend.begin(), pend.end(), (int32_t)l);
        if (pl.size[l] != cnt) return 4;
        if (pl.tile0[l + 1] - pl.tile0[l] != (uint32_t)((cnt + ROWS - 1) / ROWS)) return 5;  // every list on a tile boundary
        for (uint32_t t = pl.tile0[l]; t < pl.tile0[l + 1]; t++)
            if (pl.tile_list[t] != l) return 6;
    }
    if (pl.tile_list.size() != pl.tile0[nlist]) return 7;
    // old rows keep positions [0, old_size) of their list; pending row i sits right behind the earlier rows of its list
    std::vector<char> taken((size_t)pl.tile0[nlist] * ROWS, 0);
    for (size_t l = 0; l < nlist; l++)
        for (long long r = 0; r < old_size[l]; r++) taken[(size_t)pl.tile0[l] * ROWS + (size_t)r] = 1;
    std::vector<long long> next(old_size);
    for (size_t i = 0; i < pend.size(); i++) {
        const size_t l = (size_t)pend[i];
        const uint32_t want = pl.tile0[l] * ROWS + (uint32_t)next[l]++;
        if (pl.dest[i] != want || want >= taken.size() || taken[want]) return 8;
        taken[want] = 1;
    }
    return 0;
}

int main() {
    int cases = 0;
    // the sizes at a tile's edge, as old rows, as pending rows and as both
    const std::vector<long long> edge = {0, 1, 63, 64, 65};
    for (int mode = 0; mode < 3; mode++) {
        std::vector<long long> old_size(edge.size(), 0);
        std::vector<int32_t> pend;
        for (size_t l = 0; l < edge.size(); l++) {
            const long long old_part = mode == 0 ? edge[l] : mode == 1 ? 0 : edge[l] / 2;
            old_size[l] = old_part;
            for (long long r = old_part; r < edge[l]; r++) pend.push_back((int32_t)l);
        }
        std::mt19937 sh(3 + mode);
        std::shuffle(pend.begin(), pend.end(), sh);
        const int rc = check(old_size, pend);
        if (rc) {
            std::printf("FAIL edge sizes mode=%d: check %d\n", mode, rc);
            return 1;
        }
        IvfPlan pl;
        ivf_plan_rebuild(old_size, pend.data(), (long long)pend.size(), &pl, ROWS);
        const uint32_t want[6] = {0, 0, 1, 2, 3, 5};
        for (int l = 0; l < 6; l++)
            if (pl.tile0[(size_t)l] != want[l]) {
                std::printf("FAIL edge sizes mode=%d: tile0[%d] = %u\n", mode, l, pl.tile0[(size_t)l]);
                return 1;
            }
        cases++;
    }
    std::mt19937 rng(7);
    for (int nlist : {1, 2, 7, 64, 1000})
        for (int m : {0, 1, 63, 64, 65, 600, 5000})
            for (int rep = 0; rep < 3; rep++) {
                std::vector<long long> old_size((size_t)nlist);
                for (auto& s : old_size) s = rep == 0 ? 0 : (long long)(rng() % 150);
                std::vector<int32_t> pend((size_t)m);
                for (auto& l : pend) l = (int32_t)(rng() % (unsigned)std::max(1, rep == 2 ? nlist / 2 : nlist));
                const int rc = check(old_size, pend);
                if (rc) {
                    std::printf("FAIL nlist=%d m=%d rep=%d: check %d\n", nlist, m, rep, rc);
                    return 1;
                }
                cases++;
            }
    // slots that do not fit 32 bits are refused; one tile less is accepted
    IvfPlan pl;
    if (ivf_plan_rebuild(std::vector<long long>{(1ll << 32) - 8}, nullptr, 0, &pl, ROWS)) {
        std::printf("FAIL: 2^32 slots accepted\n");
        return 1;
    }
    if (!ivf_plan_rebuild(std::vector<long long>{(1ll << 32) - 64}, nullptr, 0, &pl, ROWS) || pl.tile0[1] != (1u << 26) - 1) {
        std::printf("FAIL: 2^32 - 64 slots refused\n");
        return 1;
    }
    // the default is the float32 lists' 16 rows
    if (!ivf_plan_rebuild(std::vector<long long>{17, 0, 16}, nullptr, 0, &pl) || pl.tile0[1] != 2 || pl.tile0[3] != 3) {
        std::printf("FAIL: the default tile is not 16 rows\n");
        return 1;
    }
    // the table, the list check and the counts (ivf_book_check.hpp)
    if (!ivf_book_check()) return 1;
    cases++;
    std::printf("ok %d cases\n", cases);
    return 0;
}
