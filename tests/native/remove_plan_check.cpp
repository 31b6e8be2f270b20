// Stand-alone check of the removal planning (csrc/ise_remove_plan.hpp) against a brute-force erase on a vector of row
// numbers.  Built and run by tests/test_remove_ids.py under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <random>
#include <set>

#include "../../image-search-engine_amd/csrc/ise_remove_plan.hpp"

// 0, or the number of the check that failed
static int check(long long n, const std::vector<int64_t>& ids) {
    // brute force: erase every named row of [0, n), each once
    std::vector<long long> want((size_t)n);
    for (long long i = 0; i < n; i++) want[(size_t)i] = i;
    const std::set<int64_t> named(ids.begin(), ids.end());
    long long want_removed = 0;
    for (auto it = named.rbegin(); it != named.rend(); ++it)
        if (*it >= 0 && *it < n) {
            want.erase(want.begin() + *it);
            want_removed++;
        }

    const std::vector<long long> v = remove_plan_ids(ids.data(), (long long)ids.size());
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i] < 0 || !named.count(v[i])) return 1;
        if (i && v[i - 1] >= v[i]) return 2;  // sorted, each once
    }
    for (int64_t id : named)
        if (id >= 0 && !std::binary_search(v.begin(), v.end(), (long long)id)) return 3;

    std::vector<RemoveRun> runs{RemoveRun{-1, -1}};  // whatever it held goes
    const long long removed = remove_plan_runs(v, n, &runs);
    if (removed != want_removed) return 4;
    long long sum = 0;
    for (size_t t = 0; t < runs.size(); t++) {
        if (runs[t].len <= 0 || runs[t].start < 0 || runs[t].start + runs[t].len > n) return 5;  // non-empty, inside
        if (t && runs[t - 1].start + runs[t - 1].len >= runs[t].start) return 6;  // sorted, disjoint, never adjacent
        for (long long i = runs[t].start; i < runs[t].start + runs[t].len; i++)
            if (!named.count(i)) return 7;
        sum += runs[t].len;
    }
    if (sum != removed) return 8;

    std::vector<uint32_t> g{7u}, cend;
    remove_plan_tables(runs, &g, &cend);
    if (g.size() != runs.size() || cend.size() != runs.size()) return 9;
    for (size_t t = 1; t < g.size(); t++)
        if (g[t - 1] >= g[t] || cend[t - 1] >= cend[t]) return 10;  // the source-map kernel bisects g
    if (!cend.empty() && (long long)cend.back() != removed) return 11;
    // src(j) = j + cend[t] for the last run with g[t] <= j
    if ((long long)want.size() != n - removed) return 12;
    for (long long j = 0; j < n - removed; j++) {
        long long src = j;
        for (size_t t = 0; t < g.size(); t++)
            if ((long long)g[t] <= j) src = j + (long long)cend[t];
        if (src != want[(size_t)j]) return 13;
    }
    return 0;
}

static int check_slab() {
    const long long MiB256 = 256ll << 20, big = 1ll << 40;
    // knob <= 0: 256 MiB of rows, for the float index (16-byte units) and the binary one (max(1, ws / 2) units of rows of ws words)
    for (long long knob : {0ll, -1ll, -1000ll}) {
        if (remove_plan_slab_rows(knob, 2048, 128, big) != MiB256 / 2048) return 1;
        if (remove_plan_slab_rows(knob, 64, 4, big) != MiB256 / 64) return 2;
        if (remove_plan_slab_rows(knob, 8, 1, big) != MiB256 / 8) return 3;
        if (remove_plan_slab_rows(knob, MiB256 + 16, (MiB256 + 16) / 16, big) != 1) return 4;  // a row beyond 256 MiB: one row
        if (remove_plan_slab_rows(knob, 3 * MiB256, 3 * MiB256 / 16, 1) != 1) return 5;
    }
    // a knob that would take a slab's units to 2^31 or past it
    if (remove_plan_slab_rows(1ll << 40, 2048, 128, big) != (1ll << 31) / 128) return 6;
    if (remove_plan_slab_rows((1ll << 31) / 128 + 1, 2048, 128, big) != (1ll << 31) / 128) return 7;
    if (remove_plan_slab_rows((1ll << 31) / 128 - 1, 2048, 128, big) != (1ll << 31) / 128 - 1) return 8;
    if (remove_plan_slab_rows(1ll << 40, 8, 1, big) != 1ll << 31) return 9;
    if (remove_plan_slab_rows(5, 1ll << 36, 1ll << 32, big) != 1) return 10;  // more units in ONE row than 2^31: one row
    // slab > moved
    if (remove_plan_slab_rows(1000, 2048, 128, 7) != 7) return 11;
    if (remove_plan_slab_rows(0, 2048, 128, 1) != 1) return 12;
    if (remove_plan_slab_rows(1ll << 40, 8, 1, 3) != 3) return 13;
    // ... and a knob inside every clamp is taken as it is
    if (remove_plan_slab_rows(48, 2048, 128, 1000) != 48) return 14;
    if (remove_plan_slab_rows(1, 2048, 128, 1000) != 1) return 15;
    return 0;
}

int main() {
    int cases = 0;
    auto run = [&](long long n, const std::vector<int64_t>& ids, const char* what) {
        const int rc = check(n, ids);
        if (rc) std::printf("FAIL n=%lld %s (%zu ids): check %d\n", n, what, ids.size(), rc);
        cases++;
        return rc == 0;
    };
    for (long long n : {1ll, 2ll, 17ll, 100ll}) {
        std::vector<int64_t> all, but_first;
        for (long long i = 0; i < n; i++) all.push_back(i);
        for (long long i = 1; i < n; i++) but_first.push_back(i);
        if (!run(n, {}, "empty") || !run(n, {0}, "first") || !run(n, {n - 1}, "last") || !run(n, all, "all") ||
            !run(n, but_first, "all but the first"))
            return 1;
        if (!run(n, {0, 0, n - 1, 0, n - 1}, "duplicates") || !run(n, {-1, -7, 0, INT64_MIN}, "negative ids") ||
            !run(n, {-5, -5}, "only negative ids") || !run(n, {n, n + 1, n - 1, 1ll << 40, INT64_MAX}, "ids >= n") ||
            !run(n, {n, n + 3}, "only ids >= n") || !run(n, {n - 1, 0, n / 2, n / 3, n - 1, -2, n + 9}, "unsorted"))
            return 1;
    }
    {   // adjacent ids merge into one run, in whatever order they come
        std::vector<RemoveRun> runs;
        const std::vector<int64_t> ids{12, 10, 11, 13, 40, 39, 50, 13};
        if (remove_plan_runs(remove_plan_ids(ids.data(), (long long)ids.size()), 100, &runs) != 7 || runs.size() != 3 ||
            runs[0].start != 10 || runs[0].len != 4 || runs[1].start != 39 || runs[1].len != 2 || runs[2].start != 50 ||
            runs[2].len != 1 || !run(100, ids, "adjacent ids")) {
            std::printf("FAIL: adjacent ids did not merge into one run\n");
            return 1;
        }
        // the first id >= ntotal ends the plan: the run before it is not extended past the index
        if (remove_plan_runs({97, 98, 99, 100, 101}, 100, &runs) != 3 || runs.size() != 1 || runs[0].len != 3) {
            std::printf("FAIL: a run crossed ntotal\n");
            return 1;
        }
    }
    std::mt19937 rng(11);
    for (int rep = 0; rep < 400; rep++) {
        const long long n = 1 + (long long)(rng() % 199);
        const unsigned dens = 1 + rng() % 100;  // percent of the rows named
        std::vector<int64_t> ids;
        for (long long i = 0; i < n; i++)
            if (rng() % 100 < dens) ids.push_back(i);
        if (rng() % 3 == 0) {  // a long run on top
            const long long a = (long long)(rng() % (unsigned)n), len = 2 + (long long)(rng() % 40);
            for (long long i = a; i < a + len; i++) ids.push_back(i);  // may pass n
        }
        for (unsigned i = rng() % 4; i > 0; i--) ids.push_back(-(int64_t)(rng() % 50) - 1);
        for (unsigned i = rng() % 4; i > 0; i--) ids.push_back(n + (int64_t)(rng() % 50));
        for (unsigned i = rng() % 4; i > 0 && !ids.empty(); i--) ids.push_back(ids[rng() % ids.size()]);
        std::shuffle(ids.begin(), ids.end(), rng);
        if (!run(n, ids, "random")) return 1;
    }
    if (const int rc = check_slab()) {
        std::printf("FAIL slab rule: check %d\n", rc);
        return 1;
    }
    std::printf("ok %d cases\n", cases);
    return 0;
}
