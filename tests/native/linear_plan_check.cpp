// linear_plan_check.cpp -- stand-alone check of the linear transform's panel packing (csrc/ise_linear_plan.hpp), built by
// tests/test_transform.py with the host compiler under AddressSanitizer and UBSan.  For shapes ragged against the 16-wide
// output tile, the 4-deep k step and the 256-long segment it packs a matrix whose entries name their own place, and
// checks that every panel float is written once and is the entry the kernels expect there: lane l of k step t of tile
// jt holds A[16 jt + (l & 15)][4 t + (l >> 4)], or zero beyond the matrix.  Prints "ok <shapes>" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../image-search-engine_amd/csrc/ise_linear_plan.hpp"

static int fail(const char* what, int d_in, int d_out, long long at) {
    std::printf("FAIL %s at d_in=%d d_out=%d index %lld\n", what, d_in, d_out, at);
    return 1;
}

static int check(int d_in, int d_out) {
    const LinearPlan p = linear_plan(d_in, d_out);
    if (p.nseg != (d_in + 255) / 256 || p.ksteps != p.nseg * 64 || p.jtiles != (d_out + 15) / 16) return fail("plan", d_in, d_out, 0);
    if (p.ksteps * 4 < d_in || p.jtiles * 16 < d_out) return fail("cover", d_in, d_out, 0);
    std::vector<float> A((size_t)d_in * d_out);
    for (int j = 0; j < d_out; j++)
        for (int k = 0; k < d_in; k++) A[(size_t)j * d_in + k] = (float)(1 + j * 4096 + k);  // < 2^24: exact, never 0
    // exactly panel_floats() floats: the sanitizer sees a write past either end
    std::vector<float> panel(p.panel_floats(), -1.f);
    linear_pack(p, A.data(), panel.data());
    size_t nonzero = 0;
    for (int jt = 0; jt < p.jtiles; jt++)
        for (int t = 0; t < p.ksteps; t++)
            for (int l = 0; l < 64; l++) {
                const int j = jt * 16 + (l & 15), k = t * 4 + (l >> 4);
                const size_t at = ((size_t)jt * p.ksteps + t) * 64 + l;
                const float want = (j < d_out && k < d_in) ? A[(size_t)j * d_in + k] : 0.f;
                if (panel[at] != want) return fail("entry", d_in, d_out, (long long)at);
                nonzero += want != 0.f;
            }
    if (nonzero != A.size()) return fail("count", d_in, d_out, (long long)nonzero);
    for (int j = 0; j < d_out; j += (d_out > 40 ? 7 : 1))
        for (int k = 0; k < d_in; k += (d_in > 40 ? 5 : 1)) {
            const size_t at = linear_panel_index(p, j, k);
            if (at >= panel.size() || panel[at] != A[(size_t)j * d_in + k]) return fail("index", d_in, d_out, (long long)at);
        }
    return 0;
}

int main() {
    const int dins[] = {1, 3, 4, 5, 255, 256, 257, 513, 2048, 4096};
    const int douts[] = {1, 15, 16, 17, 100, 256};
    int shapes = 0;
    for (int d_in : dins)
        for (int d_out : douts) {
            if (check(d_in, d_out)) return 1;
            shapes++;
        }
    if (check(300, 4096)) return 1;
    std::printf("ok %d shapes\n", shapes + 1);
    return 0;
}
