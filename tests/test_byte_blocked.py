"""CPU tests: the address map of the tile-blocked byte shadow rows (csrc/ise_byte_layout.hpp).

xq8 is [cap / 16 tiles][dpb / 64 k-steps s][4 k-groups g][16 rows r][16 B]: unit u of row i (its columns 16u .. 16u +
15) is unit (i / 16) * 16 * upr + (u / 4) * 64 + (u % 4) * 16 + i % 16.  The numpy restatement below is checked for
what the scan relies on, and the header itself is compiled on the host and compared with it entry by entry."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPRS = (4, 8, 12, 32, 64)  # dpb 64 .. 1024
TILES = (1, 2, 5)


def unit_index(row, u, upr):
    row, u = np.asarray(row, np.int64), np.asarray(u, np.int64)
    return (row // 16) * 16 * upr + (u // 4) * 64 + (u % 4) * 16 + row % 16


def table(tiles, upr):
    rows, units = np.meshgrid(np.arange(tiles * 16), np.arange(upr), indexing="ij")
    return unit_index(rows, units, upr)  # [row][u]


@pytest.mark.parametrize("upr", UPRS)
@pytest.mark.parametrize("tiles", TILES)
def test_map_is_a_bijection(tiles, upr):
    t = table(tiles, upr)
    assert np.array_equal(np.sort(t.ravel()), np.arange(tiles * 16 * upr))


@pytest.mark.parametrize("upr", UPRS)
@pytest.mark.parametrize("tiles", TILES)
def test_a_k_step_of_a_tile_is_contiguous_in_lane_order(tiles, upr):
    """Lane l = 16 g + r of the wave scoring tile t reads unit 4 s + g of row 16 t + r at tile_base + s * 64 + l."""
    t = table(tiles, upr)
    for tile in range(tiles):
        for s in range(upr // 4):
            lanes = np.array([t[16 * tile + (l % 16), 4 * s + l // 16] for l in range(64)])
            assert np.array_equal(lanes, tile * 16 * upr + s * 64 + np.arange(64)), (tile, s)


@pytest.mark.parametrize("upr", UPRS)
def test_unit_u_holds_columns_16u(upr):
    """Scatter rows whose byte j is (row, j) through the map, gather them back by unit: columns 16u .. 16u + 15."""
    tiles, dpb = 2, 16 * upr
    rows = np.arange(tiles * 16)
    code = (rows[:, None] * 131 + np.arange(dpb)[None, :]) % 251  # byte j of row i
    store = np.full((tiles * 16 * upr, 16), -1, np.int64)
    t = table(tiles, upr)
    for u in range(upr):
        store[t[:, u]] = code[:, 16 * u:16 * u + 16]
    assert (store >= 0).all()
    for i in rows:
        back = np.concatenate([store[unit_index(i, u, upr)] for u in range(upr)])
        assert np.array_equal(back, code[i])


def test_header_agrees_with_the_restatement(tmp_path):
    """The header is plain C++ on the host: a ten-line program prints the map for every shape above."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    hdr = os.path.join(ROOT, "image-search-engine_amd", "csrc", "ise_byte_layout.hpp")
    src = tmp_path / "map.cpp"
    src.write_text(
        '#include <cstdio>\n#include "%s"\n'
        "int main() {\n"
        "    const int uprs[] = {%s}, tiles[] = {%s};\n"
        "    for (int upr : uprs) for (int t : tiles)\n"
        "        for (long long row = 0; row < 16LL * t; row++) for (int u = 0; u < upr; u++)\n"
        '            printf("%%d %%d %%lld %%d %%zu\\n", upr, t, row, u, byte_unit_index(row, u, upr));\n'
        "    return 0;\n}\n" % (hdr, ", ".join(map(str, UPRS)), ", ".join(map(str, TILES))))
    exe = tmp_path / "map"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-x", "c++", "-o", str(exe), str(src)])
    got = np.array(subprocess.check_output([str(exe)]).split(), np.int64).reshape(-1, 5)
    want = unit_index(got[:, 2], got[:, 3], got[:, 0])
    assert len(got) == sum(16 * t * upr for upr in UPRS for t in TILES)
    assert np.array_equal(got[:, 4], want)
    # far rows: the index does not wrap at 2^31 units (2^32 rows are the library's limit)
    assert int(unit_index(2**32 - 1, 63, 64)) == (2**32 // 16 - 1) * 16 * 64 + 15 * 64 + 3 * 16 + 15
