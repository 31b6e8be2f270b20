"""numpy reference of the inverted-list index over 8-bit rows (tests only): which 64-row tiles a pass visits, the
statistics a search adds, and the expected results -- ``sq_ref.expected``'s complete ranking over the decoded rows cut to
``ivf_ref.probed_members``."""
import numpy as np

from tests import ivf_ref, sq_ref

TILE_ROWS = sq_ref.TILE_ROWS  # 64: a wave's unit in the byte scan


def tiles_of(sizes) -> int:
    """Total of ceil(size / 64) over the given list sizes."""
    return int(sum((int(s) + TILE_ROWS - 1) // TILE_ROWS for s in sizes))


def tile0_of(sizes) -> np.ndarray:
    """(nlist + 1,) first tile of every list in the one array, and the tiles in all."""
    return np.concatenate([[0], np.cumsum([(int(s) + TILE_ROWS - 1) // TILE_ROWS for s in sizes])]).astype(np.int64)


def pass_tile_sets(probes, sizes, d: int) -> list:
    """Per group of QT(d) queries (one scan pass per 32 results), the sorted tile numbers a pass visits: every tile of
    every list that at least one query of the group names.  Entries outside [0, nlist) name nothing, a list named twice
    counts once."""
    probes = np.asarray(probes, dtype=np.int64).reshape(len(probes), -1)
    nlist, qt, t0 = len(sizes), sq_ref.qt_of(d), tile0_of(sizes)
    out = []
    for g0 in range(0, len(probes), qt):
        grp = probes[g0:g0 + qt].reshape(-1)
        named = sorted({int(l) for l in grp if 0 <= int(l) < nlist})
        out.append([int(t) for l in named for t in range(t0[l], t0[l + 1])])
    return out


def stats_of(probes, sizes, d: int, k: int) -> dict:
    """What one search call adds to ``ivfsq_stats`` on an index that holds rows."""
    sets = pass_tile_sets(probes, sizes, d)
    per = -(-int(k) // 32)
    return {"batches": 1, "passes": len(sets) * per, "tiles_loaded": sum(len(s) for s in sets) * per}


def expected(xq, dec, probes, assign, nlist: int, k: int, metric: int, full=None):
    """-> (D, I): the k best of each query's probed members by the score against the decoded rows.  ``full``: the
    complete ranking ``sq_ref.expected(xq, dec, len(dec), metric)``, if the caller keeps one."""
    if full is None:
        full = sq_ref.expected(xq, dec, len(dec), metric)
    members = ivf_ref.probed_members(probes, assign, nlist)
    return ivf_ref.expected_from_ranking(full[0], full[1], members, k, metric)
