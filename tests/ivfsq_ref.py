"""numpy reference of the inverted-list index over 8-bit rows (tests only): which 64-row tiles a pass visits, the
statistics a search adds, the expected results -- ``sq_ref.expected``'s complete ranking over the decoded rows cut to
``ivf_ref.probed_members`` -- and the device side's tables as plain integers: the query masks, the work list and the
arrays after a rebuild (csrc/ise_ivf_tiles.hpp; tests/test_ivfsq_lists_gpu.py compares them word for word).  The layout
functions take the rows of a tile (``tile_rows``, 64 unless given): with 16 they are the float32 lists' layout, whose
rebuild runs the same kernels (tests/test_ivf_rebuild_gpu.py)."""
import numpy as np

from tests import ivf_ref, sq_ref

TILE_ROWS = sq_ref.TILE_ROWS  # 64: a wave's unit in the byte scan


def tiles_of(sizes, tile_rows: int = TILE_ROWS) -> int:
    """Total of ceil(size / tile_rows) over the given list sizes."""
    return int(sum((int(s) + tile_rows - 1) // tile_rows for s in sizes))


def tile0_of(sizes, tile_rows: int = TILE_ROWS) -> np.ndarray:
    """(nlist + 1,) first tile of every list in the one array, and the tiles in all."""
    return np.concatenate([[0], np.cumsum([(int(s) + tile_rows - 1) // tile_rows for s in sizes])]).astype(np.int64)


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


# ---- the tables of the device side (csrc/ise_ivf_tiles.hpp), as plain integers
PAD_ID = 0xFFFFFFFF  # the id of a slot behind a list's rows


def meta_of(sizes, tile_rows: int = TILE_ROWS) -> np.ndarray:
    """uint32 table the kernels read (csrc/ise_ivf_plan.hpp, ivf_plan_meta): list_tile0 [nlist + 1] | list_size [nlist]
    | tile_list [tiles]."""
    sizes = np.asarray(sizes, dtype=np.int64)
    t0 = tile0_of(sizes, tile_rows)
    tile_list = np.repeat(np.arange(len(sizes)), np.diff(t0))
    return np.concatenate([t0, sizes, tile_list]).astype(np.uint32)


def masks_of(probes, nlist: int, qt: int) -> np.ndarray:
    """uint32 [groups][nlist]: bit c of masks[g][l] is set when query g * qt + c names list l.  Entries outside
    [0, nlist) set nothing, a list named twice sets its bit once."""
    probes = np.asarray(probes, dtype=np.int64).reshape(len(probes), -1)
    nq = len(probes)
    masks = np.zeros((-(-nq // qt), nlist), np.uint32)
    q = np.repeat(np.arange(nq), probes.shape[1])
    l = probes.reshape(-1)
    ok = (l >= 0) & (l < nlist)
    np.bitwise_or.at(masks, (q[ok] // qt, l[ok]), (np.uint32(1) << (q[ok] % qt).astype(np.uint32)))
    return masks


def work_list_of(masks, sizes) -> list:
    """Per group -> (offs uint32 [nlist], count, entries uint32 [count][4]).  offs[l]: the tiles of the probed lists
    (mask != 0) before l -- for the unprobed lists too; count: their total; the entries (tile, valid rows in it, the
    list's mask, 0) in slot order: ascending lists, ascending tiles inside a list."""
    sizes = np.asarray(sizes, dtype=np.int64)
    t0 = tile0_of(sizes)
    per = np.diff(t0)
    out = []
    for gm in np.asarray(masks, dtype=np.uint32):
        contrib = np.where(gm != 0, per, 0)
        offs = np.cumsum(contrib) - contrib
        count = int(contrib.sum())
        lists = np.repeat(np.arange(len(sizes)), contrib)      # the list of every entry
        in_list = np.arange(count) - offs[lists]                # its tile within the list
        valid = np.minimum(TILE_ROWS, sizes[lists] - TILE_ROWS * in_list)
        entries = np.stack([t0[lists] + in_list, valid, gm[lists].astype(np.int64), np.zeros(count, np.int64)], axis=1)
        out.append((offs.astype(np.uint32), count, entries.astype(np.uint32).reshape(count, 4)))
    return out


def rebuild_dest(old_sizes, pend_lists, tile_rows: int = TILE_ROWS) -> np.ndarray:
    """uint32 [m]: the slot of pending row i after the rebuild -- behind the old rows of its list and the pending rows
    of that list that came before it."""
    old_sizes = np.asarray(old_sizes, dtype=np.int64)
    pend_lists = np.asarray(pend_lists, dtype=np.int64).reshape(-1)
    new_sizes = old_sizes + np.bincount(pend_lists, minlength=len(old_sizes))
    t0 = tile0_of(new_sizes, tile_rows)
    nxt = old_sizes.copy()
    dest = np.empty(len(pend_lists), np.uint32)
    for i, l in enumerate(pend_lists):
        dest[i] = t0[l] * tile_rows + nxt[l]
        nxt[l] += 1
    return dest


def rebuilt(old_sizes, old_ids, old_codes, pend_lists, pend_codes, id0: int, stride: int, old_rterm=None, pend_rterm=None,
            tile_rows: int = TILE_ROWS):
    """-> (new sizes, codes uint8 [slots][stride], rterm float64 [slots], ids uint32 [slots]) after the rebuild.
    old_ids [old slots], old_codes [old slots][stride]: the arrays before it, laid out by ``old_sizes``; pend_lists [m],
    pend_codes [m][stride]: the pending rows in insertion order, row i has id ``id0 + i``.  Every list keeps its old
    rows in their order and takes its pending rows behind them in theirs; the slots behind a list's rows (to the end of
    its last tile of ``tile_rows`` rows) are zero rows with id 0xFFFFFFFF.  The row terms travel with the rows; left out, a row's term is the sum of its squared bytes."""
    old_sizes = np.asarray(old_sizes, dtype=np.int64)
    pend_lists = np.asarray(pend_lists, dtype=np.int64).reshape(-1)
    old_codes = np.asarray(old_codes, np.uint8).reshape(-1, stride)
    pend_codes = np.asarray(pend_codes, np.uint8).reshape(-1, stride)
    if old_rterm is None:
        old_rterm = (old_codes.astype(np.float64) ** 2).sum(1)
    if pend_rterm is None:
        pend_rterm = (pend_codes.astype(np.float64) ** 2).sum(1)
    old_t0 = tile0_of(old_sizes, tile_rows)
    assert len(old_codes) == len(old_ids) == len(old_rterm) == old_t0[-1] * tile_rows and len(pend_codes) == len(pend_lists)
    new_sizes = old_sizes + np.bincount(pend_lists, minlength=len(old_sizes))
    t0 = tile0_of(new_sizes, tile_rows)
    slots = int(t0[-1]) * tile_rows
    codes = np.zeros((slots, stride), np.uint8)
    rterm = np.zeros(slots, np.float64)
    ids = np.full(slots, PAD_ID, np.uint32)
    order = np.argsort(pend_lists, kind="stable")
    first = np.searchsorted(pend_lists[order], np.arange(len(old_sizes) + 1))
    for l in range(len(old_sizes)):
        a, b, m = int(old_t0[l]) * tile_rows, int(t0[l]) * tile_rows, int(old_sizes[l])
        mine = order[first[l]:first[l + 1]]
        codes[b:b + m], rterm[b:b + m], ids[b:b + m] = old_codes[a:a + m], old_rterm[a:a + m], old_ids[a:a + m]
        b += m
        codes[b:b + len(mine)], rterm[b:b + len(mine)], ids[b:b + len(mine)] = pend_codes[mine], pend_rterm[mine], id0 + mine
    return new_sizes, codes, rterm, ids
