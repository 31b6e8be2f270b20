"""numpy reference of IndexBinaryIVF (tests/test_binary_ivf*.py), built on tests/binary_ref.py.  Given the centroid codes
``C`` uint8 (nlist, cs): the list of a row is ``binary_ref.search(C, xb, 1)[1]``, a query's probes are
``binary_ref.search(C, xq, nprobe)[1]``, and its result is ``np.lexsort((ids, dist))`` over the rows of the probed lists --
ascending Hamming distance, ties by ascending id -- padded with INT32_MAX / -1.  Everything is integer: a comparison with
it is exact.

The second half restates one pass of the device side as plain integers (csrc/ise_binary_ivf.hpp; tests/native/
binary_ivf_harness.hip hands the kernels crafted tables and tests/test_binary_ivf_lists_gpu.py compares every word): the
key of a row, which block of a launch takes which work-list entry, a block's sorted lists and the merged result with
the floors of the next pass.  The tables themselves -- ``meta_of``, ``masks_of``, ``work_list_of``, ``rebuild_dest``,
``rebuilt`` and ``PAD_ID`` -- are tests/ivfsq_ref.py's: the lists over bit codes use the 8-bit lists' kernels for them."""
import numpy as np

from tests import binary_ref
from tests.ivfsq_ref import PAD_ID, masks_of, meta_of, rebuild_dest, rebuilt, tile0_of, tiles_of, work_list_of  # noqa: F401

INT32_MAX = binary_ref.INT32_MAX
TILE = 64      # rows of a list tile
QT = 16        # queries of a pass
KPASS = 32     # results of a pass
WAVES = 4      # waves of a scan block: a block takes its entries four at a time
HOST_BATCH = 4096  # queries the host form stages at once
KEY_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)  # what fills a list behind its last key


def assign(C: np.ndarray, xb: np.ndarray) -> np.ndarray:
    """int64 (n,): the list of every row -- its nearest centroid code, ties by ascending list number."""
    return binary_ref.search(C, xb, 1)[1].reshape(-1)


def probes(C: np.ndarray, xq: np.ndarray, nprobe: int) -> np.ndarray:
    """int64 (nq, nprobe): the lists nearest to every query."""
    return binary_ref.search(C, xq, nprobe)[1]


def clean_probes(table, nlist: int) -> list:
    """Per query the set of lists its probe row names: -1 and out-of-range entries name nothing, a duplicate once."""
    return [sorted({int(l) for l in row if 0 <= l < nlist}) for row in np.asarray(table)]


def search_preassigned(xb: np.ndarray, list_no: np.ndarray, xq: np.ndarray, k: int, table, nlist: int,
                       dist: np.ndarray | None = None):
    """(D int32 (nq, k), I int64 (nq, k)) among the rows whose list (``list_no`` int64 (n,)) the query's probe row names."""
    dist = binary_ref.distances(xb, xq) if dist is None else dist
    nq = dist.shape[0]
    D = np.full((nq, k), INT32_MAX, dtype=np.int32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for i, lists in enumerate(clean_probes(table, nlist)):
        ids = np.flatnonzero(np.isin(list_no, lists)).astype(np.int64)
        order = np.lexsort((ids, dist[i, ids]))[:k]
        D[i, :order.size] = dist[i, ids[order]]
        I[i, :order.size] = ids[order]
    return D, I


def search(C: np.ndarray, xb: np.ndarray, xq: np.ndarray, k: int, nprobe: int, dist: np.ndarray | None = None):
    """What ``IndexBinaryIVF.search`` returns for centroid codes ``C``, rows ``xb`` added in order and ``index.nprobe``."""
    nlist = C.shape[0]
    return search_preassigned(xb, assign(C, xb), xq, k, probes(C, xq, min(nprobe, nlist)), nlist, dist)


def stats_of(table, sizes, k: int, batches: int = 1) -> dict:
    """What one search call adds to ``binary_ivf_stats`` on a non-empty index: a pass per group of 16 queries and 32
    results, and per pass the 64-row tiles of the lists that any query of the group probes.  ``batches``: 1 for a device
    call; the staged host form counts one per 4096 queries, ``ceil(nq / 4096)`` (a batch is whole groups, so the passes
    and the tiles are those of the one call)."""
    nlist = len(sizes)
    sets = clean_probes(table, nlist)
    tiles = [(int(s) + TILE - 1) // TILE for s in sizes]
    per_k = (k + KPASS - 1) // KPASS
    groups = (len(sets) + QT - 1) // QT
    loaded = 0
    for g in range(groups):
        probed = set().union(*sets[g * QT:(g + 1) * QT])
        loaded += per_k * sum(tiles[l] for l in probed)
    return {"batches": int(batches), "passes": groups * per_k, "tiles_loaded": loaded}


def host_batches(nq: int) -> int:
    """Batches of the staged host form (csrc/ise_ivf_lists.hpp, ivf_search_staged)."""
    return -(-int(nq) // HOST_BATCH)


def near_centroids(rng, C: np.ndarray, lists, flips: int = 2) -> np.ndarray:
    """A row per entry of ``lists``: that list's centroid code with at most ``flips`` bits flipped.  (With random centroids of
    64 bits or more the row stays nearest to its own centroid; the caller asserts it with ``assign``.)"""
    lists = np.asarray(lists, dtype=np.int64)
    x = C[lists].copy()
    d = C.shape[1] * 8
    for i in range(len(lists)):
        for bit in rng.choice(d, size=int(rng.integers(0, flips + 1)), replace=False):
            x[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return x


# ---- one pass of the device side (csrc/ise_binary_ivf.hpp), as plain integers
def bin_key(dist, ids) -> np.ndarray:
    """uint64: (distance + 1) << 32 | id -- ascending key is ascending (distance, id); ``bin_key`` of ise_binary_scan.hpp."""
    return ((np.asarray(dist).astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | np.asarray(ids).astype(np.uint64)


def tile_keys(codes: np.ndarray, ids: np.ndarray, xq: np.ndarray) -> np.ndarray:
    """uint64 [tiles][nq][64]: the key of slot ``tile * 64 + r`` against query q, for EVERY slot -- pad slots included,
    whose key a pass must never admit.  codes uint8 [tiles * 64][cs], ids uint32 [tiles * 64], xq uint8 [nq][cs]."""
    assert len(codes) == len(ids) and len(ids) % TILE == 0
    keys = bin_key(binary_ref.distances(codes, xq), np.asarray(ids, np.uint32)[None, :])
    return np.ascontiguousarray(keys.reshape(len(xq), -1, TILE).transpose(1, 0, 2))


def entries_of_block(count: int, grid: int, b: int) -> np.ndarray:
    """The work-list entries block b of ``grid`` takes: wave w of block b takes entries ``b * 4 + w + j * grid * 4``, so
    the block takes every e < count with ``(e // 4) % grid == b``."""
    e = np.arange(int(count))
    return e[(e // WAVES) % int(grid) == int(b)]


def admitted_of(keys_of_entry, entries, which, q: int, lo_q) -> np.ndarray:
    """Sorted: the keys of query q in the entries ``which`` whose mask bit q is set, of the valid rows, >= lo_q."""
    out = [np.zeros(0, np.uint64)]
    for e in which:
        if (int(entries[e][2]) >> q) & 1:
            v = np.asarray(keys_of_entry[e][q][:min(TILE, int(entries[e][1]))], np.uint64)
            out.append(v[v >= np.uint64(lo_q)])
    return np.sort(np.concatenate(out))


def block_lists_of(keys_of_entry, entries, count: int, grid: int, nqt: int, kp: int, lo=None):
    """-> (lists uint64 [grid][nqt][32], empty bool [grid]): what the scan of one pass leaves in the blocks' lists.
    keys_of_entry [>= count][>= nqt][64]: the keys of entry e's tile (``tile_keys(...)[entries[:, 0]]``); entries uint32
    [>= count][4]: (tile, valid rows, query mask, 0), in any order; lo uint64 [nqt], the smallest key admitted (None: 0).
    Block b's list of query q: the kp smallest, sorted, of the keys that belong to one of its entries
    (``entries_of_block``) whose mask bit q is set, to a valid row (row < valid rows) and are >= lo[q]; KEY_PAD behind
    the last.  ``empty[b]``: b * 4 >= count, the block has no entry: all 32 places of every query below nqt are KEY_PAD.
    Of a block with an entry only the places below kp are defined (here: KEY_PAD behind them, not to be compared)."""
    assert 1 <= nqt <= QT and 1 <= kp <= KPASS and grid >= 1 and 0 <= count <= len(entries)
    lo = np.zeros(nqt, np.uint64) if lo is None else np.asarray(lo, np.uint64)
    lists = np.full((grid, nqt, KPASS), KEY_PAD, np.uint64)
    for b in range(grid):
        mine = entries_of_block(count, grid, b)
        for q in range(nqt):
            keys = admitted_of(keys_of_entry, entries, mine, q, lo[q])[:kp]
            lists[b, q, :len(keys)] = keys
    return lists, np.arange(grid) * WAVES >= count


def results_of(keys: np.ndarray):
    """sorted keys uint64 [nqt][kp], KEY_PAD padded -> (D int32, I int64, lo_out uint64 [nqt]) as the merge writes
    them: distance = high word - 1, id = low word widened, INT32_MAX / -1 for padding; the floor of the next pass is the
    last key + 1, or KEY_PAD when the last place is padding (the query is finished)."""
    keys = np.asarray(keys, np.uint64)
    pad = keys == KEY_PAD
    D = np.where(pad, INT32_MAX, (keys >> np.uint64(32)).astype(np.int64) - 1).astype(np.int32)
    I = np.where(pad, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int64)
    last = keys[:, -1]
    lo_out = np.where(last == KEY_PAD, KEY_PAD, last + np.uint64(1)).astype(np.uint64)
    return D, I, lo_out


def merged_of(lists: np.ndarray, kp: int) -> np.ndarray:
    """uint64 [nqt][kp]: the kp smallest of the blocks' lists (their first kp places), sorted."""
    grid, nqt, _ = lists.shape
    return np.sort(lists[:, :, :kp].transpose(1, 0, 2).reshape(nqt, grid * kp), axis=1)[:, :kp]


def pass_of(keys_of_entry, entries, count: int, nqt: int, kp: int, lo=None):
    """-> (D int32 [nqt][kp], I int64 [nqt][kp], lo_out uint64 [nqt]) of one pass, whatever its grid: the kp smallest
    admitted keys (see ``block_lists_of``) over all ``count`` entries."""
    lo = np.zeros(nqt, np.uint64) if lo is None else np.asarray(lo, np.uint64)
    keys = np.full((nqt, kp), KEY_PAD, np.uint64)
    for q in range(nqt):
        mine = admitted_of(keys_of_entry, entries, range(int(count)), q, lo[q])[:kp]
        keys[q, :len(mine)] = mine
    return results_of(keys)
