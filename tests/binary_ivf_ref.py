"""numpy reference of IndexBinaryIVF (tests/test_binary_ivf*.py), built on tests/binary_ref.py.  Given the centroid codes
``C`` uint8 (nlist, cs): the list of a row is ``binary_ref.search(C, xb, 1)[1]``, a query's probes are
``binary_ref.search(C, xq, nprobe)[1]``, and its result is ``np.lexsort((ids, dist))`` over the rows of the probed lists --
ascending Hamming distance, ties by ascending id -- padded with INT32_MAX / -1.  Everything is integer: a comparison with
it is exact."""
import numpy as np

from tests import binary_ref

INT32_MAX = binary_ref.INT32_MAX
TILE = 64      # rows of a list tile
QT = 16        # queries of a pass
KPASS = 32     # results of a pass


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


def stats_of(table, sizes, k: int) -> dict:
    """What one search batch adds to ``binary_ivf_stats`` on a non-empty index: a pass per group of 16 queries and 32
    results, and per pass the 64-row tiles of the lists that any query of the group probes."""
    nlist = len(sizes)
    sets = clean_probes(table, nlist)
    tiles = [(int(s) + TILE - 1) // TILE for s in sizes]
    per_k = (k + KPASS - 1) // KPASS
    groups = (len(sets) + QT - 1) // QT
    loaded = 0
    for g in range(groups):
        probed = set().union(*sets[g * QT:(g + 1) * QT])
        loaded += per_k * sum(tiles[l] for l in probed)
    return {"batches": 1, "passes": groups * per_k, "tiles_loaded": loaded}


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
