"""numpy reference of the binary flat index (tests/test_binary_flat*.py): Hamming distances from a 256-entry popcount
table over ``xb ^ q``, ranking by ``np.lexsort((ids, dist))`` -- ascending distance, ties by ascending id -- padded with
INT32_MAX / -1, and range search as ``np.flatnonzero(dist < radius)`` per query."""
import numpy as np

INT32_MAX = int(np.iinfo(np.int32).max)
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def distances(xb: np.ndarray, xq: np.ndarray) -> np.ndarray:
    """(nq, n) int32 Hamming distances between uint8 codes xq (nq, cs) and xb (n, cs)."""
    xb = np.asarray(xb, dtype=np.uint8)
    xq = np.asarray(xq, dtype=np.uint8)
    out = np.empty((xq.shape[0], xb.shape[0]), dtype=np.int32)
    for i, q in enumerate(xq):
        out[i] = POPCOUNT[xb ^ q[None, :]].sum(axis=1, dtype=np.int32) if xb.shape[0] else 0
    return out


def search(xb: np.ndarray, xq: np.ndarray, k: int, dist: np.ndarray | None = None):
    """(D int32 (nq, k), I int64 (nq, k))."""
    dist = distances(xb, xq) if dist is None else dist
    nq, n = dist.shape
    D = np.full((nq, k), INT32_MAX, dtype=np.int32)
    I = np.full((nq, k), -1, dtype=np.int64)
    ids = np.arange(n, dtype=np.int64)
    for i in range(nq):
        order = np.lexsort((ids, dist[i]))[:k]
        D[i, :order.size] = dist[i, order]
        I[i, :order.size] = order
    return D, I


def range_search(xb: np.ndarray, xq: np.ndarray, radius: int, dist: np.ndarray | None = None):
    """(lims uint64 (nq + 1,), D int32, I int64): every row with dist < radius, per query in ascending id order."""
    dist = distances(xb, xq) if dist is None else dist
    lims = [0]
    Ds, Is = [], []
    for i in range(dist.shape[0]):
        hit = np.flatnonzero(dist[i] < radius)
        Is.append(hit.astype(np.int64))
        Ds.append(dist[i, hit].astype(np.int32))
        lims.append(lims[-1] + hit.size)
    D = np.concatenate(Ds) if Ds else np.zeros(0, dtype=np.int32)
    I = np.concatenate(Is) if Is else np.zeros(0, dtype=np.int64)
    return np.asarray(lims, dtype=np.uint64), D.astype(np.int32), I.astype(np.int64)
