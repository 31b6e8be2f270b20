"""Reference form of subset scoring and of IndexRefine's re-ranking (test infrastructure, not a kernel path): per query
the unique valid candidates in ascending id order, ``brute_knn`` (tests/knn_checks.py) over those rows alone, positions
mapped back to ids, padded with -1 / +-FLT_MAX as ``search`` pads."""
import numpy as np

from tests.knn_checks import brute_knn
from tests.sel_ref import pad_value


def refine_ref(xb: np.ndarray, xq: np.ndarray, cand: np.ndarray, k: int, metric: int):
    """xb (n, d), xq (nq, d) float32; cand (nq, kc) int64, entries outside [0, n) ignored, duplicates counted once.
    -> (D float32 (nq, k), I int64 (nq, k))."""
    n, nq = xb.shape[0], xq.shape[0]
    cand = np.asarray(cand, dtype=np.int64).reshape(nq, -1)
    D = np.full((nq, k), pad_value(metric), dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        ids = np.unique(cand[q][(cand[q] >= 0) & (cand[q] < n)])  # sorted: a position order is an id order
        if ids.size == 0:
            continue
        d_, i_ = brute_knn(xb[ids], xq[q:q + 1], k, metric)
        ok = i_[0] >= 0
        D[q, ok] = d_[0, ok]
        I[q, ok] = ids[i_[0, ok]]
    return D, I
