"""numpy reference of the product-quantised index (tests only): the codec and the expected search results."""
import numpy as np

from oracle import knn_oracle as ko
from tests.knn_checks import brute_knn


def qt_of(M: int) -> int:
    """Queries per scan pass, as include/ise_knn.h documents it."""
    return 16 if M <= 5 else 8 if M <= 15 else 4 if M <= 35 else 2


def sub_distances(x, C, m):
    """float64 squared L2 distances (n, 256) of the rows' m-th sub-vectors to the centroids of sub-quantiser m."""
    dsub = C.shape[2]
    xs = np.asarray(x, np.float64)[:, m * dsub:(m + 1) * dsub]
    return ((xs[:, None, :] - C[m].astype(np.float64)[None, :, :]) ** 2).sum(-1)


def encode(x, C) -> np.ndarray:
    """uint8 (n, M): the nearest centroid per sub-vector in float64, the lowest index among equals."""
    M = C.shape[0]
    codes = np.empty((len(x), M), np.uint8)
    for m in range(M):
        codes[:, m] = np.argmin(sub_distances(x, C, m), axis=1)  # argmin returns the first of equal minima
    return codes


def decode(codes, C) -> np.ndarray:
    """float32 (n, d): row i is the concatenation of C[m][codes[i][m]]."""
    M = C.shape[0]
    codes = np.asarray(codes).reshape(-1, M)
    return np.ascontiguousarray(np.concatenate([C[m][codes[:, m]] for m in range(M)], axis=1), dtype=np.float32)


def adc_tables(xq, C, metric) -> np.ndarray:
    """float64 (nq, M, 256): T[q, m, j] = |x_m - C[m][j]|^2 (L2) or <x_m, C[m][j]> (inner product), entry by entry."""
    M, ksub, dsub = C.shape
    x = np.asarray(xq, np.float64).reshape(-1, M, dsub)
    c = C.astype(np.float64)
    T = np.empty((x.shape[0], M, ksub))
    for m in range(M):
        if metric == ko.METRIC_L2:
            T[:, m] = ((x[:, m, None, :] - c[m][None, :, :]) ** 2).sum(-1)
        else:
            T[:, m] = (x[:, m, None, :] * c[m][None, :, :]).sum(-1)
    return T


def adc_scores(xq, C, codes, metric) -> np.ndarray:
    """float64 (nq, n): the table-lookup definition, sum over ascending m of T[q, m, codes[i, m]] from +0.0."""
    T = adc_tables(xq, C, metric)
    codes = np.asarray(codes).reshape(-1, C.shape[0])
    scores = np.zeros((T.shape[0], codes.shape[0]))
    for m in range(C.shape[0]):
        scores += T[:, m, codes[:, m]]
    return scores


def adc_topk(scores, k, metric):
    """(D float32 (nq, k), I int64 (nq, k)) of a float64 score matrix: (score, ascending id) order under Faiss's gate
    (L2 enters if < FLT_MAX, inner product if > -FLT_MAX, NaN never), -1 / +-FLT_MAX behind the last.  A partition finds
    the k-th value; only the rows at or below it are sorted, exactly."""
    nq, n = scores.shape
    ip = metric != ko.METRIC_L2
    D = np.full((nq, k), -ko.FLT_MAX if ip else ko.FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            s = scores[q]
            key = -s if ip else s
            ids = np.flatnonzero(key < float(ko.FLT_MAX))  # the gate of either metric on the key; NaN compares false
            if len(ids) > k:
                kept = key[ids]
                ids = ids[kept <= kept[np.argpartition(kept, k - 1)[k - 1]]]
            order = ids[np.lexsort((ids, key[ids]))][:k]
            D[q, :len(order)] = s[order].astype(np.float32)
            I[q, :len(order)] = order
    return D, I


def adc_expected(x, C, codes, k, metric):
    """The expected (D, I): a float64 brute force of the queries against the decoded rows."""
    return brute_knn(decode(codes, C), np.asarray(x, np.float32), k, metric)
