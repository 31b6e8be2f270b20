"""numpy reference of the product-quantised index (tests only): the codec and the expected search results."""
import numpy as np

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


def adc_expected(x, C, codes, k, metric):
    """The expected (D, I): a float64 brute force of the queries against the decoded rows."""
    return brute_knn(decode(codes, C), np.asarray(x, np.float32), k, metric)
