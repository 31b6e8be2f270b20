"""A float64 restatement of Faiss's flat range search (test infrastructure, not a kernel path).

``range_ref(xb, xq, radius, metric)`` -> (lims uint64, D float64, I int64): for every query, the rows with
squared L2 distance < radius (L2) or inner product > radius (inner product), in ascending id order."""
import numpy as np

L2, IP = 1, 0  # include/ise_knn.h: ISE_METRIC_L2, ISE_METRIC_INNER_PRODUCT


def range_ref(xb, xq, radius, metric):
    xb = np.asarray(xb, dtype=np.float64)
    xq = np.asarray(xq, dtype=np.float64)
    lims = [0]
    Ds, Is = [], []
    for x in xq:
        if metric == L2:
            s = ((xb - x) ** 2).sum(axis=1)
            keep = s < radius
        else:
            s = xb @ x
            keep = s > radius
        ids = np.nonzero(keep)[0]
        Ds.append(s[ids])
        Is.append(ids)
        lims.append(lims[-1] + len(ids))
    D = np.concatenate(Ds) if Ds else np.zeros(0)
    I = np.concatenate(Is).astype(np.int64) if Is else np.zeros(0, dtype=np.int64)
    return np.asarray(lims, dtype=np.uint64), D, I


def filter_search(D, I, radius, metric):
    """The rows of a search() result (nq, k) that pass the range comparison, re-sorted by id: (lims, D, I)."""
    lims = [0]
    Ds, Is = [], []
    for d_, i_ in zip(D, I):
        keep = (i_ >= 0) & ((d_ < radius) if metric == L2 else (d_ > radius))
        order = np.argsort(i_[keep], kind="stable")
        Ds.append(d_[keep][order])
        Is.append(i_[keep][order])
        lims.append(lims[-1] + int(keep.sum()))
    return (np.asarray(lims, dtype=np.uint64), np.concatenate(Ds).astype(np.float32),
            np.concatenate(Is).astype(np.int64))


def assert_range_shape(lims, D, I, nq, n):
    """lims monotone from 0 with nq + 1 entries, ids in range, ascending and unique within each query."""
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    assert lims.shape == (nq + 1,) and lims[0] == 0
    assert (np.diff(lims.astype(np.int64)) >= 0).all()
    assert len(D) == len(I) == int(lims[-1])
    for i in range(nq):
        ids = I[int(lims[i]):int(lims[i + 1])]
        assert (np.diff(ids) > 0).all(), f"query {i}: ids not strictly ascending"
        assert ((ids >= 0) & (ids < max(n, 1))).all()


def assert_range_identical(got, want, what=""):
    """Same lims, same ids, same float32 bits of every distance."""
    lg, Dg, Ig = got
    lw, Dw, Iw = want
    assert np.array_equal(lg, lw), f"{what}: lims differ"
    assert np.array_equal(Ig, Iw), f"{what}: ids differ"
    assert np.array_equal(Dg.view(np.uint32), np.asarray(Dw, dtype=np.float32).view(np.uint32)), \
        f"{what}: distance bits differ"
