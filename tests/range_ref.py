"""A float64 restatement of Faiss's flat range search (test infrastructure, not a kernel path).

``range_ref(xb, xq, radius, metric)`` -> (lims uint64, D float64, I int64): for every query, the rows with
squared L2 distance < radius (L2) or inner product > radius (inner product), in ascending id order.

``scores_f64`` / ``range_of_scores`` / ``range_brute``: the same brute force split in two, so that a test computes the
(nq, n) scores once and takes every radius and every member mask from them; ``segment_hits_max`` tells whether a result
makes a wave segment of the range pass overflow a given staging capacity."""
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


def scores_f64(xb, xq, metric):
    """(nq, n) float64: sum (x - y)^2 entry by entry (L2) or sum x y (inner product), one query at a time."""
    b = np.asarray(xb, dtype=np.float64)
    out = np.empty((len(xq), len(b)))
    for i, x in enumerate(np.asarray(xq, dtype=np.float64)):
        out[i] = ((b - x) ** 2).sum(axis=1) if metric == L2 else (b * x).sum(axis=1)
    return out


def range_of_scores(S, radius, metric, members=None):
    """Every row strictly inside the radius, optionally among a member mask (bool (n,)), from the float64 scores
    S (nq, n): (lims uint64, D float32, I int64), ascending ids per query.  A NaN radius keeps nothing."""
    S = np.asarray(S, dtype=np.float64)
    keep = (S < radius) if metric == L2 else (S > radius)
    if members is not None:
        keep = keep & np.asarray(members, dtype=bool)[None, :]
    lims = np.concatenate(([0], np.cumsum(keep.sum(axis=1)))).astype(np.uint64)
    q, ids = np.nonzero(keep)  # row-major: by query, ascending ids within one
    return lims, S[q, ids].astype(np.float32), ids.astype(np.int64)


def range_brute(xb, xq, radius, metric, members=None):
    """range_of_scores over the brute-force scores of (xb, xq)."""
    return range_of_scores(scores_f64(xb, xq, metric), radius, metric, members)


def segment_hits_max(res, rows_per_segment=16):
    """The most hits one query has within one run of ``rows_per_segment`` consecutive rows (aligned), 0 if none."""
    lims, _, I = res
    best = 0
    for i in range(len(lims) - 1):
        ids = I[int(lims[i]):int(lims[i + 1])]
        if len(ids):
            best = max(best, int(np.bincount(ids // rows_per_segment).max()))
    return best


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
