"""Reference forms of a selector-filtered search (test infrastructure, not a kernel path).

(A) ``filter_ranking``: the complete ranking of an UNFILTERED search (``index.search(x, n)``), with the ids a selector
    rejects dropped on the host, cut at k and padded as ``search`` pads.
(B) ``sub_index_search``: a fresh index of ``x[members]``, its ids mapped back through ``np.flatnonzero(members)``.
(C) ``knn_of_scores`` / ``masked_knn_brute``: the k best among a member mask straight from float64 brute-force scores
    (tests/range_ref.py, ``scores_f64``) -- no index takes part, so an error shared by every kernel cannot cancel."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
L2, IP = 1, 0  # include/ise_knn.h: ISE_METRIC_L2, ISE_METRIC_INNER_PRODUCT


def pad_value(metric):
    return FLT_MAX if metric == L2 else -FLT_MAX


def filter_ranking(D_full, I_full, members, k, metric):
    """D_full, I_full: (nq, K) best first, -1 padded; members(ids) -> bool.  -> (D (nq, k) float32, I (nq, k) int64)."""
    nq = D_full.shape[0]
    D = np.full((nq, k), pad_value(metric), dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        ids = I_full[q]
        keep = ids >= 0
        keep[keep] = np.asarray(members(ids[keep]), dtype=bool)
        pos = np.flatnonzero(keep)[:k]
        D[q, :len(pos)] = D_full[q, pos]
        I[q, :len(pos)] = ids[pos]
    return D, I


def sub_index_search(make_index, xb, members, xq, k, metric):
    """make_index(rows) -> an index of those rows; members: bool (n,).  The sub-index's result with its ids mapped
    back to the rows of xb (none selected: all padding)."""
    rows = np.flatnonzero(members)
    if rows.size == 0:
        return (np.full((len(xq), k), pad_value(metric), dtype=np.float32), np.full((len(xq), k), -1, dtype=np.int64))
    D, I = make_index(np.ascontiguousarray(xb[rows])).search(xq, k)
    out = np.full(I.shape, -1, dtype=np.int64)
    out[I >= 0] = rows[I[I >= 0]]
    return D, out


def knn_of_scores(S, members, k, metric):
    """The k best rows among a member mask (bool (n,)) from float64 scores S (nq, n), ties by ascending id, padded as
    ``search`` pads: (D (nq, k) float32, I (nq, k) int64).  Independent of any index."""
    S = np.asarray(S, dtype=np.float64)
    rows = np.flatnonzero(np.asarray(members, dtype=bool))
    D = np.full((S.shape[0], k), pad_value(metric), dtype=np.float32)
    I = np.full((S.shape[0], k), -1, dtype=np.int64)
    for q in range(S.shape[0]):
        s = S[q, rows]
        order = np.lexsort((rows, s if metric == L2 else -s))[:k]
        D[q, :len(order)] = s[order].astype(np.float32)
        I[q, :len(order)] = rows[order]
    return D, I


def masked_knn_brute(xb, xq, members, k, metric):
    """knn_of_scores over the float64 brute-force scores of (xb, xq)."""
    from tests.range_ref import scores_f64

    return knn_of_scores(scores_f64(xb, xq, metric), members, k, metric)


def filter_range(res, members):
    """(lims, D, I) of an unfiltered range_search with the rejected ids dropped per query."""
    lims, D, I = res
    keep = np.asarray(members(I), dtype=bool) if len(I) else np.zeros(0, dtype=bool)
    out = [0]
    for i in range(len(lims) - 1):
        out.append(out[-1] + int(keep[int(lims[i]):int(lims[i + 1])].sum()))
    return np.asarray(out, dtype=np.uint64), D[keep], I[keep]


def selector_census(members):
    """bool (n,) -> selected count, window (r0, r1), non-empty 16-row tiles, as ise_selector_info reports them."""
    rows = np.flatnonzero(members)
    if rows.size == 0:
        return {"selected": 0, "window": (0, 0), "tiles": 0}
    return {"selected": int(rows.size), "window": (int(rows[0]), int(rows[-1]) + 1),
            "tiles": int(np.unique(rows // 16).size)}
