"""Reference forms of the inverted-list search (test infrastructure, not a kernel path): pure numpy.

``list_members``: the grouping of the rows by list number, ids ascending inside every list.
``probed_members``: per query, the ids of the rows in the lists its probe row names -- entries outside [0, nlist)
(-1 among them) name nothing, a list named twice counts once.
``expected_from_ranking``: the complete ranking of a flat index over the same rows, cut per query to those members
(tests/sel_ref.filter_ranking, called per query).
``expected_brute``: tests/knn_checks.brute_knn over each query's member rows, ids mapped back."""
import numpy as np

from tests.knn_checks import brute_knn
from tests.sel_ref import filter_ranking, pad_value


def list_members(assign, nlist):
    """assign: (n,) list number of row i -> [ids of list 0, ids of list 1, ...], each ascending int64."""
    assign = np.asarray(assign, dtype=np.int64).reshape(-1)
    assert ((assign >= 0) & (assign < nlist)).all()
    return [np.flatnonzero(assign == l).astype(np.int64) for l in range(nlist)]


def probed_members(probes, assign, nlist):
    """probes: (nq, nprobe) -> per query the sorted ids of the rows of its probed lists."""
    lists = list_members(assign, nlist)
    out = []
    for row in np.asarray(probes, dtype=np.int64).reshape(len(probes), -1):
        named = sorted({int(l) for l in row if 0 <= int(l) < nlist})
        ids = np.concatenate([lists[l] for l in named]) if named else np.zeros(0, np.int64)
        out.append(np.sort(ids))
    return out


def tiles_of(sizes):
    """Total of ceil(size / 16) over the given list sizes."""
    return int(sum((int(s) + 15) // 16 for s in sizes))


def expected_from_ranking(D_full, I_full, members, k, metric):
    """D_full, I_full: (nq, N) complete ranking of the flat index; members: per-query id arrays."""
    nq = len(members)
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    for q in range(nq):
        D[q:q + 1], I[q:q + 1] = filter_ranking(D_full[q:q + 1], I_full[q:q + 1],
                                                lambda ids, m=members[q]: np.isin(ids, m), k, metric)
    return D, I


def expected_brute(xb, xq, members, k, metric):
    nq = len(members)
    D = np.full((nq, k), pad_value(metric), np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        rows = members[q]
        if rows.size == 0:
            continue
        Dq, Iq = brute_knn(np.ascontiguousarray(xb[rows]), xq[q:q + 1], k, metric)
        D[q], I[q] = Dq[0], np.where(Iq[0] >= 0, rows[np.maximum(Iq[0], 0)], -1)
    return D, I
