"""numpy reference of the selector-filtered binary searches (tests/test_binary_sel*.py), on top of tests/binary_ref.py:
filtered search is ``binary_ref.search`` on ``xb[rows]`` with the ids mapped back through ``rows =
np.flatnonzero(members)`` and padded to k; filtered range search is ``binary_ref.range_search``'s result with the
rejected ids dropped per query.  ``census`` is what a device selector's ``info()`` must report."""
import numpy as np

from tests import binary_ref as ref


def members_of(sel, n: int) -> np.ndarray:
    """bool (n,): the rows of [0, n) an IDSelector names."""
    return np.asarray(sel.members(np.arange(n, dtype=np.int64)), dtype=bool)


def search(xb: np.ndarray, xq: np.ndarray, k: int, members: np.ndarray, dist: np.ndarray | None = None):
    """(D int32 (nq, k), I int64 (nq, k)): the k best rows among ``members``, ties by ascending id, INT32_MAX / -1."""
    members = np.asarray(members, dtype=bool)
    rows = np.flatnonzero(members).astype(np.int64)
    sub = None if dist is None else dist[:, rows]
    D, I = ref.search(xb[rows], xq, k, sub)
    out = np.full(I.shape, -1, dtype=np.int64)
    ok = I >= 0
    out[ok] = rows[I[ok]]
    return D, out


def range_search(xb: np.ndarray, xq: np.ndarray, radius: int, members: np.ndarray, dist: np.ndarray | None = None):
    """(lims uint64 (nq + 1,), D int32, I int64): every row of ``members`` with dist < radius, ascending id per query."""
    members = np.asarray(members, dtype=bool)
    lims, D, I = ref.range_search(xb, xq, radius, dist)
    keep = members[I] if I.size else np.zeros(0, dtype=bool)
    new_lims = [0]
    for q in range(len(lims) - 1):
        new_lims.append(new_lims[-1] + int(keep[int(lims[q]):int(lims[q + 1])].sum()))
    return np.asarray(new_lims, dtype=np.uint64), D[keep].astype(np.int32), I[keep].astype(np.int64)


def census(members: np.ndarray) -> dict:
    """ntotal, selected rows, window [first, last + 1) ((0, 0) when empty), non-empty 64-row tiles."""
    members = np.asarray(members, dtype=bool)
    rows = np.flatnonzero(members)
    window = (int(rows[0]), int(rows[-1]) + 1) if rows.size else (0, 0)
    return {"ntotal": int(members.size), "selected": int(rows.size), "window": window,
            "tiles": int(np.unique(rows >> 6).size)}
