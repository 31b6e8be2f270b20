"""A numpy restatement of the removal planning of csrc/ise_remove_plan.hpp (ids -> runs -> the g / cend tables) and of
the source map and slab schedule the kernels of csrc/ise_remove.hpp run from them (test infrastructure, not a kernel
path).  tests/native/remove_plan_check.cpp checks the same header natively.

``runs``: the removed rows as sorted, disjoint (start, len) pairs inside [0, n).  ``source_map(n, runs)`` -> src, the
row that ends up at every destination row [0, n_new).  ``slab_schedule(n, runs, slab)`` -> the launches of the
in-place compaction in the order the stream runs them, as (reads, writes) row arrays of the index arrays (the bounce
buffer is private to a slab and not listed).  ``compact(x, runs, slab)`` runs that schedule on a numpy array."""
import numpy as np


def runs_of(removed, n):
    """Any iterable of row numbers -> sorted disjoint maximal runs inside [0, n)."""
    ids = np.unique(np.asarray(list(removed), dtype=np.int64))
    ids = ids[(ids >= 0) & (ids < n)]
    runs = []
    for i in ids.tolist():
        if runs and runs[-1][0] + runs[-1][1] == i:
            runs[-1][1] += 1
        else:
            runs.append([i, 1])
    return [tuple(r) for r in runs]


def bite_points(runs):
    """-> (g, cend): the destination row at which run t bites, and the rows removed up to and including it."""
    g, cend, c = [], [], 0
    for start, length in runs:
        g.append(start - c)
        c += length
        cend.append(c)
    return np.asarray(g, dtype=np.int64), np.asarray(cend, dtype=np.int64)


def source_rows(j, g, cend):
    """src(j) for an array of destination rows: j + rows removed in all runs with g_t <= j (one upper bound)."""
    j = np.asarray(j, dtype=np.int64)
    u = np.searchsorted(g, j, side="right")
    add = np.where(u > 0, cend[np.maximum(u - 1, 0)], 0) if len(g) else np.zeros_like(j)
    return j + add


def source_map(n, runs):
    g, cend = bite_points(runs)
    n_new = n - (int(cend[-1]) if len(cend) else 0)
    return source_rows(np.arange(n_new), g, cend)


def slab_schedule(n, runs, slab):
    """[(reads, writes)] per launch pair: slab [a, b) gathers rows src(a..b-1) (writes nothing but the bounce
    buffer), then writes rows [a, b) (reads nothing but the bounce buffer)."""
    if not runs:
        return []
    g, cend = bite_points(runs)
    n_new, first = n - int(cend[-1]), int(runs[0][0])
    out = []
    for a in range(first, n_new, slab):
        b = min(a + slab, n_new)
        dst = np.arange(a, b)
        out.append((source_rows(dst, g, cend), np.zeros(0, dtype=np.int64)))
        out.append((np.zeros(0, dtype=np.int64), dst))
    return out


def compact(x, runs, slab):
    """Run the schedule in place on a copy of x ((n, ...) array); rows [n_new, n) are zeroed as the tail is."""
    x = np.array(x, copy=True)
    n = x.shape[0]
    g, cend = bite_points(runs)
    n_new = n - (int(cend[-1]) if len(cend) else 0)
    bounce = None
    for reads, writes in slab_schedule(n, runs, slab):
        if len(reads):
            bounce = x[reads].copy()
        else:
            x[writes] = bounce
    x[n_new:] = 0
    return x, n_new
