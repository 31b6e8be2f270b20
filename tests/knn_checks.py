"""Shared comparison helpers for the kNN parity tests (tests only)."""
import numpy as np

from oracle import knn_oracle as ko

RTOL = 1e-4  # north_star: distances within 1e-4 (fp32); applied as 1e-4 * max(1, |D|)


def true_scores(xb, xq, ids, metric):
    """float64 score of (query q, row ids[q, r]); -1 ids give nan."""
    out = np.full(ids.shape, np.nan)
    b = xb.astype(np.float64)
    for q in range(ids.shape[0]):
        ok = ids[q] >= 0
        rows = b[ids[q][ok]]
        x = xq[q].astype(np.float64)
        out[q, ok] = ((rows - x) ** 2).sum(1) if metric == ko.METRIC_L2 else rows @ x
    return out


ATOL_UNIFORM = 1e-4  # north_star's absolute bound, asserted where it is attainable: uniform[0,1) data


def assert_knn_matches(D, I, D_ref, I_ref, xb, xq, metric, gap=None, rtol=RTOL, atol=None, near=None):
    """Bit-exact ids wherever the float64 ranking is unambiguous; where two
    consecutive oracle ranks are closer than float32 can resolve, the returned
    row must still be a true near-tie at that rank.  Distances always within
    rtol * max(1, |D_ref|); with ``atol`` additionally within that ABSOLUTE bound
    (north_star: 1e-4 -- used on uniform[0,1) data, where |D| ~ d/6 keeps it above
    float32 rounding).  ``near`` (a scalar or one value per query) replaces the float32 margin of a near-tie where
    the caller has raised ``rtol`` / ``atol`` to a derived error bound e of the scores: scores within e of the
    truth put a row at rank r whose true score lies within 2 e of the reference's at that rank."""
    assert D.dtype == np.float32 and I.dtype == np.int64
    assert D.shape == D_ref.shape and I.shape == I_ref.shape
    pad = I_ref < 0
    assert np.array_equal(I < 0, pad), "padding (-1) positions differ"
    assert np.array_equal(D[pad], D_ref[pad]), "padding distances must be +-FLT_MAX"
    tol = rtol * np.maximum(1.0, np.abs(D_ref.astype(np.float64)))
    err = np.abs(D.astype(np.float64) - D_ref.astype(np.float64))
    assert (err[~pad] <= tol[~pad]).all(), f"distance error {err[~pad].max():.3e} above tolerance"
    if atol is not None and (~pad).any():
        assert err[~pad].max() <= atol, f"distance error {err[~pad].max():.3e} above the absolute bound {atol:g}"
    for q in range(I.shape[0]):
        row = I[q][I[q] >= 0]
        assert len(set(row.tolist())) == len(row), "duplicate ids in one result row"
    mism = (I != I_ref) & ~pad
    if mism.any():
        ts = true_scores(xb, xq, I, metric)
        ref = D_ref.astype(np.float64)
        margin = 2e-6 * np.maximum(1.0, np.abs(ref)) + 1e-6
        if near is not None:
            margin = np.broadcast_to(np.asarray(near, np.float64).reshape(-1, 1), ref.shape)
        bad = mism & ~(np.abs(ts - ref) <= margin)
        assert not bad.any(), (
            f"{bad.sum()} id mismatches that are not float32 near-ties, e.g. q={np.argwhere(bad)[0]}")
        if gap is not None:
            qs = np.unique(np.argwhere(mism)[:, 0])
            # "well separated" is relative to what float32 resolves at the distances' magnitude
            # (SIFT-valued descriptors: |D| ~ 3e6, one float32 ulp = 0.25)
            lim = 1e-4 + 2e-6 * np.abs(D_ref.astype(np.float64)).max(axis=1)
            assert (gap[qs] < lim[qs]).all(), "id mismatch on a query whose ranks are well separated"
    return int(mism.sum())


def seeded_inputs(kind: str, seed: int, n: int, d: int, nq: int):
    """Inputs of a SEEDED golden fixture (tests/golden/seeded_*.npz): the fixture stores the seed and
    the expected (I, D, gap) only -- SURVEY.md 8c's full-size cases (4096 x 512, 2048 x 128 vs 256)
    would be megabytes as stored arrays -- and the inputs are regenerated here, bit for bit."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, d), dtype=np.float32), rng.random((nq, d), dtype=np.float32)
    if kind == "uniform_unit":   # IP on L2-normalised rows (create_search_index("cosine"))
        xb, xq = rng.random((n, d), dtype=np.float32), rng.random((nq, d), dtype=np.float32)
        return ko.normalize_rows(xb), ko.normalize_rows(xq)
    if kind == "assign":         # k = 1 assignment: n unit-norm centroids, nq SIFT-valued descriptors
        cent = ko.normalize_rows(rng.standard_normal((n, d)).astype(np.float32))
        return cent, rng.integers(0, 256, (nq, d)).astype(np.float32)
    raise ValueError(kind)


def load_fixture(path):
    """-> dict with xb, xq, k, metric, D, I, gap for stored and for seeded fixtures alike."""
    z = np.load(path)
    out = {key: z[key] for key in z.files}
    if "seed" in out:
        out["xb"], out["xq"] = seeded_inputs(str(out["kind"]), int(out["seed"]), int(out["n"]), int(out["d"]),
                                             int(out["nq"]))
    return out


# ------------------------------------------------------------------ integer data: exact arithmetic, strict order
# Small integers make every product and every partial sum of a dot product, a squared norm or sum (x - y)^2 an
# integer below 2^24: float32 arithmetic is then exact in ANY summation order, and bf16 holds every integer up
# to 256 exactly.  On such data a kernel's D must equal the exact score bit for bit, and the only correct I is
# the (score, id) order with ties by ascending id.
EXACT_LIMIT = 1 << 24

INT_KINDS = {"binary": (0, 1),    # dense ties: hundreds to thousands of rows per distance at small d
             "small": (0, 15),    # sparse, scattered tie groups
             "signed": (-2, 2)}   # many exact-zero inner products (a +0 / -0 key mismatch shows up here)


def int_data(kind: str, rng, n: int, d: int) -> np.ndarray:
    """(n, d) float32 of integers drawn uniformly from the kind's range (INT_KINDS)."""
    lo, hi = INT_KINDS[kind]
    return rng.integers(lo, hi + 1, (n, d)).astype(np.float32)


def plant_ties(xb: np.ndarray, src: int, ids) -> np.ndarray:
    """Copy row ``src`` onto every row in ``ids`` (in place; returns xb): one tie group {src} | ids for every
    query -- a consecutive run, a run straddling a block or shard boundary, or ids far apart."""
    xb[np.asarray(ids, dtype=np.int64)] = xb[src]
    return xb


def level_rows(rng, sizes, d: int, far: int, n: int) -> np.ndarray:
    """(n, d) binary rows in tie groups of the given sizes -- group j is ``sizes[j]`` copies of the row whose
    first j + 1 entries are 1 -- at random ids; every other row has ``far`` or more ones at random places.
    Against the all-zero query (L2: distance = number of ones) and the all-minus-one query (inner product:
    score = -number of ones) group j occupies ranks sum(sizes[:j]) .. sum(sizes[:j + 1]) - 1."""
    assert sum(sizes) <= n and len(sizes) < far <= d
    filler = n - sum(sizes)
    rest = (np.arange(d)[None, :] < rng.integers(far, d + 1, filler)[:, None]).astype(np.float32)
    groups = [np.repeat((np.arange(d) <= j).astype(np.float32)[None, :], s, axis=0) for j, s in enumerate(sizes)]
    xb = np.concatenate(groups + [rng.permuted(rest, axis=1)])
    return np.ascontiguousarray(xb[rng.permutation(n)])


def assert_exact_range(xb: np.ndarray, xq: np.ndarray):
    """The inputs are integers and every |partial sum| of x.y, sum (x - y)^2, |x|^2 + |y|^2 and the expanded
    form |x|^2 + |y|^2 - 2 x.y stays below 2^24 (bounded by (|x| + |y|)^2 over the largest norms)."""
    for a in (xb, xq):
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a)), "integer-valued float32 expected"
    A = float(np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64)).max(initial=0.0))
    B = float(np.einsum("ij,ij->i", xq.astype(np.float64), xq.astype(np.float64)).max(initial=0.0))
    bound = (np.sqrt(A) + np.sqrt(B)) ** 2
    assert bound < EXACT_LIMIT, f"inputs leave float32's exact integer range: bound {bound:.0f}"
    return bound


def assert_knn_identical(D, I, D_ref, I_ref, what=""):
    """Bit-for-bit equality with the exact answer: dtypes, shapes, padding positions, every id and every
    distance's float32 bits (so the sign of a zero too).  No tolerance and no near-tie escape: for integer data
    (assert_exact_range) nothing else is correct."""
    D, I = np.asarray(D), np.asarray(I)
    assert D.dtype == np.float32 and I.dtype == np.int64, (D.dtype, I.dtype, what)
    assert D.shape == D_ref.shape and I.shape == I_ref.shape, (D.shape, D_ref.shape, what)
    assert np.array_equal(I < 0, I_ref < 0), f"padding (-1) positions differ {what}"
    if not np.array_equal(I, I_ref):
        q, r = np.argwhere(I != I_ref)[0]
        raise AssertionError(f"ids differ {what}: {int((I != I_ref).sum())} slots, first at query {q} rank {r}: "
                             f"got {I[q, max(0, r - 2):r + 3].tolist()} want {I_ref[q, max(0, r - 2):r + 3].tolist()}"
                             f" at D {D_ref[q, max(0, r - 2):r + 3].tolist()}")
    bits, bits_ref = D.view(np.uint32), np.asarray(D_ref, np.float32).view(np.uint32)
    if not np.array_equal(bits, bits_ref):
        q, r = np.argwhere(bits != bits_ref)[0]
        raise AssertionError(f"distances differ {what}: {int((bits != bits_ref).sum())} slots, first at query {q} "
                             f"rank {r}: got {D[q, r]!r} want {D_ref[q, r]!r}")


# ------------------------------------------------------------- non-finite and overflowing rows and queries
# Faiss's gate decides what enters: an L2 score enters only if it is < FLT_MAX (NaN and inf never do), an inner
# product only if it is > -FLT_MAX (+inf does, with D = +inf; NaN and -inf never do).  The data stay integers, so
# every finite score is still exact in any order; the non-finite entries give inf or NaN whatever the order.
POISONS = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "all_nan": np.nan}
HUGE = np.float32(2.0 ** 64)  # an exact power of two whose square (2^128) already overflows float32


def poison(x: np.ndarray, ids, kind: str, col: int = 0) -> np.ndarray:
    """In place (returns x): rows ``ids`` get a NaN, +inf or -inf at column ``col``, or (all_nan) NaN everywhere."""
    ids = np.asarray(ids, dtype=np.int64)
    if kind == "all_nan":
        x[ids] = np.nan
    else:
        x[ids, col] = POISONS[kind]
    return x


def plant_decoys(xb: np.ndarray, xq: np.ndarray, ids, kind: str, col: int = 0) -> np.ndarray:
    """Rows ``ids`` become copies of the queries (row ids[i] <- query i mod nq) and are then poisoned: a gate that
    lets one of them through puts a wrong id at rank 0 of that query, not in the tail.  In place; returns xb."""
    ids = np.asarray(ids, dtype=np.int64)
    xb[ids] = xq[np.arange(len(ids)) % xq.shape[0]]
    return poison(xb, ids, kind, col)


def decoy_ids(n: int, extra=()) -> list:
    """Ids where a poisoned row sits: the first and last row, both sides of the 16-row tile edges next to them and
    in the middle, and the given block or shard boundaries (and their left neighbours)."""
    ids = {0, 15, 16, n // 2 - 1, n // 2, n - 17, n - 16, n - 1}
    for b in extra:
        ids |= {b - 1, b}
    return sorted(i for i in ids if 0 <= i < n)


def assert_nonfinite_range(xb: np.ndarray, xq: np.ndarray, metric: int):
    """The guard of assert_exact_range for poisoned data.  Non-finite entries are ignored; every finite entry is an
    integer, and an entry of magnitude 2^24 or more is +-HUGE (float32 L2 only).  Rows and queries without a HUGE
    entry keep every sum below 2^24 (assert_exact_range), and every float32 L2 distance of a pair with a HUGE entry
    is either at most FLT_MAX / 4 -- no partial sum overflows, and the HUGE parts cancel exactly -- or at least
    2 FLT_MAX, so every summation order overflows to inf: no score depends on the order it was summed in."""
    for a in (xb, xq):
        assert a.dtype == np.float32
        f = a[np.isfinite(a)]
        assert np.array_equal(f, np.rint(f)), "integer-valued float32 expected"
        big = np.abs(f) >= EXACT_LIMIT
        assert (np.abs(f[big]) == HUGE).all(), "large entries must be +-HUGE"
    hb = (np.abs(np.nan_to_num(xb, posinf=0, neginf=0)) >= EXACT_LIMIT).any(1)
    hq = (np.abs(np.nan_to_num(xq, posinf=0, neginf=0)) >= EXACT_LIMIT).any(1)
    assert_exact_range(np.nan_to_num(xb[~hb], nan=0, posinf=0, neginf=0),
                       np.nan_to_num(xq[~hq], nan=0, posinf=0, neginf=0))
    if hb.any() or hq.any():
        assert metric == ko.METRIC_L2, "HUGE entries are for float32 L2 only"
        fin_b, fin_q = np.isfinite(xb).all(1), np.isfinite(xq).all(1)
        for rows, qs in ((hb & fin_b, fin_q), (fin_b, hq & fin_q)):
            if rows.any() and qs.any():
                dd = ko.pairwise_f64(xq[qs], xb[rows], ko.METRIC_L2)
                lim = float(ko.FLT_MAX)
                assert ((dd <= lim / 4) | (dd >= 2 * lim)).all(), "a HUGE pair lies between FLT_MAX / 4 and 2 FLT_MAX"


def brute_knn(xb: np.ndarray, xq: np.ndarray, k: int, metric: int, id_offset: int = 0):
    """Per-query float64 brute force with Faiss's gate written out, independent of knn_oracle's blocking, centring
    and re-scoring: L2 = sum (x - y)^2 entry by entry, IP = sum x * y entry by entry (no BLAS)."""
    nq = xq.shape[0]
    D = np.full((nq, k), ko.FLT_MAX if metric == ko.METRIC_L2 else -ko.FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    b = xb.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            x = xq[q].astype(np.float64)
            if metric == ko.METRIC_L2:
                s = ((b - x) ** 2).sum(1)
                ok = s < float(ko.FLT_MAX)  # NaN, inf and >= FLT_MAX never enter
                key = s
            else:
                s = (b * x).sum(1)
                ok = s > -float(ko.FLT_MAX)  # NaN and -inf never enter; +inf does
                key = -s
            ids = np.flatnonzero(ok)
            order = ids[np.lexsort((ids, key[ids]))][:k]
            D[q, :len(order)] = s[order].astype(np.float32)
            I[q, :len(order)] = order + id_offset
    return D, I
