"""CPU tests of the oracle on NaN, inf and overflowing rows and queries (tests/knn_checks.py).

``knn_exact`` is checked against an independent per-query float64 brute force with Faiss's gate written out, on
both of its branches (direct scores, and the centred expanded form above 2^26 multiply-adds), for both metrics.
``normalize_rows`` is checked against the C restatement of fvec_renorm_L2 on its edge rows."""
import zlib

import numpy as np
import pytest

from oracle import flat_oracle as fo
from oracle import knn_oracle as ko
from tests.knn_checks import (HUGE, assert_knn_identical, assert_nonfinite_range, brute_knn, decoy_ids, int_data,
                              plant_decoys, poison)

L2, IP = ko.METRIC_L2, ko.METRIC_INNER_PRODUCT
BRANCHES = {"direct": (2000, 16, 8), "expanded": (70_000, 64, 16)}  # (n, d, nq); 70000 * 16 * 64 > 2^26


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _check(xb, xq, k, metric):
    assert_nonfinite_range(xb, xq, metric)
    D_ref, I_ref = brute_knn(xb, xq, k, metric)
    D, I = ko.knn_exact(xb, xq, k, metric)
    assert_knn_identical(D, I, D_ref, I_ref, "oracle vs brute force")
    return D, I


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf", "all_nan"])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_oracle_on_poisoned_rows(branch, metric, kind):
    """Poisoned copies of the queries at the first and last ids and on tile edges: none enters L2 (and no other
    row is lost); for inner product +inf scores enter first, ordered by id."""
    n, d, nq = BRANCHES[branch]
    assert (n * nq * d > 2**26) == (branch == "expanded")
    rng = _rng("rows", branch, metric, kind)
    xb, xq = int_data("signed", rng, n, d), int_data("signed", rng, nq, d)
    xq[:, 0] = rng.choice([-1.0, 0.0, 1.0], nq)  # +inf meets positive, zero and negative query entries
    ids = decoy_ids(n)
    plant_decoys(xb, xq, ids, kind)
    D, I = _check(xb, xq, 20, metric)
    if metric == L2 or kind not in ("inf", "-inf"):
        assert not np.isin(I, ids).any()
    else:  # +-inf times a query entry of the same sign: +inf, first; of the other sign or zero: never
        plus = xq[:, 0] * (1.0 if kind == "inf" else -1.0) > 0
        assert np.isin(I[plus, 0], ids).all() and (D[plus, 0] == np.inf).all()
        assert not np.isin(I[~plus], ids).any()


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf", "all_nan"])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_oracle_on_poisoned_queries(branch, metric, kind):
    """A batch mixing poisoned and clean queries against rows with a poisoned entry too: L2 gives the poisoned
    queries a row of padding; the clean ones keep their answers."""
    n, d, nq = BRANCHES[branch]
    rng = _rng("queries", branch, metric, kind)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    xb[: n // 3, 1] = -xb[: n // 3, 1]
    poison(xq, [1, nq - 1], kind, col=1)
    poison(xb, [7], "nan", col=2)
    D, I = _check(xb, xq, 10, metric)
    if metric == L2:
        assert (I[[1, nq - 1]] == -1).all()
    clean = np.setdiff1d(np.arange(nq), [1, nq - 1])
    Dc, Ic = ko.knn_exact(xb, xq[clean], 10, metric)
    assert_knn_identical(D[clean], I[clean], Dc, Ic, "clean queries alone")


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_oracle_on_overflowing_rows(branch):
    """float32 L2 rows and queries whose squared norms overflow: row 100 has HUGE in 8 columns and query 0 is row
    100 plus 1 in another column; queries 1.. are ordinary.  Row 100 is query 0's answer at distance 1, and every
    other row is >= 2^131 away from it."""
    n, d, nq = BRANCHES[branch]
    rng = _rng("overflow", branch)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    xb[100, 8:16] = HUGE
    xb[n - 1, 8:16] = -HUGE
    xq[0] = xb[100]
    xq[0, 3] += 1
    D, I = _check(xb, xq, 10, L2)
    assert I[0, 0] == 100 and D[0, 0] == 1.0 and (I[0, 1:] == -1).all()
    assert not np.isin(I[1:], [100, n - 1]).any()


def test_large_l2_input_with_one_nan_row_is_not_all_padding():
    """The expanded branch used to centre on a column mean that one NaN entry made NaN: every score was NaN and
    every slot padding.  The answer must equal that of the direct branch on a slice that holds every answer."""
    rng = _rng("large_nan")
    n, d, nq, k = 70_000, 64, 16, 10
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    xb[5, 3] = np.nan
    D, I = ko.knn_exact(xb, xq, k, L2)
    assert (I >= 0).all()
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert_knn_identical(D, I, D_ref, I_ref, "expanded branch with a NaN row")


def _edge_rows(d):
    rows = {"zero": np.zeros(d), "tiny": np.full(d, 1e-30), "huge": np.full(d, 1e20),
            "nan_entry": np.r_[np.nan, np.arange(1, d)], "inf_entry": np.r_[np.inf, np.arange(1, d)],
            "ninf_entry": np.r_[-np.inf, -np.ones(d - 1)]}
    return {key: v.astype(np.float32) for key, v in rows.items()}


@pytest.mark.parametrize("d", [3, 8, 100])
def test_normalize_rows_edge_rows_match_c_restatement(d):
    """Bit for bit with fvec_renorm_L2's C restatement: zero and tiny rows (float32 |x|^2 = 0) untouched, huge
    rows (|x|^2 overflows) become 0, a NaN entry leaves the row untouched, an inf entry becomes NaN and the
    finite entries 0."""
    edge = _edge_rows(d)
    x = np.stack(list(edge.values()))
    y = x.copy()
    fo.renorm_L2(y)
    got = ko.normalize_rows(x)
    assert np.array_equal(got.view(np.uint32), y.view(np.uint32))
    rows = dict(zip(edge, got))
    for key in ("zero", "tiny", "nan_entry"):
        assert np.array_equal(rows[key].view(np.uint32), edge[key].view(np.uint32)), key
    assert (rows["huge"] == 0).all()
    assert np.isnan(rows["inf_entry"][0]) and (rows["inf_entry"][1:] == 0).all()


def test_poison_helpers():
    rng = _rng("helpers")
    xb, xq = int_data("small", rng, 100, 8), int_data("small", rng, 3, 8)
    ids = decoy_ids(100, extra=[40])
    assert ids[0] == 0 and ids[-1] == 99 and {15, 16, 39, 40} <= set(ids)
    plant_decoys(xb, xq, ids, "inf", col=2)
    assert (xb[ids, 2] == np.inf).all() and np.array_equal(xb[ids[1], 3:], xq[1, 3:])
    poison(xb, [5], "all_nan")
    assert np.isnan(xb[5]).all()
    assert_nonfinite_range(xb, xq, L2)
    bad = xb.copy()
    bad[1, 1] = 2.0**30
    with pytest.raises(AssertionError):
        assert_nonfinite_range(bad, xq, L2)
    gap = xb.copy()
    gap[1, :2] = HUGE  # two HUGE columns: ~2^129 from every other row, above 2 FLT_MAX
    assert_nonfinite_range(gap, xq, L2)
    gap[1, 1] = 0.0  # a single HUGE column: ~2^128, inside the band
    with pytest.raises(AssertionError):
        assert_nonfinite_range(gap, xq, L2)
    with pytest.raises(AssertionError):
        assert_nonfinite_range(gap, xq, IP)
