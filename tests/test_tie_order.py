"""CPU tests of the integer-data tools behind the tie-order GPU tests (tests/test_tie_order_gpu.py).

On small integers float32 arithmetic is exact in any summation order, so the only correct answer is the exact
score with ties by ascending id.  These tests show that the generators stay inside that range, that the oracles
agree bit for bit with an int64 brute force on such data, and that ``assert_knn_identical`` catches a tie
misorder that ``assert_knn_matches`` lets through."""
import numpy as np
import pytest

from oracle import flat_oracle as fo
from oracle import knn_oracle as ko
from tests.knn_checks import (INT_KINDS, assert_exact_range, assert_knn_identical, assert_knn_matches, int_data,
                              level_rows, plant_ties)

L2, IP = ko.METRIC_L2, ko.METRIC_INNER_PRODUCT
KIND_D = {"binary": 16, "small": 64, "signed": 64}


def brute_int64(xb, xq, k, metric, id_offset=0):
    """int64 scores, then (score, id) order by np.lexsort: the definition, with no float anywhere."""
    b, q = xb.astype(np.int64), xq.astype(np.int64)
    S = ((q[:, None, :] - b[None, :, :]) ** 2).sum(-1) if metric == L2 else q @ b.T
    key = S if metric == L2 else -S
    ids = np.arange(xb.shape[0], dtype=np.int64) + id_offset
    D = np.full((xq.shape[0], k), ko.FLT_MAX if metric == L2 else -ko.FLT_MAX, np.float32)
    I = np.full((xq.shape[0], k), -1, np.int64)
    for i in range(xq.shape[0]):
        order = np.lexsort((ids, key[i]))[:k]
        D[i, :len(order)] = S[i, order]
        I[i, :len(order)] = ids[order]
    return D, I


# (kind, n, d, nq) of every integer data set tests/test_tie_order_gpu.py builds
GPU_SHAPES = [("binary", 100_000, 16, 64), ("small", 100_000, 64, 64), ("signed", 100_000, 64, 64),
              ("binary", 300_000, 96, 48), ("small", 300_000, 96, 48), ("small", 50_000, 64, 65),
              ("small", 3000, 2048, 16), ("small", 140_000, 128, 300),
              ("binary", 140_000, 128, 300), ("small", 256, 64, 4096), ("binary", 256, 32, 4096)]


@pytest.mark.parametrize("kind,n,d,nq", GPU_SHAPES)
def test_generated_data_stays_in_the_exact_range(kind, n, d, nq):
    rng = np.random.default_rng(n + d)
    xb, xq = int_data(kind, rng, n, d), int_data(kind, rng, nq, d)
    lo, hi = INT_KINDS[kind]
    assert xb.min() == lo and xb.max() == hi
    plant_ties(xb, 3, [n // 2, n // 2 + 1, n - 1])
    assert (xb[[n // 2, n // 2 + 1, n - 1]] == xb[3]).all()
    assert assert_exact_range(xb, xq) < 1 << 24
    # bf16 holds every one of these values exactly (8 significant bits, |x| <= 256)
    torch = pytest.importorskip("torch")
    assert np.array_equal(torch.from_numpy(xb[:1000]).to(torch.bfloat16).to(torch.float32).numpy(), xb[:1000])


def test_level_rows_and_the_range_guard():
    rng = np.random.default_rng(3)
    xb = level_rows(rng, [18, 36, 36, 10], 64, 6, 50_000)
    assert_exact_range(xb, -np.ones((1, 64), np.float32))
    D, _ = ko.knn_exact(xb, np.zeros((1, 64), np.float32), 100, L2)
    assert D[0].tolist() == [1.0] * 18 + [2.0] * 36 + [3.0] * 36 + [4.0] * 10
    with pytest.raises(AssertionError, match="exact integer range"):
        assert_exact_range(np.full((2, 512), 255, np.float32), np.full((1, 512), 255, np.float32))
    with pytest.raises(AssertionError, match="integer-valued"):
        assert_exact_range(np.full((2, 4), 0.5, np.float32), np.ones((1, 4), np.float32))
    # signed data: many exact-zero inner products
    x = int_data("signed", rng, 500, 64)
    assert ((x[:50] @ x[50:].T) == 0).sum() > 100


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", sorted(INT_KINDS))
def test_oracles_agree_bit_for_bit_on_integer_data(kind, metric):
    """knn_exact, the C restatement and an int64 brute force: the same D and I, for k beyond the number
    of distinct scores (binary rows at d = 16 have at most 17) and for k > n (padding)."""
    fo.build()
    rng = np.random.default_rng(len(kind) + metric)
    d = KIND_D[kind]
    xb, xq = int_data(kind, rng, 300, d), int_data(kind, rng, 9, d)
    plant_ties(xb, 4, [5, 150, 299])
    xq[0] = xb[4]
    for k in (40, 305):
        want = brute_int64(xb, xq, k, metric)
        if kind == "binary" and k == 40:
            assert max(len(np.unique(r)) for r in want[0]) <= 8  # 40 results over at most 8 distinct scores
        for got in (ko.knn_exact(xb, xq, k, metric), fo.knn_flat(xb, xq, k, metric, 0)[:2],
                    fo.knn_flat(xb, xq, k, metric, 3)[:2]):
            assert_knn_identical(*got, *want)


@pytest.mark.parametrize("metric", [L2, IP])
def test_oracle_keeps_tie_order_behind_the_expanded_form(metric):
    """Large enough for knn_exact's blocked expanded form (L2 around the column mean, which is no integer): the
    float64 rounding of that form used to split exact ties by rounding error instead of by id."""
    rng = np.random.default_rng(11 + metric)
    xb, xq = int_data("binary", rng, 140_000, 16), int_data("binary", rng, 40, 16)
    assert xb.shape[0] * xq.shape[0] * xb.shape[1] > 2**26
    want = brute_int64(xb, xq, 40, metric)
    assert_knn_identical(*ko.knn_exact(xb, xq, 40, metric), *want)


@pytest.mark.parametrize("metric", [L2, IP])
def test_merge_shards_with_ties_across_shard_boundaries(metric):
    """Unequal shards, one smaller than k, tie groups on both sides of every boundary: merged == unsharded."""
    rng = np.random.default_rng(21 + metric)
    n, d, k = 300, 16, 25
    xb, xq = int_data("binary", rng, n, d), int_data("binary", rng, 8, d)
    plant_ties(xb, 2, [12, 13, 179, 180, 299])
    xq[0] = xb[2]
    bounds = [0, 13, 180, n]
    parts = [ko.knn_exact(xb[lo:hi], xq, k, metric, id_offset=lo) for lo, hi in zip(bounds, bounds[1:])]
    assert (parts[0][1] == -1).any()  # the 13-row shard pads
    D, I = ko.merge_shards([p[0] for p in parts], [p[1] for p in parts], k, metric)
    assert_knn_identical(D, I, *brute_int64(xb, xq, k, metric))
    if metric == L2:  # the planted group, at distance 0, spans all three shards
        assert set(I[0][D[0] == 0]) >= {2, 12, 13, 179, 180, 299}


def test_identical_check_catches_what_the_tolerant_check_accepts():
    """Swapping two tied ids passes assert_knn_matches (an exact tie is within its near-tie bound) and fails
    assert_knn_identical; so does a distance off by one."""
    rng = np.random.default_rng(5)
    xb, xq = int_data("binary", rng, 2000, 16), int_data("binary", rng, 4, 16)
    D, I = ko.knn_exact(xb, xq, 20, L2)
    q, r = next((q, r) for q in range(4) for r in range(19) if D[q, r] == D[q, r + 1])
    bad = I.copy()
    bad[q, [r, r + 1]] = bad[q, [r + 1, r]]
    assert_knn_matches(D, bad, D, I, xb, xq, L2)
    with pytest.raises(AssertionError, match="ids differ"):
        assert_knn_identical(D, bad, D, I)
    off = D.copy()
    off[1, 7] += 1
    with pytest.raises(AssertionError, match="distances differ"):
        assert_knn_identical(off, I, D, I)
    pad = I.copy()
    pad[2, -1] = -1
    with pytest.raises(AssertionError, match="padding"):
        assert_knn_identical(D, pad, D, I)
    assert_knn_identical(D, I, D, I)
