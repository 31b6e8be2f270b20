"""CPU tests of what tests/test_flat_shapes_gpu.py is built on: the mirrored row-length classes and kp values, the
conditions that keep its chosen radii and selectors from being vacuous (all asserted on the float64 reference alone), and
the brute-force helpers of tests/range_ref.py and tests/sel_ref.py against the older references on one small case."""
import numpy as np
import pytest

from tests import test_flat_shapes_gpu as fs
from tests.knn_checks import assert_exact_range, assert_knn_identical, brute_knn, int_data
from tests.range_ref import (assert_range_identical, range_brute, range_of_scores, range_ref, scores_f64,
                             segment_hits_max)
from tests.sel_ref import IP, L2, filter_range, filter_ranking, knn_of_scores, masked_knn_brute
from tests.test_range_search_gpu import _int_brute


def counts(res):
    return np.diff(res[0].astype(np.int64))


def test_sweeps_cover_every_class_and_the_mirrored_kp():
    """Every (ch, vec_q) pair per storage, the classes the issue computed, kp = 31 / 23 / 10, and the 4-wave windows."""
    fs.test_geometry_mirrors()
    assert [fs.klass(d, "f32") for d in (1, 33, 48, 17, 32, 63, 65, 600, 1000)] == \
        [(1, 0), (1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 0), (4, 1), (4, 0)]
    assert [fs.klass(d, "bf16") for d in (17, 32, 33, 64, 100, 600, 1000)] == \
        [(1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 1), (4, 0)]
    assert fs.row_bytes(65, "f32") == 128 * 4  # padded to four steps beyond four
    assert [fs.flat_kp(d, "f32") for d in (1920, 2048, 2240)] == [fs.flat_kp(d, "bf16") for d in (3840, 4096, 4480)] == [31, 23, 10]
    # the scalar path at a d that is a multiple of 4 (8): the stride is past the threads' 16-byte slots
    assert 1000 % 8 == 0 and (fs.stride(1000, "f32") >> 2) > 8 * 32 and (fs.stride(1000, "bf16") >> 2) > 4 * 32
    # in the 4-wave window the rule has 16 threads per row; every row there is staged by the scalar path anyway
    assert all(fs.vec_staging(d, s) == 0 for s in ("f32", "bf16") for d in fs.FOUR_WAVES[s])


@pytest.mark.parametrize("metric,storage,d", fs.SWEEP_CASES)
def test_sweep_radii_and_selectors_are_not_vacuous(metric, storage, d):
    sels = fs.sweep_selectors(fs.N)
    masks = {name: sel.members(np.arange(fs.N)) for name, sel in sels.items()}
    assert [int(m.sum()) for m in masks.values()] == [288, 200, 60, 200, 600]
    assert 123 % 16 and 411 % 16 and not masks["two_pieces"][100:500].any()
    for kind in fs.KINDS:
        c = fs.sweep_case(metric, storage, d, kind)
        S, radii = c["S"], c["radii"]
        assert np.array_equal(c["xb"][77], c["xq"][0])
        res = {name: range_of_scores(S, r, metric) for name, r in radii.items()}
        assert counts(res["none"]).sum() == 0
        if d > 1:
            # one column has 2 or 16 score levels: no radius keeps 1 .. 50 of 600 rows for every query there
            assert fs.few_radius(S, metric)[1], (d, kind)
            assert counts(res["few"]).min() >= 1 and counts(res["few"]).max() <= 50, (d, kind, counts(res["few"]))
            assert counts(res["median"]).sum() > 17 and segment_hits_max(res["median"]) >= 2  # takes the second pass
        assert radii["few"] % 1 == 0.5 and radii["median"] % 1 == 0.5
        # rows at exactly the attained score exist and stay out; rows inside it exist too
        q, rows = np.nonzero(S == radii["attained"])
        assert len(q) >= 1 and counts(res["attained"]).sum() > 0
        lims = res["attained"][0].astype(np.int64)
        assert all(r not in res["attained"][2][lims[i]:lims[i + 1]] for i, r in zip(q[:20], rows[:20]))
        assert segment_hits_max(res["none"]) == 0  # ... and this radius never does
        for name, m in masks.items():
            if d > 1:
                assert segment_hits_max(range_of_scores(S, radii["median"], metric, m)) >= (1 if name == "tenth" else 2)


@pytest.mark.parametrize("metric,storage,d", fs.KP_CASES)
def test_kp_case_ties(metric, storage, d):
    kp = fs.flat_kp(d, storage)
    c = fs.kp_case(metric, storage, d)
    S = c["S"]
    for name, m in c["masks"].items():
        group = np.flatnonzero(m[:fs.TIES])
        res = range_of_scores(S, c["radii"]["ties"], metric, m)
        assert np.array_equal(res[2][:counts(res)[0]], group) and counts(res)[2:].sum() == 0  # exactly the tie group
        D, I = knn_of_scores(S, m, fs.TIES + 1, metric)
        for q in (0, 1):
            assert np.array_equal(I[q, :len(group)], group) and len(set(D[q, :len(group)].tolist())) == 1
            assert D[q, len(group)] != D[q, 0]
    # all rows selected: the floor of the second pass (rank kp - 1) falls inside the 40 ties
    assert kp < fs.TIES and len(np.flatnonzero(c["masks"]["half"][:fs.TIES])) == 20


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_mixed_overflow_premises(storage):
    c = fs.mixed_overflow_case(storage)
    res = range_of_scores(c["S"], 0.5, L2)
    n = counts(res)
    assert n[5] == 8 and n[260] == 1 and n[299] == 2 and n[:256].sum() == 8 and n[256:].sum() == 3
    assert np.array_equal(res[2][:8], np.arange(200, 208)) and 200 // 16 == 207 // 16


@pytest.mark.parametrize("metric,storage", fs.FLAVOURS)
@pytest.mark.parametrize("nq", [64, 65, 130])
def test_launches_have_their_own_nearest_rows(nq, metric, storage):
    c = fs.sel_chunks_case(metric, storage, nq)
    _, I = knn_of_scores(c["S"], fs.EveryThird().members(np.arange(fs.N)), 1, metric)
    assert (I[fs.SEL_NQ_CHUNK:, 0] != I[:-fs.SEL_NQ_CHUNK, 0]).all()


@pytest.mark.parametrize("metric,storage", fs.FLAVOURS)
@pytest.mark.parametrize("nq", [256, 257, 300])
def test_two_batch_radii_keep_rows_in_both_batches(nq, metric, storage):
    c = fs.two_batch_case(metric, storage, nq)
    for r in c["radii"].values():
        n = counts(range_of_scores(c["S"], r, metric))
        assert n[:256].sum() > 0 and (nq == 256 or n[256:].sum() > 0)


def test_bitmap_words_with_garbage():
    m = np.arange(17) % 3 == 0
    assert fs.bitmap_words(m, False).tolist() == [sum(1 << i for i in range(0, 17, 3))]
    assert fs.bitmap_words(m, True).tolist() == [sum(1 << i for i in range(0, 17, 3)) | (0xFFFFFFFF << 17) & 0xFFFFFFFF]
    assert fs.bitmap_words(np.ones(64, bool), True).tolist() == [0xFFFFFFFF] * 2  # no spare bits: nothing to add


@pytest.mark.parametrize("metric", [L2, IP])
def test_brute_force_helpers_against_the_older_references(metric):
    """range_brute / range_of_scores against _int_brute and range_ref, masked against filter_range; knn_of_scores /
    masked_knn_brute against filter_ranking over brute_knn's complete ranking."""
    rng = np.random.default_rng(5)
    n, d, nq = 200, 12, 9
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    xb[50:60] = xq[0]
    assert_exact_range(xb, xq)
    S = scores_f64(xb, xq, metric)
    mask = rng.random(n) < 0.4
    members = lambda ids: mask[np.asarray(ids, dtype=np.int64)]
    for r in (float(np.median(S)), float(np.median(S)) + 0.5, float(S[0, 50]), np.inf, -np.inf, np.nan):
        got = range_brute(xb, xq, r, metric)
        assert_range_identical(got, _int_brute(xb, xq, r, metric) if np.isfinite(r) else range_ref(xb, xq, r, metric), f"radius {r}")
        assert_range_identical(range_brute(xb, xq, r, metric, mask), filter_range(got, members), f"masked, radius {r}")
    assert segment_hits_max(range_brute(xb, xq, float(S[0, 50]) + (0.5 if metric == L2 else -0.5), metric)) >= 10
    full = brute_knn(xb, xq, n, metric)
    for k in (1, 7, 150):
        want = filter_ranking(*full, members, k, metric)
        assert_knn_identical(*knn_of_scores(S, mask, k, metric), *want, f"k={k}")
        assert_knn_identical(*masked_knn_brute(xb, xq, mask, k, metric), *want, f"k={k} from the rows")
    assert_knn_identical(*knn_of_scores(S, np.zeros(n, bool), 3, metric), *filter_ranking(*full, lambda ids: np.zeros(len(ids), bool), 3, metric), "none")
