"""CPU tests of tests/select_ref.py: the generators give what the headers require of their inputs, the path model of
merge_waves gives hand-worked answers, and the GPU test's merge families reach both of merge_waves' paths."""
import numpy as np
import pytest

from tests import select_ref as sr
from tests.select_ref import PAD, SENT, U64


def u(*v):
    return np.array(v, dtype=U64)


def assert_keys_ok(keys):
    keys = np.asarray(keys, dtype=U64).ravel()
    real = keys[keys != PAD]
    assert len(np.unique(real)) == len(real), "keys repeat"
    assert (real > 0).all() and (real != SENT).all()


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_key_families(family):
    rng = np.random.default_rng(5)
    for count in (0, 1, 2, 3, 64, 1000):
        keys = sr.make_keys(rng, count, family)
        assert keys.dtype == U64 and len(keys) == count
        assert_keys_ok(keys)
        hi, lo = keys >> U64(32), keys & U64(0xFFFFFFFF)
        if family == "tiedhi" and count:
            assert len(np.unique(hi)) <= 3 and len(np.unique(lo)) == count
        if family == "eqlo" and count:
            assert len(np.unique(lo)) == 1 and len(np.unique(hi)) == count
        if family == "extremes" and count >= 2:
            assert U64(1) in keys and PAD - U64(1) in keys


def test_score_keys_decode_to_finite_distances():
    from tests import keycodec

    for tied in (False, True):
        keys = sr.score_keys(np.random.default_rng(1), 1024 * 2048, tied)
        assert (np.diff(keys.astype(np.float64)) >= 0).all() and len(np.unique(keys)) == len(keys)
        assert (keys < PAD).all() and (keys != SENT).all()
        D, _ = keycodec.decode(keys[[0, -1]], 1)
        assert np.isfinite(D).all() and (D >= 0).all()
        if tied:
            assert len(np.unique(keys[:4096] >> U64(32))) < 4


@pytest.mark.parametrize("kpl", [1, 2, 4, 5, 8, 16])
def test_window_cases(kpl):
    """Every case keeps the input contract; the grid of the counts, sizes and placements is all there."""
    for cases, windows in ((sr.select_cases(kpl), [(k, k) for k in sr.SEL_K]),) + (
            ((sr.cut_cases(kpl), sr.CUT_WINDOWS),) if kpl in (1, 2, 4) else ()):
        seen = set()
        for c in cases:
            inp, n = c["inp"], c["n"]
            assert inp.shape == (64 * kpl,) and n % 64 == 0 and 0 <= n <= 64 * kpl
            assert (inp[n:] == PAD).all(), "an element at or beyond n is not empty"
            assert int((inp != PAD).sum()) == c["nreal"]
            assert_keys_ok(inp)
            seen.add((n, c["lo"], c["hi"], c["nreal"]))
            where = np.flatnonzero(inp != PAD)
            if c["placement"] == "lanes7":
                assert (where % 64 >= 7).all()
            if c["placement"] == "lane63":
                assert (where % 64 == 63).all()
            if c["placement"] == "lastreg" and len(where):
                assert (where >= n - 64).all()
            if c["placement"] == "onepereg":
                assert len(np.unique(where // 64)) == len(where)
        for n in range(0, 64 * kpl + 1, 64):
            for lo, hi in windows:
                for nreal in sr.counts_for(n, hi, kpl):
                    assert (n, lo, hi, nreal) in seen
        assert {c["placement"] for c in cases} == set(sr.PLACEMENTS_ANY + sr.PLACEMENTS_SHAPED)
        assert {c["family"] for c in cases} == set(sr.FAMILIES)
        # both sides of wave_select's switch to quickselect (more than k and more than 40 keys), and wave_cut's regimes
        assert any(c["nreal"] > c["hi"] and c["nreal"] > 40 for c in cases)
        assert any(c["nreal"] > c["hi"] and c["nreal"] <= 40 for c in cases)
        assert any(c["lo"] <= c["nreal"] <= c["hi"] for c in cases) and any(0 < c["nreal"] < c["lo"] for c in cases)


def test_counts_for():
    assert sr.counts_for(128, 16, 2) == [0, 1, 15, 16, 17, 40, 41, 63, 64, 65, 127, 128]
    assert sr.counts_for(64, 48, 4) == [0, 1, 40, 41, 47, 48, 49, 63, 64]


def test_topk_cases():
    cases = sr.topk_cases()
    assert {(c["n"], c["k"]) for c in cases} == {(n, k) for n in sr.TOPK_N for k in sr.TOPK_K}
    assert any(c["n"] < c["k"] for c in cases)
    for c in cases:
        assert len(c["keys"]) == c["n"]
        assert_keys_ok(c["keys"])


def test_checkers_reject_wrong_outputs():
    """check_select and check_cut fail on each kind of wrong output they exist to catch."""
    inp = np.concatenate([u(50, 10, 40, 20, 30), np.full(59, PAD, dtype=U64)])

    def sel(dst, nw, kth, k=3):
        full = np.full(72, SENT, dtype=U64)
        full[:len(dst)] = dst
        sr.check_select(inp, 64, k, full, nw, kth)

    sel(u(10, 20, 30), 3, U64(30))
    sel(u(10, 20, 30, 40, 50), 5, SENT, k=8)
    for bad in (lambda: sel(u(10, 30, 20), 3, U64(30)), lambda: sel(u(10, 20, 30, 40), 3, U64(30)),
                lambda: sel(u(10, 20, 30), 3, SENT), lambda: sel(u(10, 20, 30, 40, 50), 5, U64(50), k=8),
                lambda: sel(u(10, 20), 2, U64(20))):
        with pytest.raises(AssertionError):
            bad()

    def cut(dst, cnt, c, kmin, kmax):
        full = np.full(72, SENT, dtype=U64)
        full[:len(dst)] = dst
        sr.check_cut(inp, 64, kmin, kmax, full, cnt, c)

    cut(u(20, 10, 30), 3, U64(30), 2, 3)
    cut(u(20, 10), 2, U64(20), 2, 3)
    cut(u(50, 10, 40, 20, 30), 5, U64(50), 5, 8)
    cut(u(50, 10, 40, 20, 30), 5, SENT, 6, 8)
    for bad in (lambda: cut(u(20, 10, 30, 40), 4, U64(40), 2, 3), lambda: cut(u(20, 10, 40), 3, U64(40), 2, 3),
                lambda: cut(u(20, 10, 30), 3, U64(29), 2, 3), lambda: cut(u(50, 10, 40, 20, 30), 5, U64(50), 6, 8),
                lambda: cut(u(50, 10, 40, 20), 4, U64(50), 4, 8), lambda: cut(u(20, 10, 30, 40), 3, U64(30), 2, 3)):
        with pytest.raises(AssertionError):
            bad()


def test_merge_model_hand_worked():
    """Six written-out cases.  List l sits in wave l % 8; a wave collects its 8 smallest keys."""
    # 1. k <= 8: pre == k, the full path is never taken -- however many winners one wave holds
    res, full = sr.merge_model([u(1, 2, 3, 4, 5, 6, 7, 8), u(9)], 8)
    assert list(res) == [1, 2, 3, 4, 5, 6, 7, 8] and full == 0
    # 2. the winners spread, one per wave and a second in wave 0 (lists 0 and 8): every wave's 8th key is PAD -> fast
    res, full = sr.merge_model([u(l + 1) for l in range(9)], 9)
    assert list(res) == list(range(1, 10)) and full == 0
    # 3. nine winners in wave 0 (lists 0 and 8): it collects 1..8, wave 1 collects 100, T = 100 > 8 -> full; the
    #    fast path alone would have answered 1..8, 100
    res, full = sr.merge_model([u(1, 2, 3, 4, 5, 6, 7, 8), u(100)] + [u()] * 6 + [u(9)], 9)
    assert list(res) == list(range(1, 10)) and full == 1
    # 4. exactly eight winners in wave 0 and its 8th IS the 9th of all (T = 9): done -> fast
    res, full = sr.merge_model([u(2, 3, 4, 5, 6, 7, 8, 9), u(1, 50)], 9)
    assert list(res) == list(range(1, 10)) and full == 0
    # 5. exactly eight winners in wave 0 but the 9th of all is wave 1's: 8 < T = 9, and the rule cannot know that
    #    wave 0 holds no ninth -> full
    res, full = sr.merge_model([u(1, 2, 3, 4, 5, 6, 7, 8), u(9, 50)], 9)
    assert list(res) == list(range(1, 10)) and full == 1
    # 6. fewer than k keys collected: T = PAD, and wave 0 with 8 real keys is unfinished -> full; with 7 it is done
    res, full = sr.merge_model([u(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)], 16)
    assert list(res) == list(range(1, 11)) and full == 1
    res, full = sr.merge_model([u(1, 2, 3, 4, 5, 6, 7)], 16)
    assert list(res) == list(range(1, 8)) and full == 0


@pytest.mark.parametrize("n_lists", sr.MERGE_N_LISTS)
def test_merge_families_reach_both_paths(n_lists):
    """In every (n_lists, k > 8) family of the GPU test the model predicts both paths; the cases are valid inputs; the
    batch model agrees with the written-out one; and the placements built for one path take it."""
    for k in sr.MWAVES_K:
        names, lists = sr.merge_family_cases(n_lists, k)
        assert lists.shape[1:] == (n_lists, k)
        res, need = sr.merge_model_batch(lists, k)
        for i, name in enumerate(names):
            assert_keys_ok(lists[i])
            srt = np.sort(lists[i], axis=1)
            assert np.array_equal(srt, lists[i]), "a list is not ascending with PAD behind"
            if i % 5 == 0 or n_lists <= 9:
                r1, n1 = sr.merge_model(list(lists[i]), k)
                assert n1 == need[i] and np.array_equal(sr.padded(r1, k), res[i]), name
            if name.startswith("w8fast") or name.startswith("tiny"):
                assert need[i] == 0, name
            if k > 8 and name.startswith(("w8slow", "w9", "list:")):
                assert need[i] == 1, name
        if k > 8:
            assert need.min() == 0 and need.max() == 1, (n_lists, k)
        else:
            assert need.max() == 0
        assert "spread/rand" in names and "few/" in " ".join(names)
        if n_lists >= 64 and k > 8:
            assert any(n.startswith("w8fast") for n in names) and any(n.startswith("w9") for n in names)


def test_cand_model_and_streams():
    keys = u(9, 3, PAD, 7, 5, 1)
    assert list(sr.cand_model(keys, 0, 3)) == [1, 3, 5]
    assert list(sr.cand_model(keys, 4, 4)) == [5, 7, 9, PAD]
    assert list(sr.cand_model(keys, PAD, 2)) == [PAD, PAD]
    for order in sr.CAND_ORDERS:
        for partial in (False, True):
            s = sr.cand_stream(5, 3, order, partial, 0)
            assert s.shape == (3, 320)
            for q in range(3):
                assert_keys_ok(s[q])
                real = s[q][s[q] != PAD]
                assert len(real) == (320 - 4 * min(63, 1 + 5 * q) if partial else 320)
                if order == "asc":
                    assert (np.diff(real.astype(np.float64)) >= 0).all() and np.array_equal(np.sort(real), real)
                if order == "desc":
                    assert np.array_equal(np.sort(real)[::-1], real)
