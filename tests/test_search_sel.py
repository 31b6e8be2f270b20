"""CPU tests of the selector-filtered search's host side: how a selector is lowered, the bitmap words, the
SearchParameters checks, the numpy reference of the GPU tests, and the new entry points' argument errors."""
import ctypes

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests.knn_checks import assert_exact_range, assert_knn_identical, brute_knn, int_data
from tests.sel_ref import IP, L2, filter_range, filter_ranking, selector_census


class EveryThird(faiss.IDSelector):
    def is_member(self, i):
        return int(i) % 3 == 0


def test_lowering_picks_the_constructor():
    assert faiss.lower_selector(faiss.IDSelectorRange(5, 9), 100) == ("range", 5, 9)
    kind, ids, inv = faiss.lower_selector(faiss.IDSelectorBatch([7, 3, 3, 900]), 100)
    assert (kind, ids.tolist(), inv) == ("ids", [3, 7, 900], 0)
    kind, ids, inv = faiss.lower_selector(faiss.IDSelectorArray([4]), 100)
    assert (kind, ids.tolist(), inv) == ("ids", [4], 0)
    kind, ids, inv = faiss.lower_selector(faiss.IDSelectorNot(faiss.IDSelectorBatch([4, 2])), 100)
    assert (kind, ids.tolist(), inv) == ("ids", [2, 4], 1)
    assert faiss.lower_selector(faiss.IDSelectorNot(faiss.IDSelectorRange(2, 4)), 100)[0] == "bitmap"
    assert faiss.lower_selector(EveryThird(), 100)[0] == "bitmap"
    with pytest.raises(TypeError):
        faiss.lower_selector([1, 2, 3], 100)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 600])
@pytest.mark.parametrize("make", [lambda n: EveryThird(), lambda n: faiss.IDSelectorNot(faiss.IDSelectorRange(1, n - 1)),
                                  lambda n: faiss.IDSelectorNot(faiss.IDSelectorNot(faiss.IDSelectorBatch([0, n - 1, n])))])
def test_bitmap_words(n, make):
    sel = make(n)
    kind, words = faiss.lower_selector(sel, n)
    assert kind == "bitmap" and words.dtype == np.dtype("<u4") and words.shape == ((n + 31) // 32,)
    for r in range(32 * len(words)):
        bit = (int(words[r >> 5]) >> (r & 31)) & 1
        assert bit == (1 if r < n and sel.is_member(r) else 0), r


def test_search_parameters_validation():
    assert faiss.SearchParameters().sel is None
    s = faiss.IDSelectorRange(0, 3)
    assert faiss.SearchParameters(sel=s).sel is s
    with pytest.raises(TypeError):
        faiss.SearchParameters(sel=[1, 2])
    with pytest.raises(TypeError):
        faiss.SearchParameters(sel=np.arange(3))
    assert faiss._params_sel(None) is None
    assert faiss._params_sel(faiss.SearchParameters()) is None
    with pytest.raises(TypeError):
        faiss._params_sel(s)  # a bare selector is not a SearchParameters


@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_against_brute_force(metric):
    rng = np.random.default_rng(3)
    n, d, nq = 300, 12, 7
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    D_full, I_full = brute_knn(xb, xq, n, metric)
    for sel in (faiss.IDSelectorRange(17, 203), EveryThird(), faiss.IDSelectorBatch([5, 250, 9999]),
                faiss.IDSelectorNot(faiss.IDSelectorRange(10, 290)), faiss.IDSelectorRange(4, 4)):
        m = sel.members(np.arange(n))
        rows = np.flatnonzero(m)
        for k in (1, 10, 40):
            D, I = filter_ranking(D_full, I_full, sel.members, k, metric)
            if rows.size:
                Db, Ib = brute_knn(xb[rows], xq, k, metric)
                Ib = np.where(Ib >= 0, rows[np.maximum(Ib, 0)], -1)
            else:
                Db = np.full((nq, k), D[0, 0], np.float32)
                Ib = np.full((nq, k), -1, np.int64)
            assert_knn_identical(D, I, Db, Ib, f"{type(sel).__name__} k={k}")
        assert selector_census(m)["selected"] == rows.size


def test_reference_range_filter():
    lims = np.array([0, 3, 3, 5], dtype=np.uint64)
    D = np.arange(5, dtype=np.float32)
    I = np.array([1, 4, 6, 0, 3], dtype=np.int64)
    l2, D2, I2 = filter_range((lims, D, I), EveryThird().members)
    assert l2.tolist() == [0, 1, 1, 3] and I2.tolist() == [6, 0, 3] and D2.tolist() == [2.0, 3.0, 4.0]
    assert selector_census(np.array([0, 0, 1] + [0] * 30 + [1], bool)) == {"selected": 2, "window": (2, 34), "tiles": 2}


def test_argument_errors_through_abi():
    from image_search_engine_amd import _native as n

    s, r = ctypes.c_void_p(), ctypes.c_void_p()
    out5, out3 = (ctypes.c_int64 * 5)(), (ctypes.c_uint64 * 3)()
    ids = np.zeros(2, np.int64)
    assert n.lib.ise_selector_create_range(None, 0, 1, ctypes.byref(s)) == n.E_INVALID
    assert b"handle" in n.lib.ise_last_error()
    assert n.lib.ise_selector_create_range(None, 0, 1, None) == n.E_INVALID
    assert n.lib.ise_selector_create_ids(None, ids.ctypes.data, 2, 0, ctypes.byref(s)) == n.E_INVALID
    assert n.lib.ise_selector_create_ids(None, None, 2, 0, None) == n.E_INVALID
    assert n.lib.ise_selector_create_bitmap(None, None, 0, ctypes.byref(s)) == n.E_INVALID
    assert s.value is None
    assert n.lib.ise_selector_info(None, out5) == n.E_INVALID
    assert n.lib.ise_selector_destroy(None) == 0
    assert n.lib.ise_index_search_sel_host(None, None, 1, 1, None, None, None) == n.E_INVALID
    assert n.lib.ise_index_search_sel_device(None, None, 1, 1, None, None, None, None) == n.E_INVALID
    assert n.lib.ise_index_range_search_sel_host(None, None, 1, ctypes.c_float(1.0), None, ctypes.byref(r)) == n.E_INVALID
    assert r.value is None
    assert n.lib.ise_index_sel_stats(None, out3) == n.E_INVALID


def test_no_gpu_means_loud_failure():
    """Without a GPU there is no index to filter: the constructor raises, nothing falls back to the host."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="MI355X|HIP device"):
        faiss.IndexFlatL2(16).search(np.zeros((1, 16), np.float32), 1,
                                     params=faiss.SearchParameters(sel=faiss.IDSelectorRange(0, 1)))
