"""CPU tests of range search: the C ABI's argument errors (no GPU needed) and the float64 restatement the GPU
tests check against (tests/range_ref.py), cross-checked with sklearn and torch float64."""
import ctypes

import numpy as np
import pytest
import torch

from tests.range_ref import IP, L2, assert_range_shape, filter_search, range_ref


def test_range_abi_argument_errors():
    from image_search_engine_amd import _native as n

    out = ctypes.c_void_p(123)
    q = np.zeros((1, 4), dtype=np.float32)
    assert n.lib.ise_index_range_search_host(None, q.ctypes.data, 1, ctypes.c_float(1.0), ctypes.byref(out)) \
        == n.E_INVALID
    assert b"NULL" in n.lib.ise_last_error()
    assert n.lib.ise_index_range_search_host(None, None, -1, ctypes.c_float(1.0), None) == n.E_INVALID
    nq = ctypes.c_int64()
    assert n.lib.ise_range_result_get(None, ctypes.byref(nq), None, None, None) == n.E_INVALID
    st = (ctypes.c_uint64 * 2)()
    assert n.lib.ise_index_range_stats(None, st) == n.E_INVALID


def test_range_result_destroy_null_is_noop():
    from image_search_engine_amd import _native as n

    assert n.lib.ise_range_result_destroy(None) == 0


def test_faiss_compat_has_range_search():
    from image_search_engine_amd import faiss_compat as faiss

    assert callable(getattr(faiss.IndexFlat, "range_search", None))
    assert callable(getattr(faiss.IndexFlat, "range_stats", None))


def _gapped(rng, n, d, nq, metric):
    """Data, queries and a radius with no distance within 1e-6 (relative) of it: sklearn tests <=, we test <."""
    xb = rng.standard_normal((n, d))
    xq = rng.standard_normal((nq, d))
    s = ((xq[:, None, :] - xb[None]) ** 2).sum(-1) if metric == L2 else xq @ xb.T
    for r in np.quantile(s, np.linspace(0.05, 0.5, 40)):
        if (np.abs(s - r) > 1e-6 * max(1.0, abs(r))).all():
            return xb, xq, float(r)
    pytest.skip("no gapped radius")  # pragma: no cover


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_ref_against_torch_cdist(metric):
    rng = np.random.default_rng(3)
    xb, xq, r = _gapped(rng, 300, 12, 7, metric)
    lims, D, I = range_ref(xb, xq, r, metric)
    assert_range_shape(lims, D.astype(np.float32), I, len(xq), len(xb))
    tb, tq = torch.from_numpy(xb), torch.from_numpy(xq)
    s = (torch.cdist(tq, tb) ** 2 if metric == L2 else tq @ tb.T).numpy()
    for i in range(len(xq)):
        keep = s[i] < r if metric == L2 else s[i] > r
        assert np.array_equal(I[lims[i]:lims[i + 1]], np.nonzero(keep)[0])
        assert np.allclose(D[lims[i]:lims[i + 1]], s[i][keep], rtol=1e-9, atol=1e-9)


def test_range_ref_against_sklearn():
    sk = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(4)
    xb, xq, r = _gapped(rng, 400, 9, 5, L2)
    lims, D, I = range_ref(xb, xq, r, L2)
    nn = sk.NearestNeighbors().fit(xb)
    dist, ind = nn.radius_neighbors(xq, radius=np.sqrt(r), sort_results=False)
    for i in range(len(xq)):
        assert np.array_equal(I[lims[i]:lims[i + 1]], np.sort(ind[i]))


def test_filter_search_matches_ref_on_full_search():
    rng = np.random.default_rng(5)
    xb = rng.integers(-3, 4, (50, 6)).astype(np.float64)
    xq = rng.integers(-3, 4, (4, 6)).astype(np.float64)
    s = ((xq[:, None, :] - xb[None]) ** 2).sum(-1)
    order = np.lexsort((np.broadcast_to(np.arange(50), s.shape), s), axis=1)
    D = np.take_along_axis(s, order, 1).astype(np.float32)
    got = filter_search(D, order, 20.0, L2)
    want = range_ref(xb, xq, 20.0, L2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1].astype(np.float32))
