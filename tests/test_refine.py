"""CPU tests of subset scoring and IndexRefine's host side: the numpy reference of the GPU tests, the "IxRF" file
format, the new entry points' argument errors through the C ABI (no device is touched) and the search parameters."""
import ctypes

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests.knn_checks import assert_knn_identical, brute_knn, int_data
from tests.refine_ref import refine_ref
from tests.sel_ref import IP, L2, pad_value


@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_agrees_with_a_masked_brute_force(metric):
    """refine_ref is the brute force over the whole index with every row outside the candidate set masked out."""
    rng = np.random.default_rng(11)
    n, d, nq, kc, k = 200, 12, 7, 30, 9
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    cand = rng.integers(-3, n + 3, (nq, kc))  # some entries outside [0, n), natural duplicates
    cand[2] = -1                              # an all-invalid row
    cand[3, :] = cand[3, 0]                   # one id, kc times
    D, I = refine_ref(xb, xq, cand, k, metric)
    Dw = np.full((nq, k), pad_value(metric), np.float32)
    Iw = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        mask = np.zeros(n, dtype=bool)
        ok = (cand[q] >= 0) & (cand[q] < n)
        mask[cand[q][ok]] = True
        Df, If = brute_knn(xb, xq[q:q + 1], n, metric)  # the complete ranking
        keep = np.flatnonzero(mask[If[0]])[:k]
        Dw[q, :len(keep)] = Df[0, keep]
        Iw[q, :len(keep)] = If[0, keep]
    assert_knn_identical(D, I, Dw, Iw)
    assert (I[2] == -1).all() and (I[3, 1:] == -1).all() and I[3, 0] == cand[3, 0]


def _images(n, rng, metric):
    d, M = 6, 3
    xb = rng.standard_normal((n, d)).astype(np.float32)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    return d, xb, {"flat": faiss.serialize_flat(d, metric, xb[::-1]), "pq": faiss.serialize_pq(d, metric, C, codes)}, C, codes


@pytest.mark.parametrize("n", [0, 5])
@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_file_round_trip(kind, n):
    for metric in (L2, IP):
        d, xb, images, C, codes = _images(n, np.random.default_rng(n), metric)
        buf = faiss.serialize_refine(images[kind], d, metric, xb, 2.5)
        assert buf[:4] == b"IxRF"
        d2, metric2, kind2, base, xb2, k_factor = faiss.parse_refine(buf)
        assert (d2, metric2, kind2, k_factor) == (d, metric, kind, 2.5)
        assert xb2.dtype == np.float32 and xb2.shape == (n, d) and np.array_equal(xb2.view(np.uint32), xb.view(np.uint32))
        if kind == "flat":
            assert base[:2] == (d, metric) and np.array_equal(base[2].view(np.uint32), xb[::-1].view(np.uint32))
        else:
            assert base[:4] == (d, 3, 8, metric)
            assert np.array_equal(base[4].view(np.uint32), C.view(np.uint32)) and np.array_equal(base[5], codes)


@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_file_truncations_and_foreign_files(kind):
    d, xb, images, _, _ = _images(5, np.random.default_rng(1), L2)
    buf = faiss.serialize_refine(images[kind], d, L2, xb, 4.0)
    for cut in range(len(buf)):  # every truncation point
        with pytest.raises(RuntimeError):
            faiss.parse_refine(buf[:cut])
    with pytest.raises(RuntimeError, match="IndexRefineFlat"):
        faiss.parse_refine(b"IxF2" + buf[4:])
    hdr = faiss._HDR.size
    with pytest.raises(RuntimeError, match="sub-index"):
        faiss.parse_refine(buf[:hdr] + b"IwFl" + buf[hdr + 4:])  # a base kind that is not readable here
    other = faiss.serialize_refine(images[kind], d, L2, xb[:4], 4.0)  # the refine index one row short of the base
    with pytest.raises(RuntimeError, match="do not match"):
        faiss.parse_refine(other)


def test_null_handle_through_abi():
    from image_search_engine_amd import _native as n

    lib = n.lib
    x = np.zeros((2, 8), np.float32)
    cand = np.zeros((2, 3), np.int64)
    D, I = np.zeros((2, 4), np.float32), np.zeros((2, 4), np.int64)
    dist = np.zeros((2, 3), np.float32)
    xp, cp_, Dp, Ip, dp_ = (a.ctypes.data for a in (x, cand, D, I, dist))
    calls = (lambda: lib.ise_index_search_subset_device(None, xp, 2, 4, cp_, 3, Dp, Ip, None),
             lambda: lib.ise_index_search_subset_host(None, xp, 2, 4, cp_, 3, Dp, Ip),
             lambda: lib.ise_index_distance_subset_device(None, xp, 2, cp_, 3, dp_, None),
             lambda: lib.ise_index_distance_subset_host(None, xp, 2, cp_, 3, dp_),
             lambda: lib.ise_index_subset_stats(None, (ctypes.c_uint64 * 3)()))
    for call in calls:
        assert call() == n.E_INVALID
        assert b"NULL" in lib.ise_last_error()


def test_search_parameters():
    with pytest.raises(ValueError, match="k_factor"):
        faiss.IndexRefineSearchParameters(k_factor=0.5)
    with pytest.raises(ValueError, match="k_factor"):
        faiss.IndexRefineSearchParameters(k_factor=float("nan"))
    p = faiss.IndexRefineSearchParameters()
    assert isinstance(p, faiss.SearchParameters) and p.k_factor == 1.0 and p.base_index_params is None and p.sel is None
    inner = faiss.SearchParameters()
    p = faiss.IndexRefineSearchParameters(k_factor=3, base_index_params=inner)
    assert p.k_factor == 3.0 and p.base_index_params is inner


def test_what_stays_unprovided():
    for name in ("range_search", "remove_ids"):
        with pytest.raises(NotImplementedError):
            getattr(faiss.IndexRefine, name)(None)
