"""CPU tests of the product-quantised index's host side: the entry points' argument errors through the C ABI (no device
is touched), the numpy reference of the GPU tests, the file format, and what stays unprovided."""
import ctypes

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import pq_ref
from tests.knn_checks import assert_knn_identical, int_data
from tests.sel_ref import IP, L2


def test_argument_errors_through_abi():
    from image_search_engine_amd import _native as n

    lib = n.lib
    h = ctypes.c_void_p()
    for args, word in (((0, 1, 8, n.METRIC_L2, 0), b"d must"), ((-4, 1, 8, n.METRIC_L2, 0), b"d must"),
                       ((8, 0, 8, n.METRIC_L2, 0), b"M must"), ((8, -2, 8, n.METRIC_L2, 0), b"M must"),
                       ((8, 3, 8, n.METRIC_L2, 0), b"multiple of M"),
                       ((4 * (n.PQ_MAX_M + 1), n.PQ_MAX_M + 1, 8, n.METRIC_L2, 0), b"ISE_PQ_MAX_M"),
                       ((8, 2, 4, n.METRIC_L2, 0), b"nbits"), ((8, 2, 16, n.METRIC_L2, 0), b"nbits"),
                       ((8, 2, 8, 7, 0), b"metric")):
        assert lib.ise_pq_create(ctypes.byref(h), *args) == n.E_INVALID, args
        assert word in lib.ise_last_error(), (args, lib.ise_last_error())
        assert h.value is None
    assert n.PQ_MAX_M >= 64
    assert lib.ise_pq_create(None, 8, 2, 8, n.METRIC_L2, 0) == n.E_INVALID
    assert b"NULL" in lib.ise_last_error()
    assert lib.ise_pq_destroy(None) == 0
    assert lib.ise_pq_reset(None) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    assert lib.ise_pq_info(None, None, None, None, None, None, None, None) == n.E_INVALID
    x = np.zeros((2, 8), np.float32)
    codes = np.zeros((2, 2), np.uint8)
    cent = np.zeros((2, 256, 4), np.float32)
    D, I = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int64)
    xp, cp_, ce = x.ctypes.data, codes.ctypes.data, cent.ctypes.data
    # NULL buffers and negative counts come before the handle is looked at
    for fn in (lib.ise_pq_set_centroids_host, lib.ise_pq_get_centroids_host):
        assert fn(None, None) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert fn(None, ce) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    for call in (lambda a, b, cnt: lib.ise_pq_encode_host(None, a, cnt, b),
                 lambda a, b, cnt: lib.ise_pq_encode_device(None, a, cnt, b, None),
                 lambda a, b, cnt: lib.ise_pq_decode_host(None, b, cnt, a)):
        assert call(None, cp_, 2) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert call(xp, None, 2) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert call(xp, cp_, -1) == n.E_INVALID
        assert b"n must" in lib.ise_last_error()
        assert call(xp, cp_, 2) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    for call in (lambda a, cnt: lib.ise_pq_add_host(None, a, cnt), lambda a, cnt: lib.ise_pq_add_device(None, a, cnt, None),
                 lambda a, cnt: lib.ise_pq_add_codes_host(None, a, cnt)):
        assert call(None, 2) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert call(xp, -1) == n.E_INVALID
        assert b"n must" in lib.ise_last_error()
        assert call(xp, 2) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    assert lib.ise_pq_codes_host(None, 0, 1, cp_) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    assert lib.ise_pq_reconstruct_host(None, 0, 1, xp) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    # k outside 1 .. ISE_MAX_K and NULL buffers: before the handle is looked at
    for search, tail in ((lib.ise_pq_search_host, ()), (lib.ise_pq_search_device, (None,))):
        for k in (0, -1, n.MAX_K + 1):
            assert search(None, xp, 2, k, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
            assert b"k must" in lib.ise_last_error()
        assert search(None, xp, -1, 3, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"nq must" in lib.ise_last_error()
        assert search(None, None, 2, 3, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert search(None, xp, 2, 3, None, I.ctypes.data, *tail) == n.E_INVALID
        assert b"output pointer" in lib.ise_last_error()
        assert search(None, xp, 2, 3, D.ctypes.data, None, *tail) == n.E_INVALID
        assert b"output pointer" in lib.ise_last_error()
        assert search(None, xp, 2, 3, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    assert lib.ise_pq_stats(None, (ctypes.c_uint64 * 4)()) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    assert lib.ise_pq_stats(None, None) == n.E_INVALID
    assert b"NULL" in lib.ise_last_error()


def test_python_refuses_other_code_widths():
    for nbits in (4, 12, 16):
        with pytest.raises(NotImplementedError, match="nbits"):
            faiss.IndexPQ(16, 4, nbits)


@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_agrees_with_the_table_sum(metric):
    """On integer data adc_expected (a brute force over the decoded rows) is the table-sum definition in float64."""
    rng = np.random.default_rng(5)
    M, dsub, n, nq, k = 4, 3, 150, 5, 20
    C = int_data("signed", rng, M * 256, dsub).reshape(M, 256, dsub)
    x, xq = int_data("signed", rng, n, M * dsub), int_data("signed", rng, nq, M * dsub)
    codes = pq_ref.encode(x, C)
    assert codes.dtype == np.uint8 and codes.shape == (n, M)
    assert pq_ref.decode(codes, C).dtype == np.float32
    score = np.zeros((nq, n))
    for m in range(M):
        if metric == L2:
            T = pq_ref.sub_distances(xq, C, m)  # (nq, 256)
        else:
            T = xq[:, m * dsub:(m + 1) * dsub].astype(np.float64) @ C[m].astype(np.float64).T
        score += T[:, codes[:, m]]
    key = score if metric == L2 else -score
    I = np.stack([np.lexsort((np.arange(n), key[q]))[:k] for q in range(nq)]).astype(np.int64)
    D = np.take_along_axis(score, I, axis=1).astype(np.float32)
    assert_knn_identical(*pq_ref.adc_expected(xq, C, codes, k, metric), D, I)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M", [4, 20])
def test_table_lookup_reference_agrees_with_the_brute_force(M, metric):
    """adc_topk(adc_scores(...)), the reference of the long-index GPU tests, gives adc_expected's bits on integer data."""
    rng = np.random.default_rng(40 + M)
    dsub, n, nq = 2, 600, 9
    C = int_data("signed", rng, M * 256, dsub).reshape(M, 256, dsub)
    xq = int_data("signed", rng, nq, M * dsub)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    codes[[7, 300, 599]] = codes[2]  # one tie group for every query
    T = pq_ref.adc_tables(xq, C, metric)
    assert T.dtype == np.float64 and T.shape == (nq, M, 256)
    scores = pq_ref.adc_scores(xq, C, codes, metric)
    assert scores.dtype == np.float64 and scores.shape == (nq, n)
    assert np.array_equal(scores[:, 11], sum(T[:, m, codes[11, m]] for m in range(M)))
    for k in (1, 33, 70, 600, 650):  # 650: padding behind the 600 rows
        D, I = pq_ref.adc_topk(scores, k, metric)
        assert_knn_identical(D, I, *pq_ref.adc_expected(xq, C, codes, k, metric), f"k={k}")
    # the gate: a NaN and an overflowing score never enter; an infinite inner product enters first
    s = scores[:1].copy()
    s[0, 5], s[0, 9] = np.nan, (np.inf if metric == L2 else -np.inf)
    s[0, 11] = 2.0 ** 128 if metric == L2 else -2.0 ** 128
    s[0, 13] = 3.4e38 if metric == L2 else np.inf  # below FLT_MAX: enters last | +inf: enters first
    D, I = pq_ref.adc_topk(s, n, metric)
    assert (I[0, -3:] == -1).all() and not np.isin([5, 9, 11], I[0]).any()
    assert (D[0, -3:] == (np.float32(3.4028235e38) if metric == L2 else -np.float32(3.4028235e38))).all()
    assert I[0, n - 4 if metric == L2 else 0] == 13


def test_reference_encode_takes_the_lowest_of_equal_centroids():
    rng = np.random.default_rng(6)
    C = int_data("small", rng, 2 * 256, 3).reshape(2, 256, 3)
    C[0, 200] = C[0, 17]   # duplicates: the lower index wins
    C[1, 9] = C[1, 250] = C[1, 100]
    x = np.concatenate([C[0, 200], C[1, 250]])[None, :]
    first0 = int(np.flatnonzero((C[0] == C[0, 17]).all(1))[0])
    first1 = int(np.flatnonzero((C[1] == C[1, 100]).all(1))[0])
    assert first0 <= 17 and first1 <= 9
    assert pq_ref.encode(x, C).tolist() == [[first0, first1]]
    assert np.array_equal(pq_ref.decode(pq_ref.encode(x, C), C), x)
    assert [pq_ref.qt_of(M) for M in (1, 5, 6, 15, 16, 35, 36, 64)] == [16, 16, 8, 8, 4, 4, 2, 2]


def _file(n, rng):
    M, dsub = 3, 2
    C = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    return M, dsub, C, codes


@pytest.mark.parametrize("n", [0, 1, 37])
def test_file_round_trip(n):
    M, dsub, C, codes = _file(n, np.random.default_rng(n))
    for metric in (L2, IP):
        buf = faiss.serialize_pq(M * dsub, metric, C, codes)
        assert buf[:4] == b"IxPq"
        d, M2, nbits, metric2, C2, codes2 = faiss.parse_pq(buf)
        assert (d, M2, nbits, metric2) == (M * dsub, M, 8, metric)
        assert C2.dtype == np.float32 and np.array_equal(C2.view(np.uint32), C.view(np.uint32))
        assert codes2.dtype == np.uint8 and codes2.shape == (n, M) and np.array_equal(codes2, codes)


def test_file_truncations_and_foreign_files():
    M, dsub, C, codes = _file(5, np.random.default_rng(1))
    buf = faiss.serialize_pq(M * dsub, L2, C, codes)
    for cut in range(len(buf)):  # every truncation point
        with pytest.raises(RuntimeError):
            faiss.parse_pq(buf[:cut])
    with pytest.raises(RuntimeError, match="IndexPQ"):
        faiss.parse_pq(b"IxF2" + buf[4:])
    hdr = faiss._HDR.size
    bad_count = bytearray(buf)
    bad_count[hdr + 24:hdr + 32] = (256 * M * dsub + 1).to_bytes(8, "little")  # the centroid count
    with pytest.raises(RuntimeError):
        faiss.parse_pq(bytes(bad_count))
    off = hdr + 24 + 8 + 4 * 256 * M * dsub
    bad_codes = bytearray(buf)
    bad_codes[off:off + 8] = (5 * M - 1).to_bytes(8, "little")  # the code count
    with pytest.raises(RuntimeError):
        faiss.parse_pq(bytes(bad_codes))
    bad_bits = bytearray(buf)
    bad_bits[hdr + 16:hdr + 24] = (4).to_bytes(8, "little")  # nbits
    with pytest.raises(RuntimeError):
        faiss.parse_pq(bytes(bad_bits))


def test_what_stays_unprovided():
    from image_search_engine_amd import utils

    for name in ("range_search", "remove_ids"):
        with pytest.raises(NotImplementedError):
            getattr(faiss.IndexPQ, name)(None)
    with pytest.raises(NotImplementedError):
        utils.create_search_index(np.zeros((4, 16), np.float32), "cell-probe")
    with pytest.raises(NotImplementedError):
        faiss.IndexIVFPQ()
