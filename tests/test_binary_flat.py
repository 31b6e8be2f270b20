"""CPU tests of the binary flat index's host side: the IndexBinaryFlat file layout, the hash helpers, the numpy
reference itself, and the argument errors of the ise_binary_index_* entry points (no GPU needed for any of them)."""
import ctypes
import struct

import numpy as np
import pytest

from image_search_engine_amd import _native as n
from image_search_engine_amd import faiss_compat as faiss
from image_search_engine_amd.utils import hamming, hashes_to_codes
from tests import binary_ref as ref


def test_serialize_round_trip_and_header_offsets():
    rng = np.random.default_rng(0)
    xb = rng.integers(0, 256, (37, 12), dtype=np.uint8)
    buf = faiss.serialize_binary_flat(96, xb)
    assert buf[:4] == b"IBxF"
    assert struct.unpack_from("<i", buf, 4)[0] == 96          # d
    assert struct.unpack_from("<i", buf, 8)[0] == 12          # code_size
    assert struct.unpack_from("<q", buf, 12)[0] == 37         # ntotal
    assert buf[20] == 1                                       # is_trained
    assert struct.unpack_from("<i", buf, 21)[0] == 1          # metric_type
    assert struct.unpack_from("<Q", buf, 25)[0] == 37 * 12    # count
    assert len(buf) == 33 + 37 * 12
    assert buf[33:] == xb.tobytes()
    d, back = faiss.parse_binary_flat(buf)
    assert d == 96 and back.dtype == np.uint8 and np.array_equal(back, xb)


def test_serialize_empty_index():
    buf = faiss.serialize_binary_flat(64, np.zeros((0, 8), dtype=np.uint8))
    assert len(buf) == 33
    d, back = faiss.parse_binary_flat(buf)
    assert d == 64 and back.shape == (0, 8) and back.dtype == np.uint8


def test_parse_rejects_foreign_and_truncated():
    xb = np.arange(40, dtype=np.uint8).reshape(5, 8)
    buf = faiss.serialize_binary_flat(64, xb)
    with pytest.raises(RuntimeError):
        faiss.parse_binary_flat(b"IxF2" + buf[4:])
    with pytest.raises(RuntimeError):
        faiss.parse_binary_flat(faiss.serialize_flat(4, faiss.METRIC_L2, np.zeros((2, 4), np.float32)))
    for cut in (0, 3, 20, 32, 33, len(buf) - 1):
        with pytest.raises(RuntimeError):
            faiss.parse_binary_flat(buf[:cut])


def _popcount_rows(a, b):
    return int(ref.POPCOUNT[a ^ b].sum())


def test_hashes_to_codes_matches_hamming():
    rng = np.random.default_rng(1)
    hashes = [int(x) for x in rng.integers(0, 1 << 63, 50, dtype=np.int64)]
    hashes = [h | (int(b) << 63) for h, b in zip(hashes, rng.integers(0, 2, 50))]
    codes = hashes_to_codes(hashes)
    assert codes.dtype == np.uint8 and codes.shape == (50, 8) and codes.flags.c_contiguous
    for a in range(50):
        for b in range(0, 50, 7):
            assert _popcount_rows(codes[a], codes[b]) == hamming(hashes[a], hashes[b])
    pair = hashes_to_codes([2 ** 63 | 1, 1])
    assert _popcount_rows(pair[0], pair[1]) == hamming(2 ** 63 | 1, 1) == 1
    # little-endian: bit i of the hash is bit i % 8 of byte i // 8
    assert pair[1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and pair[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0x80]
    assert hashes_to_codes([0x0201], nbits=16).tolist() == [[1, 2]]
    assert hamming(0b1011, 0b0001) == 2


def test_binary_ref_against_brute_loop():
    rng = np.random.default_rng(2)
    xb = rng.integers(0, 4, (20, 3), dtype=np.uint8)  # few distinct codes: ties everywhere
    xq = rng.integers(0, 4, (4, 3), dtype=np.uint8)
    as_int = lambda row: int.from_bytes(row.tobytes(), "little")
    want = np.array([[bin(as_int(q) ^ as_int(r)).count("1") for r in xb] for q in xq], dtype=np.int32)
    dist = ref.distances(xb, xq)
    assert dist.dtype == np.int32 and np.array_equal(dist, want)
    D, I = ref.search(xb, xq, 25)
    assert D.dtype == np.int32 and I.dtype == np.int64
    for q in range(4):
        order = sorted(range(20), key=lambda r: (want[q, r], r))
        assert I[q, :20].tolist() == order and D[q, :20].tolist() == [want[q, r] for r in order]
        assert (I[q, 20:] == -1).all() and (D[q, 20:] == ref.INT32_MAX).all()
    lims, Dr, Ir = ref.range_search(xb, xq, 3)
    assert lims.dtype == np.uint64 and lims[0] == 0
    for q in range(4):
        hit = [r for r in range(20) if want[q, r] < 3]
        assert Ir[int(lims[q]):int(lims[q + 1])].tolist() == hit
        assert Dr[int(lims[q]):int(lims[q + 1])].tolist() == [want[q, r] for r in hit]


def test_binary_abi_argument_errors():
    lib = n.lib
    h = ctypes.c_void_p()
    for bad in (0, 12, 8200, -8):
        assert lib.ise_binary_index_create(ctypes.byref(h), bad, 0) == n.E_INVALID
        assert b"multiple of 8" in lib.ise_last_error()
        assert not h.value
    assert lib.ise_binary_index_create(None, 64, 0) == n.E_INVALID
    assert lib.ise_binary_index_destroy(None) == 0
    assert lib.ise_binary_range_result_destroy(None) == 0
    buf = np.zeros(64, dtype=np.uint8)
    out = (ctypes.c_uint64 * 3)()
    res = ctypes.c_void_p()
    assert lib.ise_binary_index_reset(None) == n.E_INVALID
    assert lib.ise_binary_index_info(None, None, None, None) == n.E_INVALID
    assert lib.ise_binary_index_add_host(None, buf.ctypes.data, 1) == n.E_INVALID
    assert lib.ise_binary_index_add_device(None, buf.ctypes.data, 1, None) == n.E_INVALID
    assert lib.ise_binary_index_reconstruct_host(None, 0, 1, buf.ctypes.data) == n.E_INVALID
    assert lib.ise_binary_index_search_host(None, buf.ctypes.data, 1, 1, buf.ctypes.data, buf.ctypes.data) == n.E_INVALID
    assert lib.ise_binary_index_search_device(None, buf.ctypes.data, 1, 1, buf.ctypes.data, buf.ctypes.data,
                                              None) == n.E_INVALID
    assert lib.ise_binary_index_range_search_host(None, buf.ctypes.data, 1, 3, ctypes.byref(res)) == n.E_INVALID
    assert not res.value
    assert lib.ise_binary_index_range_search_host(None, buf.ctypes.data, 1, 3, None) == n.E_INVALID
    assert lib.ise_binary_range_result_get(None, None, None, None, None) == n.E_INVALID
    assert lib.ise_binary_index_stats(None, out) == n.E_INVALID
    assert b"NULL" in lib.ise_last_error()


def test_binary_constructor_needs_a_gpu():
    """No CPU path: without a GPU the constructor raises; with one it gives an empty index."""
    import torch

    if torch.cuda.is_available():
        index = faiss.IndexBinaryFlat(64)
        assert (index.d, index.code_size, index.ntotal, index.is_trained) == (64, 8, 0, True)
        return
    with pytest.raises(RuntimeError, match="MI355X|HIP device"):
        faiss.IndexBinaryFlat(64)
