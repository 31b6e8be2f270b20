"""CPU tests of the binary index's selectors, removal and id map, host side only: the numpy reference
tests/binary_sel_ref.py itself, the IndexBinaryIDMap file layout, the argument errors of the new ise_binary_* entry
points and the Python types (no GPU needed for any of them)."""
import ctypes
import struct

import numpy as np
import pytest

from image_search_engine_amd import _native as n
from image_search_engine_amd import faiss_compat as faiss
from tests import binary_ref as ref
from tests import binary_sel_ref as sref


def test_binary_sel_ref_against_brute_loop():
    rng = np.random.default_rng(3)
    xb = rng.integers(0, 4, (40, 3), dtype=np.uint8)  # few distinct codes: ties everywhere
    xq = rng.integers(0, 4, (5, 3), dtype=np.uint8)
    as_int = lambda row: int.from_bytes(row.tobytes(), "little")
    want = [[bin(as_int(q) ^ as_int(r)).count("1") for r in xb] for q in xq]
    for sel in (faiss.IDSelectorRange(7, 23), faiss.IDSelectorBatch([39, 0, 5, 5, 77, -2]),
                faiss.IDSelectorNot(faiss.IDSelectorBatch([3])), faiss.IDSelectorRange(9, 9)):
        members = sref.members_of(sel, 40)
        chosen = [r for r in range(40) if sel.is_member(r)]
        assert np.flatnonzero(members).tolist() == chosen
        D, I = sref.search(xb, xq, 12, members)
        assert D.dtype == np.int32 and I.dtype == np.int64 and D.shape == I.shape == (5, 12)
        lims, Dr, Ir = sref.range_search(xb, xq, 3, members)
        assert lims.dtype == np.uint64 and Dr.dtype == np.int32 and Ir.dtype == np.int64 and lims[0] == 0
        for q in range(5):
            order = sorted(chosen, key=lambda r: (want[q][r], r))[:12]
            m = len(order)
            assert I[q, :m].tolist() == order and D[q, :m].tolist() == [want[q][r] for r in order]
            assert (I[q, m:] == -1).all() and (D[q, m:] == ref.INT32_MAX).all()
            hit = [r for r in chosen if want[q][r] < 3]
            assert Ir[int(lims[q]):int(lims[q + 1])].tolist() == hit
            assert Dr[int(lims[q]):int(lims[q + 1])].tolist() == [want[q][r] for r in hit]
        c = sref.census(members)
        assert c["ntotal"] == 40 and c["selected"] == len(chosen)
        assert c["window"] == ((chosen[0], chosen[-1] + 1) if chosen else (0, 0))
    # the dist argument is a shortcut, not another answer
    dist = ref.distances(xb, xq)
    members = sref.members_of(faiss.IDSelectorRange(7, 23), 40)
    for a, b in zip(sref.search(xb, xq, 5, members), sref.search(xb, xq, 5, members, dist)):
        assert np.array_equal(a, b)
    big = np.zeros(200, dtype=bool)
    big[[0, 63, 64, 191]] = True
    assert sref.census(big) == {"ntotal": 200, "selected": 4, "window": (0, 192), "tiles": 3}


def test_serialize_idmap_round_trip_and_header_offsets():
    rng = np.random.default_rng(0)
    xb = rng.integers(0, 256, (37, 12), dtype=np.uint8)
    ids = rng.permutation(np.arange(37, dtype=np.int64) * 7919 + (1 << 40))
    buf = faiss.serialize_binary_idmap(96, xb, ids)
    assert buf[:4] == b"IBMp"
    assert struct.unpack_from("<i", buf, 4)[0] == 96          # d
    assert struct.unpack_from("<i", buf, 8)[0] == 12          # code_size
    assert struct.unpack_from("<q", buf, 12)[0] == 37         # ntotal
    assert buf[20] == 1                                       # is_trained
    assert struct.unpack_from("<i", buf, 21)[0] == 1          # metric_type
    sub = faiss.serialize_binary_flat(96, xb)
    assert buf[25:25 + len(sub)] == sub                       # the sub-index, as "IBxF" writes it
    off = 25 + len(sub)
    assert off == 25 + 33 + 37 * 12
    assert struct.unpack_from("<Q", buf, off)[0] == 37        # count of the id vector
    assert buf[off + 8:] == ids.astype("<i8").tobytes() and len(buf) == off + 8 + 8 * 37
    d, back, ids2 = faiss.parse_binary_idmap(buf)
    assert d == 96 and back.dtype == np.uint8 and np.array_equal(back, xb)
    assert ids2.dtype == np.int64 and np.array_equal(ids2, ids)


def test_serialize_idmap_empty_index():
    buf = faiss.serialize_binary_idmap(64, np.zeros((0, 8), dtype=np.uint8), np.zeros(0, dtype=np.int64))
    assert len(buf) == 25 + 33 + 8
    d, back, ids = faiss.parse_binary_idmap(buf)
    assert d == 64 and back.shape == (0, 8) and back.dtype == np.uint8 and ids.shape == (0,) and ids.dtype == np.int64


def test_parse_idmap_rejects_foreign_truncated_and_mismatched():
    xb = np.arange(40, dtype=np.uint8).reshape(5, 8)
    ids = np.arange(5, dtype=np.int64) + 100
    buf = faiss.serialize_binary_idmap(64, xb, ids)
    for foreign in (b"IBxF" + buf[4:], b"IxMp" + buf[4:], faiss.serialize_binary_flat(64, xb),
                    faiss.serialize_idmap(4, faiss.METRIC_L2, np.zeros((2, 4), np.float32), [1, 2])):
        with pytest.raises(RuntimeError):
            faiss.parse_binary_idmap(foreign)
    with pytest.raises(RuntimeError):
        faiss.parse_binary_flat(buf)  # and the flat parser refuses the wrapper
    off = 25 + 33 + 40
    for cut in (0, 3, 24, 25, 57, off - 1, off, off + 7, off + 8, len(buf) - 8, len(buf) - 1):  # incl. a truncated id vector
        with pytest.raises(RuntimeError):
            faiss.parse_binary_idmap(buf[:cut])
    for count in (4, 6):  # a count that is not ntotal
        bad = buf[:off] + struct.pack("<Q", count) + buf[off + 8:] + b"\0" * 8
        with pytest.raises(RuntimeError, match="one id per row"):
            faiss.parse_binary_idmap(bad)
    bad = buf[:12] + struct.pack("<q", 4) + buf[20:]  # the wrapper's ntotal against the sub-index's
    with pytest.raises(RuntimeError, match="does not match"):
        faiss.parse_binary_idmap(bad)
    with pytest.raises(AssertionError):
        faiss.serialize_binary_idmap(64, xb, ids[:4])


def test_new_binary_abi_argument_errors():
    lib = n.lib
    buf = np.zeros(64, dtype=np.uint8)
    ids = (ctypes.c_int64 * 2)(1, 2)
    words = (ctypes.c_uint32 * 2)(1, 2)
    out = ctypes.c_int64(-7)
    out3 = (ctypes.c_uint64 * 3)()
    out5 = (ctypes.c_int64 * 5)()
    s = ctypes.c_void_p(1)
    res = ctypes.c_void_p(1)
    # never dereferenced: the NULL handle or output is refused first.  The arguments checked behind the handle
    # (a NULL selector, NULL D / I) need a real one: tests/test_binary_sel_gpu.py::test_null_arguments_behind_a_handle
    fake = ctypes.c_void_p(buf.ctypes.data)

    def invalid(rc):
        assert rc == n.E_INVALID
        assert b"NULL" in lib.ise_last_error()

    invalid(lib.ise_binary_index_remove_ids_host(None, ids, 2, ctypes.byref(out)))
    invalid(lib.ise_binary_index_remove_range(None, 0, 1, ctypes.byref(out)))
    invalid(lib.ise_binary_index_remove_range(None, 0, 1, None))
    invalid(lib.ise_binary_index_remove_stats(None, out3))
    invalid(lib.ise_binary_selector_create_range(None, 0, 1, ctypes.byref(s)))
    assert not s.value  # *out is NULL on error
    invalid(lib.ise_binary_selector_create_range(fake, 0, 1, None))
    s.value = 1
    invalid(lib.ise_binary_selector_create_ids(None, ids, 2, 0, ctypes.byref(s)))
    assert not s.value
    invalid(lib.ise_binary_selector_create_ids(fake, ids, 2, 0, None))
    s.value = 1
    invalid(lib.ise_binary_selector_create_bitmap(None, words, 2, ctypes.byref(s)))
    assert not s.value
    invalid(lib.ise_binary_selector_create_bitmap(fake, words, 2, None))
    invalid(lib.ise_binary_selector_info(None, out5))
    invalid(lib.ise_binary_selector_info(fake, None))
    assert lib.ise_binary_selector_destroy(None) == 0
    invalid(lib.ise_binary_index_search_sel_host(None, buf.ctypes.data, 1, 1, fake, buf.ctypes.data, buf.ctypes.data))
    invalid(lib.ise_binary_index_search_sel_device(None, buf.ctypes.data, 1, 1, fake, buf.ctypes.data, buf.ctypes.data,
                                                   None))
    invalid(lib.ise_binary_index_range_search_sel_host(None, buf.ctypes.data, 1, 3, fake, ctypes.byref(res)))
    assert not res.value
    invalid(lib.ise_binary_index_range_search_sel_host(fake, buf.ctypes.data, 1, 3, fake, None))
    invalid(lib.ise_binary_index_sel_stats(None, out3))


def test_search_parameters_accept_the_binary_device_selector():
    assert issubclass(faiss.BinaryDeviceSelector, faiss.DeviceSelector)
    ds = object.__new__(faiss.BinaryDeviceSelector)  # no device object behind it: close() / __del__ have nothing to free
    assert faiss.SearchParameters(sel=ds).sel is ds
    ds.close()
    with pytest.raises(TypeError):
        faiss.SearchParameters(sel=[1, 2, 3])
    for name in ("remove_ids", "remove_stats", "make_selector", "sel_stats"):
        assert callable(getattr(faiss.IndexBinaryFlat, name))
    for name in ("add", "add_with_ids", "search", "range_search", "remove_ids", "reset", "d", "code_size", "ntotal",
                 "is_trained"):
        assert hasattr(faiss.IndexBinaryIDMap, name)


def test_a_selector_of_the_other_index_kind_never_reaches_the_device():
    """The type decides, before any handle is touched: the indexes here are bare objects without one."""
    flat = object.__new__(faiss.IndexFlat)
    binary = object.__new__(faiss.IndexBinaryFlat)
    fsel = object.__new__(faiss.DeviceSelector)
    bsel = object.__new__(faiss.BinaryDeviceSelector)
    called = []
    with pytest.raises(TypeError, match="float index's selector"):
        binary._with_selector(fsel, called.append)
    with pytest.raises(TypeError, match="binary index's selector"):
        flat._with_selector(bsel, called.append)
    assert not called
    idmap = object.__new__(faiss.IndexBinaryIDMap)
    with pytest.raises(TypeError, match="external ids"):
        idmap._row_params(faiss.SearchParameters(sel=bsel))
