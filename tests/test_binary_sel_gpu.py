"""GPU tests of the selector-filtered searches of IndexBinaryFlat (include/ise_knn.h, ise_binary_index_search_sel_* /
ise_binary_selector_*; the masked kernels of csrc/ise_binary_scan.hpp) against the numpy reference
tests/binary_sel_ref.py.  Every score is an integer, so every comparison is exact: np.array_equal on D and on I, dtypes
asserted, no tolerance anywhere."""
import ctypes
import functools

import numpy as np
import pytest

from image_search_engine_amd import _native as n
from image_search_engine_amd import faiss_compat as faiss
from image_search_engine_amd._native import IseError
from tests import binary_ref as ref
from tests import binary_sel_ref as sref
from tests.test_binary_flat_gpu import (N_SWEEP, assert_range_same, assert_same, big_data, make_index, one_block_data,
                                        sweep_data)

pytestmark = pytest.mark.gpu

# ws = 1 with pad, ws = 1, ws = 2, an odd word count stored as 4, the LDS chunk loop
CODE_SIZES = (1, 8, 16, 24, 256)
KPASS = 32


class EveryThird(faiss.IDSelector):
    """A user's selector: reaches the device as a bitmap."""

    def is_member(self, i):
        return int(i) % 3 == 0


class Mask(faiss.IDSelector):
    def __init__(self, mask):
        self.mask = np.asarray(mask, dtype=bool)

    def is_member(self, i):
        return 0 <= int(i) < self.mask.size and bool(self.mask[int(i)])

    def members(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        ok = (ids >= 0) & (ids < self.mask.size)
        out = np.zeros(ids.shape, dtype=bool)
        out[ok] = self.mask[ids[ok]]
        return out


SCATTERED = [3, 599, 64, 65, 127, 128, 300, 301, 17, 63, 0, 511, 512, 575, 576, 3, 599, 64, 600, 601, -1, 1 << 40,
             -(1 << 40), 250, 251]
assert len(SCATTERED) == 25


def sweep_selectors():
    return [
        ("every third row", EveryThird()),
        ("inside one tile", faiss.IDSelectorRange(70, 75)),
        ("three tiles, unaligned ends", faiss.IDSelectorRange(60, 130)),
        ("row 0", faiss.IDSelectorBatch([0])),
        ("row 599", faiss.IDSelectorBatch([599])),
        ("scattered batch", faiss.IDSelectorBatch(SCATTERED)),
        ("not myself", faiss.IDSelectorNot(faiss.IDSelectorBatch([17]))),
        ("every row", faiss.IDSelectorRange(0, 600)),
        ("empty", faiss.IDSelectorRange(5, 5)),
    ]


def params(sel):
    return faiss.SearchParameters(sel=sel)


@pytest.mark.parametrize("code_size", CODE_SIZES)
def test_masked_search_sweep(code_size):
    xb, xq, dist = sweep_data(code_size)
    index = make_index(xb)
    plain = {k: index.search(xq, k) for k in (1, 10, 33, 70)}
    for name, sel in sweep_selectors():
        members = sref.members_of(sel, N_SWEEP)
        ds = index.make_selector(sel)
        assert ds.info() == sref.census(members), name
        for k in (1, 10, 33, 70):
            want = sref.search(xb, xq, k, members, dist)
            for nq in (1, 16, 17, 40):
                before = index.sel_stats()["sel_passes"]
                got = index.search(xq[:nq], k, params=params(sel))
                assert_same(got, (want[0][:nq], want[1][:nq]))
                if name == "empty":
                    assert index.sel_stats()["sel_passes"] == before
                    assert (got[0] == ref.INT32_MAX).all() and (got[1] == -1).all()
            assert_same(index.search(xq, k, params=params(ds)), want)  # the reused device selector
            filled = min(k, int(members.sum()))
            assert (want[1][:, :filled] >= 0).all() and (want[1][:, filled:] == -1).all()  # smaller than k: padding
            if name == "every row":
                assert_same(want, plain[k])
                assert_same(got, plain[k])
            if name == "not myself":
                assert 17 not in got[1][3] and plain[k][0][3, 0] == 0
                if code_size >= 8:  # one byte: 600 rows share 256 codes, row 17 need not be the first of its ties
                    assert plain[k][1][3, 0] == 17
        ds.close()
    if code_size == 8:  # the tie rule is exercised, not assumed: most queries tie at the 10th place
        D, _ = sref.search(xb, xq, 11, sref.members_of(EveryThird(), N_SWEEP), dist)
        assert int((D[:, 9] == D[:, 10]).sum()) == 29


@pytest.mark.parametrize("code_size", (8, 16, 24))  # one word, two words, the queries in LDS
def test_one_block_cut_beside_a_cleared_tile(code_size):
    """512 rows in one block, in descending distance to query 0: wave 0 streams tiles 0 and 4 and cuts after the second,
    wave 1 skips its second tile (5), which the selector clears whole.  k = 33: the floor-keyed second pass; k = 513:
    fourteen full passes over the 448 selected rows, then passes that find nothing -- every list ends short."""
    xb, xq, dist = one_block_data(code_size)
    mask = np.ones(512, dtype=bool)
    mask[5 * 64:6 * 64] = False
    sel = Mask(mask)
    members = sref.members_of(sel, 512)
    index = make_index(xb)
    ds = index.make_selector(sel)
    assert ds.info() == sref.census(members) and ds.info()["selected"] == 448
    for k in (KPASS + 1, 513):
        got = index.search(xq, k, params=params(ds))
        assert_same(got, sref.search(xb, xq, k, members, dist))
    assert (got[1][:, 448:] == -1).all() and (got[0][:, 448:] == ref.INT32_MAX).all() and (got[1][:, :448] >= 0).all()
    assert not np.isin(got[1], np.arange(5 * 64, 6 * 64)).any()
    ds.close()


def test_ties_among_selected_rows():
    row = np.arange(12, dtype=np.uint8)[None, :] * 19 + 5
    xb = np.repeat(row, 5000, axis=0)
    index = make_index(xb)
    xq = np.concatenate([row, row ^ np.uint8(1)])  # distance 0 and distance 12 to every row
    ds = index.make_selector(Mask(np.arange(5000) % 7 == 0))
    assert ds.info()["selected"] == 715
    for k in (1, 10, 33, 100):
        D, I = index.search(xq, k, params=params(ds))
        assert D.dtype == np.int32 and I.dtype == np.int64
        assert np.array_equal(I, np.tile(7 * np.arange(k, dtype=np.int64), (2, 1)))
        assert (D[0] == 0).all() and (D[1] == 12).all()


@functools.lru_cache(maxsize=None)
def big_selectors():
    n = 70_001
    return (
        ("random 1 %", Mask(np.random.default_rng(8).random(n) < 0.01), 28),
        ("clustered window", faiss.IDSelectorRange(30_000, 30_500), 28),
        ("not three copies", faiss.IDSelectorNot(faiss.IDSelectorBatch([1, 64, 4096])), 20),
    )


@pytest.mark.parametrize("which", (0, 1, 2))
def test_many_blocks(which):
    xb, xq, dist = big_data()
    name, sel, radius = big_selectors()[which]
    members = sref.members_of(sel, xb.shape[0])
    index = make_index(xb)
    ds = index.make_selector(sel)
    assert ds.info() == sref.census(members)
    if which == 0:
        assert ds.info()["selected"] == 678 and ds.info()["tiles"] < (xb.shape[0] + 63) // 64 // 2  # most tiles empty
    for k in (5, 10, 40):
        got = index.search(xq, k, params=params(ds))
        assert_same(got, sref.search(xb, xq, k, members, dist))
        if which == 2:
            assert got[1][0, :4].tolist() == [0, 63, 4095, 70_000] and (got[0][0, :4] == 0).all()
    got = index.range_search(xq, radius, params=params(ds))
    want = sref.range_search(xb, xq, radius, members, dist)
    counts = np.diff(want[0].astype(np.int64))
    assert counts.min() > 0  # not vacuous: every query matches selected rows
    assert_range_same(got, want)
    assert_range_same(index.range_search(xq, radius, params=params(sel)), want)  # a per-call selector


@pytest.mark.parametrize("code_size", (1, 8, 256))
def test_masked_range_search(code_size):
    xb, xq, dist = sweep_data(code_size)
    index = make_index(xb)
    for sel in (EveryThird(), faiss.IDSelectorRange(60, 130)):
        members = sref.members_of(sel, N_SWEEP)
        rows = np.flatnonzero(members).astype(np.int64)
        ds = index.make_selector(sel)
        for radius in (0, 1, int(np.median(dist)), 8 * code_size + 1):
            for nq in (1, 17):
                before = index.sel_stats()["sel_range_batches"]
                got = index.range_search(xq[:nq], radius, params=params(ds))
                assert_range_same(got, sref.range_search(xb, xq[:nq], radius, members, dist[:nq]))
                assert index.sel_stats()["sel_range_batches"] == before + (1 if radius > 0 else 0)
                if radius == 8 * code_size + 1:  # exactly the selected ids, for every query
                    assert got[0].tolist() == [rows.size * i for i in range(nq + 1)]
                    assert np.array_equal(got[2], np.tile(rows, nq))
    empty = index.range_search(xq[:17], 8 * code_size + 1, params=params(faiss.IDSelectorRange(5, 5)))
    assert empty[0].tolist() == [0] * 18 and empty[1].size == 0 and empty[2].size == 0


def test_device_forms():
    import torch

    xb, xq, dist = sweep_data(16)
    dev = torch.device("cuda", torch.cuda.current_device())
    index = make_index(xb)
    sel = EveryThird()
    members = sref.members_of(sel, N_SWEEP)
    ds = index.make_selector(sel)
    side = torch.cuda.Stream(device=dev)
    xq_dev = torch.from_numpy(xq[:17].copy()).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for k in (10, 33):
        host = index.search(xq[:17], k, params=params(ds))
        want = sref.search(xb, xq, k, members, dist)
        assert_same(host, (want[0][:17], want[1][:17]))
        with torch.cuda.stream(side):
            D, I = index.search_torch(xq_dev, k, params=params(ds))  # the selector is reused across the calls
        side.synchronize()
        assert D.is_cuda and I.is_cuda and D.dtype == torch.int32 and I.dtype == torch.int64
        assert_same((D.cpu().numpy(), I.cpu().numpy()), host)
    D, I = index.search_torch(xq_dev, 10, params=params(sel))  # built and destroyed inside the call
    torch.cuda.synchronize()
    assert_same((D.cpu().numpy(), I.cpu().numpy()), index.search(xq[:17], 10, params=params(ds)))


def _every_filtered_call_raises(index, ds, xq, match):
    import torch

    xq_dev = torch.from_numpy(xq.copy()).to(torch.device("cuda", index.device))
    p = params(ds)
    for call in (lambda: index.search(xq, 5, params=p), lambda: index.search_torch(xq_dev, 5, params=p),
                 lambda: index.range_search(xq, 20, params=p), lambda: index.search(xq[:0], 5, params=p),
                 lambda: index.range_search(xq[:0], 20, params=p)):
        with pytest.raises(IseError, match=match):
            call()
    torch.cuda.synchronize()


def test_validity():
    xb, xq, _ = sweep_data(8)
    xq = xq[:3]
    index = make_index(xb[:500])
    stats = index.sel_stats()
    ds = index.make_selector(faiss.IDSelectorRange(10, 400))
    index.search(xq, 5, params=params(ds))
    index.add(xb[500:])  # made before an add
    _every_filtered_call_raises(index, ds, xq, "ntotal changed")
    ds = index.make_selector(faiss.IDSelectorRange(10, 400))
    assert index.remove_ids([3]) == 1  # made before a removal
    _every_filtered_call_raises(index, ds, xq, "ntotal changed|row epoch")
    ds = index.make_selector(faiss.IDSelectorRange(10, 400))
    index.add(xb[:1])
    assert index.remove_ids([0]) == 1 and index.ntotal == ds.info()["ntotal"]  # add, then remove: ntotal is back
    _every_filtered_call_raises(index, ds, xq, "row epoch")
    ds = index.make_selector(faiss.IDSelectorRange(10, 400))
    index.reset()  # made before a reset; the index is empty now, and the check still comes first
    _every_filtered_call_raises(index, ds, xq, "row epoch|ntotal changed")
    ds0 = index.make_selector(faiss.IDSelectorRange(0, 10))  # of an empty index: valid until rows arrive
    D, I = index.search(xq, 4, params=params(ds0))
    assert (D == ref.INT32_MAX).all() and (I == -1).all()
    index.add(xb)
    _every_filtered_call_raises(index, ds0, xq, "ntotal changed")
    other = make_index(xb)  # the same rows, another handle
    _every_filtered_call_raises(index, other.make_selector(faiss.IDSelectorRange(0, 10)), xq, "another index")
    assert index.sel_stats()["sel_passes"] == stats["sel_passes"] + 1  # nothing stale ever ran a pass
    # a float index's selector: refused by its type, before any call into the library
    flat = faiss.IndexFlatL2(8)
    flat.add(np.zeros((600, 8), dtype=np.float32))
    fsel = flat.make_selector(faiss.IDSelectorRange(0, 10))
    before = (index.sel_stats(), index.binary_stats())
    for call in (lambda: index.search(xq, 5, params=params(fsel)), lambda: index.range_search(xq, 5, params=params(fsel))):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(TypeError):
        flat.search(np.zeros((1, 8), dtype=np.float32), 5, params=params(index.make_selector(faiss.IDSelectorRange(0, 10))))
    assert (index.sel_stats(), index.binary_stats()) == before


def test_counters():
    xb, xq, _ = sweep_data(8)
    index = make_index(xb)
    ds = index.make_selector(EveryThird())
    base_b = index.binary_stats()
    assert index.sel_stats() == {"sel_batches": 0, "sel_passes": 0, "sel_range_batches": 0}
    passes = lambda nq, k: -(-nq // 16) * -(-k // KPASS)
    total = 0
    for i, (nq, k) in enumerate(((1, 1), (16, 32), (17, 33), (40, 70), (5, 605))):
        index.search(xq[:nq], k, params=params(ds))
        total += passes(nq, k)
        s = index.sel_stats()
        assert s == {"sel_batches": i + 1, "sel_passes": total, "sel_range_batches": 0}
    index.range_search(xq[:17], 0, params=params(ds))
    index.range_search(xq[:17], 20, params=params(ds))
    assert index.sel_stats() == {"sel_batches": 5, "sel_passes": total, "sel_range_batches": 1}
    index.search(xq[:3], 5, params=params(faiss.IDSelectorRange(5, 5)))  # an empty selection: a batch, no pass
    assert index.sel_stats() == {"sel_batches": 6, "sel_passes": total, "sel_range_batches": 1}
    assert index.binary_stats() == base_b  # filtered calls count in sel_stats only
    index.search(xq[:3], 5)
    assert index.sel_stats()["sel_batches"] == 6 and index.binary_stats()["search_batches"] == base_b["search_batches"] + 1


def test_null_arguments_behind_a_handle():
    """ISE_E_INVALID for the arguments that the library checks after the handle: a NULL selector and NULL outputs on a
    live index, through the ABI."""
    lib = n.lib
    index = faiss.IndexBinaryFlat(64)
    index.add(np.arange(80, dtype=np.uint8).reshape(10, 8))
    buf = np.zeros(64, dtype=np.uint8)
    res = ctypes.c_void_p(1)
    ds = index.make_selector(faiss.IDSelectorRange(0, 5))
    before = index.sel_stats()
    for rc in (lambda: lib.ise_binary_index_search_sel_host(index._h, buf.ctypes.data, 1, 1, None, buf.ctypes.data,
                                                            buf.ctypes.data),
               lambda: lib.ise_binary_index_search_sel_device(index._h, buf.ctypes.data, 1, 1, None, buf.ctypes.data,
                                                              buf.ctypes.data, None),
               lambda: lib.ise_binary_index_range_search_sel_host(index._h, buf.ctypes.data, 1, 3, None,
                                                                  ctypes.byref(res)),
               lambda: lib.ise_binary_index_search_sel_host(index._h, buf.ctypes.data, 1, 1, ds._s, None,
                                                            buf.ctypes.data),
               lambda: lib.ise_binary_index_search_sel_host(index._h, buf.ctypes.data, 1, 1, ds._s, buf.ctypes.data,
                                                            None),
               lambda: lib.ise_binary_index_search_sel_device(index._h, buf.ctypes.data, 1, 1, ds._s, None, None, None),
               lambda: lib.ise_binary_index_remove_stats(index._h, None),
               lambda: lib.ise_binary_index_sel_stats(index._h, None),
               lambda: lib.ise_binary_index_remove_ids_host(index._h, None, 3, None)):
        assert rc() == n.E_INVALID
        assert b"NULL" in lib.ise_last_error()
    assert not res.value  # *out is NULL on error
    assert index.sel_stats() == before and index.ntotal == 10
    ds.close()
