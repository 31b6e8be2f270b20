"""CPU tests of IndexBinaryIVF: the "IBwF" file layout (``serialize_binary_ivf`` / ``parse_binary_ivf``), the argument
errors of ise_binary_ivf_* through the ABI, the pinned surface of the new public names and the numpy reference
(tests/binary_ivf_ref.py) against tests/binary_ref.py.  No GPU needed.

The surface fixture tests/golden/faiss_compat_surface_binary_ivf.json holds the names in ``_BINARY_IVF`` with the
attributes of a class that do not start with ``_`` plus ``__init__`` and ``__del__``, as the coded fixture of
tests/test_compat_surface.py does:  python -m tests.test_binary_ivf > tests/golden/faiss_compat_surface_binary_ivf.json"""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import binary_ivf_ref, binary_ref
from tests.test_compat_surface import _KEPT_DUNDERS, _problems, describe_surface

_BINARY_IVF = ("IndexBinaryIVF", "serialize_binary_ivf", "parse_binary_ivf")


# ---------------------------------------------------------------- the file layout
def example(rng, d=72, sizes=(3, 0, 5, 0, 0, 1, 0)):
    """(d, nlist, nprobe, centroids, lists) with empty lists; the ids are a permutation of 0 .. n - 1 dealt to the lists."""
    cs, nlist, n = d // 8, len(sizes), int(sum(sizes))
    centroids = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    ids = rng.permutation(n).astype(np.int64)
    lists, at = [], 0
    for m in sizes:
        lists.append((np.sort(ids[at:at + m]), rng.integers(0, 256, (m, cs), dtype=np.uint8)))
        at += m
    return d, nlist, 3, centroids, lists


def assert_parts_equal(got, want):
    d, nlist, nprobe, centroids, lists = got
    assert (d, nlist, nprobe) == tuple(want[:3])
    assert centroids.dtype == np.uint8 and np.array_equal(centroids, want[3])
    assert len(lists) == len(want[4])
    for (ids, codes), (wids, wcodes) in zip(lists, want[4]):
        assert ids.dtype == np.int64 and codes.dtype == np.uint8 and codes.shape == wcodes.shape
        assert np.array_equal(ids, wids) and np.array_equal(codes, wcodes)


def field_boundaries(d, nlist, centroids, lists):
    """The offsets at which a field of a "full" image ends (the whole file's length last)."""
    cs = d // 8
    ends = [4, 8, 12, 20, 21, 25]                 # fourcc, d, code_size, ntotal, is_trained, metric_type
    ends += [33, 41]                              # nlist, nprobe
    q0 = 41
    ends += [q0 + 4, q0 + 8, q0 + 12, q0 + 20, q0 + 21, q0 + 25, q0 + 33, q0 + 33 + centroids.size]  # the "IBxF" image
    at = ends[-1]
    ends += [at + 1, at + 9]                      # the direct map
    ends += [at + 13, at + 21, at + 29, at + 33, at + 41, at + 41 + 8 * nlist]  # "ilar", nlist, code_size, "full", count, sizes
    at = ends[-1]
    for ids, _ in lists:
        if ids.size:
            ends += [at + ids.size * cs, at + ids.size * (cs + 8)]
            at = ends[-1]
    return ends


def test_round_trip_with_empty_lists():
    rng = np.random.default_rng(1)
    for d, sizes in ((72, (3, 0, 5, 0, 0, 1, 0)), (8, (0, 0)), (256, (64, 65))):
        want = example(rng, d, sizes)
        buf = faiss.serialize_binary_ivf(*want)
        assert buf[:4] == b"IBwF"
        assert_parts_equal(faiss.parse_binary_ivf(buf), want)
        assert len(buf) == field_boundaries(want[0], want[1], want[3], want[4])[-1]
    # an untrained quantiser: no centroid codes, no rows
    want = (64, 4, 1, np.zeros((0, 8), np.uint8), [(np.zeros(0, np.int64), np.zeros((0, 8), np.uint8))] * 4)
    assert_parts_equal(faiss.parse_binary_ivf(faiss.serialize_binary_ivf(*want)), want)


def sparse_image(d, nlist, nprobe, centroids, lists):
    """The same index with the sizes as Faiss's "sprs" form: (list, size) pairs of the lists that hold rows."""
    buf = faiss.serialize_binary_ivf(d, nlist, nprobe, centroids, lists)
    at = buf.index(b"full")
    pairs = [v for l, (ids, _) in enumerate(lists) if ids.size for v in (l, ids.size)]
    return buf[:at] + b"sprs" + struct.pack("<Q", len(pairs)) + struct.pack(f"<{len(pairs)}Q", *pairs) + buf[at + 12 + 8 * nlist:]


def test_sparse_sizes_are_readable():
    want = example(np.random.default_rng(2))
    buf = sparse_image(*want)
    assert b"sprs" in buf and b"full" not in buf
    assert_parts_equal(faiss.parse_binary_ivf(buf), want)
    bad = bytearray(buf)
    at = buf.index(b"sprs") + 12
    bad[at:at + 8] = struct.pack("<Q", want[1])  # a list number outside [0, nlist)
    with pytest.raises(RuntimeError, match="outside"):
        faiss.parse_binary_ivf(bytes(bad))


def test_truncation_at_every_field_boundary_raises():
    want = example(np.random.default_rng(3))
    buf = faiss.serialize_binary_ivf(*want)
    ends = field_boundaries(want[0], want[1], want[3], want[4])
    assert ends[-1] == len(buf) and ends == sorted(set(ends))
    for cut in [0, 2] + ends[:-1] + [len(buf) - 1]:
        with pytest.raises(RuntimeError, match="truncated IndexBinaryIVF"):
            faiss.parse_binary_ivf(buf[:cut])
    sp = sparse_image(*want)
    for cut in range(sp.index(b"sprs"), len(sp), 7):
        with pytest.raises(RuntimeError, match="truncated IndexBinaryIVF"):
            faiss.parse_binary_ivf(sp[:cut])


def test_miscounted_and_foreign_files_raise():
    want = example(np.random.default_rng(4))
    d, nlist, nprobe, centroids, lists = want
    buf = faiss.serialize_binary_ivf(*want)
    n = sum(ids.size for ids, _ in lists)

    def patched(at, fmt, value):
        out = bytearray(buf)
        out[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
        return bytes(out)

    with pytest.raises(RuntimeError, match="add up"):  # a wrong size sum: ntotal in the header
        faiss.parse_binary_ivf(patched(12, "<q", n + 1))
    sizes_at = buf.index(b"full") + 12
    with pytest.raises(RuntimeError, match="add up"):  # ... and a size in the vector
        faiss.parse_binary_ivf(patched(sizes_at, "<Q", lists[0][0].size + 1))
    with pytest.raises(RuntimeError, match="nlist entries"):
        faiss.parse_binary_ivf(patched(sizes_at - 8, "<Q", nlist + 1))
    with pytest.raises(RuntimeError, match="do not match"):  # the lists' code_size
        faiss.parse_binary_ivf(patched(sizes_at - 20, "<Q", d // 8 + 1))
    with pytest.raises(RuntimeError, match="header"):  # d no multiple of 8
        faiss.parse_binary_ivf(patched(4, "<i", d + 4))
    with pytest.raises(RuntimeError, match="header"):  # nlist = 0
        faiss.parse_binary_ivf(patched(25, "<Q", 0))
    with pytest.raises(RuntimeError, match="quantiser"):  # the quantiser holds one code too few for its count
        faiss.parse_binary_ivf(faiss.serialize_binary_ivf(d, nlist, nprobe, centroids[:-1], lists))
    with pytest.raises(RuntimeError, match="direct map"):
        faiss.parse_binary_ivf(patched(buf.index(b"ilar") - 9, "<B", 1))
    with pytest.raises(RuntimeError, match="unsupported quantiser"):
        faiss.parse_binary_ivf(patched(41, "<4s", b"IBMp"))
    with pytest.raises(RuntimeError, match="unsupported inverted lists"):
        faiss.parse_binary_ivf(patched(buf.index(b"ilar"), "<4s", b"ilxx"))
    with pytest.raises(RuntimeError, match="unsupported list size form"):
        faiss.parse_binary_ivf(patched(buf.index(b"full"), "<4s", b"fulx"))
    for foreign in (faiss.serialize_binary_flat(d, centroids), faiss.serialize_flat(4, faiss.METRIC_L2, np.zeros((1, 4), np.float32)),
                    b"IwSq" + buf[4:]):
        with pytest.raises(RuntimeError, match="not an IndexBinaryIVF"):
            faiss.parse_binary_ivf(foreign)
    with pytest.raises(RuntimeError):  # the flat binary reader refuses the new image as before
        faiss.parse_binary_flat(buf)


# ---------------------------------------------------------------- argument errors through the ABI
def test_argument_errors_through_abi():
    from image_search_engine_amd import _native as n

    h = ctypes.c_void_p()
    assert n.lib.ise_binary_ivf_create(None, 64, 4, 0) == n.E_INVALID
    for d_bits in (0, 12, -8, 8192 + 8):
        assert n.lib.ise_binary_ivf_create(ctypes.byref(h), d_bits, 4, 0) == n.E_INVALID
        assert b"multiple of 8" in n.lib.ise_last_error() and not h.value
    for nlist in (0, -3):
        assert n.lib.ise_binary_ivf_create(ctypes.byref(h), 64, nlist, 0) == n.E_INVALID
        assert b"nlist" in n.lib.ise_last_error()
    assert n.lib.ise_binary_ivf_search_host(None, None, 1, 1, None, 1, None, None) == n.E_INVALID
    q = np.zeros((1, 8), np.uint8)
    p = np.zeros((1, 1), np.int64)
    D, I = np.zeros((1, 1), np.int32), np.zeros((1, 1), np.int64)
    args = lambda k, nprobe: (q.ctypes.data, 1, k, p.ctypes.data, nprobe, D.ctypes.data, I.ctypes.data)
    assert n.lib.ise_binary_ivf_search_host(None, *args(1, 1)) == n.E_INVALID  # a NULL handle
    assert b"handle" in n.lib.ise_last_error()
    assert n.lib.ise_binary_ivf_search_host(None, *args(0, 1)) == n.E_INVALID
    assert n.lib.ise_binary_ivf_search_host(None, *args(n.MAX_K + 1, 1)) == n.E_INVALID
    assert n.lib.ise_binary_ivf_search_host(None, *args(1, 0)) == n.E_INVALID
    assert n.lib.ise_binary_ivf_search_device(None, None, 1, 1, None, 1, None, None, None) == n.E_INVALID
    assert n.lib.ise_binary_ivf_add_host(None, None, None, 1) == n.E_INVALID
    assert n.lib.ise_binary_ivf_list_sizes_host(None, None) == n.E_INVALID
    assert n.lib.ise_binary_ivf_list_host(None, 0, None, None) == n.E_INVALID
    assert n.lib.ise_binary_ivf_stats(None, None) == n.E_INVALID
    assert n.lib.ise_binary_ivf_info(None, None, None, None, None) == n.E_INVALID
    assert n.lib.ise_binary_ivf_reset(None) == n.E_INVALID
    assert n.lib.ise_binary_ivf_destroy(None) == 0


# ---------------------------------------------------------------- the surface
def describe_binary_ivf_surface() -> dict:
    out = {name: desc for name, desc in describe_surface().items() if name in _BINARY_IVF}
    for desc in out.values():
        if desc["kind"] == "class":
            desc["attrs"] = {a: v for a, v in desc["attrs"].items() if not a.startswith("_") or a in _KEPT_DUNDERS}
    return out


def test_nothing_recorded_of_the_binary_ivf_has_gone_or_changed(golden_dir):
    with open(os.path.join(golden_dir, "faiss_compat_surface_binary_ivf.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(_BINARY_IVF)
    problems = _problems(recorded, describe_binary_ivf_surface())
    assert not problems, "\n".join(problems)
    attrs = recorded["IndexBinaryIVF"]["attrs"]
    for name in ("train", "add", "add_torch", "search", "search_preassigned", "search_torch", "list_size", "get_list", "reset",
                 "binary_ivf_stats", "range_search", "remove_ids", "ntotal"):
        assert name in attrs, name
    assert attrs["__init__"] == "(self, quantizer: 'IndexBinaryFlat', d: 'int', nlist: 'int')"


# ---------------------------------------------------------------- the reference against the flat reference
def test_reference_with_every_list_probed_is_the_flat_reference():
    rng = np.random.default_rng(5)
    for d, nlist, n, k in ((64, 7, 300, 10), (8, 3, 100, 120), (136, 5, 50, 1)):
        cs = d // 8
        C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
        xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
        xq = rng.integers(0, 256, (9, cs), dtype=np.uint8)
        D, I = binary_ivf_ref.search(C, xb, xq, k, nlist)
        Df, If = binary_ref.search(xb, xq, k)
        assert np.array_equal(D, Df) and np.array_equal(I, If)
        # fewer probes: a subset of the rows, in the same order, and never better than the flat answer
        D1, I1 = binary_ivf_ref.search(C, xb, xq, k, 2)
        assert (D1 >= Df).all()
        lists = binary_ivf_ref.assign(C, xb)
        pr = binary_ivf_ref.probes(C, xq, 2)
        for i in range(len(xq)):
            got = I1[i][I1[i] >= 0]
            assert np.isin(lists[got], pr[i]).all() and len(set(got.tolist())) == got.size


def test_reference_probe_tables_and_stats():
    rng = np.random.default_rng(6)
    C = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    lists = np.repeat(np.arange(4), [0, 1, 64, 65])
    xb = binary_ivf_ref.near_centroids(rng, C, lists)
    assert np.array_equal(binary_ivf_ref.assign(C, xb), lists)
    xq = rng.integers(0, 256, (3, 8), dtype=np.uint8)
    table = np.array([[-1, 4, 99], [2, 2, 2], [3, -1, 1]])
    assert binary_ivf_ref.clean_probes(table, 4) == [[], [2], [1, 3]]
    D, I = binary_ivf_ref.search_preassigned(xb, lists, xq, 70, table, 4)
    assert (I[0] == -1).all() and (D[0] == binary_ref.INT32_MAX).all()
    assert sorted(I[1][:64].tolist()) == list(range(1, 65)) and (I[1][64:] == -1).all()
    assert sorted(I[2][:66].tolist()) == [0] + list(range(65, 130)) and (I[2][66:] == -1).all()
    # one group of three queries, three passes for k = 70: the tiles of lists 1, 2, 3 are 1 + 1 + 2
    assert binary_ivf_ref.stats_of(table, [0, 1, 64, 65], 70) == {"batches": 1, "passes": 3, "tiles_loaded": 12}


# ---------------------------------------------------------------- the reference of one pass (tests/test_binary_ivf_lists_gpu.py)
def pass_example(rng, cs=9):
    """Lists of 0 .. 129 rows laid out as a rebuild leaves them, 16 queries (the first the zero code, which every pad slot
    equals) and a probe table with -1, out-of-range and repeated lists -> what ``block_lists_of`` takes, and the rows."""
    sizes = np.array([0, 1, 63, 64, 65, 128, 129], np.int64)
    nlist, n = len(sizes), int(sizes.sum())
    list_no = rng.permutation(np.repeat(np.arange(nlist), sizes))
    xb = rng.integers(0, 256, (12, cs), dtype=np.uint8)[rng.integers(0, 12, n)]  # 12 distinct codes: ties everywhere
    xq = np.concatenate([np.zeros((1, cs), np.uint8), xb[:3], rng.integers(0, 256, (12, cs), dtype=np.uint8)])
    none = np.zeros(nlist, np.int64), np.zeros(0, np.uint32), np.zeros((0, cs), np.uint8)
    got_sizes, codes, _, ids = binary_ivf_ref.rebuilt(*none, list_no, xb, 0, cs)
    assert np.array_equal(got_sizes, sizes) and (ids == binary_ivf_ref.PAD_ID).sum() == len(ids) - n
    table = rng.integers(-1, nlist + 1, (16, 3))
    table[1] = (5, 5, -1)
    table[2] = -1
    table[3] = (0, nlist, 2 ** 40)  # the empty list and nothing else
    masks = binary_ivf_ref.masks_of(table, nlist, 16)
    (offs, count, entries), = binary_ivf_ref.work_list_of(masks, sizes)
    keys = binary_ivf_ref.tile_keys(codes, ids, xq)
    return sizes, list_no, xb, xq, table, count, entries, keys


def test_block_lists_merge_to_search_preassigned():
    rng = np.random.default_rng(7)
    sizes, list_no, xb, xq, table, count, entries, keys = pass_example(rng)
    nlist = len(sizes)
    assert count >= 9 and (entries[:, 1] < 64).any() and len(set(entries[:, 2].tolist())) > 3
    order = rng.permutation(count)  # the result does not depend on the order of the entries, the blocks' lists do
    for nqt, kp in ((16, 1), (16, 7), (5, 32), (16, 32)):
        want = binary_ivf_ref.search_preassigned(xb, list_no, xq[:nqt], kp, table[:nqt], nlist)
        assert (want[1][2] == -1).all() and (want[1][3] == -1).all() and (want[1][1] >= 0).any()
        for ent in (entries, entries[order]):
            koe = keys[ent[:, 0]]
            D, I, lo_out = binary_ivf_ref.pass_of(koe, ent, count, nqt, kp)
            assert np.array_equal(D, want[0]) and np.array_equal(I, want[1])
            assert np.array_equal(lo_out == binary_ivf_ref.KEY_PAD, want[1][:, -1] == -1)
            for grid in (1, 2, 3, -(-count // 4), -(-count // 4) + 1, 64):
                lists, empty = binary_ivf_ref.block_lists_of(koe, ent, count, grid, nqt, kp)
                assert lists.shape == (grid, nqt, 32) and empty.sum() == max(0, grid - -(-count // 4))
                assert (lists[empty] == binary_ivf_ref.KEY_PAD).all() and (lists[:, :, 1:kp] >= lists[:, :, :kp - 1]).all()
                got = binary_ivf_ref.results_of(binary_ivf_ref.merged_of(lists, kp))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], lo_out)
    # a floor: the second pass of k = 40 continues where the first ended
    koe = keys[entries[:, 0]]
    first = binary_ivf_ref.pass_of(koe, entries, count, 16, 32)
    second = binary_ivf_ref.pass_of(koe, entries, count, 16, 8, first[2])
    want = binary_ivf_ref.search_preassigned(xb, list_no, xq, 40, table, nlist)
    assert np.array_equal(np.concatenate([first[0], second[0]], axis=1), want[0])
    assert np.array_equal(np.concatenate([first[1], second[1]], axis=1), want[1])


def test_blocks_partition_the_work_list_in_slot_order():
    """``work_list_of`` gives the entries in slot order; ``entries_of_block`` deals them to the blocks four at a time, each
    to exactly one block, and a block's entries stay in slot order.  A key of an id at or above 2^31 keeps it."""
    rng = np.random.default_rng(8)
    sizes, list_no, xb, xq, table, count, entries, keys = pass_example(rng)
    assert (np.diff(entries[:, 0].astype(np.int64)) > 0).all()
    for grid in (1, 2, 3, 4, 64):
        taken = [binary_ivf_ref.entries_of_block(count, grid, b) for b in range(grid)]
        assert sorted(np.concatenate(taken).tolist()) == list(range(count))
        for b, mine in enumerate(taken):
            assert (np.diff(entries[mine, 0].astype(np.int64)) > 0).all()
            assert all((e // 4) % grid == b for e in mine) and (len(mine) > 0) == (b * 4 < count)
        assert taken[0][:4].tolist() == list(range(min(4, count)))
    key = binary_ivf_ref.bin_key(np.array([0, 3]), np.array([0xFFFFFFFE, 2 ** 31], np.uint32))
    assert key.tolist() == [(1 << 32) | 0xFFFFFFFE, (4 << 32) | 2 ** 31]
    D, I, lo = binary_ivf_ref.results_of(np.array([[key[0], key[1], binary_ivf_ref.KEY_PAD]], np.uint64))
    assert D.tolist() == [[0, 3, binary_ref.INT32_MAX]] and I.tolist() == [[0xFFFFFFFE, 2 ** 31, -1]] and lo[0] == binary_ivf_ref.KEY_PAD
    assert binary_ivf_ref.stats_of(table, sizes, 70, batches=2)["batches"] == 2 and binary_ivf_ref.host_batches(4101) == 2
    assert binary_ivf_ref.host_batches(4096) == 1


if __name__ == "__main__":
    print(json.dumps(describe_binary_ivf_surface(), indent=1, sort_keys=True))
