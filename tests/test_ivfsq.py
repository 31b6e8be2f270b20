"""CPU tests of IndexIVFScalarQuantizer's host side: the "IwSq" file image, the numpy reference of the GPU tests, the
pass rule, the reference of the work list and of the rebuilt arrays, what raises before the device is touched, and the rebuild plan with 64-row tiles under the host sanitizers."""
import ctypes
import struct

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref, ivfsq_ref, sq_ref
from tests.knn_checks import assert_knn_identical, int_data
from tests.sel_ref import IP, L2

SQ = faiss.ScalarQuantizer


def image_args(rng, d, nlist, sizes, qtype, metric=L2, qmetric=L2, trained_quantizer=True):
    t = rng.standard_normal(2 if qtype == SQ.QT_8bit_uniform else 2 * d).astype(np.float32)
    t[t.size // 2:] = np.abs(t[t.size // 2:])
    cent = rng.standard_normal((nlist if trained_quantizer else 0, d)).astype(np.float32)
    ids = rng.permutation(int(sum(sizes))).astype(np.int64)
    lists, at = [], 0
    for s in sizes:
        lists.append((np.sort(ids[at:at + s]), rng.integers(0, 256, (s, d)).astype(np.uint8)))
        at += s
    return (d, metric, nlist, 3, qmetric, cent, qtype, t, lists, 0, 0.0, False)


def assert_same_parts(a, b):
    assert a[:5] == b[:5] and a[6] == b[6] and a[9:] == b[9:], (a[:5], b[:5], a[9:], b[9:])
    assert a[5].shape == b[5].shape and np.array_equal(a[5].view(np.uint32), b[5].view(np.uint32))
    assert np.array_equal(a[7].view(np.uint32), b[7].view(np.uint32))
    assert len(a[8]) == len(b[8])
    for (ia, ca), (ib, cb) in zip(a[8], b[8]):
        assert ib.dtype == np.int64 and cb.dtype == np.uint8 and cb.shape == (len(ib), a[0])
        assert np.array_equal(ia, ib) and np.array_equal(ca, cb)


@pytest.mark.parametrize("qtype", [SQ.QT_8bit, SQ.QT_8bit_uniform])
@pytest.mark.parametrize("sizes", [[4, 0, 1, 0, 7], [0, 0, 0]])
def test_file_round_trip(qtype, sizes):
    """serialize_ivfsq -> parse_ivfsq is the identity: empty lists, n = 0, both types, either metric."""
    rng = np.random.default_rng(3 + len(sizes) + qtype)
    for metric, qmetric, full in ((L2, L2, True), (IP, IP, True), (IP, L2, False)):
        args = image_args(rng, 5, len(sizes), sizes, qtype, metric, qmetric, full)
        buf = faiss.serialize_ivfsq(*args)
        assert buf[:4] == b"IwSq"
        parts = faiss.parse_ivfsq(buf)
        assert_same_parts(args, parts)
        assert faiss.serialize_ivfsq(*parts) == buf
        assert_same_parts(args, faiss.parse_ivfsq(buf + b"trailing bytes are ignored"))


def test_file_layout_and_sparse_sizes():
    """The fields where the comment in faiss_compat.py says they are, and the "sprs" form of the sizes."""
    rng = np.random.default_rng(9)
    d, nlist, sizes = 3, 4, [2, 0, 0, 1]
    args = image_args(rng, d, nlist, sizes, SQ.QT_8bit)
    buf = faiss.serialize_ivfsq(*args)
    hdr = struct.Struct("<4siqqqBi")
    assert hdr.unpack_from(buf, 0) == (b"IwSq", d, 3, 1 << 20, 1 << 20, 1, L2)
    off = hdr.size
    assert struct.unpack_from("<QQ", buf, off) == (nlist, 3)
    off += 16
    assert hdr.unpack_from(buf, off) == (b"IxF2", d, nlist, 1 << 20, 1 << 20, 1, L2)
    off += hdr.size + 8 + 4 * nlist * d
    assert struct.unpack_from("<BQ", buf, off) == (0, 0)  # no direct map
    off += 9
    assert struct.unpack_from("<iifQQQ", buf, off) == (SQ.QT_8bit, 0, 0.0, d, d, 2 * d)
    off += struct.calcsize("<iifQQQ") + 4 * 2 * d
    assert struct.unpack_from("<QB", buf, off) == (d, 0)  # code size, by_residual
    off += 9
    assert buf[off:off + 4] == b"ilar" and struct.unpack_from("<QQ", buf, off + 4) == (nlist, d)
    off += 20
    assert buf[off:off + 4] == b"full" and struct.unpack_from("<Q", buf, off + 4) == (nlist,)
    assert struct.unpack_from("<4Q", buf, off + 12) == tuple(sizes)
    tail = off + 12 + 8 * nlist
    assert len(buf) == tail + sum(sizes) * (d + 8)
    sparse = buf[:off] + b"sprs" + struct.pack("<Q", 4) + struct.pack("<4Q", 0, 2, 3, 1) + buf[tail:]
    assert_same_parts(args, faiss.parse_ivfsq(sparse))
    for bad in (struct.pack("<Q", 3) + struct.pack("<3Q", 0, 2, 3), struct.pack("<Q", 2) + struct.pack("<2Q", 4, 3)):
        with pytest.raises(RuntimeError):
            faiss.parse_ivfsq(buf[:off] + b"sprs" + bad + buf[tail:])
    with pytest.raises(RuntimeError, match="size form"):
        faiss.parse_ivfsq(buf[:off] + b"what" + buf[off + 4:])


def test_file_errors():
    """Every truncation point, a wrong count in each counted field, a foreign fourcc and a foreign quantiser type."""
    rng = np.random.default_rng(4)
    d, nlist = 3, 3
    args = image_args(rng, d, nlist, [2, 0, 3], SQ.QT_8bit)
    buf = faiss.serialize_ivfsq(*args)
    for cut in range(len(buf)):  # headers, the quantiser image, the trained vector, the sizes, codes and ids
        with pytest.raises(RuntimeError):
            faiss.parse_ivfsq(buf[:cut])
    hdr = struct.calcsize("<4siqqqBi")
    q_at = hdr + 16
    sq_at = q_at + hdr + 8 + 4 * nlist * d + 9
    lists_at = sq_at + struct.calcsize("<iifQQQ") + 4 * 2 * d + 9

    def patched(at, fmt, *v):
        b = bytearray(buf)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    for what, blob in (("ntotal", patched(8, "<q", 6)), ("nlist", patched(hdr, "<Q", 4)), ("quantiser d", patched(q_at + 4, "<i", 4)),
                       ("quantiser rows", patched(q_at + 8, "<q", 2)), ("quantiser count", patched(q_at + hdr, "<Q", 8)),
                       ("direct map", patched(sq_at - 9, "<B", 1)), ("sq d", patched(sq_at + 12, "<Q", 4)),
                       ("sq code size", patched(sq_at + 20, "<Q", 4)), ("trained count", patched(sq_at + 28, "<Q", 2)),
                       ("code size", patched(lists_at - 9, "<Q", 4)), ("lists fourcc", patched(lists_at, "<4s", b"ilxx")),
                       ("lists nlist", patched(lists_at + 4, "<Q", 2)), ("lists code size", patched(lists_at + 12, "<Q", 1)),
                       ("size count", patched(lists_at + 24, "<Q", 2)), ("a size", patched(lists_at + 32, "<Q", 3))):
        with pytest.raises(RuntimeError):
            faiss.parse_ivfsq(blob)
            pytest.fail(f"accepted a wrong {what}")
    with pytest.raises(RuntimeError, match="not an IndexIVFScalarQuantizer"):
        faiss.parse_ivfsq(b"IwFl" + buf[4:])
    with pytest.raises(RuntimeError, match="not an IndexIVFScalarQuantizer"):
        faiss.parse_ivfsq(faiss.serialize_sq(d, L2, SQ.QT_8bit, args[7], np.zeros((0, d), np.uint8)))
    with pytest.raises(RuntimeError, match="quantiser type"):
        faiss.parse_ivfsq(patched(q_at, "<4s", b"IxPq"))
    for qtype in (SQ.QT_4bit, SQ.QT_fp16, SQ.QT_8bit_direct):
        with pytest.raises(RuntimeError, match="scalar quantiser type"):
            faiss.parse_ivfsq(patched(sq_at, "<i", qtype))
    # by_residual = true parses (the flag is data); reading such a file into an index is refused (GPU tests)
    assert faiss.parse_ivfsq(patched(lists_at - 1, "<B", 1))[-1] is True


@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_results(metric):
    """The ranking form agrees with the brute force over the probed members: empty probed lists, a row of -1 probes
    and a duplicate probe."""
    rng = np.random.default_rng(21)
    n, d, nlist = 200, 12, 5
    t, m, s = sq_ref.integer_trained(rng, d, sq_ref.QT_8BIT)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    vmin, vdiff = sq_ref.expand(t, d, sq_ref.QT_8BIT)
    dec = sq_ref.decode(sq_ref.encode(xb, vmin, vdiff), vmin, vdiff)
    assert np.array_equal(dec, xb)
    xq = int_data("small", rng, 6, d)
    assign = rng.integers(0, nlist - 1, n)  # the last list stays empty
    probes = np.array([[0, 1], [4, 4], [3, -1], [2, 2], [-1, -1], [1, 0]], np.int64)
    members = ivf_ref.probed_members(probes, assign, nlist)
    assert members[1].size == 0 and members[4].size == 0 and np.array_equal(members[3], np.flatnonzero(assign == 2))
    full = sq_ref.expected(xq, dec, n, metric)
    for k in (1, 10, 150):
        Da, Ia = ivfsq_ref.expected(xq, dec, probes, assign, nlist, k, metric, full)
        Db, Ib = ivf_ref.expected_brute(dec, xq, members, k, metric)
        assert_knn_identical(Da, Ia, Db + np.float32(0.0), Ib, f"k={k}")
        assert_knn_identical(*ivfsq_ref.expected(xq, dec, probes, assign, nlist, k, metric), Da, Ia, f"own ranking k={k}")
        assert (Ia[1] == -1).all() and (Ia[4] == -1).all()


def test_pass_rule():
    """Hand-counted: the tiles of a pass, groups of 16 queries up to d = 1472 and of 8 above."""
    sizes = [0, 1, 63, 64, 65, 128, 129]
    assert ivfsq_ref.tile0_of(sizes).tolist() == [0, 0, 1, 2, 3, 5, 7, 10]
    assert ivfsq_ref.tiles_of(sizes) == 10 and ivfsq_ref.tiles_of([]) == 0
    probes = np.array([[4, 4], [0, -1], [7, 6], [-1, -1]], np.int64)  # a duplicate, the empty list, out of range
    assert ivfsq_ref.pass_tile_sets(probes, sizes, 24) == [[3, 4, 7, 8, 9]]
    assert ivfsq_ref.stats_of(probes, sizes, 24, 10) == {"batches": 1, "passes": 1, "tiles_loaded": 5}
    assert ivfsq_ref.stats_of(probes, sizes, 24, 33) == {"batches": 1, "passes": 2, "tiles_loaded": 10}
    assert ivfsq_ref.stats_of(np.full((3, 2), -1), sizes, 24, 70) == {"batches": 1, "passes": 3, "tiles_loaded": 0}
    # 17 queries: two groups of 16 at d = 1472, three of 8 at d = 1473 .. 2048
    probes = np.array([[1]] * 8 + [[5]] * 8 + [[2]], np.int64)
    assert sq_ref.qt_of(1472) == 16 and sq_ref.qt_of(1473) == 8 and sq_ref.qt_of(2048) == 8
    assert ivfsq_ref.pass_tile_sets(probes, sizes, 1472) == [[0, 5, 6], [1]]
    assert ivfsq_ref.pass_tile_sets(probes, sizes, 2048) == [[0], [5, 6], [1]]
    assert ivfsq_ref.stats_of(probes, sizes, 2048, 64) == {"batches": 1, "passes": 6, "tiles_loaded": 8}
    assert ivfsq_ref.stats_of(probes, sizes, 512, 64) == {"batches": 1, "passes": 4, "tiles_loaded": 8}


@pytest.mark.parametrize("d", [24, 2048])  # groups of 16 and of 8 queries
def test_work_list_reference(d):
    """``masks_of`` / ``work_list_of`` on random tables against ``pass_tile_sets`` and ``stats_of``: the entries of a
    group are the tiles of its pass, ascending, each with the rows its list has left and the mask of the queries that
    name the list; the offsets are the running count, on the unprobed lists too."""
    qt = sq_ref.qt_of(d)
    rng = np.random.default_rng(d)
    for trial in range(30):
        nlist = int(rng.integers(1, 400))
        sizes = rng.choice([0, 0, 1, 63, 64, 65, 128, 129, 300], nlist)
        nq, nprobe = int(rng.integers(1, 70)), int(rng.integers(1, 9))
        probes = rng.integers(-3, nlist + 3, (nq, nprobe))
        if trial % 5 == 0:
            probes[:] = -1
        masks = ivfsq_ref.masks_of(probes, nlist, qt)
        assert masks.dtype == np.uint32 and masks.shape == (-(-nq // qt), nlist) and (masks >> qt == 0).all()
        for q in range(nq):
            named = {int(l) for l in probes[q] if 0 <= l < nlist}
            assert set(np.flatnonzero(masks[q // qt] >> (q % qt) & 1).tolist()) == named
        wl = ivfsq_ref.work_list_of(masks, sizes)
        sets = ivfsq_ref.pass_tile_sets(probes, sizes, d)
        t0, meta = ivfsq_ref.tile0_of(sizes), ivfsq_ref.meta_of(sizes)
        assert np.array_equal(meta[:nlist + 1], t0) and np.array_equal(meta[nlist + 1:2 * nlist + 1], sizes) and len(meta) == 2 * nlist + 1 + t0[-1]
        assert len(wl) == len(sets) == len(masks)
        for g, ((offs, count, entries), tiles) in enumerate(zip(wl, sets)):
            assert offs.dtype == entries.dtype == np.uint32 and entries.shape == (count, 4) and count == len(tiles)
            assert entries[:, 0].tolist() == tiles and (entries[:, 3] == 0).all()
            lists = meta[2 * nlist + 1:][entries[:, 0]]
            assert np.array_equal(entries[:, 2], masks[g][lists]) and (entries[:, 2] != 0).all()
            assert np.array_equal(entries[:, 1], np.minimum(64, sizes[lists] - 64 * (entries[:, 0] - t0[lists])))
            assert (entries[:, 1] >= 1).all()
            run = 0
            for l in range(nlist):
                assert offs[l] == run
                run += int(t0[l + 1] - t0[l]) if masks[g][l] else 0
            assert run == count
        for k in (10, 70):
            assert ivfsq_ref.stats_of(probes, sizes, d, k)["tiles_loaded"] == sum(c for _, c, _ in wl) * -(-k // 32)
    # hand-counted (test_pass_rule's table): lists 4 and 6 of sizes 65 and 129
    masks = ivfsq_ref.masks_of(np.array([[4, 4], [0, -1], [7, 6], [-1, -1]]), 7, qt)
    assert masks.tolist() == [[2, 0, 0, 0, 1, 0, 4]]
    (offs, count, entries), = ivfsq_ref.work_list_of(masks, [0, 1, 63, 64, 65, 128, 129])
    assert offs.tolist() == [0, 0, 0, 0, 0, 2, 2] and count == 5
    assert entries.tolist() == [[3, 64, 1, 0], [4, 1, 1, 0], [7, 64, 4, 0], [8, 64, 4, 0], [9, 1, 4, 0]]


def test_rebuilt_reference():
    """``rebuilt`` in two steps is ``rebuilt`` in one; every list holds its ids ascending, its rows' bytes and terms,
    and pad slots behind them; ``rebuild_dest`` names the slot each pending row lands in."""
    rng = np.random.default_rng(77)
    nlist, stride, n = 23, 32, 1500
    lists = np.minimum(rng.integers(0, nlist + 8, n), nlist - 1)  # the last list is long
    lists[lists == 3] = 4                                        # list 3 stays empty
    codes = rng.integers(0, 256, (n, stride)).astype(np.uint8)
    terms = rng.random(n)
    none = (np.zeros(nlist, np.int64), np.zeros(0, np.uint32), np.zeros((0, stride), np.uint8))
    one = ivfsq_ref.rebuilt(*none, lists, codes, 0, stride, np.zeros(0), terms)
    cut = 611
    half = ivfsq_ref.rebuilt(*none, lists[:cut], codes[:cut], 0, stride, np.zeros(0), terms[:cut])
    two = ivfsq_ref.rebuilt(half[0], half[3], half[1], lists[cut:], codes[cut:], cut, stride, half[2], terms[cut:])
    for a, b in zip(one, two):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    sizes, new_codes, new_terms, ids = one
    assert sizes.tolist() == np.bincount(lists, minlength=nlist).tolist() and sizes[3] == 0 and sizes[-1] > 128
    t0 = ivfsq_ref.tile0_of(sizes)
    assert len(ids) == 64 * t0[-1] and ids.dtype == np.uint32 and new_codes.shape == (len(ids), stride)
    for l, want in enumerate(ivf_ref.list_members(lists, nlist)):
        a, m = 64 * t0[l], len(want)
        assert np.array_equal(ids[a:a + m], want) and np.array_equal(new_codes[a:a + m], codes[want])
        assert np.array_equal(new_terms[a:a + m], terms[want])
        pad = slice(a + m, 64 * t0[l + 1])
        assert (ids[pad] == ivfsq_ref.PAD_ID).all() and not new_codes[pad].any() and not new_terms[pad].any()
    dest = ivfsq_ref.rebuild_dest(half[0], lists[cut:])
    assert dest.dtype == np.uint32 and np.array_equal(ids[dest], cut + np.arange(n - cut)) and len(set(dest.tolist())) == n - cut
    # the default row term: the sum of the squared bytes
    dflt = ivfsq_ref.rebuilt(*none, lists[:9], codes[:9], 0, stride)
    assert np.array_equal(dflt[2][dflt[3] != ivfsq_ref.PAD_ID], (codes[:9].astype(np.float64) ** 2).sum(1)[dflt[3][dflt[3] != ivfsq_ref.PAD_ID]])


def test_rebuilt_reference_with_16_row_tiles():
    """The layout functions at ``tile_rows = 16``, the float32 lists' tiles: every list starts on a 16-row tile, holds its
    rows in id order and pad slots to the end of its last tile; the tables are ``ivf_plan_meta``'s; two steps are one."""
    rng = np.random.default_rng(16)
    nlist, stride, n = 9, 48, 400
    lists = rng.integers(0, nlist, n)
    lists[lists == 4] = 5                # list 4 stays empty
    lists[:32] = 2                       # list 2 holds at least two tiles
    codes = rng.integers(0, 256, (n, stride)).astype(np.uint8)
    none = (np.zeros(nlist, np.int64), np.zeros(0, np.uint32), np.zeros((0, stride), np.uint8))
    one = ivfsq_ref.rebuilt(*none, lists, codes, 0, stride, tile_rows=16)
    half = ivfsq_ref.rebuilt(*none, lists[:150], codes[:150], 0, stride, tile_rows=16)
    two = ivfsq_ref.rebuilt(half[0], half[3], half[1], lists[150:], codes[150:], 150, stride, half[2], tile_rows=16)
    for a, b in zip(one, two):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    sizes, new_codes, _, ids = one
    t0 = ivfsq_ref.tile0_of(sizes, 16)
    assert t0[-1] == ivfsq_ref.tiles_of(sizes, 16) == ivf_ref.tiles_of(sizes) > ivfsq_ref.tiles_of(sizes)
    assert np.diff(t0).tolist() == [-(-int(s) // 16) for s in sizes] and len(ids) == 16 * t0[-1] and sizes[4] == 0
    for l, want in enumerate(ivf_ref.list_members(lists, nlist)):
        a, m = 16 * t0[l], len(want)
        assert np.array_equal(ids[a:a + m], want) and np.array_equal(new_codes[a:a + m], codes[want])
        pad = slice(a + m, 16 * t0[l + 1])
        assert (ids[pad] == ivfsq_ref.PAD_ID).all() and not new_codes[pad].any()
    meta = ivfsq_ref.meta_of(sizes, 16)
    assert meta.dtype == np.uint32 and len(meta) == 2 * nlist + 1 + t0[-1]
    assert meta[:nlist + 1].tolist() == t0.tolist() and meta[nlist + 1:2 * nlist + 1].tolist() == sizes.tolist()
    assert meta[2 * nlist + 1:].tolist() == [l for l in range(nlist) for _ in range(t0[l], t0[l + 1])]
    dest = ivfsq_ref.rebuild_dest(half[0], lists[150:], 16)
    assert np.array_equal(ids[dest], 150 + np.arange(n - 150)) and len(set(dest.tolist())) == n - 150
    # ids near the top of the range keep their bits
    top = ivfsq_ref.rebuilt(*none, lists[:5], codes[:5], 2 ** 32 - 6, stride, tile_rows=16)
    assert sorted(top[3][top[3] != ivfsq_ref.PAD_ID].tolist()) == list(range(2 ** 32 - 6, 2 ** 32 - 1))


def test_early_raises():
    """by_residual = True (the default) and the unprovided quantiser types raise before anything else is looked at."""
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFScalarQuantizer(None, 16, 4, SQ.QT_8bit)
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFScalarQuantizer(None, 16, 4, SQ.QT_8bit, faiss.METRIC_L2, True)
    for qtype in (SQ.QT_4bit, SQ.QT_4bit_uniform, SQ.QT_fp16, SQ.QT_8bit_direct, SQ.QT_6bit, SQ.QT_bf16, SQ.QT_8bit_direct_signed):
        with pytest.raises(NotImplementedError, match="qtype"):
            faiss.IndexIVFScalarQuantizer(None, 16, 4, qtype, faiss.METRIC_L2, by_residual=False)
    for name in ("range_search", "remove_ids"):
        with pytest.raises(NotImplementedError, match="IndexIVFScalarQuantizer"):
            getattr(faiss.IndexIVFScalarQuantizer, name)(faiss.IndexIVFScalarQuantizer.__new__(faiss.IndexIVFScalarQuantizer))
    assert issubclass(faiss.IndexIVFScalarQuantizer, faiss._IndexIVF) and issubclass(faiss.IndexIVFFlat, faiss._IndexIVF)
    assert not issubclass(faiss.IndexIVFScalarQuantizer, faiss.IndexIVFFlat)


def test_argument_errors_through_abi():
    from image_search_engine_amd import _native as n

    h = ctypes.c_void_p()
    for args, word in (((0, 0, n.METRIC_L2, 4, 0), b"d must"), ((n.SQ_MAX_D + 1, 0, n.METRIC_L2, 4, 0), b"ISE_SQ_MAX_D"),
                       ((8, 0, n.METRIC_L2, 0, 0), b"nlist"), ((8, 1, n.METRIC_L2, 4, 0), b"qtype"), ((8, 3, n.METRIC_L2, 4, 0), b"qtype"),
                       ((8, 2, 7, 4, 0), b"metric")):
        assert n.lib.ise_ivfsq_create(ctypes.byref(h), *args) == n.E_INVALID, args
        assert word in n.lib.ise_last_error(), (args, n.lib.ise_last_error())
        assert h.value is None
    assert n.lib.ise_ivfsq_create(None, 8, 0, n.METRIC_L2, 4, 0) == n.E_INVALID
    assert n.lib.ise_ivfsq_destroy(None) == 0
    assert n.lib.ise_ivfsq_reset(None) == n.E_INVALID
    assert n.lib.ise_ivfsq_info(None, None, None, None, None, None, None, None) == n.E_INVALID
    x = np.zeros((2, 8), np.float32)
    codes = np.zeros((2, 8), np.uint8)
    lists = np.zeros(2, np.int64)
    D, I = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int64)
    assert n.lib.ise_ivfsq_set_trained_host(None, None) == n.E_INVALID and b"NULL" in n.lib.ise_last_error()
    assert n.lib.ise_ivfsq_get_trained_host(None, x.ctypes.data) == n.E_INVALID and b"handle" in n.lib.ise_last_error()
    for add, rows in ((n.lib.ise_ivfsq_add_host, x), (n.lib.ise_ivfsq_add_codes_host, codes)):
        assert add(None, None, lists.ctypes.data, 2) == n.E_INVALID and b"pointer is NULL" in n.lib.ise_last_error()
        assert add(None, rows.ctypes.data, None, 2) == n.E_INVALID and b"pointer is NULL" in n.lib.ise_last_error()
        assert add(None, rows.ctypes.data, lists.ctypes.data, -1) == n.E_INVALID and b"n must" in n.lib.ise_last_error()
        assert add(None, rows.ctypes.data, lists.ctypes.data, 2) == n.E_INVALID and b"handle" in n.lib.ise_last_error()
    assert n.lib.ise_ivfsq_add_device(None, None, None, 2, None) == n.E_INVALID
    assert n.lib.ise_ivfsq_list_sizes_host(None, lists.ctypes.data) == n.E_INVALID
    assert n.lib.ise_ivfsq_list_host(None, 0, None, None) == n.E_INVALID
    for search, tail in ((n.lib.ise_ivfsq_search_host, ()), (n.lib.ise_ivfsq_search_device, (None,))):
        for k in (0, -1, n.MAX_K + 1):
            assert search(None, x.ctypes.data, 2, k, lists.ctypes.data, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
            assert b"k must" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 0, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"nprobe" in n.lib.ise_last_error()
        assert search(None, None, 2, 3, lists.ctypes.data, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"pointer is NULL" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, None, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"pointer is NULL" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 1, None, I.ctypes.data, *tail) == n.E_INVALID
        assert b"output pointer" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"handle" in n.lib.ise_last_error()
    assert n.lib.ise_ivfsq_stats(None, (ctypes.c_uint64 * 3)()) == n.E_INVALID


def test_rebuild_bookkeeping_standalone(tmp_path):
    """csrc/ise_ivf_plan.hpp with 64-row tiles in a stand-alone host program with its own main, under the address and
    undefined-behaviour sanitizers (linked statically).  A missing compiler or sanitizer runtime fails the test."""
    import os
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone check (it is a tool of the build, not hardware)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "ivfsq_plan_check.cpp")
    exe = str(tmp_path / "ivfsq_plan_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized build failed (no unsanitized fallback):\n" + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
