"""GPU tests of IndexIVFScalarQuantizer's work list and rebuild at many lists (csrc/ise_ivf_tiles.hpp: ivf_mask_kernel,
ivf_offsets_kernel, ivf_work_kernel, ivf_move_tiles_kernel<64, u32x4>, ivf_scatter_rows_kernel<u32x4>).
tests/test_ivfsq_gpu.py builds at most 8 lists: every thread of the offsets kernel owns one list or none, the work
kernel writes a handful of entries and the rebuild maps a handful of tiles.  Here the lists are in the hundreds and
thousands.

The first two tests call the kernels directly through tests/native/ivfsq_lists_harness.hip, whose launches are the
product's own (ivf_work_list_launch, ivf_rebuild_launch), and compare every table they write with
tests/ivfsq_ref.py; the others go through the index.  The device tables are plain integers and the data is the integer
construction of tests/sq_ref.py: every comparison is bit for bit.  The work buffer is never cleared between searches,
so no test repeats a probe table in consecutive calls.

The harness is built by `make -C image-search-engine_amd/csrc` (target libise_ivfsq_check.so); without it the tests
fail, they do not skip."""
import ctypes
import functools
import os

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref, ivfsq_ref, sq_ref
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data
from tests.sel_ref import IP, L2
from tests.test_ivfsq_gpu import check_lists, counted, force_add, new_index, pass_blocks, search_pre, sizes_of, sq_index

pytestmark = pytest.mark.gpu

SQ = faiss.ScalarQuantizer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "image-search-engine_amd", "csrc", "libise_ivfsq_check.so")
EDGE_SIZES = (0, 1, 63, 64, 65, 128, 129)  # list l has EDGE_SIZES[l % 7] rows: 7 is coprime to every span length used
SENT = 0xA5A5A5A5                           # what the harness' outputs hold before a launch: no table ever holds it

_vp, _int, _ll, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint32
PROTOTYPES = {
    "chk_ivfsq_work_list": [_vp, _int, _int, _int, _int, _vp, _ll, _vp, _vp, _vp, _vp],
    "chk_ivfsq_rebuild": [_vp, _vp, _vp, _vp, _ll, _vp, _vp, _ll, _vp, _u32, _int, _int, _vp, _ll, _vp, _vp, _vp],
    "chk_ivf_rebuild": [_int, _int, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _u32, _int, _vp, _ll, _vp, _vp],  # tests/test_ivf_rebuild_gpu.py
}


@pytest.fixture(scope="module")
def lib():
    import torch  # first: the harness binds to the HIP runtime torch has loaded

    assert torch.cuda.is_available()
    if not os.path.exists(LIB_PATH):
        pytest.fail("csrc/libise_ivfsq_check.so is missing: build it with "
                    "`make -C image-search-engine_amd/csrc libise_ivfsq_check.so`")
    handle = ctypes.CDLL(LIB_PATH)
    for name, args in PROTOTYPES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _int, args
    return handle


def dev(a):
    """numpy -> a CUDA tensor of the same bits (uint32 as int32)"""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def dev_filled(shape, value=SENT):
    """a CUDA int32 tensor with every word the 32-bit pattern ``value``"""
    import torch

    return torch.full(shape, int(np.array(value, np.uint32).view(np.int32)), dtype=torch.int32, device="cuda")


def host_u32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def run(fn, *args):
    """launch on the null stream (torch's default stream), wait, and take any error the kernels left"""
    import torch

    rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    assert rc == 0, f"launch failed: hip error {rc}"
    torch.cuda.synchronize()


def edge_sizes(nlist: int) -> np.ndarray:
    return np.array(EDGE_SIZES, np.int64)[np.arange(nlist) % 7]


# ---------------------------------------------------------------- a. the work-list kernels, direct
def work_list(lib, probes, sizes, qshift):
    """-> (masks [groups][nlist], offs [groups][nlist], counts [groups], work [groups][tiles][4]) uint32, as the three
    kernels leave them; every output holds SENT on entry (the masks too: the launch has to clear them)."""
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    nq, nprobe = probes.shape
    nlist, tiles = len(sizes), ivfsq_ref.tiles_of(sizes)
    meta = ivfsq_ref.meta_of(sizes)
    groups = -(-nq // (1 << qshift))
    assert nq >= 1 and nprobe >= 1 and meta.dtype == np.uint32 and len(meta) == 2 * nlist + 1 + tiles
    assert meta[nlist] == tiles and (meta[2 * nlist + 1:] < nlist).all()  # the tables name lists and tiles that exist
    masks, offs, counts = dev_filled((groups, nlist)), dev_filled((groups, nlist)), dev_filled((groups,))
    work = dev_filled((groups, tiles, 4))
    run(lib.chk_ivfsq_work_list, dev(probes), nq, nprobe, nlist, qshift, dev(meta), tiles, masks, offs, counts, work)
    return host_u32(masks), host_u32(offs), host_u32(counts), host_u32(work)


def span_of(nlist: int, t: int):
    """the lists [l0, l1) thread t of ivf_offsets_kernel owns"""
    per = -(-nlist // 256)
    l0 = min(nlist, t * per)
    return l0, min(nlist, l0 + per)


def probe_tables(rng, nq: int, nlist: int, sizes):
    """(name, int64 [nq][nprobe]) -- the rows differ, so the masks differ from list to list"""
    some = rng.random(nq) < 0.6  # the queries that probe in the sparse tables
    some[rng.integers(0, nq)] = True
    last_thread = (nlist - 1) // -(-nlist // 256)  # the last thread with a list: a short span when per does not divide nlist
    mid = span_of(nlist, last_thread // 2)
    end = span_of(nlist, last_thread)
    ends = np.array([mid[0], mid[1] - 1, end[0], end[1] - 1], np.int64)
    empty = np.flatnonzero(sizes == 0)
    tenth = max(1, nlist // 10)
    odd = np.array([-1, nlist, nlist + 7, 2 ** 40, -2 ** 40], np.int64)
    mixed = rng.integers(0, nlist, (nq, 8))
    mixed[:, 1] = mixed[:, 0]                                   # a duplicate in every row
    mixed[np.arange(nq), rng.integers(2, 8, nq)] = odd[rng.integers(0, 5, nq)]
    mixed[:, 5] = odd[np.arange(nq) % 5]                         # each of the five at least once per five queries
    mixed[0] = [-1, nlist, nlist + 7, 2 ** 40, -2 ** 40, nlist - 1, nlist - 1, -1]
    return [
        ("nothing but -1", np.full((nq, 3), -1, np.int64)),
        ("every list", np.tile(np.arange(nlist, dtype=np.int64), (nq, 1))),
        ("only list 0", np.where(some, 0, -1).reshape(nq, 1)),
        ("only the last list", np.where(some, nlist - 1, -1).reshape(nq, 1)),
        ("the ends of a thread's span", np.stack([ends[np.arange(nq) % 4], ends[(np.arange(nq) // 2 + 1) % 4]], axis=1)),
        ("only empty lists", empty[rng.integers(0, len(empty), (nq, 4))]),
        ("a tenth of the lists", np.stack([rng.choice(nlist, tenth, replace=False) for _ in range(nq)]).astype(np.int64)),
        ("-1, nlist, nlist + 7, +-2^40 and duplicates", mixed),
    ]


@pytest.mark.parametrize("qshift,groups", [(4, 1), (4, 3), (4, 4), (3, 1), (3, 3), (3, 8)])  # 4 | 8 groups: a full chunk
@pytest.mark.parametrize("nlist", [1, 2, 255, 256, 257, 511, 512, 513, 1000, 4099])
def test_work_list_kernels(lib, nlist, qshift, groups):
    """per = ceil(nlist / 256) is 1, 2, 3, 4 and 17; the last thread with a list owns a full span (256, 512), a short
    one (257, 511, 513, 1000, 4099) and the threads behind it own none."""
    qt = 1 << qshift
    nq = groups * qt - 3  # not a multiple of QT
    sizes = edge_sizes(nlist)
    tiles = ivfsq_ref.tiles_of(sizes)
    assert nlist < 257 or tiles > 256  # more than one block of ivf_work_kernel in x
    rng = np.random.default_rng([nlist, qshift, groups])
    failures = []
    for name, probes in probe_tables(rng, nq, nlist, sizes):
        assert probes.shape[0] == nq and probes.dtype == np.int64
        want_masks = ivfsq_ref.masks_of(probes, nlist, qt)
        want = ivfsq_ref.work_list_of(want_masks, sizes)
        masks, offs, counts, work = work_list(lib, probes, sizes, qshift)
        assert masks.shape == want_masks.shape and len(want) == groups
        if name == "only empty lists":
            assert want_masks.any() and all(c == 0 for _, c, _ in want)
        if name == "every list":
            assert all(c == tiles for _, c, _ in want)
        if not np.array_equal(masks, want_masks):
            g, l = np.argwhere(masks != want_masks)[0]
            failures.append(f"{name}: masks[{g}][{l}] = {masks[g, l]:#x}, want {want_masks[g, l]:#x}")
        if (masks >> qt).any():
            failures.append(f"{name}: a mask has a bit at or above {qt}")
        for g, (want_offs, want_count, want_entries) in enumerate(want):
            if not np.array_equal(offs[g], want_offs):
                l = np.flatnonzero(offs[g] != want_offs)[0]
                failures.append(f"{name}: offs[{g}][{l}] = {offs[g, l]}, want {want_offs[l]}")
            if counts[g] != want_count:
                failures.append(f"{name}: count[{g}] = {counts[g]}, want {want_count}")
            if not np.array_equal(work[g, :want_count], want_entries):
                e = np.flatnonzero((work[g, :want_count] != want_entries).any(1))[0]
                failures.append(f"{name}: work[{g}][{e}] = {work[g, e].tolist()}, want {want_entries[e].tolist()}")
            if not (work[g, want_count:] == SENT).all():
                e = want_count + np.flatnonzero((work[g, want_count:] != SENT).any(1))[0]
                failures.append(f"{name}: work[{g}][{e}] = {work[g, e].tolist()} was written behind count = {want_count}")
    assert not failures, f"{len(failures)} differences; the first: " + " | ".join(failures[:5])


# ---------------------------------------------------------------- b. the rebuild kernels, direct
def rebuild(lib, old_sizes, old, pend_lists, pend_codes, pend_rterm, id0, stride):
    """-> (codes, rterm, ids) of the new arrays as ivf_rebuild_launch leaves them; old = (codes, rterm, ids) laid out
    by old_sizes.  The slot numbers come from the reference's plan; the new arrays hold SENT words on entry."""
    nlist = len(old_sizes)
    old_codes, old_rterm, old_ids = old
    old_tiles = ivfsq_ref.tiles_of(old_sizes)
    new_sizes = old_sizes + np.bincount(pend_lists, minlength=nlist)
    new_tiles = ivfsq_ref.tiles_of(new_sizes)
    dest = ivfsq_ref.rebuild_dest(old_sizes, pend_lists)
    meta, nmeta = ivfsq_ref.meta_of(old_sizes), ivfsq_ref.meta_of(new_sizes)
    m = len(pend_lists)
    # every array is as large as the tables say, every slot lies in the new arrays, and no two rows share one
    assert stride % 16 == 0 and m >= 1 and new_tiles >= 1
    assert old_codes.shape == (old_tiles * 64, stride) and old_codes.dtype == np.uint8
    assert old_rterm.shape == (old_tiles * 64,) and old_rterm.dtype == np.float64
    assert old_ids.shape == (old_tiles * 64,) and old_ids.dtype == np.uint32
    assert pend_codes.shape == (m, stride) and pend_codes.dtype == np.uint8 and pend_rterm.shape == (m,) and pend_rterm.dtype == np.float64
    assert len(meta) == 2 * nlist + 1 + old_tiles and len(nmeta) == 2 * nlist + 1 + new_tiles
    assert (np.diff(nmeta[:nlist + 1].astype(np.int64)) >= np.diff(meta[:nlist + 1].astype(np.int64))).all()  # no list shrinks
    assert dest.shape == (m,) and dest.max() < new_tiles * 64 and len(np.unique(dest)) == m
    nx = dev_filled((new_tiles * 64, stride // 4))
    nr = dev_filled((new_tiles * 64, 2))
    nids = dev_filled((new_tiles * 64,))
    run(lib.chk_ivfsq_rebuild, dev(old_codes), dev(old_rterm), dev(old_ids), dev(meta), old_tiles, dev(pend_codes), dev(pend_rterm), m,
        dev(dest), id0, stride, nlist, dev(nmeta), new_tiles, nx, nr, nids)
    return nx.cpu().numpy().view(np.uint8).reshape(-1, stride), nr.cpu().numpy().view(np.float64).reshape(-1), host_u32(nids)


def assert_arrays(got, want, what):
    for name, a, b in zip(("codes", "row terms", "ids"), got, want):
        a, b = (a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else (a, b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        if not np.array_equal(a, b):
            slot = np.argwhere(a != b)[0][0]
            raise AssertionError(f"{what}: the {name} differ in {int((a != b).sum())} places, first at slot {slot} "
                                 f"(tile {slot // 64}, row {slot % 64})")


@pytest.mark.parametrize("stride", [64, 128, 2048])  # a row is 4, 8 and 128 sixteen-byte units: fewer than a wave's lanes | two rounds
def test_rebuild_kernels(lib, stride):
    nlist = 300
    rng = np.random.default_rng(stride)
    none = (np.zeros((0, stride), np.uint8), np.zeros(0), np.zeros(0, np.uint32))
    zero = np.zeros(nlist, np.int64)
    # no old tile at all: the move kernel is not launched.  The ids interleave in every list
    old_sizes = edge_sizes(nlist)
    n0 = int(old_sizes.sum())
    lists0 = rng.permutation(np.repeat(np.arange(nlist), old_sizes))
    codes0 = rng.integers(0, 256, (n0, stride)).astype(np.uint8)
    rterm0 = rng.random(n0)
    assert n0 % 4 != 0
    sizes1, *want0 = ivfsq_ref.rebuilt(zero, none[2], none[0], lists0, codes0, 0, stride, none[1], rterm0)
    assert np.array_equal(sizes1, old_sizes)
    got0 = rebuild(lib, zero, none, lists0, codes0, rterm0, 0, stride)
    assert_arrays(got0, want0, "no old tiles")
    # over those arrays: per seven lists, three kinds of growth
    grow = np.array([[1, 0, 1, 1, 0, 1, 0],      # 0 -> 1, 63 -> 64, 64 -> 65, 128 -> 129; 1, 65 and 129 stay
                     [0, 2, 0, 65, 64, 0, 3],    # 0 stays empty, 1 -> 3, 64 -> 129, 65 -> 129 (one tile more each), 129 -> 132
                     [0, 0, 0, 0, 0, 0, 0]])     # nothing changes
    add = grow[(np.arange(nlist) // 7) % 3, np.arange(nlist) % 7]
    add[1] += (4 - int(add.sum()) % 4) % 4 + 1   # pend_n % 4 != 0: the scatter's last block has idle waves
    new_sizes = old_sizes + add
    moves = set(zip(old_sizes.tolist(), new_sizes.tolist()))
    assert {(0, 1), (63, 64), (64, 65), (64, 129), (0, 0), (64, 64), (129, 129)} <= moves and add.sum() % 4 != 0
    t_old, t_new = ivfsq_ref.tile0_of(old_sizes), ivfsq_ref.tile0_of(new_sizes)
    assert len(set((t_new - t_old)[:-1].tolist())) > 50  # the tiles move by many different distances
    lists1 = rng.permutation(np.repeat(np.arange(nlist), add))
    codes1 = rng.integers(0, 256, (len(lists1), stride)).astype(np.uint8)
    rterm1 = rng.random(len(lists1))
    old = (want0[0], want0[1], want0[2])
    sizes2, *want1 = ivfsq_ref.rebuilt(old_sizes, old[2], old[0], lists1, codes1, n0, stride, old[1], rterm1)
    assert np.array_equal(sizes2, new_sizes)
    assert_arrays(rebuild(lib, old_sizes, old, lists1, codes1, rterm1, n0, stride), want1, "over 427 old tiles")


# ---------------------------------------------------------------- c. end to end at many lists
@functools.lru_cache(maxsize=1)
def many_lists_case(nlist: int):
    """The rows, queries and probe tables of ``test_many_lists``, shared by the two metrics; read-only."""
    d, nq = 24, 40
    sizes = edge_sizes(nlist)
    n = int(sizes.sum())
    rng = np.random.default_rng(7000 + nlist)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    assign = rng.permutation(np.repeat(np.arange(nlist), sizes))  # every list interleaves ids
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    last = int(np.flatnonzero(sizes)[-1])
    one = rng.integers(0, nlist, (nq, 1))
    one[:5, 0] = [0, 255, 256, nlist - 1, 7]  # lists 0 and 7 are empty
    eight = rng.integers(0, nlist, (nq, 8))
    eight[:, 3] = eight[:, 6]
    eight[np.arange(nq), rng.integers(0, 3, nq)] = np.array([-1, nlist])[rng.integers(0, 2, nq)]
    eight[1] = [-1, nlist, -1, 5, 5, 5, nlist, -1]
    tables = [("one list per query", one, nq), ("8 probes with -1, nlist and duplicates", eight, nq),
              ("every list", np.tile(np.arange(nlist), (17, 1)), 17), ("only the last list with rows", np.full((nq, 1), last), nq)]
    out = (sizes, t, xb, base, xq, assign, cent, tables)
    for a in (sizes, t, xb, base, xq, assign, cent, one, eight):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nlist", [257, 513, 1000])
def test_many_lists(nlist, metric):
    d = 24
    sizes, t, xb, base, xq, assign, cent, tables = many_lists_case(nlist)
    n = len(xb)
    qz, index = new_index(d, SQ.QT_8bit, metric, cent, t)
    force_add(index, xb, assign)
    assert sizes_of(index) == sizes.tolist() and index.ntotal == n
    check_lists(index, assign, base)
    # the last table: at most 3 entries for a grid in the tens or hundreds -- nearly every block finds no entry
    last = int(tables[3][1][0, 0])
    blocks = pass_blocks(ivfsq_ref.tiles_of(sizes), d, index.device)
    assert 1 <= -(-sizes[last] // 64) <= 3 and blocks >= 40, (sizes[last], blocks)
    full = sq_ref.expected(xq, xb, n, metric)  # the complete ranking, computed once
    sqi = sq_index(d, SQ.QT_8bit, metric, t, xb)
    members = [ivf_ref.probed_members(probes, assign, nlist) for _, probes, _ in tables]
    for k in (1, 10, 33, 70):
        for (name, probes, nq), mem in zip(tables, members):  # never the same table twice in a row
            D, I = search_pre(index, xq[:nq], k, probes)
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full[0][:nq], full[1][:nq], mem, k, metric), f"{name} k={k}")
            if name == "every list":
                assert_knn_identical(D, I, *sqi.search(xq[:nq], k), f"IndexScalarQuantizer.search k={k}")


# ---------------------------------------------------------------- d. groups of 8 over two staging chunks
@pytest.mark.parametrize("metric", [L2, IP])
def test_groups_of_eight_over_two_chunks(metric):
    """70 queries at d = 1473: eight groups of 8 in the first staging chunk of 64 -- every group row of the masks, the
    offsets and the work buffer in use -- and one group of 6 in the second."""
    d, nlist, nq = 1473, 257, 70
    assert sq_ref.qt_of(d) == 8
    sizes = np.array([0, 1, 2, 65], np.int64)[np.arange(nlist) % 4]
    n = int(sizes.sum())
    assert n <= 5000
    rng = np.random.default_rng(1473)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s, "binary")
    xq = int_data("binary", rng, nq, d)
    assert_exact_range(xb, xq)
    assign = rng.permutation(np.repeat(np.arange(nlist), sizes))
    qz, index = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    force_add(index, xb, assign)
    assert sizes_of(index) == sizes.tolist()
    check_lists(index, assign, base)
    one = rng.integers(0, nlist, (nq, 1))
    one[[0, 7, 8, 63, 64, 69], 0] = [255, 256, 3, 0, 7, 251]  # the first and last query of a group and of a chunk
    four = rng.integers(-1, nlist + 1, (nq, 4))
    four[:, 2] = four[:, 0]
    full = sq_ref.expected(xq, xb, n, metric)
    members = [ivf_ref.probed_members(p, assign, nlist) for p in (one, four)]
    for k in (10, 40):
        for probes, mem in zip((one, four), members):  # in alternation
            D, I = search_pre(index, xq, k, probes)
            assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(*full, mem, k, metric), f"nprobe={probes.shape[1]} k={k}")


# ---------------------------------------------------------------- e. rebuilds at many lists
@pytest.mark.parametrize("metric", [L2, IP])
def test_rebuilds_at_many_lists(metric):
    """Five adds of 1, 299, 4000, 1 and 9000 rows, a search (and so a rebuild) after each.  List 10 holds 63, 64 and 65
    rows after the third, fourth and fifth, list 20 goes from 64 to 129 in the fifth; the other rows fall on the lists
    unevenly (list 0 takes about a seventh), lists 7 and 299 stay empty."""
    d, nlist, nq = 24, 300, 40
    calls = [1, 299, 4000, 1, 9000]
    n = sum(calls)
    rng = np.random.default_rng(300)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    free = np.setdiff1d(np.arange(nlist), [7, 10, 20, 299])
    assign = free[(rng.random(n) ** 3 * len(free)).astype(np.int64)]
    ends = np.cumsum(calls)
    third, fifth = np.arange(ends[1], ends[2]), np.arange(ends[3], ends[4])
    assign[rng.choice(third, 63 + 64, replace=False)] = np.repeat([10, 20], [63, 64])
    assign[ends[2]] = 10  # the fourth call's one row
    assign[rng.choice(fifth, 1 + 65, replace=False)] = np.repeat([10, 20], [1, 65])
    qz, index = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    have, history = 0, []
    for c in calls:
        force_add(index, xb[have:have + c], assign[have:have + c])
        have += c
        sizes = sizes_of(index)
        assert sizes == np.bincount(assign[:have], minlength=nlist).tolist() and index.ntotal == have
        history.append(sizes)
        probes = rng.integers(0, nlist, (nq, 3))  # a fresh table every time
        probes[:4, 0] = [10, 20, 7, 0]
        full = sq_ref.expected(xq, xb[:have], have, metric)
        for k in (10, 40):
            probes = np.roll(probes, 1, axis=0)
            D, I = search_pre(index, xq, k, probes)
            assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb[:have], probes, assign[:have], nlist, k, metric, full), f"n={have} k={k}")
        check_lists(index, assign[:have], base)
    assert [h[10] for h in history[2:]] == [63, 64, 65] and [h[20] for h in history[3:]] == [64, 129]
    assert [h[7] for h in history] == [0] * 5 and sum(history[0]) == 1 and history[4][0] > 1000
    grew = [sum(-(-b // 64) > -(-a // 64) for a, b in zip(history[i], history[i + 1])) for i in range(4)]
    assert grew[1] > 30 and grew[3] > 10, grew  # many lists gain tiles in one rebuild, each its own number
    index.reset()
    assert index.ntotal == 0 and sizes_of(index) == [0] * nlist
    force_add(index, xb[:500], assign[:500])
    probes = rng.integers(0, nlist, (nq, 3))
    D, I = search_pre(index, xq, 10, probes)
    assert_knn_identical(D, I, *ivfsq_ref.expected(xq, xb[:500], probes, assign[:500], nlist, 10, metric), "after reset")
    check_lists(index, assign[:500], base)


# ---------------------------------------------------------------- f. one handle from two streams
def test_one_handle_from_two_streams():
    """A small search on the default stream, an ``add_torch`` that more than doubles the tiles, a search on a side stream
    with more queries and a larger k, a third search on the default stream: nothing is waited for in between.  The side
    stream's search rebuilds the lists and has to replace the staged queries, the blocks' lists and the work buffer
    while the first search may still be in flight.  (The masks and the offsets are sized by nlist and the chunk alone:
    the first search of a handle allocates them, no later one can outgrow them.)  Every result is the host form's of a
    twin index, bit for bit, and so are the lists."""
    import torch

    d, nlist, n1, n = 24, 300, 100, 20100
    rng = np.random.default_rng(24300)
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, 70, d)
    assert_exact_range(xb, xq)
    cent = xb[rng.choice(n, nlist, replace=False)]
    assert len(np.unique(cent, axis=0)) == nlist
    qz, twin = new_index(d, SQ.QT_8bit, L2, cent, t)
    qz2, index = new_index(d, SQ.QT_8bit, L2, cent, t)
    twin.nprobe = index.nprobe = 3
    twin.add(xb[:n1])
    tiles1 = ivfsq_ref.tiles_of(sizes_of(twin))
    want_first = twin.search(xq[:3], 10)
    twin.add(xb[n1:])
    tiles2 = ivfsq_ref.tiles_of(sizes_of(twin))
    assert tiles2 >= 2 * tiles1 > 0 and pass_blocks(tiles2, d, twin.device) > pass_blocks(tiles1, d, twin.device)
    want = {(70, 33): twin.search(xq, 33), (3, 10): twin.search(xq[:3], 10)}
    dev_ = torch.device("cuda", index.device)
    side = torch.cuda.Stream(device=dev_)
    xb_t, xq_t = torch.from_numpy(xb).to(dev_), torch.from_numpy(xq).to(dev_)
    index.add_torch(xb_t[:n1])
    torch.cuda.synchronize(dev_)
    first = index.search_torch(xq_t[:3], 10)  # rebuilds the first rows' lists
    index.add_torch(xb_t[n1:])
    with torch.cuda.stream(side):
        second = index.search_torch(xq_t, 33)  # rebuilds, two chunks of two k-passes
    third = index.search_torch(xq_t[:3], 10)
    torch.cuda.synchronize(dev_)
    for name, got, ref in (("first", first, want_first), ("side stream", second, want[(70, 33)]), ("third", third, want[(3, 10)])):
        assert_knn_identical(got[0].cpu().numpy(), got[1].cpu().numpy(), *ref, name)
    probes = qz.search(xq, 3)[1]
    for (nq, k), ref in want.items():
        D, I = counted(index, probes[:nq], k, lambda: index.search(xq[:nq], k))
        assert_knn_identical(D, I, *ref, f"the index's host form nq={nq} k={k}")
    assert index.ntotal == twin.ntotal == n and sizes_of(index) == sizes_of(twin)
    assign = qz.search(xb, 1)[1].reshape(-1)
    check_lists(twin, assign, base)
    for l in range(nlist):
        (ids, rows), (ids2, rows2) = twin.get_list(l), index.get_list(l)
        assert np.array_equal(ids, ids2) and np.array_equal(rows, rows2)
