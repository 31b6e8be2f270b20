"""GPU tests of IndexBinaryIVF's pass and rebuild, called directly and across chunks (csrc/ise_binary_ivf.hpp:
binary_ivf_scan_kernel; csrc/ise_ivf_tiles.hpp: ivf_move_tiles_kernel<64, u64>, ivf_scatter_rows_kernel<u64>;
csrc/ise_binary_ivf.hip: search_enqueue).  tests/test_binary_ivf_gpu.py reaches the kernels through the Python class only: at most 50 queries (one
chunk of 64), rows of at most 1024 bits, at most two work-list entries per wave below 2^19 rows, ids that are small.

Tests a to e call the kernels through tests/native/binary_ivf_harness.hip, whose launches are the product's own
(binary_ivf_scan_launch, pass_merge_launch<int>, ivf_rebuild_launch), on crafted work lists, floors and tables,
and compare every word they write with tests/binary_ivf_ref.py: each block's lists place for place (block b takes the
entries e with (e // 4) % grid == b), then D, I and the floors.  No input can fault a kernel that is wrong: every tile
number in the work buffer -- behind ``count`` too -- names a tile that exists, ids and codes cover whole tiles, and the
entries behind ``count`` are visible poison (a full tile, mask 0xFFFF, holding a row equal to every query).  Every
output holds the pattern 0xA5A5A5A5 on entry; the words a launch must not write are checked to hold it still.

Tests f to j go through the index: several chunks and batches, the longest rows, many lists, workspaces that grow.  The
work buffer is never cleared between searches, so no test repeats a probe table in consecutive calls.  Everything is
integer: every comparison is exact.

The harness is built by `make -C image-search-engine_amd/csrc` (target libise_binary_ivf_check.so); without it the
tests fail, they do not skip."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

from image_search_engine_amd import _native as native
from tests import binary_ivf_ref as ref
from tests import binary_ref
from tests.test_binary_ivf_gpu import SIZES, assert_ordered, assert_same, check_lists, counted, flat_index, new_index, search_pre, sizes_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "image-search-engine_amd", "csrc", "libise_binary_ivf_check.so")
EDGE_SIZES = (0, 1, 63, 64, 65, 128, 129)  # list l has EDGE_SIZES[l % 7] rows before a rebuild
SENT = 0xA5A5A5A5                           # every 32-bit word of an output before a launch
SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
KEY_PAD = ref.KEY_PAD
MERGE_LISTS_MAX = 1024                      # csrc/ise_merge.hpp: the most blocks a pass may have
WORK_LEN = 2 * 4 * 64                       # entries of a crafted work buffer: twice what the largest grid here deals in a round
TILES0 = 1000                               # what the tiles-loaded counter holds before a launch

_vp, _int, _ll, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint32
PROTOTYPES = {
    "chk_binary_ivf_pass": [_vp, _vp, _int, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _int, _int],
    "chk_binary_ivf_rebuild": [_vp, _vp, _vp, _ll, _vp, _ll, _vp, _u32, _int, _int, _vp, _ll, _vp, _vp],
}


@pytest.fixture(scope="module")
def lib():
    import torch  # first: the harness binds to the HIP runtime torch has loaded

    assert torch.cuda.is_available()
    if not os.path.exists(LIB_PATH):
        pytest.fail("csrc/libise_binary_ivf_check.so is missing: build it with "
                    "`make -C image-search-engine_amd/csrc libise_binary_ivf_check.so`")
    handle = ctypes.CDLL(LIB_PATH)
    for name, args in PROTOTYPES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _int, args
    return handle


def dev(a):
    """numpy -> a CUDA tensor of the same bits (uint32 as int32, uint64 as int64)"""
    import torch

    a = np.array(a, order="C")  # a copy: the shared inputs are read-only
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def dev_filled(*shape):
    """a CUDA int32 tensor with every word the pattern SENT"""
    import torch

    return torch.full(shape, int(np.array(SENT, np.uint32).view(np.int32)), dtype=torch.int32, device="cuda")


def host_u32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def host_u64(t) -> np.ndarray:
    """an int32 tensor [..., 2] -> uint64 [...]"""
    return t.cpu().numpy().view(np.uint64).reshape(t.shape[:-1])


def run(fn, *args):
    """launch on the null stream (torch's default stream), wait, and take any error the kernels left"""
    import torch

    rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    assert rc == 0, f"launch failed: hip error {rc}"
    torch.cuda.synchronize()


def words_of(codes: np.ndarray, ws: int) -> np.ndarray:
    """uint8 [rows][ws * 8] -> the rows as the device holds them, uint64 [rows][ws] (little-endian words)"""
    assert codes.dtype == np.uint8 and codes.shape[1] == ws * 8
    return np.ascontiguousarray(codes).view("<u8").reshape(len(codes), ws)


# ---------------------------------------------------------------- the crafted lists of tests a, c and d
LIVE, POISON = 37, 3  # tiles the entries may name | full tiles that only the stale entries behind `count` name
PLANT_TILE, PLANT_ROW, PLANT_Q, NEAR_Q = 7, 5, 3, 1  # test d: the row equal to query 3, one bit from query 1


@functools.lru_cache(maxsize=None)
def world(ws: int):
    """40 tiles of rows of ``ws`` words.  The live tiles hold 1, 63 or 64 rows; the slots behind them are zero codes with
    id 0xFFFFFFFF, and query 0 is the zero code: an unmasked pad slot would win at distance 0.  The ids are a permutation
    unrelated to the slots, half of them in [2^31, 2^32 - 2].  The poison tiles hold a row equal to every query.
    Read-only."""
    rng = np.random.default_rng(9000 + ws)
    cs, tiles = ws * 8, LIVE + POISON
    slots = tiles * ref.TILE
    valid = np.concatenate([rng.permutation(np.resize([1, 63, 64], LIVE)), np.full(POISON, 64)])
    valid[PLANT_TILE] = 64
    codes = rng.integers(0, 256, (slots, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (ref.QT, cs), dtype=np.uint8)
    xq[0] = 0
    xq[NEAR_Q] = xq[PLANT_Q]
    xq[NEAR_Q, 0] ^= 1
    codes[PLANT_TILE * 64 + PLANT_ROW] = xq[PLANT_Q]
    small = rng.choice(1 << 20, slots // 2, replace=False)
    large = 2 ** 31 + 1 + rng.choice(2 ** 31 - 4, slots - len(small) - 2, replace=False)
    ids = rng.permutation(np.concatenate([small, large, [2 ** 31, 2 ** 32 - 2]])).astype(np.uint32)
    assert len(np.unique(ids)) == slots and (ids >= 2 ** 31).sum() > slots // 3 and ids.max() == 2 ** 32 - 2
    for t in range(tiles):
        codes[t * 64 + valid[t]:(t + 1) * 64] = 0
        ids[t * 64 + valid[t]:(t + 1) * 64] = ref.PAD_ID
    for i, t in enumerate(range(LIVE, tiles)):  # a row equal to every query in each poison tile, at other rows each time
        codes[t * 64 + 16 * i:t * 64 + 16 * i + 16] = xq
    keys = ref.tile_keys(codes, ids, xq)
    # visible poison: in every poison tile the row equal to query q is nearer to q than every valid live row but the planted
    # one; a pad slot is nearer to the zero query than every valid row
    dist = (keys >> np.uint64(32)).astype(np.int64) - 1
    live_min = np.array([min(dist[t, q, :valid[t]].min() for t in range(LIVE) if t != PLANT_TILE) for q in range(ref.QT)])
    assert (live_min > 0).all() and (dist[LIVE:].min(axis=2) == 0).all() and dist[PLANT_TILE, PLANT_Q, PLANT_ROW] == 0
    assert (dist[:LIVE, 0][np.arange(64)[None, :] >= valid[:LIVE, None]] == 0).all()
    w = types.SimpleNamespace(ws=ws, tiles=tiles, valid=valid, codes=words_of(codes, ws), ids=ids, qpad=words_of(xq, ws), keys=keys,
                              poison=np.array([[t, 64, 0xFFFF, 0] for t in range(LIVE, tiles)], np.uint32))
    for a in (w.valid, w.codes, w.ids, w.qpad, w.keys, w.poison):
        a.setflags(write=False)
    return w


def launch_pass(lib, w, entries, count, grid, nqt, kp, lo=None, k=None, off=0):
    """One pass over entries[:count] -> (lists uint64 [grid + 1][16][32], D uint32 [16][k], I uint64 [16][k], lo_out uint64
    [16], tiles loaded).  The work buffer holds WORK_LEN entries: the poison tiles' behind ``count``."""
    k = kp + 5 if k is None else k
    entries = np.asarray(entries, np.uint32).reshape(-1, 4)
    work = np.concatenate([entries[:count], np.resize(w.poison, (WORK_LEN - count, 4))])
    # what the kernels trust: every entry of the buffer names a tile that exists and at most 64 rows of it, the arrays
    # cover whole tiles, the scalars are in range
    assert work.shape == (WORK_LEN, 4) and 0 <= count <= len(entries) and WORK_LEN >= 4 * 64 + count
    assert (work[:, 0] < w.tiles).all() and (work[:, 1] <= 64).all() and (work[count:, 2] == 0xFFFF).all()
    assert w.codes.shape == (w.tiles * 64, w.ws) and w.ids.shape == (w.tiles * 64,) and w.qpad.shape == (16, w.ws)
    assert 1 <= grid <= 64 and 1 <= nqt <= 16 and 1 <= kp <= 32 and 0 <= off <= k - kp
    assert lo is None or (lo.dtype == np.uint64 and lo.shape == (nqt,))
    lists, D, I, lo_out = dev_filled(grid + 1, 16, 32, 2), dev_filled(16, k), dev_filled(16, k, 2), dev_filled(16, 2)
    loaded = dev(np.array([TILES0], np.int64))
    run(lib.chk_binary_ivf_pass, dev(w.codes), dev(w.ids), w.ws, dev(w.qpad), nqt, kp, None if lo is None else dev(lo), lists, dev(work),
        dev(np.array([count], np.uint32)), loaded, grid, D, I, lo_out, k, off)
    return host_u64(lists), host_u32(D), host_u64(I), host_u64(lo_out), int(loaded.cpu().numpy()[0])


def differences(got, want_lists, empty, want, count, grid, nqt, kp, off, what):
    """The words of one launch that differ from the reference: [] when all is well."""
    lists, D, I, lo_out, loaded = got
    want_D, want_I, want_lo = want
    out = []
    for b in range(grid):
        places = 32 if empty[b] else kp  # behind place kp a block with an entry may leave anything
        if not np.array_equal(lists[b, :nqt, :places], want_lists[b, :nqt, :places]):
            q, i = np.argwhere(lists[b, :nqt, :places] != want_lists[b, :nqt, :places])[0]
            out.append(f"{what}: lists[{b}][{q}][{i}] = {int(lists[b, q, i]):#x}, want {int(want_lists[b, q, i]):#x}")
    if not (lists[:grid, nqt:] == SENT64).all():
        out.append(f"{what}: the lists of a query at or above nqt = {nqt} were written")
    if not (lists[grid] == SENT64).all():
        out.append(f"{what}: the guard block behind lists[{grid}] was written")
    k = D.shape[1]
    if not np.array_equal(D[:nqt, off:off + kp].view(np.int32), want_D) or not np.array_equal(I[:nqt, off:off + kp].view(np.int64), want_I):
        q = np.flatnonzero((D[:nqt, off:off + kp].view(np.int32) != want_D).any(1) | (I[:nqt, off:off + kp].view(np.int64) != want_I).any(1))[0]
        out.append(f"{what}: query {q}: D {D[q, off:off + kp].view(np.int32)[:6]} I {I[q, off:off + kp].view(np.int64)[:6]}, "
                   f"want D {want_D[q][:6]} I {want_I[q][:6]}")
    outside = np.ones((16, k), bool)
    outside[:nqt, off:off + kp] = False
    if not (D[outside] == SENT).all() or not (I[outside] == SENT64).all():
        out.append(f"{what}: D or I was written outside [{off}, {off + kp}) of the first {nqt} queries")
    if not np.array_equal(lo_out[:nqt], want_lo) or not (lo_out[nqt:] == SENT64).all():
        out.append(f"{what}: lo_out {[hex(int(v)) for v in lo_out[:nqt + 1]]}, want {[hex(int(v)) for v in want_lo]}")
    if loaded != TILES0 + count:
        out.append(f"{what}: the tiles loaded grew by {loaded - TILES0}, want {count}")
    return out


def check_pass(lib, w, entries, koe, count, grid, nqt, kp, lo=None, off=0, what="", full=None):
    """Launch and compare.  ``full``: the blocks' lists at nqt = 16, kp = 32 and no floor, if the caller keeps them -- a
    block's list at a smaller kp is its first kp places, at a smaller nqt its first queries."""
    got = launch_pass(lib, w, entries, count, grid, nqt, kp, lo, off=off)
    if full is None or lo is not None:
        full = ref.block_lists_of(koe, entries, count, grid, nqt, kp, lo)
    want_lists, empty = full
    want_lists = np.where(np.arange(32)[None, None, :] < kp, want_lists[:, :nqt], KEY_PAD)
    want = ref.results_of(ref.merged_of(want_lists, kp))
    what = f"{what} count={count} grid={grid} nqt={nqt} kp={kp}"
    return got, differences(got, want_lists, empty, want, count, grid, nqt, kp, off, what)


def random_masks(rng, n):
    """uint32 [n]: random 16-bit query masks, never 0, every fifth a single bit"""
    m = rng.integers(1, 1 << 16, n).astype(np.uint32)
    m[::5] = np.uint32(1) << rng.integers(0, 16, len(m[::5])).astype(np.uint32)
    return m


# ---------------------------------------------------------------- a. partition and padding
REDUCED = [(0, 1, 16, 32), (1, 2, 1, 1), (3, 1, 5, 7), (4, 2, 16, 32), (5, 3, 5, 7), ("all", "ceil", 16, 32), ("all", "ceil+1", 1, 32),
           ("all", 64, 16, 1), ("all", 3, 16, 7), (5, 64, 16, 32)]


@pytest.mark.parametrize("ws", [1, 2, 4, 6, 10, 18, 66, 128])
def test_partition_and_padding(lib, ws):
    """WT = 1 (ws 1), 2 (ws 2) and 0; hamming16<0> runs 2, 3, 5, 9, 33 and 64 chunks of 16 bytes -- 3, 5 and 9 are no
    multiple of its unroll of 4, 64 is the longest row.  The entries are a shuffled subset of the live tiles, not in
    slot order.  ws 1, 2 and 6 run the full cross of count x grid x nqt x kp, the others ten cases."""
    w = world(ws)
    rng = np.random.default_rng(ws)
    tiles = rng.permutation(LIVE)[:33]
    entries = np.stack([tiles, w.valid[tiles], random_masks(rng, 33), np.zeros(33, np.int64)], axis=1).astype(np.uint32)
    assert (np.diff(tiles) < 0).any() and {1, 63, 64} <= set(entries[:, 1].tolist())
    koe = w.keys[entries[:, 0]]
    everything = len(entries)
    if ws in (1, 2, 6):
        cases = []
        for count in (0, 1, 3, 4, 5, everything):
            ceil = -(-count // 4)
            for grid in sorted({1, 2, 3, max(1, ceil), ceil + 1, 64}):
                cases += [(count, grid, nqt, kp) for nqt in (1, 5, 16) for kp in (1, 7, 32)]
    else:
        ceil = -(-everything // 4)
        named = {"all": everything, "ceil": ceil, "ceil+1": ceil + 1}
        cases = [(named.get(c, c), named.get(g, g), nqt, kp) for c, g, nqt, kp in REDUCED]
    full = {}
    failures = []
    for count, grid, nqt, kp in cases:
        if (count, grid) not in full:
            full[count, grid] = ref.block_lists_of(koe, entries, count, grid, 16, 32)
        got, bad = check_pass(lib, w, entries, koe, count, grid, nqt, kp, off=3, what=f"ws={ws}", full=full[count, grid])
        failures += bad
        if count == 0:  # nothing to rank: padding everywhere, no tile counted
            assert (got[1][:nqt, 3:3 + kp].view(np.int32) == binary_ref.INT32_MAX).all() and (got[3][:nqt] == KEY_PAD).all()
    assert not failures, f"{len(failures)} differences; the first: " + " | ".join(failures[:5])
    # the merged result of the whole list is the numpy ranking of the admitted rows, whatever the reference's blocks say
    D, I, _ = ref.pass_of(koe, entries, everything, 16, 32)
    got = launch_pass(lib, w, entries, everything, 5, 16, 32)
    assert np.array_equal(got[1][:, :32].view(np.int32), D) and np.array_equal(got[2][:, :32].view(np.int64), I)
    assert (I >= 2 ** 31).any() and (I < 2 ** 32 - 1).all() and (I[0] >= 0).all() and (D[0] > 0).all()  # no pad slot for the zero query


def test_harness_refuses_what_is_out_of_range(lib):
    bad = 1  # hipErrorInvalidValue: nothing is launched, no pointer is read
    for ws, nqt, kp, grid, k, off in ((0, 1, 1, 1, 1, 0), (3, 1, 1, 1, 1, 0), (130, 1, 1, 1, 1, 0), (2, 0, 1, 1, 1, 0), (2, 17, 1, 1, 17, 0),
                                      (2, 1, 0, 1, 1, 0), (2, 1, 33, 1, 40, 0), (2, 1, 1, 0, 1, 0), (2, 1, 1, MERGE_LISTS_MAX + 1, 1, 0),
                                      (2, 1, 4, 1, 3, 0), (2, 1, 4, 1, 6, 3), (2, 1, 1, 1, 1, -1)):
        assert lib.chk_binary_ivf_pass(None, None, ws, None, nqt, kp, None, None, None, None, None, grid, None, None, None, k, off) == bad
    for old_tiles, pend_n, ws, nlist, new_tiles in ((-1, 1, 2, 1, 1), (0, 0, 2, 1, 1), (0, 1, 3, 1, 1), (0, 1, 130, 1, 1), (0, 1, 2, 0, 1),
                                                    (0, 1, 2, 1, 0), (2, 1, 2, 1, 1), (0, 1, 2, 1, 1 << 26)):
        assert lib.chk_binary_ivf_rebuild(None, None, None, old_tiles, None, pend_n, None, 0, ws, nlist, None, new_tiles, None, None) == bad


# ---------------------------------------------------------------- b. repeated cuts at small size
@functools.lru_cache(maxsize=None)
def cut_world(ws: int):
    """24 full tiles in slot order, wave w of the one block takes tiles w, w + 4, .. w + 20.  Against query 0 the j-th
    tile of a wave holds distances in (bits - (j + 1) bw, bits - j bw], bw = bits / 6: wholly below the tile before.
    Query 1 is query 0's complement: the same tiles in ascending order.  A tile has 64 rows at no more than bw distances
    (the ten just below the band's upper end): equal distances everywhere, and the ids DESCEND in slot order across 2^31."""
    rng = np.random.default_rng(7000 + ws)
    cs, bits, live = ws * 8, ws * 64, 24
    bw = bits // 6
    tiles, slots = live + 1, (live + 1) * 64
    xq = rng.integers(0, 256, (ref.QT, cs), dtype=np.uint8)
    xq[1] = ~xq[0]
    flips = np.zeros((slots, bits), np.uint8)
    for s in range(live * 64):
        j = (s // 64) // 4
        flips[s, rng.choice(bits, int(rng.integers(bits - j * bw - 9, bits - j * bw + 1)), replace=False)] = 1
    codes = np.packbits(flips, axis=1, bitorder="little") ^ xq[0]
    codes[live * 64:live * 64 + 16] = xq  # the poison tile
    ids = (2 ** 31 + 700 - np.arange(slots)).astype(np.uint32)
    keys = ref.tile_keys(codes, ids, xq)
    w = types.SimpleNamespace(ws=ws, tiles=tiles, valid=np.full(tiles, 64), codes=words_of(codes, ws), ids=ids, qpad=words_of(xq, ws),
                              keys=keys, poison=np.array([[live, 64, 0xFFFF, 0]], np.uint32))
    for a in (w.codes, w.ids, w.qpad, w.keys, w.poison):
        a.setflags(write=False)
    return w


@pytest.mark.parametrize("kp", [1, 20, 32])
@pytest.mark.parametrize("ws", [1, 2, 4])
def test_cuts_repeat_at_small_size(lib, ws, kp):
    w = cut_world(ws)
    kmax = min(kp + kp // 2 + 4, 48)
    assert kmax == {1: 5, 20: 34, 32: 48}[kp]  # a cut keeps between kp and kmax keys; 48 is BIN_CUT_MAX
    dist = (w.keys[:24] >> np.uint64(32)).astype(np.int64) - 1  # [tile][query][row]
    for e in range(4, 24):  # every tile after a wave's first lies wholly below the one before: it fills the buffer past
        assert dist[e, 0].max() < dist[e - 4, 0].min()  # BIN_CAP - 64 keys and forces a cut
        assert dist[e, 1].min() > dist[e - 4, 1].max()  # ascending: nothing after the first cut's threshold
    assert all(len(np.unique(dist[e, 0])) <= 10 for e in range(24))  # 64 rows at ten distances
    assert (np.diff(w.ids.astype(np.int64)) == -1).all() and w.ids[0] > 2 ** 31 > w.ids[24 * 64 - 1]
    entries = np.stack([np.arange(24), np.full(24, 64), np.full(24, 0xFFFF), np.zeros(24, np.int64)], axis=1).astype(np.uint32)
    koe = w.keys[:24]
    got, bad = check_pass(lib, w, entries, koe, 24, 1, 16, kp, what=f"ws={ws}")
    assert not bad, " | ".join(bad[:5])
    # query 0's results are the last tiles' rows: the keys every wave met last
    assert (np.isin(got[2][0, :kp].view(np.int64), w.ids[20 * 64:24 * 64].astype(np.int64))).all()


# ---------------------------------------------------------------- c. floors
@pytest.mark.parametrize("kp,grid", [(7, 1), (7, 3), (32, 3)])
@pytest.mark.parametrize("ws", [1, 2, 10])
def test_floors(lib, ws, kp, grid):
    """lo_in per query: 0 | a key that exists (admitted) | that key + 1 (not admitted) | bin_key(dist, 0), a distance
    boundary | KEY_PAD, a finished query | behind the last key | three keys from the end | 0."""
    w = world(ws)
    rng = np.random.default_rng(100 + ws)
    tiles = rng.permutation(LIVE)
    entries = np.stack([tiles, w.valid[tiles], random_masks(rng, LIVE) | np.uint32(0xFF), np.zeros(LIVE, np.int64)], axis=1).astype(np.uint32)
    koe, count, nqt = w.keys[entries[:, 0]], LIVE, 8
    adm = [ref.admitted_of(koe, entries, range(count), q, 0) for q in range(nqt)]  # every admitted key, sorted
    assert all(len(a) > 100 for a in adm)
    boundary = (adm[3][40] >> np.uint64(32)) << np.uint64(32)  # bin_key(distance of the 41st, 0)
    lo = np.array([0, adm[1][2], adm[2][2] + np.uint64(1), boundary, KEY_PAD, adm[5][-1] + np.uint64(1), adm[6][-3], 0], np.uint64)
    got, bad = check_pass(lib, w, entries, koe, count, grid, nqt, kp, lo=lo, what=f"ws={ws} floors")
    assert not bad, " | ".join(bad[:5])
    # what the reference says about these floors, spelt out
    D, I, lo_out = ref.pass_of(koe, entries, count, nqt, kp, lo)
    first = ref.bin_key(D[:, 0], I[:, 0].astype(np.uint64))
    assert first[0] == adm[0][0] and first[1] == adm[1][2] and first[2] == adm[2][3]
    assert first[3] == adm[3][np.searchsorted(adm[3], boundary)] and first[3] >= boundary and D[3, 0] == int(boundary >> np.uint64(32)) - 1
    assert (adm[3] < boundary).any()  # the boundary cuts keys off
    assert (I[4] == -1).all() and lo_out[4] == KEY_PAD and (I[5] == -1).all() and lo_out[5] == KEY_PAD
    assert (I[6, :3] >= 0).all() and (I[6, 3:] == -1).all() and (lo_out[6] == KEY_PAD) == (kp > 3)
    assert (I[[0, 1, 2, 3, 7]] >= 0).all() and (lo_out[[0, 1, 2, 3, 7]] != KEY_PAD).all()


# ---------------------------------------------------------------- d. masks
@pytest.mark.parametrize("ws", [1, 2, 10])
def test_masks(lib, ws):
    """The row equal to query 3 sits in an entry whose bit 3 is clear and whose bit 1 is set: it is not among query 3's
    results, where it would be the first, and it is query 1's first.  Mask bits at or above nqt change nothing."""
    w = world(ws)
    rng = np.random.default_rng(200 + ws)
    tiles = rng.permutation(LIVE)
    masks = random_masks(rng, LIVE)
    at = int(np.flatnonzero(tiles == PLANT_TILE)[0])
    masks[at] = (masks[at] | np.uint32(1 << NEAR_Q)) & ~np.uint32(1 << PLANT_Q)
    entries = np.stack([tiles, w.valid[tiles], masks, np.zeros(LIVE, np.int64)], axis=1).astype(np.uint32)
    koe, count = w.keys[entries[:, 0]], LIVE
    planted = int(w.ids[PLANT_TILE * 64 + PLANT_ROW])
    # the masked row would otherwise be the nearest: with the bit set the reference puts it first, at distance 0
    with_bit = entries.copy()
    with_bit[at, 2] |= 1 << PLANT_Q
    D, I, _ = ref.pass_of(w.keys[with_bit[:, 0]], with_bit, count, 16, 7)
    assert I[PLANT_Q, 0] == planted and D[PLANT_Q, 0] == 0 and D[PLANT_Q, 1] > 0
    D, I, _ = ref.pass_of(koe, entries, count, 16, 7)
    assert planted not in I[PLANT_Q].tolist() and D[PLANT_Q, 0] > 0 and I[NEAR_Q, 0] == planted and D[NEAR_Q, 0] == 1
    for kp, grid in ((7, 1), (32, 4)):
        got, bad = check_pass(lib, w, entries, koe, count, grid, 16, kp, what=f"ws={ws} masks")
        assert not bad, " | ".join(bad[:5])
        assert planted not in got[2][PLANT_Q, :kp].tolist() and got[2][NEAR_Q, 0] == planted and got[1][NEAR_Q, 0] == 1
    # nqt = 5: the bits of queries 5 .. 15 and the bits 16 .. 31 are never looked at
    noisy = entries.copy()
    noisy[:, 2] = (entries[:, 2] & 0x1F) | (rng.integers(0, 1 << 27, LIVE).astype(np.uint32) << np.uint32(5))
    quiet = entries.copy()
    quiet[:, 2] &= 0x1F
    assert (noisy[:, 2] >> 16).any() and ((noisy[:, 2] >> 5) & 0x7FF).any() and (quiet[:, 2] == 0).any()
    a, bad_a = check_pass(lib, w, noisy, koe, count, 3, 5, 7, what=f"ws={ws} bits above nqt")
    b, bad_b = check_pass(lib, w, quiet, koe, count, 3, 5, 7, what=f"ws={ws} no bits above nqt")
    assert not bad_a + bad_b, " | ".join((bad_a + bad_b)[:5])
    assert all(np.array_equal(x[:, :5, :7] if x.ndim == 3 else x, y[:, :5, :7] if y.ndim == 3 else y) for x, y in zip(a[:4], b[:4]))


# ---------------------------------------------------------------- e. the rebuild kernels, direct
def edge_sizes(nlist: int) -> np.ndarray:
    return np.array(EDGE_SIZES, np.int64)[np.arange(nlist) % 7]


def rebuild(lib, old_sizes, old_codes, old_ids, pend_lists, pend_codes, id0, ws):
    """-> (codes uint8 [slots][ws * 8], ids uint32 [slots]) of the new arrays as ivf_rebuild_launch leaves them.
    The slot numbers come from the reference's plan; the new arrays hold SENT words on entry."""
    nlist, cs = len(old_sizes), ws * 8
    old_tiles = ref.tiles_of(old_sizes)
    new_sizes = old_sizes + np.bincount(pend_lists, minlength=nlist)
    new_tiles = ref.tiles_of(new_sizes)
    dest = ref.rebuild_dest(old_sizes, pend_lists)
    meta, nmeta = ref.meta_of(old_sizes), ref.meta_of(new_sizes)
    m = len(pend_lists)
    # every array is as large as the tables say, every slot lies in the new arrays, and no two rows share one
    assert m >= 1 and new_tiles >= 1 and 0 <= id0 and id0 + m <= 2 ** 32 - 1
    assert old_codes.shape == (old_tiles * 64, cs) and old_codes.dtype == np.uint8 and old_ids.shape == (old_tiles * 64,)
    assert old_ids.dtype == np.uint32 and pend_codes.shape == (m, cs) and pend_codes.dtype == np.uint8
    assert len(meta) == 2 * nlist + 1 + old_tiles and len(nmeta) == 2 * nlist + 1 + new_tiles
    assert (meta[2 * nlist + 1:] < nlist).all() and meta[nlist] == old_tiles and nmeta[nlist] == new_tiles
    assert (np.diff(nmeta[:nlist + 1].astype(np.int64)) >= np.diff(meta[:nlist + 1].astype(np.int64))).all()  # no list shrinks
    assert dest.shape == (m,) and dest.max() < new_tiles * 64 and len(np.unique(dest)) == m
    nx, nids = dev_filled(new_tiles * 64, ws * 2), dev_filled(new_tiles * 64)
    # (without an old tile the old arrays are one unused word each: the move kernel is not launched)
    run(lib.chk_binary_ivf_rebuild, dev(words_of(old_codes, ws) if old_tiles else np.zeros((1, ws), np.uint64)),
        dev(old_ids if old_tiles else np.zeros(1, np.uint32)), dev(meta), old_tiles, dev(words_of(pend_codes, ws)), m, dev(dest), id0, ws,
        nlist, dev(nmeta), new_tiles, nx, nids)
    return nx.cpu().numpy().view(np.uint8).reshape(-1, cs), host_u32(nids), dest


def assert_arrays(got, want, what):
    for name, a, b in zip(("codes", "ids"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        if not np.array_equal(a, b):
            slot = np.argwhere(a != b)[0][0]
            raise AssertionError(f"{what}: the {name} differ in {int((a != b).sum())} places, first at slot {slot} "
                                 f"(tile {slot // 64}, row {slot % 64})")


def kinds_of(old_sizes, new_sizes) -> set:
    """What happens to the lists of a rebuild, as the names the test asks for."""
    t_old, t_new = ref.tile0_of(old_sizes), ref.tile0_of(new_sizes)
    out = set()
    for l, (a, b) in enumerate(zip(old_sizes.tolist(), new_sizes.tolist())):
        same_tiles = -(-a // 64) == -(-b // 64)
        if a == 0 < b:
            out.add("empty to non-empty")
        elif b > a and same_tiles:
            out.add("fills to exactly 64" if b % 64 == 0 else "grows inside its last tile")
        elif b > a:
            out.add("crosses a tile edge")
        elif a > 0:
            out.add("untouched, moves" if t_new[l] != t_old[l] else "untouched, stays")
    return out


# per seven lists (0, 1, 63, 64, 65, 128, 129 rows): two kinds of growth and none
GROW = np.array([[0, 2, 1, 0, 64, 0, 3],     # 1 -> 3, 63 -> 64, 64 stays in place, 65 -> 129 (a tile more), 128 moves, 129 -> 132
                 [1, 0, 0, 1, 0, 65, 0],     # 0 -> 1, 64 -> 65, 128 -> 193; 1, 63, 65 and 129 move
                 [0, 0, 0, 0, 0, 0, 0]])


@pytest.mark.parametrize("nlist", [7, 300])
@pytest.mark.parametrize("ws", [1, 2, 4, 66, 128])  # a row is fewer words than a wave has lanes | two rounds of the scatter's loop
def test_rebuild_kernels(lib, ws, nlist):
    cs = ws * 8
    rng = np.random.default_rng([ws, nlist])
    none = np.zeros((0, cs), np.uint8), np.zeros(0, np.uint32)
    zero = np.zeros(nlist, np.int64)
    # a first build, no old tile at all: the move kernel is not launched, meta is not read.  The ids interleave in every list
    old_sizes = edge_sizes(nlist)
    n0 = int(old_sizes.sum())
    lists0 = rng.permutation(np.repeat(np.arange(nlist), old_sizes))
    codes0 = rng.integers(0, 256, (n0, cs), dtype=np.uint8)
    sizes1, want_codes, _, want_ids = ref.rebuilt(zero, none[1], none[0], lists0, codes0, 0, cs, np.zeros(0), np.zeros(n0))
    assert np.array_equal(sizes1, old_sizes) and n0 % 4 != 0  # the scatter's last block has idle waves
    got_codes, got_ids, dest = rebuild(lib, zero, none[0], none[1], lists0, codes0, 0, ws)
    assert (dest % 2 == 1).any()  # odd slots: at ws = 1 a row is half a 16-byte unit
    assert_arrays((got_codes, got_ids), (want_codes, want_ids), "no old tiles")
    assert ((got_ids == ref.PAD_ID) == np.concatenate([np.arange(64) >= min(64, s - 64 * t) for s in old_sizes for t in range(-(-s // 64))])).all()
    old = want_codes, want_ids
    # over those arrays; at nlist = 7 one rebuild per kind of growth, at 300 the kinds alternate every seven lists
    seen = set()
    kinds = [np.full(nlist, 0), np.full(nlist, 1)] if nlist == 7 else [(np.arange(nlist) // 7) % 3]
    rounds = [GROW[kind, np.arange(nlist) % 7] for kind in kinds]
    for r, add in enumerate(rounds):
        add = add.copy()
        add[6] += (4 - int(add.sum()) % 4) % 4 + 1   # pend_n % 4 != 0
        new_sizes = old_sizes + add
        seen |= kinds_of(old_sizes, new_sizes)
        lists1 = rng.permutation(np.repeat(np.arange(nlist), add))
        codes1 = rng.integers(0, 256, (len(lists1), cs), dtype=np.uint8)
        id0 = 2 ** 32 - 1 - len(lists1) if r == 0 else n0  # the last pending row has id 2^32 - 2, one below the pad id
        no_terms = np.zeros(len(old[1])), np.zeros(len(lists1))  # a code row carries no row term
        sizes2, want_codes, _, want_ids = ref.rebuilt(old_sizes, old[1], old[0], lists1, codes1, id0, cs, *no_terms)
        assert np.array_equal(sizes2, new_sizes) and len(lists1) % 4 != 0 and want_ids[want_ids != ref.PAD_ID].max() == id0 + len(lists1) - 1
        got_codes, got_ids, dest = rebuild(lib, old_sizes, old[0], old[1], lists1, codes1, id0, ws)
        assert (dest % 2 == 1).any() and (dest % 2 == 0).any()
        assert_arrays((got_codes, got_ids), (want_codes, want_ids), f"over {ref.tiles_of(old_sizes)} old tiles, round {r}")
        assert (got_codes[got_ids == ref.PAD_ID] == 0).all()
    assert seen == {"empty to non-empty", "fills to exactly 64", "grows inside its last tile", "crosses a tile edge", "untouched, moves",
                    "untouched, stays"}, seen
    if nlist == 300:
        t_old, t_new = ref.tile0_of(old_sizes), ref.tile0_of(new_sizes)
        assert len(set((t_new - t_old)[:-1].tolist())) > 50  # the tiles move by many different distances


# ---------------------------------------------------------------- f. chunks
@functools.lru_cache(maxsize=None)
def sized_index(d: int):
    """tests/test_binary_ivf_gpu.py's ``sized`` lists at d bits, with 200 queries: lists of 0, 1, 63, 64, 65, 128 and
    129 rows, every row its list's centroid with at most two bits flipped, added in shuffled order."""
    nlist, cs = len(SIZES), d // 8
    rng = np.random.default_rng(300 + d)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    want = rng.permutation(np.repeat(np.arange(nlist), SIZES))
    xb = ref.near_centroids(rng, C, want)
    assert np.array_equal(ref.assign(C, xb), want)
    index = new_index(C)
    index.add(xb)
    assert sizes_of(index) == list(SIZES)
    xq = rng.integers(0, 256, (200, cs), dtype=np.uint8)
    xq[:7] = C
    xq[7:60] = xb[rng.integers(0, len(xb), 53)]
    dist = binary_ref.distances(xb, xq)
    for a in (C, xb, want, xq, dist):
        a.setflags(write=False)
    return index, C, xb, want, xq, dist


CHUNK_POOLS = ([6, 5, 4], [3, 2], [1], [0])  # the lists a chunk's queries name: 7, 2, 1 and 0 tiles


def chunk_table(rng, nq: int) -> np.ndarray:
    """int64 [nq][3], every row different from the one before: chunk c (64 queries) names the lists of CHUNK_POOLS[c] in
    an order and with a padding of its own (-1, nlist, a list twice)."""
    table = np.empty((nq, 3), np.int64)
    for i in range(nq):
        pool = CHUNK_POOLS[i // 64]
        row = [pool[(i + j) % len(pool)] for j in range(len(pool))]
        if len(pool) > 1 and i % 5 == 4:
            row = row[:-1]  # one list less; the other queries of the group still name it
        pad = ([-1, len(SIZES), row[0]][i % 3], [row[-1], -1, 2 ** 40][(i // 3) % 3], -1)
        table[i] = (row + list(pad))[:3]
        if len(row) < 3:  # (a full row differs from its neighbours by its order already)
            table[i] = np.roll(table[i], i % 3)
    return table


@pytest.mark.parametrize("nq", [63, 64, 65, 130, 200])
@pytest.mark.parametrize("d", [64, 136])
def test_chunks(d, nq):
    """One, two, three and four chunks of 64 queries: the padded queries, the masks, the offsets and the work buffer
    are reused from chunk to chunk, and D, I and the probes are indexed by chunk and group."""
    import torch

    index, C, xb, list_no, xq, dist = sized_index(d)
    nlist = len(C)
    xq, dist = xq[:nq], dist[:nq]
    rng = np.random.default_rng([d, nq])
    table = chunk_table(rng, nq)
    assert (np.abs(np.diff(table, axis=0)).sum(axis=1) > 0).all()  # a different probe row per query
    # consecutive chunks name different lists, and a later chunk's work lists are shorter than the earlier one's: the
    # entries of the chunk before lie behind them in the buffer
    counts, named = [], []
    for c0 in range(0, nq, 64):
        masks = ref.masks_of(table[c0:c0 + 64], nlist, 16)
        counts.append([count for _, count, _ in ref.work_list_of(masks, SIZES)])
        named.append(set(np.flatnonzero(masks.any(axis=0)).tolist()))
    assert counts[0][0] == 7
    for before, after, nb, na in zip(counts, counts[1:], named, named[1:]):
        assert all(a < b for a, b in zip(after, before)) and not (nb & na)
    xq_dev = torch.from_numpy(xq.copy()).cuda()  # (the shared queries are read-only)
    for k in (1, 33):
        for nprobe in (2, 3):  # the crafted table and the quantiser's in alternation: never the same table twice in a row
            got = search_pre(index, xq, k, table)
            assert_same(got, ref.search_preassigned(xb, list_no, xq, k, table, nlist, dist))
            assert_ordered(*got)
            index.nprobe = nprobe
            probes = ref.probes(C, xq, nprobe)
            D, I = counted(index, probes, k, lambda: index.search_torch(xq_dev, k))
            assert_same((D.cpu().numpy(), I.cpu().numpy()), ref.search_preassigned(xb, list_no, xq, k, probes, nlist, dist))


# ---------------------------------------------------------------- g. the staged host form past one batch
def test_host_form_past_one_batch():
    """4096 + 5 queries: the host form stages two batches, the second of 5 queries -- one group of 5 over work lists that
    still hold the last chunk of the first batch."""
    d, nlist, n, cs, k = 64, 7, 500, 8, 3
    nq = ref.HOST_BATCH + 5
    rng = np.random.default_rng(41)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
    xq[-5:] = xb[[0, 1, 2, n - 2, n - 1]]
    index = new_index(C)
    index.add(xb)
    list_no = ref.assign(C, xb)
    table = rng.integers(0, nlist, (nq, 2))
    table[-5:] = [[0, 1], [2, 2], [-1, 3], [6, 5], [4, nlist]]
    assert ref.host_batches(nq) == 2
    want_stats = ref.stats_of(table, sizes_of(index), k, batches=2)
    before = index.binary_ivf_stats()
    got = index.search_preassigned(xq, k, table)
    after = index.binary_ivf_stats()
    assert {key: after[key] - before[key] for key in want_stats} == want_stats
    assert want_stats["passes"] == 257 and want_stats["batches"] == 2
    assert_same(got, ref.search_preassigned(xb, list_no, xq, k, table, nlist))


# ---------------------------------------------------------------- h. row lengths through the lists
@pytest.mark.parametrize("d", [320, 576, 1088, 4160, 8192])
def test_long_rows_through_the_lists(d):
    """ws = 6, 10, 18, 66 and 128: 3, 5, 9, 33 and 64 chunks in hamming16<0>, one and two rounds of the scatter's word
    loop, 64 ws words a tile in the move.  Two adds with a search after each: the second rebuild moves the first's tiles."""
    nlist, nq, cs = 7, 37, d // 8
    ws = (-(-cs // 8) + 1) // 2 * 2
    assert ws == {320: 6, 576: 10, 1088: 18, 4160: 66, 8192: 128}[d]
    rng = np.random.default_rng(500 + d)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (700, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
    xq[:4] = xb[[0, 299, 300, 699]]
    index = new_index(C)
    list_no = ref.assign(C, xb)
    have = 0
    for m in (300, 400):
        index.add(xb[have:have + m])
        have += m
        check_lists(index, list_no[:have], xb[:have])
        dist = binary_ref.distances(xb[:have], xq)
        flat = flat_index(xb[:have])
        for k in (1, 33):
            for nprobe in (1, 3, nlist):
                index.nprobe = nprobe
                table = ref.probes(C, xq, nprobe)
                got = counted(index, table, k, lambda: index.search(xq, k))
                assert_same(got, ref.search_preassigned(xb[:have], list_no[:have], xq, k, table, nlist, dist))
                if nprobe == nlist:
                    assert_same(got, flat.search(xq, k))
    if d == 8192:  # one word more is refused
        h = ctypes.c_void_p()
        assert native.lib.ise_binary_ivf_create(ctypes.byref(h), 8200, nlist, index.device) == native.E_INVALID and not h.value


# ---------------------------------------------------------------- i. rebuilds at many lists
@pytest.mark.parametrize("d", [64, 136])
@pytest.mark.parametrize("nlist", [257, 1000])
def test_rebuilds_at_many_lists(nlist, d):
    """Four adds, a search (and so a rebuild) after each: rows all over the lists with exactly 64 in list 0; rows for the
    upper half of the lists only; a single row for list 0, whose second tile moves every later tile by one; rows all
    over again."""
    cs, nq = d // 8, 40
    rng = np.random.default_rng([nlist, d])
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    calls = [np.concatenate([np.zeros(64, np.int64), rng.integers(1, nlist, 1500)]), rng.integers(nlist // 2, nlist, 600),
             np.zeros(1, np.int64), rng.integers(0, nlist, 800)]
    calls = [rng.permutation(c) for c in calls]
    list_no = np.concatenate(calls)
    xb = ref.near_centroids(rng, C, list_no)
    assert np.array_equal(ref.assign(C, xb), list_no)  # the assignment came out as intended
    xq = ref.near_centroids(rng, C, rng.integers(0, nlist, nq), flips=6)
    index = new_index(C)
    have, history = 0, []
    for c in calls:
        index.add(xb[have:have + len(c)])
        have += len(c)
        sizes = sizes_of(index)
        assert sizes == np.bincount(list_no[:have], minlength=nlist).tolist() and index.ntotal == have
        history.append(np.array(sizes))
        dist = binary_ref.distances(xb[:have], xq)
        for k in (10, 40):
            table = rng.integers(0, nlist, (nq, 3))  # a fresh table every time
            table[:3, 0] = [0, 1, nlist - 1]
            table[np.arange(nq), 1] = ref.probes(C, xq, 1)[:, 0]  # the query's own list: results at small distances
            got = search_pre(index, xq, k, table)
            assert_same(got, ref.search_preassigned(xb[:have], list_no[:have], xq, k, table, nlist, dist))
        check_lists(index, list_no[:have], xb[:have])
    assert history[0][0] == 64 and history[2][0] == 65 and np.array_equal(history[0][:nlist // 2], history[1][:nlist // 2])
    assert (history[1][nlist // 2:] > history[0][nlist // 2:]).sum() > nlist // 4
    t1, t2 = ref.tile0_of(history[1]), ref.tile0_of(history[2])
    assert np.array_equal(t2[1:], t1[1:] + 1)  # every tile behind list 0 moved by one


# ---------------------------------------------------------------- j. workspaces that grow and are then too large
def test_workspaces_grow_and_stay():
    """One handle: 100 rows (a grid of 1), 40 000 more (the grid, the blocks' lists and the work buffer grow), then a
    reset and 100 other rows -- a grid of 1 again over buffers that hold the large index's lists and entries."""
    d, nlist, cs, nq, k = 64, 7, 8, 70, 33
    rng = np.random.default_rng(43)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (40100, cs), dtype=np.uint8)
    other = rng.integers(0, 256, (100, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
    xq[:3] = xb[[0, 99, 40099]]
    index = new_index(C)
    list_no, other_no = ref.assign(C, xb), ref.assign(C, other)

    def check(rows, lists, what):
        table = rng.integers(-1, nlist, (nq, 3))
        got = search_pre(index, xq, k, table)
        assert_same(got, ref.search_preassigned(rows, lists, xq, k, table, nlist))
        assert_ordered(*got)
        return ref.tiles_of(sizes_of(index))

    index.add(xb[:100])
    assert check(xb[:100], list_no[:100], "100 rows") <= 8  # two tiles per wave, four waves: one block
    index.add(xb[100:])
    assert check(xb, list_no, "40 100 rows") > 600
    index.nprobe = nlist
    assert_same(counted(index, ref.probes(C, xq, nlist), k, lambda: index.search(xq, k)), binary_ref.search(xb, xq, k))
    index.reset()
    assert index.ntotal == 0
    index.add(other)
    assert check(other, other_no, "100 other rows") <= 8
    check_lists(index, other_no, other)
