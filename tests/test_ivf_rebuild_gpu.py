"""GPU test of the inverted lists' rebuild kernels called directly, for every kind's instantiation and first of all the
float32 lists' (csrc/ise_ivf_tiles.hpp: ivf_move_tiles_kernel<16, u32x4>, ivf_scatter_rows_kernel<u32x4>), which the
other tests reach through the index only.  The harness entry ``chk_ivf_rebuild`` (tests/native/ivfsq_lists_harness.hip,
built into libise_ivfsq_check.so) takes the rows of a tile and the bytes of a copy unit and calls the product's own
``ivf_rebuild_launch``; every word of the new rows and ids, pad slots included, is compared with the numpy model of
tests/ivfsq_ref.py at that tile size.

The new arrays hold the pattern 0xA5A5A5A5 on entry, every array is as large as the tables say and every slot lies in
the new arrays (asserted before the launch): no input here can make a wrong kernel read or write outside its buffers."""
import numpy as np
import pytest

from tests import ivfsq_ref
from tests.test_ivfsq_lists_gpu import dev, dev_filled, host_u32, lib, run  # noqa: F401  (lib: the harness fixture)

pytestmark = pytest.mark.gpu


def rebuild(lib, tile_rows, unit_bytes, row_bytes, old_sizes, old, pend_lists, pend_rows, id0):
    """-> (rows uint8 [slots][row_bytes], ids uint32 [slots]) of the new arrays as ivf_rebuild_launch leaves them; old =
    (rows, ids) laid out by old_sizes.  The slot numbers come from the reference's plan."""
    nlist = len(old_sizes)
    old_rows, old_ids = old
    old_tiles = ivfsq_ref.tiles_of(old_sizes, tile_rows)
    new_sizes = old_sizes + np.bincount(pend_lists, minlength=nlist)
    new_tiles = ivfsq_ref.tiles_of(new_sizes, tile_rows)
    dest = ivfsq_ref.rebuild_dest(old_sizes, pend_lists, tile_rows)
    meta, nmeta = ivfsq_ref.meta_of(old_sizes, tile_rows), ivfsq_ref.meta_of(new_sizes, tile_rows)
    m = len(pend_lists)
    # every array is as large as the tables say, every slot lies in the new arrays, and no two rows share one
    assert row_bytes % unit_bytes == 0 and row_bytes % 4 == 0 and m >= 1 and 1 <= new_tiles < 2 ** 26 and old_tiles <= new_tiles
    assert old_rows.shape == (old_tiles * tile_rows, row_bytes) and old_rows.dtype == np.uint8
    assert old_ids.shape == (old_tiles * tile_rows,) and old_ids.dtype == np.uint32
    assert pend_rows.shape == (m, row_bytes) and pend_rows.dtype == np.uint8
    assert len(meta) == 2 * nlist + 1 + old_tiles and len(nmeta) == 2 * nlist + 1 + new_tiles
    assert meta[nlist] == old_tiles and nmeta[nlist] == new_tiles
    assert (meta[2 * nlist + 1:] < nlist).all() and (nmeta[2 * nlist + 1:] < nlist).all()
    assert (np.diff(nmeta[:nlist + 1].astype(np.int64)) >= np.diff(meta[:nlist + 1].astype(np.int64))).all()  # no list shrinks
    assert dest.shape == (m,) and dest.max() < new_tiles * tile_rows and len(np.unique(dest)) == m
    assert 0 <= id0 and id0 + m - 1 <= 2 ** 32 - 2
    nx = dev_filled((new_tiles * tile_rows, row_bytes // 4))
    nids = dev_filled((new_tiles * tile_rows,))
    run(lib.chk_ivf_rebuild, tile_rows, unit_bytes, row_bytes, dev(old_rows), dev(old_ids), dev(meta), old_tiles, dev(pend_rows), m,
        dev(dest), id0, nlist, dev(nmeta), new_tiles, nx, nids)
    return nx.cpu().numpy().view(np.uint8).reshape(-1, row_bytes), host_u32(nids)


def assert_arrays(got, want, tile_rows, what):
    for name, a, b in zip(("rows", "ids"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        if not np.array_equal(a, b):
            slot = np.argwhere(a != b)[0][0]
            raise AssertionError(f"{what}: the {name} differ in {int((a != b).sum())} places, first at slot {slot} "
                                 f"(tile {slot // tile_rows}, row {slot % tile_rows})")


# a row of 16 bytes is one 16-byte unit (fewer than a wave's lanes); 1040 bytes are 65 units (a wave's second round
# of one lane); at 1088 bytes a 16-row tile is 1088 units (the block's 256 threads take five rounds).  The other two
# instantiations: 64-row tiles moved in 16-byte units and in 8-byte units (a row of one unit, and of 65)
@pytest.mark.parametrize("tile_rows,unit_bytes,row_bytes", [(16, 16, 16), (16, 16, 1040), (16, 16, 1088),
                                                            (64, 16, 1040), (64, 8, 8), (64, 8, 520)])
def test_rebuild_kernels_of_every_kind(lib, tile_rows, unit_bytes, row_bytes):
    T = tile_rows
    rng = np.random.default_rng([tile_rows, unit_bytes, row_bytes])
    nlist = 7
    zero = np.zeros(nlist, np.int64)
    none = (np.zeros((0, row_bytes), np.uint8), np.zeros(0, np.uint32))
    # list 0 is one row short of a tile, 1 and 3 end exactly on a tile, 2 is empty between full ones, 6 is empty at the end
    sizes1 = np.array([T - 1, T, 0, 2 * T, 1, 3, 0], np.int64)
    # list 0 grows across the tile boundary: every later tile shifts by one, and by one more behind list 4; list 4 comes
    # to end exactly on its second tile, lists 1 to 3 keep their rows, the last list gets its first
    add = np.array([3, 0, 0, 0, 2 * T - 1, 0, 3], np.int64)
    n1, m2 = int(sizes1.sum()), int(add.sum())
    assert n1 % 4 != 0 and m2 % 4 != 0  # the scatter's last block has idle waves
    id0 = 2 ** 32 - 1 - m2 - n1         # the last id is 2^32 - 2: the largest that is not the pad id
    lists1 = rng.permutation(np.repeat(np.arange(nlist), sizes1))  # the ids interleave in every list
    rows1 = rng.integers(0, 256, (n1, row_bytes)).astype(np.uint8)
    got_sizes, want_rows, _, want_ids = ivfsq_ref.rebuilt(zero, none[1], none[0], lists1, rows1, id0, row_bytes, tile_rows=T)
    assert np.array_equal(got_sizes, sizes1) and len(want_ids) == 6 * T
    # no old tile at all: the move kernel is not launched
    assert_arrays(rebuild(lib, T, unit_bytes, row_bytes, zero, none, lists1, rows1, id0), (want_rows, want_ids), T, "no old tiles")
    t_old, t_new = ivfsq_ref.tile0_of(sizes1, T), ivfsq_ref.tile0_of(sizes1 + add, T)
    assert (t_new - t_old).tolist() == [0, 1, 1, 1, 1, 2, 2, 3]
    lists2 = rng.permutation(np.repeat(np.arange(nlist), add))
    rows2 = rng.integers(0, 256, (m2, row_bytes)).astype(np.uint8)
    old = (want_rows, want_ids)
    sizes2, want_rows2, _, want_ids2 = ivfsq_ref.rebuilt(sizes1, old[1], old[0], lists2, rows2, id0 + n1, row_bytes, tile_rows=T)
    assert np.array_equal(sizes2, sizes1 + add) and int(want_ids2[want_ids2 != ivfsq_ref.PAD_ID].max()) == 2 ** 32 - 2
    assert (want_ids2 == ivfsq_ref.PAD_ID).sum() == len(want_ids2) - n1 - m2 > 0
    assert_arrays(rebuild(lib, T, unit_bytes, row_bytes, sizes1, old, lists2, rows2, id0 + n1), (want_rows2, want_ids2), T,
                  "over six old tiles")
