"""The deep plan of the byte shadow scan, restated (make_plan, csrc/ise_knn.hip).  A batch that has
other batches in flight beside it is scanned by slots / depth blocks of depth times the rows, so that `depth`
consecutive batches are resident together and a block pays its fixed phases once per depth times the rows.  Depth 1 is
the isolated plan (tests/test_block_phases_gpu.py, _tiles_per_block); the exact fallback scan keeps that plan's grid
whatever depth the filter ran at, and the workspace slots are sized by it: the deep plan never has more blocks, which
make_plan checks (no accessor shows a slot's pointers, so that no allocation follows a change of plan is checked
there, in the C code, and by the block counts below)."""
import types

import pytest

SLOTS_PER_CU = 2   # two 8-wave blocks per CU at one query tile
WAVES = 8
SEED_MIN_TILES = (WAVES - 1) + 2 * WAVES + 4 * WAVES  # ise_scan.hpp, nboot: t1 - (t0 + W - 1 + 2 W) >= 4 W
XGRID = 512        # blocks the folded exchange read covers: a larger grid boots with the cut
XONE = 256         # ... and those one request covers


def deep_plan(n, depth, num_cu=256):
    """blocks, tiles per block and the depth taken for the byte route's one-tile scan of n rows, with the grid the
    exact fallback gets."""
    slots = SLOTS_PER_CU * num_cu
    tiles = (n + 15) // 16
    nb = min(slots, (tiles + WAVES - 1) // WAVES)  # (shadow rows exist past 262144 rows: the spread plan never exceeds this)
    tpb = (tiles + nb - 1) // nb
    plan = {"depth": 1, "tiles": tiles, "tpb": tpb, "blocks": (tiles + tpb - 1) // tpb}
    plan["fb_tpb"], plan["fb_blocks"] = plan["tpb"], plan["blocks"]
    if depth > 1 and nb == slots and slots // depth >= 1:
        nbd = slots // depth
        tpbd = (tiles + nbd - 1) // nbd
        if tpbd >= SEED_MIN_TILES:
            plan.update(depth=depth, tpb=tpbd, blocks=(tiles + tpbd - 1) // tpbd)
    return plan


def block_tiles(plan, b):
    t0 = b * plan["tpb"]
    return min(plan["tiles"], t0 + plan["tpb"]) - t0


def seeded(plan, b):
    """Block b takes the seeded boot: every wave has 4 W tiles behind its two window tiles, on a grid the folded read
    covers."""
    return plan["blocks"] <= XGRID and block_tiles(plan, b) >= SEED_MIN_TILES


def block_row0(plan, b):
    return b * 16 * plan["tpb"]


@pytest.fixture
def cu256(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda *a: types.SimpleNamespace(multi_processor_count=256))


@pytest.mark.parametrize("n", [262_145, 300_000, 350_000, 499_995, 500_000, 1_000_000, 3_000_000])
def test_depth_one_is_the_isolated_plan(cu256, n):
    from tests.test_block_phases_gpu import _tiles_per_block

    for depth in (0, 1):
        p = deep_plan(n, depth)
        assert p["depth"] == 1 and p["tpb"] == _tiles_per_block(n)
        assert (p["fb_tpb"], p["fb_blocks"]) == (p["tpb"], p["blocks"])


@pytest.mark.parametrize("n, depth, blocks, tpb, took", [
    (500_000, 1, 505, 62, 1),
    (500_000, 2, 255, 123, 2),
    (500_000, 4, 128, 245, 4),
    (350_000, 1, 509, 43, 1),
    (350_000, 2, 255, 86, 2),
    (350_000, 4, 128, 171, 4),
    (1_000_000, 2, 256, 245, 2),
    (300_000, 2, 254, 74, 2),
    (270_000, 1, 512, 33, 1),
    (270_000, 2, 256, 66, 2),
])
def test_shapes(n, depth, blocks, tpb, took):
    p = deep_plan(n, depth)
    assert (p["blocks"], p["tpb"], p["depth"]) == (blocks, tpb, took)


def test_demoted_where_a_full_block_would_lose_the_seeded_boot():
    p = deep_plan(262_145, 2, num_cu=304)  # 16385 tiles on 304 blocks: 54 per block, one short of the seeded boot
    assert p["depth"] == 1 and p == deep_plan(262_145, 1, num_cu=304)
    assert deep_plan(262_145, 2)["depth"] == 2  # 256 CUs: 65 per block


def test_which_blocks_are_seeded():
    p = deep_plan(500_000, 2)
    assert all(seeded(p, b) for b in range(254)) and block_tiles(p, 254) == 8 and not seeded(p, 254)
    p = deep_plan(500_000, 4)
    assert all(seeded(p, b) for b in range(128))
    p1, p2 = deep_plan(350_000, 1), deep_plan(350_000, 2)
    assert not any(seeded(p1, b) for b in range(p1["blocks"]))  # depth changes which boot runs
    assert all(seeded(p2, b) for b in range(254)) and not seeded(p2, 254)
    assert p2["blocks"] <= XONE and deep_plan(1_000_000, 2)["blocks"] <= XONE  # the one-request exchange read


@pytest.mark.parametrize("depth", [2, 3, 4, 8, 16, 1000])
def test_fallback_grid_and_slot_sizes(depth):
    """The exact fallback keeps the depth-1 grid, which covers every row; the deep plan covers every row with no more
    blocks (the slots' lists and exchange entries are sized by the depth-1 grid) and demotes itself rather than leave a
    full block without the seeded boot."""
    for n in list(range(262_145, 1_200_000, 7919)) + [5_000_000, 50_000_000]:
        p1, p = deep_plan(n, 1), deep_plan(n, depth)
        assert (p["fb_blocks"], p["fb_tpb"]) == (p1["blocks"], p1["tpb"])
        assert p["fb_blocks"] * p["fb_tpb"] >= p["tiles"] > (p["fb_blocks"] - 1) * p["fb_tpb"]
        assert p["blocks"] * p["tpb"] >= p["tiles"] > (p["blocks"] - 1) * p["tpb"]
        assert 1 <= p["blocks"] <= p["fb_blocks"]
        if p["depth"] > 1:
            assert p["tpb"] >= SEED_MIN_TILES and seeded(p, 0)
        else:
            assert p == p1
