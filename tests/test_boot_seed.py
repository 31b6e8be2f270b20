"""CPU model of the seeded boot of the byte shadow scan (csrc/ise_scan.hpp, NBOOT).

A block of the seeded kind keeps the keys (score << 32 | id) of a boot window -- the first two row tiles of each of its
waves -- unfiltered, publishes the score of the best row of its FIRST tiles, and after the window reads the exchange:
the kc-th smallest of the published scores it happens to see, or nothing when fewer than kc are there.  It then seeds
its block list with the window keys <= (bound << 32) | 0xFFFFFFFF and takes the bound as its threshold; without a
bound, or with more than kb window keys under it, it cuts the window keys exactly (the kc..kb smallest, threshold = the
cut).  Rows behind the window are admitted by key < threshold, the list is folded to its kc smallest whenever it
overflows (the threshold then drops to the list's kc-th key), and the final phase drops what lies above the bound.
Blocks too short for the exchange boot with the cut over their first tiles and never hold a bound.

The claim: the block lists merge to the kc smallest keys of the launch, in every situation the kernel can meet."""
import numpy as np
import pytest

from tests.test_final_filter import KEY_PAD, _block_list, _bound, _keys, _merge

TAU0 = np.uint64(0xFF7FFFFF) << np.uint64(32)
WINDOW = 256  # rows of a seeded block's boot window (8 waves x 2 tiles x 16 rows); the publish covers the first 128


def _cut(keys, kmin, kmax, rng):
    """wave_cut: a key P with kmin <= #(keys <= P) <= kmax and the keys <= P (all of them when at most kmax); the
    threshold is P when kmin were reached, else none."""
    keys = np.sort(keys)
    if len(keys) <= kmax:
        return keys, (keys[-1] if len(keys) >= kmin else TAU0)
    n = int(rng.integers(kmin, kmax + 1))
    return keys[:n], keys[n - 1]


def _block(keys, kc, kb, seeded, seen, rng, stats):
    keys = np.asarray(keys, np.uint64)
    window = keys[:WINDOW if seeded else WINDOW // 2]
    rest = keys[len(window):]
    bound = _bound(seen, kc) if seeded else None
    under = window[window <= bound] if bound is not None else None
    if bound is not None and len(under) <= kb:
        lst, tau = under, bound
        stats["seeded"] += 1
    else:
        lst, tau = _cut(window, kc, kb, rng)
        stats["overflow" if bound is not None else "no_bound"] += seeded
        if bound is not None:
            tau = min(tau, bound)
    lst = list(lst)
    for key in rest:  # steady state: admission by < tau, fold at overflow
        if key < tau:
            lst.append(key)
            if len(lst) > kb + 12:
                lst = sorted(lst)[:kc]
                tau = min(tau, lst[-1]) if len(lst) == kc else tau
    return _block_list(np.asarray(lst, np.uint64), kc, bound)


def _run(rng, blocks, kc, kb, see_prob, seeded_prob=1.0):
    published = []
    kinds = [rng.random() < seeded_prob for _ in blocks]
    for keys in blocks:
        first = keys[:WINDOW // 2]
        published.append(int(first.min() >> np.uint64(32)) if len(first) else 0xFFFFFFFF)
    stats = {"seeded": 0, "overflow": 0, "no_bound": 0}
    lists = []
    for keys, seeded in zip(blocks, kinds):
        seen = [s for s in published if rng.random() < see_prob]
        lists.append(_block(keys, kc, kb, seeded, seen, rng, stats))
    want = _block_list(np.concatenate(blocks) if blocks else np.zeros(0, np.uint64), kc)
    assert np.array_equal(_merge(lists, kc), want)
    return stats


def _uniform_blocks(rng, nb, rows, hi=2 ** 32 - 1):
    return [_keys(rng.integers(0, hi, rows), b * rows + rng.permutation(rows)) for b in range(nb)]


@pytest.mark.parametrize("kc,kb", [(1, 16), (14, 16), (32, 32), (32, 48)])
@pytest.mark.parametrize("see_prob", [1.0, 0.6, 0.1])
def test_seeded_lists_merge_to_the_same_keys(kc, kb, see_prob):
    rng = np.random.default_rng([kc, kb, int(see_prob * 10)])
    total = {"seeded": 0, "overflow": 0, "no_bound": 0}
    for trial in range(6):
        blocks = _uniform_blocks(rng, int(rng.integers(40, 90)), int(rng.integers(300, 900)))
        for key, v in _run(rng, blocks, kc, kb, see_prob, seeded_prob=0.8).items():
            total[key] += v
    if see_prob == 1.0:
        assert total["seeded"] > 0


@pytest.mark.parametrize("kc,kb", [(1, 16), (32, 32), (32, 48)])
def test_ties_on_the_score_at_the_bound(kc, kb):
    rng = np.random.default_rng([7, kc])
    for levels in (1, 2, 5):
        blocks = _uniform_blocks(rng, 50, 400, hi=levels)  # every key ties on one of a few scores
        _run(rng, blocks, kc, kb, 0.9)
    for s in (0x00800000, 0):  # ord(-FLT_MAX) for every row, and 0 itself
        blocks = [_keys(np.full(300, s), b * 300 + np.arange(300)) for b in range(40)]
        _run(rng, blocks, kc, kb, 1.0)


def test_fewer_than_kc_rows_in_all_and_empty_blocks():
    rng = np.random.default_rng(11)
    blocks = [_keys(rng.integers(0, 1000, 1), [b]) for b in range(20)] + [np.zeros(0, np.uint64)] * 30
    stats = _run(rng, blocks, 32, 32, 1.0)
    assert stats["seeded"] == 0 and stats["no_bound"] == 50
    # empty blocks beside full ones: they publish 0xFFFFFFFF, which no reader counts
    blocks = _uniform_blocks(rng, 60, 500) + [np.zeros(0, np.uint64)] * 20
    stats = _run(rng, blocks, 32, 32, 1.0)
    assert stats["seeded"] > 0


def test_more_than_kb_window_keys_under_the_bound():
    """One block's window holds more than kb keys under the bound (copies of a near row): the block cuts exactly."""
    rng = np.random.default_rng(13)
    kc, kb = 32, 32
    for copies in (kb, kb + 1, 100):
        blocks = _uniform_blocks(rng, 60, 500, hi=2 ** 31)
        blocks = [(k | (np.uint64(1) << np.uint64(63))) for k in blocks]  # far rows
        ids = blocks[3][:copies] & np.uint64(0xFFFFFFFF)
        blocks[3][:copies] = _keys(np.full(copies, 5), ids)  # near copies inside one window
        ids = blocks[9][100:100 + copies // 2] & np.uint64(0xFFFFFFFF)
        blocks[9][100:100 + copies // 2] = _keys(np.full(copies // 2, 5), ids)  # ... and spread over a second window
        stats = _run(rng, blocks, kc, kb, 1.0)
        assert stats["overflow"] >= (1 if copies > kb else 0)


def test_readers_without_a_bound():
    rng = np.random.default_rng(17)
    blocks = _uniform_blocks(rng, 64, 600)
    stats = _run(rng, blocks, 32, 32, 0.0)  # nobody sees an entry: every block cuts its window
    assert stats["seeded"] == 0 and stats["no_bound"] == 64
    stats = _run(rng, blocks, 32, 32, 0.55)  # some readers see kc entries, others do not
    assert stats["seeded"] > 0 and stats["no_bound"] > 0


def test_a_foreign_bound_would_be_caught():
    """Not vacuous: seeding from the entries of another launch (closer queries) loses keys."""
    rng = np.random.default_rng(19)
    kc = 8
    blocks = [k | (np.uint64(1) << np.uint64(40)) for k in _uniform_blocks(rng, 40, 300, hi=2 ** 20)]
    stats = {"seeded": 0, "overflow": 0, "no_bound": 0}
    lists = [_block(k, kc, 16, True, [5] * 40, rng, stats) for k in blocks]
    assert not np.array_equal(_merge(lists, kc), _block_list(np.concatenate(blocks), kc))
