"""CPU model of the filtered final phase of the exchange kernels (csrc/ise_scan.hpp, FFILT).

A block's list is the kc smallest of its keys (score << 32 | id), sorted, KEY_PAD behind them.  With the one-shot
threshold exchange a block may hold a bound: the kc-th smallest of the scores that kc or more OTHER blocks published,
each the score of one of that block's own rows, so of kc distinct rows of the launch.  The final phase then drops every
key above (bound << 32) | 0xFFFFFFFF before it selects.  The claim checked here: merging the filtered lists gives the
same kc keys as merging the full ones -- whatever subset of the published entries each block happened to see, with
ties on the score, with fewer than kc rows in all, and with empty and short (KEY_PAD padded) lists."""
import numpy as np
import pytest

KEY_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def _block_list(keys, kc, bound=None):
    keys = np.asarray(keys, np.uint64)
    keys = keys[keys != KEY_PAD]
    if bound is not None:
        keys = keys[keys <= bound]
    out = np.full(kc, KEY_PAD, np.uint64)
    best = np.sort(keys)[:kc]
    out[:len(best)] = best
    return out


def _merge(lists, kc):
    allk = np.concatenate(lists)
    out = np.full(kc, KEY_PAD, np.uint64)
    best = np.sort(allk[allk != KEY_PAD])[:kc]
    out[:len(best)] = best
    return out


def _bound(published, kc):
    """The exchange of one reader: the kc-th smallest published score, or None when fewer than kc entries were there
    (absent entries read as 0xFFFFFFFF; a published 0xFFFFFFFF -- a block without a row -- counts as absent too)."""
    p = np.sort(np.asarray([s for s in published if s != 0xFFFFFFFF], np.uint64))
    if len(p) < kc:
        return None
    return (p[kc - 1] << np.uint64(32)) | np.uint64(0xFFFFFFFF)


def _run(rng, blocks, kc, see_prob):
    """blocks: list of uint64 key arrays.  Every block publishes the score of the best of its first rows (its boot
    tile: a prefix of its keys); every block reads a random subset of the entries (the exchange is best-effort)."""
    published = []
    for keys in blocks:
        real = keys[keys != KEY_PAD]
        boot = real[:max(1, len(real) // 4)] if len(real) else real
        published.append(int(boot.min() >> np.uint64(32)) if len(boot) else 0xFFFFFFFF)
    full = [_block_list(k, kc) for k in blocks]
    filt, n_bounds, n_dropped = [], 0, 0
    for b, keys in enumerate(blocks):
        seen = [s for s in published if rng.random() < see_prob]
        bound = _bound(seen, kc)
        n_bounds += bound is not None
        lst = _block_list(keys, kc, bound)
        n_dropped += int((full[b] != KEY_PAD).sum() - (lst != KEY_PAD).sum())
        # what the merge relies on: sorted, the pads behind the keys
        real = lst[lst != KEY_PAD]
        assert (np.diff(real.astype(np.float64)) >= 0).all() and (lst[len(real):] == KEY_PAD).all()
        filt.append(lst)
    want = _merge(full, kc)
    got = _merge(filt, kc)
    assert np.array_equal(got, want)
    allk = np.concatenate(blocks)
    assert np.array_equal(want, _block_list(allk, kc))  # and both are the kc smallest keys of the launch
    return n_bounds, n_dropped


def _keys(scores, ids):
    return (np.asarray(scores, np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


@pytest.mark.parametrize("kc", [1, 5, 14, 32])
@pytest.mark.parametrize("see_prob", [1.0, 0.7, 0.2])
def test_filtered_lists_merge_to_the_same_keys(kc, see_prob):
    rng = np.random.default_rng([kc, int(see_prob * 10)])
    bounds = dropped = 0
    for trial in range(20):
        nb = int(rng.integers(1, 80))
        rows = int(rng.integers(1, 200))
        blocks, base = [], 0
        for b in range(nb):
            n = int(rng.integers(0, rows + 1))
            blocks.append(_keys(rng.integers(0, 2 ** 32 - 1, n), base + rng.permutation(n)))
            base += n
        nbnd, ndrop = _run(rng, blocks, kc, see_prob)
        bounds += nbnd
        dropped += ndrop
    if see_prob == 1.0:
        assert bounds > 0 and dropped > 0  # the model does exercise the filter


@pytest.mark.parametrize("kc", [1, 4, 32])
def test_ties_on_the_score(kc):
    """Few distinct scores (integer data: many equal distances): keys tie on the score part and differ in the id;
    every id at the bound's score stays admissible."""
    rng = np.random.default_rng(kc)
    for levels in (1, 2, 5):
        for trial in range(10):
            nb, n = 40, 60
            blocks = [_keys(rng.integers(7, 7 + levels, n), b * n + rng.permutation(n)) for b in range(nb)]
            nbnd, ndrop = _run(rng, blocks, kc, 0.9)
            assert nbnd > 0
    # the extreme scores: ord(-FLT_MAX) = 0x00800000 for every row (overflowing norms), and 0 itself
    for s in (0x00800000, 0):
        blocks = [_keys(np.full(50, s), b * 50 + np.arange(50)) for b in range(40)]
        _run(rng, blocks, kc, 1.0)


def test_fewer_rows_than_kc_and_padded_lists():
    rng = np.random.default_rng(3)
    kc = 32
    # fewer than kc rows in all: no reader can obtain a bound, every key survives
    blocks = [_keys(rng.integers(0, 1000, 1), [b]) for b in range(20)] + [np.zeros(0, np.uint64)] * 30
    nbnd, ndrop = _run(rng, blocks, kc, 1.0)
    assert nbnd == 0 and ndrop == 0
    # exactly kc blocks with one row each: the bound is the largest of them and drops nothing
    blocks = [_keys([b * 3 + 1], [b]) for b in range(kc)]
    nbnd, ndrop = _run(rng, blocks, kc, 1.0)
    assert nbnd == kc and ndrop == 0
    # short lists: KEY_PAD entries inside the inputs (empty slots of a block's candidate lists) are never keys
    blocks = []
    for b in range(60):
        k = _keys(rng.integers(0, 2 ** 20, 40), b * 40 + np.arange(40))
        k[rng.random(40) < 0.5] = KEY_PAD
        blocks.append(k)
    nbnd, ndrop = _run(rng, blocks, kc, 1.0)
    assert nbnd == 60 and ndrop > 0


def test_a_stale_or_foreign_bound_would_be_caught():
    """The model is not vacuous: a bound that is NOT from kc distinct rows of this launch (an older launch's entries
    read as present) does change the merged keys."""
    rng = np.random.default_rng(9)
    kc = 8
    blocks = [_keys(rng.integers(1000, 2000, 30), b * 30 + np.arange(30)) for b in range(20)]
    stale = (np.uint64(500) << np.uint64(32)) | np.uint64(0xFFFFFFFF)  # scores of an earlier, closer batch
    full = _merge([_block_list(k, kc) for k in blocks], kc)
    wrong = _merge([_block_list(k, kc, stale) for k in blocks], kc)
    assert not np.array_equal(full, wrong)
