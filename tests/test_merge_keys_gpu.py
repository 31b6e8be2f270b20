"""GPU tests of the public list merge, ise_merge_keys_device, through faiss.merge_keys_torch alone: merge_small_kernel
(64 lists or fewer, four queries per block) and merge_kernel<false> (up to 1024 lists; merge_waves for k <= 40,
merge_rounds above) at list counts, query counts and k the search paths never give it, with the winners placed on
chosen lists.  Expected D, I: tests/keycodec.decode of the sorted k smallest keys -- bit for bit."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import keycodec
from tests import select_ref as sr
from tests.select_ref import PAD, U64

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
N_LISTS = (1, 2, 63, 64, 65, 512, 1024)
NQ = (1, 3, 5)  # not multiples of 4: merge_small_kernel's last block serves fewer than four queries
K = (1, 10, 40, 41, 100, 2048)
PLACEMENTS = ("spread", "one_list", "one_wave", "short")
KEYS_PER_QUERY = 300_000  # the most keys a query's lists hold together (the lists' slots behind them are PAD)


def query_lists(rng, n_lists, k, placement, tied):
    """[n_lists][k] ascending lists, PAD behind; the k smallest keys of all are the winners.
    spread: winners on random lists; one_list: all on one list; one_wave: all on lists l = w mod 8 (the lists of one
    wave of merge_kernel); short: every list holds fewer than k keys (fewer than k in all where the lists are few)."""
    full = max(1, min(k, KEYS_PER_QUERY // n_lists))
    if placement == "short":
        counts = rng.integers(0, min(k - 1, max(1, full // 2)) + 1, size=n_lists)
    else:
        counts = np.full(n_lists, full)
    tokens = np.repeat(np.arange(n_lists), counts)  # one per key slot in use
    if placement == "one_list":
        home = np.flatnonzero(tokens == rng.integers(0, n_lists))
    elif placement == "one_wave":
        home = np.flatnonzero(tokens % 8 == rng.integers(0, min(8, n_lists)))
    else:
        home = np.arange(len(tokens))
    win = rng.permutation(home)[:k]  # the slots of the winners: on the home lists, as many as fit
    rest = np.setdiff1d(np.arange(len(tokens)), win)
    owner = np.concatenate([tokens[win], tokens[rng.permutation(rest)]])
    keys = sr.score_keys(rng, len(owner), tied)  # ascending: the first k are the winners
    order = np.argsort(owner, kind="stable")  # by list, ascending within a list
    owner, keys = owner[order], keys[order]
    pos = np.arange(len(owner)) - np.searchsorted(owner, owner)
    out = np.full((n_lists, k), PAD, dtype=U64)
    out[owner, pos] = keys
    return out


@pytest.mark.parametrize("n_lists", N_LISTS)
def test_merge_keys(n_lists):
    import torch

    seen = set()
    for ki, k in enumerate(K):
        for pi, placement in enumerate(PLACEMENTS):
            j = ki * len(PLACEMENTS) + pi
            nq, metric = NQ[(j + ki) % 3], (L2, IP)[(j // 2 + ki) % 2]
            if n_lists * k > 512 * 2048:
                nq = min(nq, 3)  # the largest key tensor: 1024 x 3 x 2048
            seen.add((nq, metric))
            rng = np.random.default_rng([n_lists, k, pi])
            per_q = np.stack([query_lists(rng, n_lists, k, placement, tied=(q + j) % 2 == 1) for q in range(nq)])
            keys = np.ascontiguousarray(per_q.transpose(1, 0, 2))  # (n_lists, nq, k)
            D, I = faiss.merge_keys_torch(torch.from_numpy(keys.view(np.int64)).cuda(), metric)
            want = np.stack([sr.padded(sr.smallest(per_q[q], k), k) for q in range(nq)])
            want_D, want_I = keycodec.decode(want, metric)
            tag = f"n_lists={n_lists} nq={nq} k={k} metric={metric} {placement}"
            assert np.array_equal(I.cpu().numpy(), want_I), tag
            assert np.array_equal(D.cpu().numpy().view(np.uint32), want_D.view(np.uint32)), tag
    assert seen == {(nq, m) for nq in NQ for m in (L2, IP)}, "every nq with both metrics"
