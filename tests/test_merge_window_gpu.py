"""GPU tests of the key WINDOW of ListHeads (csrc/ise_merge.hpp): every list of a merge keeps its next MERGE_WIN = 4
keys in registers, fetched together (16-byte requests where k and the stride are even and the lists aligned, 8-byte
ones otherwise) and refilled only when all four have won.  The cases put the winners where the window can go wrong:
all in one list (it refills ceil(k / 4) - 1 times), alternating between the two lists of one thread, only in lists
whose keys end one, three or four slots in, in lists that are all pads, and exactly k or fewer keys in all -- at k
below, at and past the window and MERGE_PRE, odd and even, and through merge_rounds (k > 40).  A list's slots behind
its k keys hold POISON, a key below every real one: a window that read past k would return it.

Entry points: the existing libise_select_check.so (tests/native/select_harness.hip).  Reference: np.sort on uint64
(tests/select_ref.py), bit for bit; need_full against the path model where chk_mwaves returns it."""
import numpy as np
import pytest

from tests import keycodec
from tests import select_ref as sr
from tests.select_ref import ISENT, PAD, SENT, U64
from tests.test_select_gpu import dev, host, lib, run  # noqa: F401  (lib is the harness fixture)

pytestmark = pytest.mark.gpu

WIN = 4
K_WAVES = (1, 2, 3, 4, 5, 7, 8, 9, 32, 33, 36, 40)  # merge_waves
K_ROUNDS = (41, 70)  # merge_rounds
N_LISTS = (1, 2, 8, 511, 512, 513, 1024)  # a thread's second list (l + 512) absent, present, and the last one
POISON = U64(1)  # below every crafted key
INT_MAX = 2**31 - 1
L2, IP = 1, 0


def craft(n_lists, k, pattern, float_keys=False):
    """lists [n_lists][k] (ascending, PAD behind) or None where the pattern does not fit.  The k smallest keys are the
    winners; keys are unique and above POISON."""
    rng = np.random.default_rng([n_lists, k, sr.hash_int(pattern)])
    name, _, arg = pattern.partition(":")
    room = np.full(n_lists, k, dtype=np.int64)
    if name == "allpad":
        return np.full((n_lists, k), PAD, dtype=U64)
    if name == "exactk":
        total = min(k, n_lists * k)
    elif name == "fewer":
        total = k // 2
    else:
        total = min(int(room.sum()), 2 * k + n_lists)
    nwin = min(k, total)
    keys = sr.score_keys(rng, total) if float_keys else np.sort(sr.make_keys(rng, total, "rand"))  # all above POISON
    owner = np.full(total, -1, dtype=np.int64)
    if name == "onelist":  # every winner in one list: the window is refilled ceil(k / WIN) - 1 times
        l = int(arg) if int(arg) >= 0 else n_lists - 1
        if l >= n_lists or nwin < k:
            return None
        owner[:k] = l
        room[l] = 0
    elif name == "alt":  # winners alternate between the two lists of one thread, l and l + 512
        l = int(arg)
        if l + 512 >= n_lists or nwin < k:
            return None
        owner[:k] = np.where(np.arange(k) % 2 == 0, l, l + 512)
        room[l] -= (k + 1) // 2
        room[l + 512] -= k // 2
    elif name == "padadj":  # winners only in lists that hold exactly p keys: a pad at position p of the window
        p = int(arg)
        if p >= k or n_lists * p < k + p or nwin < k:
            return None
        homes = rng.permutation(n_lists)[:-(-k // p)]
        slots = np.repeat(homes, p)[:k]
        owner[:k] = rng.permutation(slots)
        extra = p * len(homes) - k  # losers that complete the last home to p keys
        if extra:
            owner[k:k + extra] = homes[-1]
        room[homes] = 0
    elif name in ("spread", "exactk", "fewer"):
        pass
    else:
        raise ValueError(pattern)
    rest = np.flatnonzero(owner < 0)
    slots = rng.permutation(np.repeat(np.arange(n_lists), room))[:len(rest)]
    if len(slots) < len(rest):
        return None
    owner[rest] = slots
    return sr.lists_from_owner(keys, owner, n_lists, k)


def patterns(n_lists):
    out = ["spread", "allpad", "exactk", "fewer", "onelist:0", "onelist:-1", "padadj:1", "padadj:3", "padadj:4"]
    out += [f"onelist:{l}" for l in (7, 512) if l < n_lists - 1]
    out += [f"alt:{l}" for l in (0, 5, 511) if l + 512 < n_lists]
    return out


def family(n_lists, k, float_keys=False):
    names, lists = [], []
    for pattern in patterns(n_lists):
        got = craft(n_lists, k, pattern, float_keys)
        if got is not None:
            names.append(pattern)
            lists.append(got)
    return names, np.stack(lists)


def test_patterns_hold_what_they_say():
    """(no GPU needed, but it belongs to this file's cases) the crafted lists are what the docstring promises."""
    lists = craft(1024, 33, "onelist:512")
    assert (np.sort(lists.ravel())[:33] == lists[512]).all()
    lists = craft(1024, 9, "alt:5")
    win = np.sort(lists.ravel())[:9]
    assert set(win[0::2]) <= set(lists[5]) and set(win[1::2]) <= set(lists[517])
    for p in (1, 3, 4):
        lists = craft(513, 8, f"padadj:{p}")
        win = np.sort(lists.ravel())[:8]
        homes = np.flatnonzero(np.isin(lists, win).any(axis=1))
        assert ((lists[homes] != PAD).sum(axis=1) == p).all(), "every winner's list ends with a pad at position p"
    assert (craft(8, 5, "allpad") == PAD).all()
    assert (craft(8, 7, "exactk") != PAD).sum() == 7 and (craft(8, 7, "fewer") != PAD).sum() == 3


@pytest.mark.parametrize("n_lists", N_LISTS)
def test_merge_waves_window(lib, n_lists):
    failures, total = [], 0
    for k in K_WAVES:
        names, lists = family(n_lists, k)
        nc = len(names)
        want, want_full = sr.merge_model_batch(lists, k)
        res = dev(np.full((nc, sr.MERGE_FAST_K), SENT, dtype=U64))
        full = dev(np.full(nc, ISENT, dtype=np.int32))
        run(lib.chk_mwaves, nc, dev(lists), n_lists, k, res, full)
        res, full = host(res, U64), host(full)
        for i, name in enumerate(names):
            if not np.array_equal(res[i, :k], want[i]) or not (res[i, k:] == SENT).all():
                failures.append(f"k={k} {name}: result differs (path flag {full[i]}, model {want_full[i]})")
            elif full[i] != want_full[i]:
                failures.append(f"k={k} {name}: need_full {full[i]}, the model says {want_full[i]}")
        total += nc
    assert not failures, f"{len(failures)} of {total} cases failed; the first: " + " | ".join(failures[:5])


@pytest.mark.parametrize("n_lists", N_LISTS)
def test_merge_kernel_window(lib, n_lists):
    """merge_kernel<false> (merge_waves up to k = 40, merge_rounds above) with a list stride of k + 1 and of k + 2:
    the slots behind every list hold POISON; an even k meets an odd stride (8-byte requests) and an even one (16-byte
    requests whose last pair ends at k), an odd k both (8-byte requests: k decides)."""
    failures, total = [], 0
    for j, (k, gap) in enumerate((k, gap) for k in K_WAVES + K_ROUNDS for gap in (1, 2)):
        names, lists = family(n_lists, k, float_keys=True)
        nq, stride = len(names), k + gap
        mem = np.full((nq, n_lists, stride), POISON, dtype=U64)
        mem[:, :, :k] = lists
        metric = (L2, IP)[j % 2]
        keys_out = dev(np.full((nq, k), SENT, dtype=U64))
        D = dev(np.full((nq, k), -1234.5, dtype=np.float32))
        I = dev(np.full((nq, k), ISENT, dtype=np.int64))
        run(lib.chk_merge, dev(mem), stride, n_lists * stride, 1, n_lists, nq, k, metric, keys_out, D, I)
        want = np.stack([sr.padded(sr.smallest(lists[q], k), k) for q in range(nq)])
        want_D, want_I = keycodec.decode(want, metric)
        got, got_D, got_I = host(keys_out, U64), host(D), host(I)
        for i, name in enumerate(names):
            if not (np.array_equal(got[i], want[i]) and np.array_equal(got_I[i], want_I[i])
                    and np.array_equal(got_D[i].view(np.uint32), want_D[i].view(np.uint32))):
                failures.append(f"k={k} stride={stride} {name}")
        total += nq
    assert not failures, f"{len(failures)} of {total} cases failed; the first: " + " | ".join(failures[:8])


# n_lists, nqt, kp, k, off: off > 0, and kp below the lists' stride kpass = 32 except in the last shape
PASS_SHAPES = [(513, 9, 1, 40, 39), (1024, 9, 3, 12, 9), (8, 6, 4, 70, 32), (512, 11, 5, 70, 64), (2, 6, 8, 20, 12),
               (511, 11, 9, 41, 32), (1, 5, 31, 64, 33), (1024, 12, 32, 96, 64)]


@pytest.mark.parametrize("kind", ["float_l2", "float_ip", "int"])
def test_pass_merge_window(lib, kind):
    """pass_merge_kernel: lists [n_lists][qt][kpass] with kp < kpass -- the slots [kp, kpass) of every list, its
    neighbour's keys in a real pass, hold POISON -- written at off > 0 of each query's k."""
    qt, kpass = 16, sr.CAND_KPASS
    ip = int(kind == "float_ip")
    for n_lists, nqt, kp, k, off in PASS_SHAPES:
        names, per_q = family(n_lists, kp, float_keys=kind != "int")
        per_q = per_q[:nqt]
        nqt = len(per_q)
        assert 0 < off and off + kp <= k and nqt <= qt and kp <= kpass
        mem = np.full((n_lists, qt, kpass), POISON, dtype=U64)
        mem[:, :nqt, :kp] = per_q.transpose(1, 0, 2)
        blank_D = np.full((qt, k), ISENT, dtype=np.int32) if kind == "int" else np.full((qt, k), -1234.5, dtype=np.float32)
        D, I, lo = dev(blank_D), dev(np.full((qt, k), ISENT, dtype=np.int64)), dev(np.full(qt, SENT, dtype=U64))
        fn = lib.chk_pass_merge_i32 if kind == "int" else lib.chk_pass_merge_f32
        run(fn, dev(mem), qt, kpass, n_lists, nqt, kp, D, I, lo, k, off, ip)
        D, I, lo = host(D), host(I), host(lo, U64)
        want_D, want_I, want_lo = blank_D.copy(), np.full((qt, k), ISENT, dtype=np.int64), np.full(qt, SENT, dtype=U64)
        for q in range(nqt):
            res = sr.padded(sr.smallest(per_q[q], kp), kp)
            pad = res == PAD
            if kind == "int":  # the key's high word is the distance + 1
                d = ((res >> U64(32)).astype(np.uint32) - np.uint32(1)).view(np.int32)
                want_D[q, off:off + kp] = np.where(pad, INT_MAX, d)
                want_I[q, off:off + kp] = np.where(pad, -1, (res & U64(0xFFFFFFFF)).astype(np.int64))
            else:
                want_D[q, off:off + kp], want_I[q, off:off + kp] = keycodec.decode(res, IP if ip else L2)
            want_lo[q] = PAD if pad[-1] else res[-1] + U64(1)
        tag = f"{kind} n_lists={n_lists} nqt={nqt} kp={kp} k={k} off={off} ({names[:nqt]})"
        assert np.array_equal(I, want_I), tag
        assert np.array_equal(D.view(np.uint32), want_D.view(np.uint32)), tag
        assert np.array_equal(lo, want_lo), tag
