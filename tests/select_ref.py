"""numpy reference models and case generators for the selection and merge primitives of csrc/ (ise_select.hpp,
ise_merge.hpp, ise_cand.hpp), as tests/native/select_harness.hip launches them (tests only).

Everything is integer-exact: the reference is ``np.sort`` on uint64 and nothing has a tolerance.  The generators are
deterministic (every case derives its seed from its own parameters) and every case holds unique keys strictly between
0 and PAD, as the headers require; no key equals SENT, the value the outputs are pre-filled with.
"""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
SENT = np.uint64(0xDEADBEEFDEADBEEF)  # what the tests pre-fill key outputs with
ISENT = -12345  # ... and int outputs

# constants of the headers, restated
MERGE_THREADS, MERGE_LISTS_MAX, MERGE_FAST_K, MERGE_PRE, MERGE_WAVES = 512, 1024, 40, 8, 8
CAND_WAVES, CAND_CAP, CAND_KPASS, CAND_CUT_MAX = 4, 128, 32, 48

U64 = np.uint64


# ---------------------------------------------------------------- models
def smallest(keys, k):
    """The real keys sorted, then the first k."""
    keys = np.asarray(keys, dtype=U64).ravel()
    return np.sort(keys[keys != PAD])[:k]


def padded(keys, k):
    out = np.full(k, PAD, dtype=U64)
    out[:len(keys)] = keys
    return out


def check_select(inp, n, k, dst, nw, kth, sentinel=SENT):
    """wave_select on the registers loaded from inp[0 .. n): dst, nw, kth as the harness left them."""
    real = inp[:n][inp[:n] != PAD]
    want = np.sort(real)[:k]
    assert nw == min(k, len(real)), f"count {nw}, want {min(k, len(real))}"
    assert np.array_equal(dst[:nw], want), "the sorted k smallest"
    assert (dst[nw:] == sentinel).all(), f"a slot at or beyond dst[{nw}] was written"
    if nw == k:
        assert kth == want[k - 1], "kth is the k-th smallest"
    else:
        assert kth == sentinel, "kth written although fewer than k keys were"


def check_cut(inp, n, kmin, kmax, dst, cnt, cut, sentinel=SENT):
    """wave_cut on the registers loaded from inp[0 .. n)."""
    real = np.sort(inp[:n][inp[:n] != PAD])
    if len(real) > kmax:
        assert kmin <= cnt <= kmax, f"count {cnt} outside [{kmin}, {kmax}]"
    else:
        assert cnt == len(real), f"count {cnt}, want all {len(real)}"
    assert np.array_equal(np.sort(dst[:cnt]), real[:cnt]), "the kept keys are the cnt smallest"
    assert (dst[cnt:] == sentinel).all(), f"a slot at or beyond dst[{cnt}] was written"
    if cnt >= kmin:
        assert cnt > 0 and cut == real[cnt - 1], "cut is the largest kept key"
    else:
        assert cut == sentinel, "cut written although fewer than kmin keys were kept"


def merge_model(lists, k):
    """(result, need_full) of merge_waves over ``lists`` ([n_lists][<= k], each sorted, PAD allowed behind the keys).

    The path is merge_waves' own rule restated: list l sits in wave l % 8 (lane (l % 512) / 8, slot l / 512); each wave
    collects its pre = min(k, 8) smallest heads; T is the k-th smallest collected key, or PAD; the full path runs iff
    pre < k and some wave's 8th collected key is < T.  The result is plain smallest(all keys, k): the model never
    decides the expected result, only the expected path."""
    lists = [np.asarray(l, dtype=U64)[:k] for l in lists]
    pre = min(k, MERGE_PRE)
    collected = []
    for w in range(MERGE_WAVES):
        mine = [l for i, l in enumerate(lists) if i % MERGE_WAVES == w]
        got = smallest(np.concatenate(mine), pre) if mine else np.zeros(0, dtype=U64)
        collected.append(padded(got, pre))
    allc = smallest(np.concatenate(collected), k)
    T = allc[k - 1] if len(allc) >= k else PAD
    need_full = int(pre < k and any(c[MERGE_PRE - 1] < T for c in collected))
    every = np.concatenate(lists) if lists else np.zeros(0, dtype=U64)
    return smallest(every, k), need_full


def merge_model_batch(lists, k):
    """merge_model for lists [ncases][n_lists][k] at once: (result [ncases][k] PAD padded, need_full [ncases])."""
    lists = np.asarray(lists, dtype=U64)
    nc, nl, kk = lists.shape
    assert kk == k
    pre = min(k, MERGE_PRE)
    coll = np.full((nc, MERGE_WAVES, pre), PAD, dtype=U64)
    for w in range(min(MERGE_WAVES, nl)):
        coll[:, w, :] = np.sort(lists[:, w::MERGE_WAVES, :].reshape(nc, -1), axis=1)[:, :pre]
    allc = np.sort(coll.reshape(nc, -1), axis=1)
    T = allc[:, k - 1] if allc.shape[1] >= k else np.full(nc, PAD, dtype=U64)
    if pre < k:
        need = (coll[:, :, MERGE_PRE - 1] < T[:, None]).any(axis=1).astype(np.int32)
    else:
        need = np.zeros(nc, dtype=np.int32)
    res = np.sort(lists.reshape(nc, -1), axis=1)[:, :k]
    if res.shape[1] < k:
        res = np.concatenate([res, np.full((nc, k - res.shape[1]), PAD, dtype=U64)], axis=1)
    return res, need


def cand_model(keys, lo, kp):
    """The sorted kp smallest keys >= lo of a query's stream, PAD behind."""
    keys = np.asarray(keys, dtype=U64).ravel()
    keys = keys[(keys != PAD) & (keys >= U64(lo))]
    return padded(np.sort(keys)[:kp], kp)


# ---------------------------------------------------------------- key families
FAMILIES = ("rand", "tiedhi", "eqlo", "extremes")


def _draw_unique(rng, count, lo, hi):
    """count distinct integers of [lo, hi), in random order."""
    got = np.zeros(0, dtype=U64)
    while len(got) < count:
        more = rng.integers(lo, hi, size=2 * count + 16, dtype=U64)
        got = np.unique(np.concatenate([got, more]))
    return rng.permutation(got)[:count]


def make_keys(rng, count, family):
    """count unique keys strictly between 0 and PAD, none equal to SENT, in random order.
    rand: random 64-bit keys.  tiedhi: one to three distinct high words, distinct low words -- what equal distances
    look like, so a comparison must use all 64 bits.  eqlo: one low word, distinct high words.  extremes: random, with
    1 and PAD - 1 among them."""
    if count == 0:
        return np.zeros(0, dtype=U64)
    if family == "rand" or family == "extremes":
        keys = _draw_unique(rng, count, 2, 0xFFFFFFFFFFFFFFFE)
        if family == "extremes":
            keys[0] = U64(1)
            if count > 1:
                keys[1] = PAD - U64(1)
            keys = rng.permutation(keys)
    elif family == "tiedhi":
        his = _draw_unique(rng, int(rng.integers(1, 4)), 1, 0xFFFFFFFE)
        lows = _draw_unique(rng, count, 0, 1 << 32)
        keys = (his[rng.integers(0, len(his), size=count)] << U64(32)) | lows
    elif family == "eqlo":
        low = U64(rng.integers(0, 1 << 32))
        keys = (_draw_unique(rng, count, 1, 0xFFFFFFFE) << U64(32)) | low
    else:
        raise ValueError(family)
    keys = keys.astype(U64)
    assert len(np.unique(keys)) == count and (keys > 0).all() and (keys < PAD).all() and (keys != SENT).all()
    return keys


def score_keys(rng, count, tied=False):
    """count unique ascending keys whose high words are ord() of finite positive floats (so that a decoded distance is
    an ordinary number): a random walk up from ord(0.0) << 32; tied: steps so short that long runs share a high word."""
    gaps = rng.integers(1, (1 << 20) if tied else (1 << 40), size=count, dtype=U64)
    return (U64(0x80000000) << U64(32)) + np.cumsum(gaps, dtype=U64)


# ---------------------------------------------------------------- wave_select / wave_cut cases
PLACEMENTS_ANY = ("scatter", "asc", "desc", "segments")  # possible for every nreal <= n
PLACEMENTS_SHAPED = ("lastreg", "lanes7", "lane63", "onepereg")  # their capacity depends on n
SEL_K = (1, 2, 8, 16, 31, 32, 36, 48, 64)
CUT_WINDOWS = ((16, 16), (32, 32), (1, 5), (10, 19), (32, 48), (36, 48), (16, 32))


def placement_capacity(placement, n):
    return {"lastreg": min(n, 64), "lanes7": 57 * (n // 64), "lane63": n // 64, "onepereg": n // 64}.get(placement, n)


def place(rng, keys, kpl, n, placement):
    """in[64 kpl]: element i sits in lane i % 64, register i // 64; the keys at the placement's slots (< n), PAD elsewhere."""
    nreal = len(keys)
    assert n % 64 == 0 and 0 <= n <= 64 * kpl and nreal <= placement_capacity(placement, n)
    out = np.full(64 * kpl, PAD, dtype=U64)
    idx = np.arange(n)
    if placement == "scatter":
        slots = rng.permutation(idx)[:nreal]
    elif placement == "asc":  # ascending by lane, register after register
        slots, keys = idx[:nreal], np.sort(keys)
    elif placement == "desc":
        slots, keys = idx[:nreal], np.sort(keys)[::-1]
    elif placement == "segments":  # contiguous from 0 in every 128-key segment, holes between: what fold selects from
        seg = rng.permutation(idx // 128)[:nreal]  # a random segment for every key, no segment over its size
        cnt = np.bincount(seg, minlength=(n + 127) // 128)
        slots = np.concatenate([np.zeros(0, dtype=np.int64)] + [128 * s + np.arange(c) for s, c in enumerate(cnt)])
    elif placement == "lastreg":  # only the last loaded register
        slots = rng.permutation(np.arange(n - 64, n))[:nreal] if n else idx
    elif placement == "lanes7":  # only lanes >= 7
        slots = rng.permutation(idx[idx % 64 >= 7])[:nreal]
    elif placement == "lane63":
        slots = rng.permutation(idx[idx % 64 == 63])[:nreal]
    elif placement == "onepereg":  # one key in each loaded register, in a lane of its own
        slots = (np.arange(n // 64) * 64 + rng.integers(0, 64, size=n // 64))[:nreal]
    else:
        raise ValueError(placement)
    out[slots] = keys
    return out


def counts_for(n, k, kpl):
    """nreal in {0, 1, k-1, k, k+1, 40, 41, 64e-1, 64e, 64e+1 .., 64 kpl}, those that fit n."""
    c = {0, 1, k - 1, k, k + 1, 40, 41, 64 * kpl}
    for e in range(1, kpl + 1):
        c |= {64 * e - 1, 64 * e, 64 * e + 1}
    return sorted(x for x in c if 0 <= x <= n)


def _case_rng(*parts):
    return np.random.default_rng([abs(hash_int(p)) for p in parts])


def hash_int(p):
    """A stable integer of an int or a short ASCII name (Python's own hash of a str changes from run to run)."""
    if isinstance(p, (int, np.integer)):
        return int(p)
    return int.from_bytes(str(p).encode(), "little") % (1 << 62)


def window_cases(kpl, windows):
    """Cases of one wave-level instantiation: dicts with inp [64 kpl], n, lo, hi (k = lo = hi for wave_select) and the
    names of their family and placement.  Every (n, window, nreal) of the grid appears once, its family and placement
    taken in rotation; every shaped placement appears with every family at the smallest and the largest n."""
    cases = []

    def add(n, lo, hi, nreal, family, placement):
        rng = _case_rng(kpl, n, lo, hi, nreal, family, placement)
        keys = make_keys(rng, nreal, family)
        cases.append(dict(inp=place(rng, keys, kpl, n, placement), n=n, lo=lo, hi=hi, nreal=nreal, family=family,
                          placement=placement))

    i = 0
    for n in range(0, 64 * kpl + 1, 64):
        for lo, hi in windows:
            for nreal in sorted(set(counts_for(n, hi, kpl)) | {x for x in (lo - 1, lo, lo + 1) if 0 <= x <= n}):
                add(n, lo, hi, nreal, FAMILIES[i % 4], PLACEMENTS_ANY[(i // 4) % 4])
                i += 1
    for placement in PLACEMENTS_SHAPED:
        for family in FAMILIES:
            for lo, hi in windows:
                for n in sorted({64, 64 * kpl}):
                    cap = placement_capacity(placement, n)
                    for nreal in sorted({cap, min(cap, hi + 1), min(cap, 41)}):
                        add(n, lo, hi, nreal, family, placement)
    return cases


def select_cases(kpl):
    return window_cases(kpl, [(k, k) for k in SEL_K])


def cut_cases(kpl):
    return window_cases(kpl, CUT_WINDOWS)


# ---------------------------------------------------------------- block_topk_u64 cases
TOPK_N = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
TOPK_K = (1, 10, 32, 64)
TOPK_ORDERS = ("random", "asc", "desc")  # asc: every winner in wave 0's slice; desc: in the last wave's


def topk_cases():
    cases = []
    for n in TOPK_N:
        for k in TOPK_K:
            for family in FAMILIES:
                for order in TOPK_ORDERS:
                    rng = _case_rng("topk", n, k, family, order)
                    keys = make_keys(rng, n, family)
                    if order != "random":
                        keys = np.sort(keys) if order == "asc" else np.sort(keys)[::-1]
                    cases.append(dict(keys=keys.copy(), n=n, k=k, family=family, order=order))
    return cases


# ---------------------------------------------------------------- merge cases
MERGE_N_LISTS = (1, 2, 8, 9, 64, 65, 511, 512, 513, 1023, 1024)
MWAVES_K = (1, 2, 8, 9, 16, 32, 36, 40)


def lists_from_owner(keys, owner, n_lists, k):
    """[n_lists][k]: list l holds the keys whose owner is l, ascending, PAD behind.  At most k keys per list."""
    keys, owner = np.asarray(keys, dtype=U64), np.asarray(owner, dtype=np.int64)
    out = np.full((n_lists, k), PAD, dtype=U64)
    order = np.lexsort((keys, owner))
    keys, owner = keys[order], owner[order]
    first = np.searchsorted(owner, np.arange(n_lists))
    pos = np.arange(len(keys)) - first[owner] if len(keys) else np.zeros(0, dtype=np.int64)
    assert (pos < k).all(), "a list was given more than k keys"
    out[owner, pos] = keys
    return out


def _fill_rest(rng, room, want):
    """owners of up to `want` further keys: random lists with room left (room [n_lists], changed in place)."""
    slots = rng.permutation(np.repeat(np.arange(len(room)), room))[:want]
    np.subtract.at(room, slots, 1)
    return slots


def merge_case(n_lists, k, placement, family, seed=0):
    """One merge case: lists [n_lists][k] or None where the placement is impossible at this (n_lists, k).
    The k smallest keys of the case are its winners; the placement says which lists own them:
      spread       winners and the rest on random lists
      list:<l>     every winner in list l (l = -1: the last list)
      wave:<w>     every winner in lists of wave w (l = w mod 8), on random ones of them
      w8fast:<w>   exactly 8 winners in wave w, the largest winner among them (the wave's 8th key IS T: done), at most
                   7 in every other wave
      w8slow:<w>   exactly 8 winners in wave w, the largest winner elsewhere (the wave's 8th key is below T: the rule
                   cannot tell that the wave holds no 9th and takes the full path)
      w9:<w>       exactly 9 winners in wave w, at most 8 in every other wave: the fast path would lose one
      few          k - 1 real keys in total
      tiny         fewer real keys than min(k, 8) in total: no wave collects an 8th key
      holes        two lists in three are empty
      short        every list is shorter than k
    """
    rng = _case_rng("merge", n_lists, k, placement, family, seed)
    name, _, arg = placement.partition(":")
    waves = [np.arange(w, n_lists, MERGE_WAVES) for w in range(MERGE_WAVES)]
    live = np.ones(n_lists, dtype=bool)
    cap = k
    nwin = k
    if name == "holes":
        live = np.arange(n_lists) % 3 == 0
    if name == "short":
        if k == 1:
            return None
        cap = max(1, k // 4)
    room = np.where(live, cap, 0).astype(np.int64)
    if name == "few":
        total = k - 1
    elif name == "tiny":
        total = min(k, MERGE_PRE) - 1 if k > 1 else 0
    else:
        total = min(int(room.sum()), 3 * k + 2 * n_lists)
    nwin = min(nwin, total)
    keys = np.sort(make_keys(rng, total, family))
    owner = np.full(total, -1, dtype=np.int64)

    def give(which, lists_allowed):
        """winners `which` (indices into keys) go to random lists of lists_allowed with room"""
        slots = rng.permutation(np.repeat(lists_allowed, room[lists_allowed]))[:len(which)]
        if len(slots) < len(which):
            return False
        owner[which] = slots
        np.subtract.at(room, slots, 1)
        return True

    win = np.arange(nwin)
    if name in ("spread", "few", "tiny", "holes", "short"):
        ok = give(win, np.flatnonzero(live))
    elif name == "list":
        l = int(arg) if int(arg) >= 0 else n_lists - 1
        ok = l < n_lists and nwin == k and give(win, np.array([l]))
    elif name == "wave":
        w = int(arg)
        ok = len(waves[w]) > 0 and nwin == k and give(win, waves[w])
    elif name in ("w8fast", "w8slow", "w9"):
        w = int(arg)
        inw = 9 if name == "w9" else 8
        others = [v for v in range(MERGE_WAVES) if v != w and len(waves[v])]
        per_other = 7 if name == "w8fast" else 8
        ok = nwin == k and k >= inw and len(waves[w]) > 0 and (k - inw) <= per_other * len(others)
        if name == "w8slow":
            ok = ok and k > inw
        if ok:
            body = rng.permutation(k - 1)  # every winner but the largest
            if name == "w8fast":
                mine, rest = np.concatenate([body[:inw - 1], [k - 1]]), body[inw - 1:]
            elif name == "w8slow":
                mine, rest = body[:inw], np.concatenate([body[inw:], [k - 1]])
            else:
                body = rng.permutation(k)
                mine, rest = body[:inw], body[inw:]
            ok = give(mine, waves[w])
            quota = np.zeros(MERGE_WAVES, dtype=np.int64)
            for j in range(len(rest)):  # deal the rest round-robin over the other waves, per_other each at most
                quota[others[j % len(others)]] += 1
            ok = ok and (quota <= per_other).all()
            at = 0
            for v in others:
                ok = ok and give(rest[at:at + quota[v]], waves[v])
                at += quota[v]
    else:
        raise ValueError(placement)
    if not ok:
        return None
    owner[nwin:] = _fill_rest(rng, room, total - nwin)
    assert (owner >= 0).all()
    return lists_from_owner(keys, owner, n_lists, k)


def merge_placements(n_lists, k):
    names = ["spread", "holes", "short", "few", "tiny"]
    names += [f"list:{l}" for l in sorted({0, 7, 8, 511, 512}) if l < n_lists - 1] + ["list:-1"]
    names += [f"wave:{w}" for w in (0, 3, 7)]
    names += [f"{p}:{w}" for p in ("w8fast", "w8slow", "w9") for w in (0, 5)]
    return names


def merge_family_cases(n_lists, k):
    """The cases of one (n_lists, k) launch: (names, lists [ncases][n_lists][k])."""
    names, lists = [], []
    for i, placement in enumerate(merge_placements(n_lists, k)):
        for family in (FAMILIES[i % 4], "tiedhi") if placement == "spread" else (FAMILIES[i % 4],):
            got = merge_case(n_lists, k, placement, family)
            if got is not None:
                names.append(f"{placement}/{family}")
                lists.append(got)
    return names, np.stack(lists)


# ---------------------------------------------------------------- CandBuf cases
CAND_TILES_PER_WAVE = (1, 2, 5, 8, 40)
CAND_ORDERS = ("asc", "desc", "random", "tiedhi")


def cand_stream(ntiles, nqt, order, partial, seed):
    """keys [nqt][ntiles * 64] of one case: every query its own keys.  asc: one fill, then every key is rejected by the
    threshold; desc: every tile beats the threshold, so a cut follows every tile; partial: the stream's last tiles end
    early (PAD lanes), query q's by 1 + 5 q lanes."""
    rng = _case_rng("cand", ntiles, nqt, order, int(partial), seed)
    n = ntiles * 64
    out = np.full((nqt, n), PAD, dtype=U64)
    for q in range(nqt):
        keys = make_keys(rng, n, "tiedhi" if order == "tiedhi" else "rand")
        if order == "asc":
            keys = np.sort(keys)
        elif order == "desc":
            keys = np.sort(keys)[::-1]
        out[q] = keys
        if partial and n:
            # tile t is keys [64 t, 64 t + 64): the last min(4, ntiles) tiles (one per wave) lose their last lanes
            cutoff = min(63, 1 + 5 * q)
            for t in range(max(0, ntiles - CAND_WAVES), ntiles):
                out[q, 64 * t + 64 - cutoff:64 * t + 64] = PAD
    return out
