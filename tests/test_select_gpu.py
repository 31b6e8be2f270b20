"""GPU tests of the selection and merge primitives every search path ends in -- wave_select, wave_cut, block_topk_u64
(csrc/ise_select.hpp), merge_waves, merge_rounds, merge_kernel, pass_merge_kernel (csrc/ise_merge.hpp) and CandBuf
(csrc/ise_cand.hpp) -- called directly through tests/native/select_harness.hip on crafted key sets, so that the test
decides which lane, register, wave and list every key sits in.  The reference is np.sort on uint64
(tests/select_ref.py); every comparison is bit for bit.  The merge_waves test also reads back the block's need_full
flag and compares it with the path model: it proves which of the two paths ran.

The harness is built by `make -C image-search-engine_amd/csrc` (target libise_select_check.so); without it the tests
fail, they do not skip."""
import ctypes
import os

import numpy as np
import pytest

from tests import keycodec
from tests import select_ref as sr
from tests.select_ref import ISENT, PAD, SENT, U64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "image-search-engine_amd", "csrc", "libise_select_check.so")
INT_MAX = 2**31 - 1
FLT_MAX = np.float32(np.finfo(np.float32).max)
L2, IP = 1, 0

_vp, _int, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
PROTOTYPES = {
    "chk_sel": [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp],
    "chk_cut": [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "chk_topk": [_int, _vp, _int, _vp, _vp, _vp],
    "chk_mwaves": [_int, _vp, _int, _int, _vp, _vp],
    "chk_pass_merge_f32": [_vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int],
    "chk_pass_merge_i32": [_vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int],
    "chk_merge": [_vp, _ll, _ll, _int, _int, _int, _int, _int, _vp, _vp, _vp],
    "chk_cand": [_int, _int, _vp, _int, _int, _int, _vp, _vp],
}


@pytest.fixture(scope="module")
def lib():
    import torch  # first: the harness binds to the HIP runtime torch has loaded

    assert torch.cuda.is_available()
    if not os.path.exists(LIB_PATH):
        pytest.fail("csrc/libise_select_check.so is missing: build it with "
                    "`make -C image-search-engine_amd/csrc libise_select_check.so`")
    handle = ctypes.CDLL(LIB_PATH)
    for name, args in PROTOTYPES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _int, args
    return handle


def dev(a):
    """numpy (uint64 / int32 / ..) -> a CUDA tensor of the same bits"""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == U64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(U64) if a.dtype == np.int64 and dtype is U64 else a


def run(fn, *args):
    """launch on the null stream (torch's default stream), wait, and take any error the kernel left"""
    import torch

    rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    assert rc == 0, f"launch failed: hip error {rc}"
    torch.cuda.synchronize()


def report(failures, total):
    assert not failures, f"{len(failures)} of {total} cases failed; the first: " + " | ".join(failures[:5])


# ---------------------------------------------------------------- wave_select, wave_cut
@pytest.mark.parametrize("kpl", [1, 2, 4, 5, 8, 16])
def test_wave_select(lib, kpl):
    cases = sr.select_cases(kpl)
    nc = len(cases)
    inp = np.stack([c["inp"] for c in cases])
    n = np.array([c["n"] for c in cases], dtype=np.int32)
    k = np.array([c["hi"] for c in cases], dtype=np.int32)
    assert inp.shape == (nc, 64 * kpl) and (n % 64 == 0).all() and (n <= 64 * kpl).all() and (k >= 1).all() and (k <= 64).all()
    dst = dev(np.full((nc, 64 * kpl + 8), SENT, dtype=U64))
    nw = dev(np.full(nc, ISENT, dtype=np.int32))
    kth = dev(np.full(nc, SENT, dtype=U64))
    run(lib.chk_sel, kpl, nc, dev(inp), dev(n), dev(k), dst, nw, kth)
    dst, nw, kth = host(dst, U64), host(nw), host(kth, U64)
    failures = []
    for i, c in enumerate(cases):
        try:
            sr.check_select(c["inp"], c["n"], c["hi"], dst[i], int(nw[i]), kth[i])
        except AssertionError as e:
            failures.append(f"n={c['n']} k={c['hi']} nreal={c['nreal']} {c['family']} {c['placement']}: {e}")
    report(failures, nc)


@pytest.mark.parametrize("kpl", [1, 2, 4])
def test_wave_cut(lib, kpl):
    cases = sr.cut_cases(kpl)
    nc = len(cases)
    inp = np.stack([c["inp"] for c in cases])
    n = np.array([c["n"] for c in cases], dtype=np.int32)
    kmin = np.array([c["lo"] for c in cases], dtype=np.int32)
    kmax = np.array([c["hi"] for c in cases], dtype=np.int32)
    assert inp.shape == (nc, 64 * kpl) and (n % 64 == 0).all() and (n <= 64 * kpl).all()
    assert (kmin >= 1).all() and (kmin <= kmax).all() and (kmax <= 64).all()
    dst = dev(np.full((nc, 64 * kpl + 8), SENT, dtype=U64))
    cnt = dev(np.full(nc, ISENT, dtype=np.int32))
    cut = dev(np.full(nc, SENT, dtype=U64))
    run(lib.chk_cut, kpl, nc, dev(inp), dev(n), dev(kmin), dev(kmax), dst, cnt, cut)
    dst, cnt, cut = host(dst, U64), host(cnt), host(cut, U64)
    failures = []
    for i, c in enumerate(cases):
        try:
            sr.check_cut(c["inp"], c["n"], c["lo"], c["hi"], dst[i], int(cnt[i]), cut[i])
        except AssertionError as e:
            failures.append(f"n={c['n']} window=({c['lo']},{c['hi']}) nreal={c['nreal']} {c['family']} {c['placement']}: {e}")
    report(failures, nc)


# ---------------------------------------------------------------- block_topk_u64
def test_block_topk(lib):
    cases = sr.topk_cases()
    nc, stride = len(cases), 4096
    inp = np.full((nc, stride), PAD, dtype=U64)
    for i, c in enumerate(cases):
        inp[i, :c["n"]] = c["keys"]
    n = np.array([c["n"] for c in cases], dtype=np.int32)
    k = np.array([c["k"] for c in cases], dtype=np.int32)
    assert (n <= stride).all() and (k >= 1).all() and (k <= 64).all()
    out = dev(np.full((nc, 64), SENT, dtype=U64))
    run(lib.chk_topk, nc, dev(inp), stride, dev(n), dev(k), out)
    out = host(out, U64)
    failures = []
    for i, c in enumerate(cases):
        want = np.full(64, SENT, dtype=U64)
        want[:c["k"]] = sr.padded(sr.smallest(c["keys"], c["k"]), c["k"])
        if not np.array_equal(out[i], want):
            failures.append(f"n={c['n']} k={c['k']} {c['family']} {c['order']}: first difference at "
                            f"{int(np.flatnonzero(out[i] != want)[0])}")
    report(failures, nc)


# ---------------------------------------------------------------- merge_waves, with the path it took
@pytest.mark.parametrize("n_lists", sr.MERGE_N_LISTS)
def test_merge_waves(lib, n_lists):
    failures, total = [], 0
    for k in sr.MWAVES_K:
        names, lists = sr.merge_family_cases(n_lists, k)
        nc = len(names)
        assert lists.shape == (nc, n_lists, k) and n_lists <= sr.MERGE_LISTS_MAX and k <= sr.MERGE_FAST_K
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
        if k > sr.MERGE_PRE:  # both paths demonstrably ran, by the kernel's own flag
            assert full.min() == 0 and full.max() == 1, f"k={k}: flags {full.tolist()}"
        else:
            assert (full == 0).all()
        total += nc
    report(failures, total)


# ---------------------------------------------------------------- helpers of the kernels that decode keys
def rekey(lists, rng, tied):
    """The same lists with their keys replaced, order kept, by keys that decode to finite distances (score_keys)."""
    out = lists.copy()
    mask = out != PAD
    vals = out[mask]
    new = np.empty_like(vals)
    new[np.argsort(vals, kind="stable")] = sr.score_keys(rng, len(vals), tied)
    out[mask] = new
    return out


def query_lists(n_lists, k, nq, seed, float_keys):
    """[nq][n_lists][k]: one merge case per query, the placements of the (n_lists, k) family in rotation."""
    places = sr.merge_placements(n_lists, k)
    rng = np.random.default_rng([n_lists, k, nq, seed])
    out, j = [], seed
    while len(out) < nq:
        got = sr.merge_case(n_lists, k, places[j % len(places)], sr.FAMILIES[j % 4], seed)
        j += 1
        if got is not None:
            out.append(rekey(got, rng, tied=len(out) % 2 == 1) if float_keys else got)
    return np.stack(out)


# ---------------------------------------------------------------- pass_merge_kernel<float | int>
PASS_SHAPES = [  # n_lists, nqt, kp, k, off
    (1, 1, 1, 1, 0), (9, 16, 10, 70, 0), (65, 5, 32, 70, 32), (512, 16, 32, 96, 64), (1024, 3, 6, 70, 64),
    (513, 2, 32, 32, 0), (8, 16, 1, 40, 39),
]


@pytest.mark.parametrize("kind", ["float_l2", "float_ip", "int"])
def test_pass_merge(lib, kind):
    qt, kpass = 16, sr.CAND_KPASS
    saw_pad_floor = saw_key_floor = saw_pad_result = False
    for n_lists, nqt, kp, k, off in PASS_SHAPES:
        per_q = query_lists(n_lists, kp, nqt, 7, kind != "int")  # [nqt][n_lists][kp]
        lists = np.full((n_lists, qt, kpass), PAD, dtype=U64)  # as the scan's blocks leave them
        lists[:, :nqt, :kp] = per_q.transpose(1, 0, 2)
        assert off + kp <= k and nqt <= qt and kp <= kpass
        ip = int(kind == "float_ip")
        blank_D = np.full((qt, k), ISENT, dtype=np.int32) if kind == "int" else np.full((qt, k), -1234.5, dtype=np.float32)
        D = dev(blank_D)
        I = dev(np.full((qt, k), ISENT, dtype=np.int64))
        lo = dev(np.full(qt, SENT, dtype=U64))
        fn = lib.chk_pass_merge_i32 if kind == "int" else lib.chk_pass_merge_f32
        run(fn, dev(lists), qt, kpass, n_lists, nqt, kp, D, I, lo, k, off, ip)
        D, I, lo = host(D), host(I), host(lo, U64)
        tag = f"{kind} n_lists={n_lists} nqt={nqt} kp={kp} k={k} off={off}"
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
            saw_pad_floor, saw_key_floor = saw_pad_floor or bool(pad[-1]), saw_key_floor or not pad[-1]
            saw_pad_result = saw_pad_result or bool(pad.any() and not pad.all())
        assert np.array_equal(I, want_I), tag
        assert np.array_equal(D.view(np.uint32), want_D.view(np.uint32)), tag
        assert np.array_equal(lo, want_lo), tag
        if kind != "int":  # unfilled float results are +-FLT_MAX by ip
            unfilled = want_I[:nqt, off:off + kp] == -1
            assert (D[:nqt, off:off + kp][unfilled] == (-FLT_MAX if ip else FLT_MAX)).all(), tag
    assert saw_pad_floor and saw_key_floor and saw_pad_result, "the shapes reach both kinds of floor and a part-filled pass"


# ---------------------------------------------------------------- merge_kernel<false>, the qt = 16 layout
@pytest.mark.parametrize("n_lists", [1, 9, 65, 512, 1024])
def test_merge_kernel_query_tiles(lib, n_lists):
    """Lists laid out as the selector scan and IVF leave them: [query tile][list][16 queries][k].  k <= 40 goes
    through merge_waves, larger k through merge_rounds."""
    qt, nq = 16, 19  # two tiles, the second with three queries
    for j, k in enumerate((1, 9, 40, 41, 64)):
        metric = (L2, IP)[j % 2]
        per_q = query_lists(n_lists, k, nq, 3, True)  # [nq][n_lists][k]
        ntile = -(-nq // qt)
        lists = np.full((ntile, n_lists, qt, k), PAD, dtype=U64)
        for q in range(nq):
            lists[q // qt, :, q % qt, :] = per_q[q]
        keys_out = dev(np.full((nq, k), SENT, dtype=U64))
        D = dev(np.full((nq, k), -1234.5, dtype=np.float32))
        I = dev(np.full((nq, k), ISENT, dtype=np.int64))
        run(lib.chk_merge, dev(lists), qt * k, n_lists * qt * k, qt, n_lists, nq, k, metric, keys_out, D, I)
        want = np.stack([sr.padded(sr.smallest(per_q[q], k), k) for q in range(nq)])
        want_D, want_I = keycodec.decode(want, metric)
        tag = f"n_lists={n_lists} k={k} metric={metric}"
        assert np.array_equal(host(keys_out, U64), want), tag
        assert np.array_equal(host(I), want_I), tag
        assert np.array_equal(host(D).view(np.uint32), want_D.view(np.uint32)), tag


# ---------------------------------------------------------------- CandBuf: cut, make_room, fold
CAND_KINDS = {"pq16": (0, 16), "pq2": (1, 2), "sq16": (2, 16), "sq8": (3, 8)}  # harness variant, QT


def cand_launches(qt):
    """(tiles in the stream, queries, kp): 1, 2, 5, 8 and 40 tiles per wave; a stream of 4 t - 1 or 4 t - 3 tiles leaves
    some waves a tile short (at t = 1: with none)."""
    small = max(1, qt // 2 - 1)
    out = []
    for t in (1, 2, 5, 8):
        out += [(4 * t, qt, 32), (4 * t - 1, small, 10), (4 * t - 3, qt, 1), (4 * t, 1, 10)]
    out += [(160, qt, 32), (159, small, 10), (157, 1, 1)]
    return out


@pytest.mark.parametrize("kind", list(CAND_KINDS))
def test_cand_buffer(lib, kind):
    which, qt = CAND_KINDS[kind]
    failures, total = [], 0
    for ntiles, nqt, kp in cand_launches(qt):
        assert 1 <= nqt <= qt and 1 <= kp <= sr.CAND_KPASS
        combos = [(o, p, l) for o in sr.CAND_ORDERS for p in (False, True) for l in ("zero", "mid", "pad")]
        if ntiles > 100:  # the long streams: every order once, the floor kinds in rotation
            combos = [(o, i % 2 == 1, ("mid", "zero", "mid", "zero")[i]) for i, o in enumerate(sr.CAND_ORDERS)]
        keys = np.stack([sr.cand_stream(ntiles, nqt, o, p, which) for o, p, _ in combos])  # [nc][nqt][ntiles * 64]
        nc = len(combos)
        lo = np.full((nc, qt), SENT, dtype=U64)  # entries at or beyond nqt are never read
        for i, (_, _, lk) in enumerate(combos):
            for q in range(nqt):
                real = np.sort(keys[i, q][keys[i, q] != PAD])
                mid = real[len(real) // 2]
                # "mid": a key of the stream itself; queries take the three kinds in rotation
                lo[i, q] = {"zero": U64(0), "pad": PAD, "mid": (mid, U64(0), PAD)[q % 3]}[lk]
        lists = dev(np.full((nc, qt, sr.CAND_KPASS), SENT, dtype=U64))
        run(lib.chk_cand, which, nc, dev(keys), ntiles, nqt, kp, dev(lo), lists)
        lists = host(lists, U64)
        for i, (o, p, lk) in enumerate(combos):
            want = np.full((qt, sr.CAND_KPASS), SENT, dtype=U64)
            for q in range(nqt):
                want[q, :kp] = sr.cand_model(keys[i, q], lo[i, q], kp)
            if not np.array_equal(lists[i], want):
                q, s = [int(x[0]) for x in np.nonzero(lists[i] != want)]
                failures.append(f"ntiles={ntiles} nqt={nqt} kp={kp} {o} partial={p} lo={lk}: query {q} slot {s}")
        total += nc
    report(failures, total)
