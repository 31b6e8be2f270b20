"""GPU tests of the exact re-rank (csrc/ise_exact.hpp, rerank_block) in both of its kernels -- rerank_kernel (4 waves,
candidates in memory) and merge_kernel<true> (8 waves, candidates merged from lists) -- on crafted rows, queries and
candidate keys, through tests/native/rerank_harness.hip.  The re-rank asks for the rows of a group of candidates two
column blocks ahead (a ring of 2 x 4 row loads per lane); the shapes stand on every edge of that: rows of one column
block, of two (the ring exactly full), of more (the ring turns), padded rows, lists shorter than a group, longer than
a wave's 4, longer than 64 (the block-wide sort), counts of 0, 1, kc - 1 and kc.

The reference (tests/rerank_ref.py) restates d() in the kernel's order with exactly emulated fused multiply-adds:
every comparison is bit for bit.  Integer-valued rows make the order irrelevant and check the restatement itself; the
exact fallback scan (ISE_FORCE_EXACT=1) must report the same distances for the same rows."""
import ctypes
import os

import numpy as np
import pytest

from tests import keycodec
from tests import rerank_ref as rr
from tests import select_ref as sr
from tests.rerank_ref import FLT_MAX, PAD, U64
from tests.test_select_gpu import dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "image-search-engine_amd", "csrc", "libise_rerank_check.so")
L2 = 1
SEQ = 7
DIMS = (4, 60, 256, 260, 512, 768, 1024, 2048)
KCS = (1, 5, 14, 32, 36, 40, 68)
N_LISTS = 37

_vp, _int, _ll, _u = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint
_COMMON = [_vp, _vp, _ll, _int, _int, _int, _int, _int, _u]
_TAIL = [_vp, _vp, _vp, _vp, _vp, _u, _vp, _int]


@pytest.fixture(scope="module")
def rlib():
    import torch  # first: the harness binds to the HIP runtime torch has loaded

    assert torch.cuda.is_available()
    if not os.path.exists(LIB_PATH):
        pytest.fail("csrc/libise_rerank_check.so is missing: build it with "
                    "`make -C image-search-engine_amd/csrc libise_rerank_check.so`")
    handle = ctypes.CDLL(LIB_PATH)
    handle.chk_rerank.restype, handle.chk_rerank.argtypes = _int, _COMMON + [_vp] + _TAIL
    handle.chk_merge_rerank.restype, handle.chk_merge_rerank.argtypes = _int, _COMMON + [_vp, _int] + _TAIL
    return handle


def spread_over_lists(keys_in, seed):
    """[n_lists][nq][kc]: every query's real keys dealt onto random lists, ascending in each, PAD behind."""
    nq, kc = keys_in.shape
    rng = np.random.default_rng([seed, nq, kc])
    out = np.full((N_LISTS, nq, kc), PAD, dtype=U64)
    for i in range(nq):
        real = keys_in[i][keys_in[i] != PAD]
        out[:, i, :] = sr.lists_from_owner(real, rng.integers(0, N_LISTS, len(real)), N_LISTS, kc)
    return out


def launch(rlib, kind, xbp, q, keys_in, k, n, id_base=0, tau=None, force_fail=False):
    """-> keys_out [nq][k], D, I, fl_state, fl_list [nq] as the kernel left them"""
    import torch

    nq, kc = keys_in.shape
    d, dp = q.shape[1], xbp.shape[1]
    xb_d = dev(xbp) if len(xbp) else torch.zeros(4, device="cuda")
    q_d, tau_d = dev(q), (dev(np.asarray(tau, dtype=np.float32)) if tau is not None else None)
    D = dev(np.full((nq, k), -1234.5, dtype=np.float32))
    I = dev(np.full((nq, k), sr.ISENT, dtype=np.int64))
    keys_out = dev(np.full((nq, k), sr.SENT, dtype=U64))
    fl_state, fl_list = dev(np.zeros(1, dtype=U64)), dev(np.full(nq, -1, dtype=np.int32))
    ids = (keys_in[keys_in != PAD] & U64(0xFFFFFFFF)).astype(np.int64) - id_base
    assert ((ids >= 0) & (ids < n)).all() and n <= len(xbp) or (n == 0 and not len(ids)), "every candidate names a row"
    head = [xb_d.data_ptr(), q_d.data_ptr(), n, d, dp, nq, k, kc, id_base]
    tail = [D.data_ptr(), I.data_ptr(), keys_out.data_ptr(), fl_state.data_ptr(), fl_list.data_ptr(), SEQ,
            tau_d.data_ptr() if tau is not None else None, int(force_fail)]
    if kind == "rerank":
        src = dev(keys_in)
        rc = rlib.chk_rerank(*head, src.data_ptr(), *tail)
    else:
        src = dev(spread_over_lists(keys_in, k))
        rc = rlib.chk_merge_rerank(*head, src.data_ptr(), N_LISTS, *tail)
    assert rc == 0, f"launch failed: hip error {rc}"
    torch.cuda.synchronize()
    return (keys_out.cpu().numpy().view(U64), D.cpu().numpy(), I.cpu().numpy(), int(fl_state.cpu().numpy().view(U64)[0]),
            fl_list.cpu().numpy())


def check(got, want_keys, want_failed, tag):
    keys_out, D, I, fl_state, fl_list = got
    assert np.array_equal(keys_out, want_keys), f"{tag}: keys_out"
    want_D, want_I = keycodec.decode(want_keys, L2)
    assert np.array_equal(I, want_I), f"{tag}: I"
    assert np.array_equal(D.view(np.uint32), want_D.view(np.uint32)), f"{tag}: D"
    nfail = int(want_failed.sum())
    assert fl_state == ((SEQ << 32) | nfail if nfail else 0), f"{tag}: fl_state {fl_state:#x}, {nfail} queries fail"
    assert sorted(fl_list[:nfail].tolist()) == np.flatnonzero(want_failed).tolist(), f"{tag}: fl_list"
    assert (fl_list[nfail:] == -1).all(), f"{tag}: fl_list written beyond its count"


def both_kernels(rlib, xbp, q, keys_in, k, n, tag, **kw):
    want_keys, want_failed = rr.rerank_model(xbp, q, keys_in, k, n, id_base=kw.get("id_base", 0), tau=kw.get("tau"),
                                             force_fail=kw.get("force_fail", False), d_fn=kw.pop("d_fn", rr.d_kernel_order))
    for kind in ("rerank", "merge"):
        check(launch(rlib, kind, xbp, q, keys_in, k, n, **kw), want_keys, want_failed, f"{tag} {kind}")
    return want_keys, want_failed


def candidates(rng, xbp, qp, kc, n, id_base=0, shrink=0.75):
    """keys_in [nq][kc]: query i keeps count = (0, 1, kc - 1, kc)[i % 4] candidates -- random distinct rows, rows 0 and
    n - 1 among them from the fifth query on -- keyed by lo = shrink x d (ascending), so that some certificates hold and
    some fail."""
    nq = len(qp)
    keys_in = np.full((nq, kc), PAD, dtype=U64)
    for i in range(nq):
        count = (0, 1, kc - 1, kc)[i % 4]
        rows = rng.permutation(n)[:count]
        if i >= 4 and count >= 2:
            rows[:2] = (0, n - 1)
            rows = np.unique(rows)  # (a clash with the two forced rows costs a candidate)
        lo = (np.float32(shrink) * rr.d_kernel_order(xbp[rows], qp[i])).astype(np.float32)
        order = np.lexsort((rows, lo))
        keys_in[i, :len(rows)] = rr.lo_keys(lo[order], rows[order] + id_base)
    return keys_in


@pytest.mark.parametrize("d", DIMS)
def test_rerank_shapes(rlib, d):
    dp, n, nq = rr.pad_dim(d), 1000, 8
    rng = np.random.default_rng([d, 1])
    xbp = rr.pad_rows(rng.random((n, d), dtype=np.float32), dp)
    q = rng.random((nq, d), dtype=np.float32)
    qp = rr.pad_rows(q, dp)
    saw = set()
    for kc in KCS:
        keys_in = candidates(rng, xbp, qp, kc, n)
        for k in sorted({1, kc}):
            _, failed = both_kernels(rlib, xbp, q, keys_in, k, n, f"d={d} kc={kc} k={k}")
            saw |= set(failed.tolist())
    assert saw == {False, True}, "certificates of both kinds"


def test_rerank_long_list(rlib):
    """kc = 300: a wave of rerank_kernel takes 75 candidates, more than the 64 keys its lanes hold at a time (the
    window of keys moves on); merge_kernel<true> merges them by merge_rounds."""
    d, kc, n, nq = 60, 300, 1000, 8
    dp = rr.pad_dim(d)
    rng = np.random.default_rng(5)
    xbp = rr.pad_rows(rng.random((n, d), dtype=np.float32), dp)
    q = rng.random((nq, d), dtype=np.float32)
    keys_in = candidates(rng, xbp, rr.pad_rows(q, dp), kc, n)
    for k in (1, kc):
        both_kernels(rlib, xbp, q, keys_in, k, n, f"kc={kc} k={k}")


@pytest.mark.parametrize("d", (60, 512, 2048))
def test_rerank_integer_rows(rlib, d):
    """Integer-valued data below 2^12: every partial sum is exact, so d() is the plain integer sum whatever the order."""
    dp, n, nq, kc, id_base = rr.pad_dim(d), 777, 8, 36, 1 << 20
    rng = np.random.default_rng([d, 2])
    xbp = rr.pad_rows(rng.integers(0, 8, (n, d)).astype(np.float32), dp)
    q = rng.integers(0, 8, (nq, d)).astype(np.float32)

    def d_int(rows, x):
        return ((rows.astype(np.int64) - x.astype(np.int64)[None, :]) ** 2).sum(axis=1).astype(np.float32)

    keys_in = candidates(rng, xbp, rr.pad_rows(q, dp), kc, n, id_base=id_base, shrink=0.5)
    assert np.array_equal(rr.d_kernel_order(xbp[:50], rr.pad_rows(q, dp)[0]), d_int(xbp[:50], rr.pad_rows(q, dp)[0]))
    for k in (1, 10, kc):
        both_kernels(rlib, xbp, q, keys_in, k, n, f"int d={d} k={k}", id_base=id_base, d_fn=d_int)


def test_rerank_edges(rlib):
    d, kc, k, n, id_base = 260, 14, 5, 1000, 5000
    dp = rr.pad_dim(d)
    rng = np.random.default_rng(3)
    xb = rng.random((n, d), dtype=np.float32)
    xb[11, 7] = np.nan  # a NaN row ...
    xb[12] = 3e19  # ... and one whose distance overflows: Faiss's gate drops both
    xbp = rr.pad_rows(xb, dp)
    q = rng.random((6, d), dtype=np.float32)
    qp = rr.pad_rows(q, dp)
    keys_in = np.full((6, kc), PAD, dtype=U64)
    tiny = (np.arange(kc) * 1e-3).astype(np.float32)  # bounds far below every distance, ascending
    # 0: the same row as every candidate (the bounds tell the keys apart)
    keys_in[0] = rr.lo_keys(tiny, np.full(kc, 7 + id_base))
    # 1: the NaN row and the overflowing row among the candidates
    rows1 = np.array([11, 12] + list(range(20, 20 + kc - 2)))
    keys_in[1] = rr.lo_keys(tiny, rows1 + id_base)
    # 2, 3: a full list whose last bound equals d_k (fails), and one an ulp above it (holds)
    rows = np.arange(100, 100 + kc)
    d_k = [np.sort(rr.d_kernel_order(xbp[rows], qp[i]))[k - 1] for i in range(6)]
    for i, last in ((2, d_k[2]), (3, np.nextafter(d_k[3], np.float32(np.inf))), (4, FLT_MAX), (5, FLT_MAX)):
        lo = tiny.copy()
        lo[-1] = last
        keys_in[i] = rr.lo_keys(lo, rows + id_base)
    want_keys, failed = both_kernels(rlib, xbp, q, keys_in, k, n, "edges", id_base=id_base)
    assert failed.tolist() == [True, True, True, False, False, False]
    assert (want_keys[0] & U64(0xFFFFFFFF) == U64(7 + id_base)).all() and len(np.unique(want_keys[0])) == 1
    assert not np.isin(want_keys[1] & U64(0xFFFFFFFF), [11 + id_base, 12 + id_base]).any()
    # 4, 5: the admit threshold of the large-batch path: tau = d_k holds, an ulp below fails; the others' is +inf
    tau = np.full(6, np.inf, dtype=np.float32)
    tau[4], tau[5] = d_k[4], np.nextafter(d_k[5], np.float32(-np.inf))
    _, failed = both_kernels(rlib, xbp, q, keys_in, k, n, "edges tau", id_base=id_base, tau=tau)
    assert failed.tolist() == [True, True, True, False, False, True]
    _, failed = both_kernels(rlib, xbp, q, keys_in, k, n, "edges forced", id_base=id_base, force_fail=True)
    assert failed.all()
    # n <= kc: the list holds every row and needs no certificate, whatever its last bound
    small = rr.pad_rows(xb[100:100 + kc], dp)
    keys_small = np.stack([rr.lo_keys(tiny, np.arange(kc) + id_base)] * 6)
    _, failed = both_kernels(rlib, small, q, keys_small, k, kc, "n = kc", id_base=id_base)
    assert not failed.any()
    # an empty index: no candidate, no row to read
    _, failed = both_kernels(rlib, np.zeros((0, dp), dtype=np.float32), q, np.full((6, kc), PAD, dtype=U64), k, 0, "n = 0")
    assert not failed.any()


@pytest.mark.parametrize("d", (60, 512, 2048))
def test_rerank_matches_exact_scan(rlib, d):
    """The distances of the re-rank against exact_scan_kernel's (every certificate failed: ISE_FORCE_EXACT=1) on the
    same rows: both must be d() bit for bit."""
    import image_search_engine_amd.faiss_compat as faiss
    from tests.test_exact_l2_gpu import forced_exact

    n, nq, kc = 3000, 6, 14
    rng = np.random.default_rng([d, 4])
    xb, q = rng.random((n, d), dtype=np.float32), rng.random((nq, d), dtype=np.float32)
    index = faiss.IndexFlatL2(d)
    index.add(xb)
    with forced_exact():
        before = index.exact_stats()["exact_scan"]
        D_e, I_e = index.search(q, kc)
        assert index.exact_stats()["exact_scan"] == before + nq, "the exact scan answered every query"
    dp = rr.pad_dim(d)
    xbp = rr.pad_rows(xb, dp)
    keys_in = np.stack([rr.lo_keys(np.float32(0.5) * D_e[i], I_e[i]) for i in range(nq)])
    for kind in ("rerank", "merge"):
        keys_out, D, I, _, _ = launch(rlib, kind, xbp, q, keys_in, kc, n)
        assert np.array_equal(I, I_e) and np.array_equal(D.view(np.uint32), D_e.view(np.uint32)), f"d={d} {kind}"
    want = np.stack([rr.d_kernel_order(xbp[I_e[i]], rr.pad_rows(q, dp)[i]) for i in range(nq)])
    assert np.array_equal(want.view(np.uint32), D_e.view(np.uint32)), "the restatement is the exact scan's d() too"
