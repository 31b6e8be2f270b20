"""CPU tests of the scalar-quantised index's host side: the entry points' argument errors through the C ABI (no device
is touched), the numpy reference of the GPU tests (tests/sq_ref.py), the file format, and what stays unprovided."""
import ctypes

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import sq_ref
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data
from tests.sel_ref import IP, L2

SQ = faiss.ScalarQuantizer


def test_constants():
    assert (SQ.QT_8bit, SQ.QT_4bit, SQ.QT_8bit_uniform, SQ.QT_4bit_uniform, SQ.QT_fp16, SQ.QT_8bit_direct, SQ.QT_6bit,
            SQ.QT_bf16, SQ.QT_8bit_direct_signed) == (0, 1, 2, 3, 4, 5, 6, 7, 8)
    assert (SQ.RS_minmax, SQ.RS_meanstd, SQ.RS_quantiles, SQ.RS_optim) == (0, 1, 2, 3)
    assert (sq_ref.QT_8BIT, sq_ref.QT_8BIT_UNIFORM) == (SQ.QT_8bit, SQ.QT_8bit_uniform)


def test_argument_errors_through_abi():
    from image_search_engine_amd import _native as n

    lib = n.lib
    h = ctypes.c_void_p()
    assert n.SQ_MAX_D >= 2048 and n.SQ_MAX_D == sq_ref.MAX_D
    for args, word in (((0, 0, n.METRIC_L2, 0), b"d must"), ((-4, 0, n.METRIC_L2, 0), b"d must"),
                       ((n.SQ_MAX_D + 1, 0, n.METRIC_L2, 0), b"ISE_SQ_MAX_D"), ((8, 1, n.METRIC_L2, 0), b"qtype"),
                       ((8, 4, n.METRIC_L2, 0), b"qtype"), ((8, -1, n.METRIC_L2, 0), b"qtype"), ((8, 0, 7, 0), b"metric")):
        assert lib.ise_sq_create(ctypes.byref(h), *args) == n.E_INVALID, args
        assert word in lib.ise_last_error(), (args, lib.ise_last_error())
        assert h.value is None
    assert lib.ise_sq_create(None, 8, 0, n.METRIC_L2, 0) == n.E_INVALID
    assert b"NULL" in lib.ise_last_error()
    assert lib.ise_sq_destroy(None) == 0
    assert lib.ise_sq_reset(None) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    assert lib.ise_sq_info(None, None, None, None, None, None, None) == n.E_INVALID
    x = np.zeros((2, 8), np.float32)
    codes = np.zeros((2, 8), np.uint8)
    tr = np.zeros(16, np.float32)
    D, I = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int64)
    xp, cp_ = x.ctypes.data, codes.ctypes.data
    # NULL buffers and negative counts come before the handle is looked at
    for fn in (lib.ise_sq_set_trained_host, lib.ise_sq_get_trained_host):
        assert fn(None, None) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert fn(None, tr.ctypes.data) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    for call in (lambda a, b, cnt: lib.ise_sq_encode_host(None, a, cnt, b),
                 lambda a, b, cnt: lib.ise_sq_encode_device(None, a, cnt, b, None),
                 lambda a, b, cnt: lib.ise_sq_decode_host(None, b, cnt, a)):
        assert call(None, cp_, 2) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert call(xp, None, 2) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert call(xp, cp_, -1) == n.E_INVALID
        assert b"n must" in lib.ise_last_error()
        assert call(xp, cp_, 2) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    for call in (lambda a, cnt: lib.ise_sq_add_host(None, a, cnt), lambda a, cnt: lib.ise_sq_add_device(None, a, cnt, None),
                 lambda a, cnt: lib.ise_sq_add_codes_host(None, a, cnt)):
        assert call(None, 2) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert call(xp, -1) == n.E_INVALID
        assert b"n must" in lib.ise_last_error()
        assert call(xp, 2) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    assert lib.ise_sq_codes_host(None, 0, 1, cp_) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    assert lib.ise_sq_reconstruct_host(None, 0, 1, xp) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    # k outside 1 .. ISE_MAX_K and NULL buffers: before the handle is looked at
    for search, tail in ((lib.ise_sq_search_host, ()), (lib.ise_sq_search_device, (None,))):
        for k in (0, -1, n.MAX_K + 1):
            assert search(None, xp, 2, k, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
            assert b"k must" in lib.ise_last_error()
        assert search(None, xp, -1, 3, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"nq must" in lib.ise_last_error()
        assert search(None, None, 2, 3, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"pointer is NULL" in lib.ise_last_error()
        assert search(None, xp, 2, 3, None, I.ctypes.data, *tail) == n.E_INVALID
        assert b"output pointer" in lib.ise_last_error()
        assert search(None, xp, 2, 3, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"handle" in lib.ise_last_error()
    assert lib.ise_sq_stats(None, (ctypes.c_uint64 * 3)()) == n.E_INVALID
    assert b"handle" in lib.ise_last_error()
    assert lib.ise_sq_stats(None, None) == n.E_INVALID
    assert b"NULL" in lib.ise_last_error()


def test_what_stays_unprovided():
    for qtype in (SQ.QT_4bit, SQ.QT_4bit_uniform, SQ.QT_fp16, SQ.QT_8bit_direct, SQ.QT_6bit, SQ.QT_bf16,
                  SQ.QT_8bit_direct_signed):
        with pytest.raises(NotImplementedError, match="qtype"):
            faiss.IndexScalarQuantizer(16, qtype)
    for name in ("range_search", "remove_ids"):
        with pytest.raises(NotImplementedError):
            getattr(faiss.IndexScalarQuantizer, name)(None)
    with pytest.raises(NotImplementedError):
        faiss.IndexIVFPQ()


def test_pass_rule_and_block_size():
    assert [sq_ref.qt_of(d) for d in (1, 64, 512, 1024, 1472, 1473, 1536, 2048)] == [16, 16, 16, 16, 16, 8, 8, 8]
    assert sq_ref.passes_of(512, 40, 70) == 3 * 3 and sq_ref.passes_of(2048, 40, 70) == 5 * 3
    assert sq_ref.passes_of(64, 1, 1) == 1 and sq_ref.passes_of(64, 16, 32) == 1 and sq_ref.passes_of(64, 17, 33) == 4
    assert sq_ref.BLOCK_ROWS == 512 and sq_ref.BLOCK_ROWS % sq_ref.TILE_ROWS == 0


@pytest.mark.parametrize("qtype", [sq_ref.QT_8BIT, sq_ref.QT_8BIT_UNIFORM])
@pytest.mark.parametrize("d", [1, 17, 100, 512])
def test_integer_construction(d, qtype):
    """Rows m + s * base encode to base, decode to themselves, and keep every sum an exact float32 integer."""
    rng = np.random.default_rng(100 + d + qtype)
    t, m, s = sq_ref.integer_trained(rng, d, qtype)
    assert t.size == (2 if qtype == sq_ref.QT_8BIT_UNIFORM else 2 * d)
    vmin, vdiff = sq_ref.expand(t, d, qtype)
    assert np.array_equal(sq_ref.step_of(vdiff), s)
    xb, base = sq_ref.integer_rows(rng, 300, d, m, s)
    codes = sq_ref.encode(xb, vmin, vdiff)
    assert codes.dtype == np.uint8 and np.array_equal(codes, base)
    dec = sq_ref.decode(codes, vmin, vdiff)
    assert dec.dtype == np.float32 and np.array_equal(dec, xb)
    xq = int_data("small", rng, 9, d)
    bound = assert_exact_range(dec, xq)
    # the kernel's own expansion, about o = vmin + s / 2 = m: |x - m|^2, sum (s c)^2 and the cross term
    about = assert_exact_range((s[None, :] * base).astype(np.float32), (xq - m[None, :]).astype(np.float32))
    print(f"d={d}: exact-range bound {bound:.0f} about the origin, {about:.0f} about vmin + s/2")
    for metric in (L2, IP):
        D, I = sq_ref.expected(xq, dec, 20, metric)
        score = ((xq[:, None, :].astype(np.float64) - xb[None].astype(np.float64)) ** 2).sum(2) if metric == L2 else \
            xq.astype(np.float64) @ xb.astype(np.float64).T
        key = score if metric == L2 else -score
        Iw = np.stack([np.lexsort((np.arange(300), key[q]))[:20] for q in range(9)]).astype(np.int64)
        Dw = np.take_along_axis(score, Iw, axis=1).astype(np.float32) + np.float32(0)
        assert_knn_identical(D, I, Dw, Iw)
        assert not np.signbit(D[D == 0]).any()


def test_wide_integer_construction_stays_exact():
    """d = 2048 with "binary" bases and binary queries (the GPU sweep's widest case)."""
    rng = np.random.default_rng(2048)
    t, m, s = sq_ref.integer_trained(rng, 2048, sq_ref.QT_8BIT)
    xb, base = sq_ref.integer_rows(rng, 300, 2048, m, s, "binary")
    xq = int_data("binary", rng, 9, 2048)
    assert_exact_range(xb, xq)
    assert_exact_range((s[None, :] * base).astype(np.float32), (xq - m[None, :]).astype(np.float32))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", [sq_ref.QT_8BIT, sq_ref.QT_8BIT_UNIFORM])
@pytest.mark.parametrize("d,kind", [(1, "small"), (17, "small"), (130, "small"), (320, "small"), (576, "small"),
                                    (1473, "binary")])
def test_scan_emulation_is_exact_on_integer_construction(d, kind, qtype, metric):
    """``sq_ref.emulate_scores`` -- the scan's arithmetic in numpy -- gives the exact score, bit for bit, where the
    scan's own condition holds: 128 sum |w_j| < 2^24, so every accumulator holds an integer times 2^sh."""
    rng = np.random.default_rng(300 + d + qtype)
    t, m, s = sq_ref.integer_trained(rng, d, qtype)
    vmin, vdiff = sq_ref.expand(t, d, qtype)
    assert np.array_equal(sq_ref.offset_of(vmin, vdiff), m)
    xb, base = sq_ref.integer_rows(rng, 150, d, m, s, kind)
    xq = int_data(kind, rng, 7, d)
    xq[3] = 0.0  # the all-zero query: sh = 0 for the inner product
    xq[4] = xb[11]  # a zero distance
    assert_exact_range(xb, xq)
    w = s[None, :] * (xq - m[None, :] if metric == L2 else xq)
    assert 128.0 * np.abs(w.astype(np.float64)).sum(1).max() < 1 << 24
    x64, y64 = xq.astype(np.float64), xb.astype(np.float64)
    want = ((x64[:, None, :] - y64[None]) ** 2).sum(2) if metric == L2 else x64 @ y64.T
    got = sq_ref.emulate_scores(xq, base, vmin, vdiff, metric)
    assert got.dtype == np.float32 and got.shape == (7, 150)
    assert np.array_equal(got.view(np.uint32), (want.astype(np.float32) + np.float32(0)).view(np.uint32))
    assert not np.signbit(got[got == 0]).any()
    # the same scores through the BLAS form the long-index test uses, and its top-k against the brute force
    assert np.array_equal(sq_ref.scores_from_codes(base, m, s, xq, metric, chunk=64), want.T)
    D, I = sq_ref.expected(xq, xb, 20, metric)
    for q in range(7):
        Dq, Iq = sq_ref.top_of_scores(want[q], np.arange(150, dtype=np.int64), 20, metric)
        assert_knn_identical(Dq[None, :], Iq[None, :], D[q:q + 1], I[q:q + 1], f"q={q}")
    # exact scores: the bound has nothing but the reference's own rounding terms to cover
    E, parts = sq_ref.score_bound(xq, base, vmin, vdiff, metric)
    assert E.shape == (7,) and (E >= 0).all() and all(v.shape == (7,) for v in parts.values())


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", [sq_ref.QT_8BIT, sq_ref.QT_8BIT_UNIFORM])
@pytest.mark.parametrize("family", [3, 30, 900, "offset", "relu"])
@pytest.mark.parametrize("d", [64, 512])
def test_scan_emulation_stays_within_the_derived_bound(d, family, qtype, metric):
    """The emulation's error against float64 over the decoded rows lies under ``sq_ref.score_bound`` on every family the
    GPU test uses (the emulation is a lower estimate of the device's error: a bound it broke would be wrong)."""
    train, xb, xq = sq_ref.stretched_case(family, d, qtype)
    vmin, vdiff = sq_ref.expand(sq_ref.train_minmax(train, qtype), d, qtype)
    codes = sq_ref.encode(xb, vmin, vdiff)
    dec = sq_ref.decode(codes, vmin, vdiff).astype(np.float64)
    x64 = xq.astype(np.float64)
    want = ((x64[:, None, :] - dec[None]) ** 2).sum(2) if metric == L2 else x64 @ dec.T
    got = sq_ref.emulate_scores(xq, codes, vmin, vdiff, metric).astype(np.float64)
    E, parts = sq_ref.score_bound(xq, codes, vmin, vdiff, metric)
    bound = E[:, None] * (1 + sq_ref.U) + sq_ref.U * np.abs(want)
    err = np.abs(got - want)
    rel = err / np.maximum(1.0, np.abs(want))
    print(f"d={d} family={family} qtype={qtype} metric={metric}: largest |D - D64| / max(1, |D64|) = {rel.max():.3e}, "
          f"largest error / bound = {(err / bound).max():.3e}")
    assert (err <= bound).all()
    if family == 3:  # data that fill their trained range: the 1e-4 of the real-data tests holds with room
        assert rel.max() < 2e-5


@pytest.mark.parametrize("qtype", [sq_ref.QT_8BIT, sq_ref.QT_8BIT_UNIFORM])
def test_encode_and_decode_on_real_data(qtype):
    rng = np.random.default_rng(7)
    n, d = 2000, 64
    x = (3 + rng.standard_normal((n, d))).astype(np.float32)
    t = sq_ref.train_minmax(x[:1500], qtype)  # the last 500 rows may leave the trained range
    vmin, vdiff = sq_ref.expand(t, d, qtype)
    s = sq_ref.step_of(vdiff)
    if qtype == sq_ref.QT_8BIT:
        assert np.array_equal(vmin, x[:1500].min(0)) and np.array_equal(vdiff, x[:1500].max(0) - x[:1500].min(0))
    else:
        assert vmin[0] == x[:1500].min() and (vdiff == x[:1500].max() - x[:1500].min()).all()
    c32, c64 = sq_ref.encode(x, vmin, vdiff), sq_ref.encode(x, vmin, vdiff, np.float64)
    t64 = sq_ref.encode_t64(x, vmin, vdiff)
    band = np.abs(t64 - np.rint(t64)) <= 1e-3
    print(f"entries within 1e-3 of an integer quotient: {band.mean():.4%}; float32/float64 mismatches: "
          f"{(c32 != c64).sum()}")
    assert band.mean() < 0.01
    diff = c32.astype(np.int64) - c64.astype(np.int64)
    assert (diff[~band] == 0).all() and (np.abs(diff) <= 1).all()
    dec = sq_ref.decode(c32, vmin, vdiff)
    inside = (t64 >= 0) & (t64 < 256)
    err = np.abs(dec.astype(np.float64) - x.astype(np.float64))
    lim = 0.5 * s.astype(np.float64)[None, :] * (1 + 1e-3)
    print(f"largest |decoded - x| / s over in-range entries: {(err / s[None, :])[inside].max():.5f}")
    assert (err[inside] <= np.broadcast_to(lim, err.shape)[inside]).all()
    assert (c32[t64 < 0] == 0).all() and (c32[t64 >= 256] == 255).all()
    assert (t64 < 0).any() or (t64 >= 256).any() or qtype == sq_ref.QT_8BIT_UNIFORM
    # far outside: clamped
    far = np.stack([np.full(d, -1e6, np.float32), np.full(d, 1e6, np.float32)])
    assert np.array_equal(sq_ref.encode(far, vmin, vdiff), np.stack([np.zeros(d, np.uint8), np.full(d, 255, np.uint8)]))


def test_zero_step_encodes_to_zero_and_decodes_to_vmin():
    vmin = np.array([1.5, -2.0, 0.25], np.float32)
    vdiff = np.array([0.0, 0.0, 255.0], np.float32)
    x = np.array([[1.5, 7.0, 3.3], [-9.0, -2.0, 0.25]], np.float32)
    codes = sq_ref.encode(x, vmin, vdiff)
    assert codes.tolist() == [[0, 0, 3], [0, 0, 0]]
    assert np.array_equal(sq_ref.decode(codes, vmin, vdiff), np.array([[1.5, -2.0, 3.75], [1.5, -2.0, 0.75]], np.float32))


def _file(n, qtype, rng):
    d = 6
    t = rng.standard_normal(2 if qtype == 2 else 2 * d).astype(np.float32)
    t[t.size // 2:] = np.abs(t[t.size // 2:])
    return d, t, rng.integers(0, 256, (n, d)).astype(np.uint8)


@pytest.mark.parametrize("qtype", [0, 2])
@pytest.mark.parametrize("n", [0, 1, 37])
def test_file_round_trip(n, qtype):
    d, t, codes = _file(n, qtype, np.random.default_rng(n))
    for metric in (L2, IP):
        buf = faiss.serialize_sq(d, metric, qtype, t, codes)
        assert buf[:4] == b"IxSQ"
        d2, metric2, qtype2, rs, rs_arg, t2, codes2 = faiss.parse_sq(buf)
        assert (d2, metric2, qtype2, rs, rs_arg) == (d, metric, qtype, 0, 0.0)
        assert t2.dtype == np.float32 and np.array_equal(t2.view(np.uint32), t.view(np.uint32))
        assert codes2.dtype == np.uint8 and codes2.shape == (n, d) and np.array_equal(codes2, codes)
        # as the base image of an IndexRefineFlat file
        xb = np.random.default_rng(1).standard_normal((n, d)).astype(np.float32)
        rf = faiss.parse_refine(faiss.serialize_refine(buf, d, metric, xb, 3.0))
        assert rf[2] == "sq" and np.array_equal(rf[3][6], codes) and np.array_equal(rf[4], xb) and rf[5] == 3.0


def test_file_truncations_and_foreign_files():
    d, t, codes = _file(5, 0, np.random.default_rng(1))
    buf = faiss.serialize_sq(d, L2, 0, t, codes)
    for cut in range(len(buf)):  # every truncation point
        with pytest.raises(RuntimeError):
            faiss.parse_sq(buf[:cut])
    with pytest.raises(RuntimeError, match="IndexScalarQuantizer"):
        faiss.parse_sq(b"IxF2" + buf[4:])
    with pytest.raises(RuntimeError, match="IndexScalarQuantizer"):
        faiss.parse_sq(b"IxPq" + buf[4:])
    hdr = faiss._HDR.size
    for qtype in (1, 3, 4, 5, 6, 7, 8, -1):
        bad = bytearray(buf)
        bad[hdr:hdr + 4] = int(qtype).to_bytes(4, "little", signed=True)
        with pytest.raises(RuntimeError, match="quantiser type"):
            faiss.parse_sq(bytes(bad))
    at = hdr + faiss._SQ_HEAD.size
    bad_count = bytearray(buf)
    bad_count[at:at + 8] = (2 * d + 1).to_bytes(8, "little")  # the trained count
    with pytest.raises(RuntimeError):
        faiss.parse_sq(bytes(bad_count))
    at += 8 + 4 * 2 * d
    bad_codes = bytearray(buf)
    bad_codes[at:at + 8] = (5 * d - 1).to_bytes(8, "little")  # the code count
    with pytest.raises(RuntimeError):
        faiss.parse_sq(bytes(bad_codes))
    bad_size = bytearray(buf)
    bad_size[hdr + 20:hdr + 28] = (d + 1).to_bytes(8, "little")  # code_size
    with pytest.raises(RuntimeError):
        faiss.parse_sq(bytes(bad_size))
    # a truncated base image inside an IndexRefineFlat file
    xb = np.zeros((5, d), np.float32)
    whole = faiss.serialize_refine(buf, d, L2, xb, 2.0)
    for cut in (hdr + 10, hdr + len(buf) - 3, len(whole) - 2):
        with pytest.raises(RuntimeError):
            faiss.parse_refine(whole[:cut])
