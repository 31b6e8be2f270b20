"""numpy restatement of the exact re-rank of csrc/ise_exact.hpp (rerank_block), for tests/test_rerank_gpu.py (tests only).

d(x, y) is restated in the kernel's own order, so the comparison is bit for bit: lane l of 64 takes the elements
4l .. 4l + 3 of each 256-element column block of the padded row in sequence, s = fmaf(t, t, s) with t = y - x in
float32, then the xor butterfly v += v[lane ^ o], o = 32 .. 1.  Each fmaf is emulated exactly: the product of two
float32 is exact in float64; the float64 sum is made round-to-odd with the error term of TwoSum, after which the
rounding to float32 is the single rounding of the fused operation (53 >= 2 * 24 + 2 bits)."""
import numpy as np

from tests import keycodec

PAD = keycodec.PAD
U64 = np.uint64
FLT_MAX = np.float32(np.finfo(np.float32).max)


def pad_dim(d):
    """dp of a float32 index (csrc/ise_geometry.hpp): whole 16-float steps, whole groups of four beyond four."""
    steps = -(-d // 16)
    return (-(-steps // 4) * 4 if steps > 4 else steps) * 16


def pad_rows(x, dp):
    out = np.zeros((x.shape[0], dp), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def fmaf_sq(t, s):
    """float32 fmaf(t, t, s) for s >= 0 or NaN, elementwise and exact."""
    with np.errstate(all="ignore"):
        p = t.astype(np.float64) * t.astype(np.float64)  # exact
        a = s.astype(np.float64)
        r = p + a
        bb = r - a
        err = (a - (r - bb)) + (p - bb)  # TwoSum: p + a = r + err exactly
        fin = np.isfinite(r) & np.isfinite(err) & (err != 0)
        bits = r.view(np.int64).copy()
        bits = np.where(fin & (err < 0), bits - 1, bits)  # r >= 0: truncate towards zero ...
        bits = np.where(fin, bits | 1, bits)  # ... and make the inexact sum odd
        return bits.view(np.float64).astype(np.float32)


def d_kernel_order(rows, x):
    """rows [m][dp], x [dp] (zero padded) -> [m] float32, the kernel's d()."""
    m, dp = rows.shape
    lane = np.arange(64)
    s = np.zeros((m, 64), dtype=np.float32)
    for j0 in range(0, dp, 256):
        j = j0 + 4 * lane
        on = j < dp
        for e in range(4):
            col = np.where(on, j + e, 0)
            with np.errstate(all="ignore"):
                t = (rows[:, col] - x[col][None, :]).astype(np.float32)
            s = np.where(on[None, :], fmaf_sq(t, s), s)
    for o in (32, 16, 8, 4, 2, 1):
        with np.errstate(all="ignore"):
            s = (s + s[:, lane ^ o]).astype(np.float32)
    assert (s.view(np.uint32) == s[:, :1].view(np.uint32)).all(), "every lane ends with the same sum"
    return s[:, 0].copy()


def rerank_model(xbp, q, keys_in, k, n, id_base=0, tau=None, force_fail=False, d_fn=d_kernel_order):
    """xbp [rows][dp] padded rows, q [nq][d], keys_in [nq][kc] ascending lo-keys with PAD behind.
    -> keys_out [nq][k] (exact keys, PAD behind), failed [nq] bool (the certificate sent the query to the exact scan)."""
    nq, kc = keys_in.shape
    dp = xbp.shape[1]
    qp = pad_rows(q, dp)
    keys_out = np.full((nq, k), PAD, dtype=U64)
    failed = np.zeros(nq, dtype=bool)
    for i in range(nq):
        kin = keys_in[i]
        count = int((kin != PAD).sum())
        assert (kin[count:] == PAD).all() and (np.diff(kin[:count].astype(object)) > 0).all()
        ids = (kin[:count] & U64(0xFFFFFFFF)).astype(np.int64)
        dd = d_fn(xbp[ids - id_base], qp[i]) if count else np.zeros(0, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            gate = dd < FLT_MAX  # false for NaN
        kex = np.where(gate, (keycodec.ord_f32(dd).astype(U64) << U64(32)) | ids.astype(U64), PAD)
        kex = np.concatenate([np.sort(kex), np.full(kc - count + k, PAD, dtype=U64)])
        keys_out[i] = np.where(np.arange(k) < count, kex[:k], PAD)
        d_k = keycodec.unord_f32(np.uint32(kex[k - 1] >> U64(32)))  # NaN for an empty slot
        ok = True
        with np.errstate(invalid="ignore"):
            if count == kc and n > kc:
                ok = bool(keycodec.unord_f32(np.uint32(kin[kc - 1] >> U64(32))) > d_k)
            if tau is not None:
                ok = ok and (bool(tau[i] >= d_k) if count >= k else count >= n)
        failed[i] = force_fail or not ok
    return keys_out, failed


def lo_keys(lo, ids):
    """ascending (lo, id) keys from float32 bounds and ids (the caller passes them in ascending order)."""
    keys = (keycodec.ord_f32(np.asarray(lo, dtype=np.float32)).astype(U64) << U64(32)) | np.asarray(ids).astype(U64)
    assert (np.diff(keys.astype(object)) > 0).all(), "lower-bound keys ascend"
    return keys
