"""numpy reference of the scalar-quantised index (tests only): the step, encode, decode and min/max training as
include/ise_knn.h states them, the expected kNN (a float64 brute force over the DECODED rows), the kernel's pass rule
and block size, and the integer construction on which every score is exact."""
import numpy as np

from tests.knn_checks import brute_knn, int_data

QT_8BIT, QT_8BIT_UNIFORM = 0, 2
MAX_D = 2048
LDS_LIMIT = 160 * 1024
BLOCK_ROWS = 2 * 4 * 64  # rows per block a short index's grid is sized for: 2 tiles of 64 rows for each of 4 waves
TILE_ROWS = 64


def qt_of(d: int) -> int:
    """Queries per scan pass (csrc/ise_sq.hpp, sq_qt): 16 while two limb images of 2 dpad + 16 bytes, 4 KiB of selection
    buffers and 16 bytes per query fit 160 KiB, else 8."""
    dpad = -(-d // 64) * 64
    return 16 if 16 * (2 * (2 * dpad + 16) + 4 * 128 * 8 + 16) <= LDS_LIMIT else 8


def passes_of(d: int, nq: int, k: int) -> int:
    return -(-nq // qt_of(d)) * -(-k // 32)


def expand(trained, d: int, qtype: int):
    """-> (vmin, vdiff) float32 (d,) of a trained vector in Faiss's layout."""
    t = np.asarray(trained, dtype=np.float32).reshape(-1)
    if qtype == QT_8BIT_UNIFORM:
        assert t.size == 2
        return np.full(d, t[0], np.float32), np.full(d, t[1], np.float32)
    assert t.size == 2 * d
    return t[:d].copy(), t[d:].copy()


def step_of(vdiff) -> np.ndarray:
    """s = vdiff / 255.0f: one float32 division."""
    return (np.asarray(vdiff, np.float32) / np.float32(255.0)).astype(np.float32)


def train_minmax(x, qtype: int) -> np.ndarray:
    x = np.asarray(x, np.float32)
    if qtype == QT_8BIT_UNIFORM:
        return np.array([x.min(), x.max() - x.min()], dtype=np.float32)
    return np.concatenate([x.min(0), x.max(0) - x.min(0)]).astype(np.float32)


def encode(x, vmin, vdiff, dtype=np.float32) -> np.ndarray:
    """uint8 codes; ``dtype=np.float64`` gives the float64 reference of the real-data checks."""
    s = step_of(vdiff).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.floor((np.asarray(x, np.float32).astype(dtype) - np.asarray(vmin, np.float32).astype(dtype)) / s)
    t = np.where(s == 0, 0, np.clip(np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0), 0, 255))
    return t.astype(np.uint8)


def encode_t64(x, vmin, vdiff) -> np.ndarray:
    """The float64 quotient (x - vmin) / s before the floor (s the float32 step)."""
    s = step_of(vdiff).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(x, np.float64) - np.asarray(vmin, np.float64)) / s


def decode(codes, vmin, vdiff) -> np.ndarray:
    """fmaf(c + 0.5, s, vmin) as float32.  (c + 0.5) * s is exact in float64 (9 x 24 bits), so the float64 sum is the
    exact value rounded once to 53 bits; the second rounding to float32 differs from the fused one only if that sum is
    inexact AND lands on a float32 midpoint."""
    s = step_of(vdiff).astype(np.float64)
    y = (np.asarray(codes, np.float64) + 0.5) * s + np.asarray(vmin, np.float64)
    return y.astype(np.float32)


def expected(xq, dec, k: int, metric: int):
    """The kNN over the decoded rows; a zero score is +0."""
    D, I = brute_knn(dec, xq, k, metric)
    return D + np.float32(0.0), I


# ---- the integer construction: (vmin_j, vdiff_j) is (m_j - 0.5, 255) [s = 1] or (m_j - 1, 510) [s = 2] with integer
# m_j in [-2, 2]; a row m_j + s_j * base_j encodes to base_j and decodes to itself
def integer_trained(rng, d: int, qtype: int):
    """-> (trained vector, m (d,), s (d,))"""
    cnt = 1 if qtype == QT_8BIT_UNIFORM else d
    m = rng.integers(-2, 3, cnt).astype(np.float32)
    s = rng.integers(1, 3, cnt).astype(np.float32)
    vmin = m - np.float32(0.5) * s
    vdiff = np.float32(255.0) * s
    t = np.concatenate([vmin, vdiff]).astype(np.float32)
    return t, np.broadcast_to(m, (d,)).copy(), np.broadcast_to(s, (d,)).copy()


def integer_rows(rng, n: int, d: int, m, s, kind: str = "small"):
    """-> (rows float32 (n, d), their codes uint8 (n, d))"""
    base = int_data(kind, rng, n, d)
    return (m[None, :] + s[None, :] * base).astype(np.float32), base.astype(np.uint8)
