"""GPU tests of the k = 1 assignment kernel (csrc/ise_assign.hpp, ise_index_assign_device) at every row-length class.

The kernel is instantiated per ns = dp / 16 with XT = 4, 2 or 1 row tiles per wave, loads a row of x by vector only
when d % 4 == 0 and the pointer is 16-byte aligned, clamps the rows behind n, streams the centroids through LDS in
stages of CS (fewer than 128 once rows are long) and lets a block take a further slab of rows once n exceeds what the
grid covers.  Every case below asserts, with Python mirrors of the host's geometry, that it reaches the path it is meant
for; the mirrors never produce an expected result.  On integer data (tests/knn_checks.py) with the L2 shift pinned to
zero the kernel's arithmetic is exact, so D and I must equal the float64 oracle's bit for bit, ties to the lowest id."""
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.knn_checks import assert_exact_range, assert_knn_identical, assert_knn_matches, int_data, plant_ties

pytestmark = pytest.mark.gpu

L2, IP = ko.METRIC_L2, ko.METRIC_INNER_PRODUCT
KINDS = ("small", "signed", "binary")


# ------------------------------------------------------------------ mirrors of the host geometry (inputs and premises only)
def pad_dim(d):
    """csrc/ise_geometry.hpp, pad_dim for float32 rows: whole 16-float steps, in fours beyond four."""
    steps = -(-d // 16)
    return (steps if steps <= 4 else -(-steps // 4) * 4) * 16


def qs_stride_units(units):
    """csrc/ise_geometry.hpp, qs_stride_units: the LDS row stride in 4-byte units, (stride / 4) % 16 == 2."""
    return units + (2 - units // 4) % 16 * 4


ASSIGN_CS_MAX = 128


def assign_stage_rows(dp):
    """csrc/ise_knn.hip, assign_stage_rows: centroids per LDS stage, what fits 150 KB in whole tiles of 16."""
    per = (qs_stride_units(dp) + 1) * 4
    return min(ASSIGN_CS_MAX, (150 * 1024) // per) // 16 * 16


def assign_xt(ns):
    """csrc/ise_knn.hip, ise_index_assign_device: row tiles of 16 per wave."""
    return 4 if ns <= 8 else (2 if ns <= 16 else 1)


def block_rows(d):
    """Rows of x one block of 8 waves takes per slab."""
    return 8 * assign_xt(pad_dim(d) // 16) * 16


def test_geometry_mirrors():
    """The constants this file's cases are built on, as read off the host code."""
    assert [pad_dim(d) for d in (1, 16, 17, 48, 49, 64, 65, 128, 129, 192, 449, 512)] == \
        [16, 16, 32, 48, 64, 64, 128, 128, 192, 192, 512, 512]
    assert [qs_stride_units(u) for u in (16, 64, 320, 512, 2048)] == [72, 72, 328, 520, 2056]
    assert all(qs_stride_units(u) // 4 % 16 == 2 for u in range(16, 2500, 16))
    assert {dp: assign_stage_rows(dp) for dp in (64, 256, 320, 384, 448, 512)} == \
        {64: 128, 256: 128, 320: 112, 384: 96, 448: 80, 512: 64}
    assert [assign_xt(ns) for ns in NS_ALL] == [4, 4, 4, 4, 4, 2, 2, 1, 1, 1, 1]


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _index(faiss, cent, metric, zero_shift=True):
    """A float32 flat index over the centroids; L2 with the shift pinned to zero (exact arithmetic on integers:
    tests/test_tie_order_gpu.py::test_assignment_kernel_tie_order)."""
    index = faiss.IndexFlat(cent.shape[1], metric)
    index.add(cent)
    if metric == L2 and zero_shift:
        index.set_shift(np.zeros(cent.shape[1], np.float32))
    return index


def _ref(cent, X, metric):
    assert_exact_range(cent, X)
    return ko.knn_exact(cent, X, 1, metric)


def _assign(index, X):
    """assign_torch on a fresh aligned device copy -> host (D, I); the vector load runs iff d % 4 == 0."""
    import torch

    x = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    assert x.data_ptr() % 16 == 0
    D, I = index.assign_torch(x)
    return D.cpu().numpy(), I.cpu().numpy()


def _tied_case(rng, kind, K, d, n):
    """Integer centroids with copies of centroid 5 at ids far apart, and rows on that centroid at the first, the middle
    and the last position.  Ids 21 and 69 fall to the lane that holds id 5 (id % 16: the running best of a lane
    decides among them), K // 2 and K - 1 to other lanes (the reduction over the 16 lanes of a row decides)."""
    cent, X = int_data(kind, rng, K, d), int_data(kind, rng, n, d)
    if K > 5:
        plant_ties(cent, 5, sorted({i for i in (21, K // 2, 69, K - 1) if 5 < i < K}))
        X[[0, n // 2, n - 1]] = cent[5]
    return cent, X


# ------------------------------------------------------------- 1. every instantiation, both load paths
NS_ALL = [1, 2, 3, 4, 8, 12, 16, 20, 24, 28, 32]
NS_D = {1: (13, 16), 2: (29, 32), 3: (45, 48), 4: (61, 64), 8: (127, 100), 12: (130, 192), 16: (255, 256),
        20: (257, 320), 24: (383, 384), 28: (401, 448), 32: (449, 512)}  # (scalar load, vector load)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("ns", NS_ALL)
def test_every_instantiation_and_load_path(faiss, ns, metric):
    """assign_kernel<NS, XT> for each of the eleven NS, at a d that is no multiple of 4 (scalar row load) and one that
    is (vector load): one full block of rows plus a ragged tile, 77 centroids (a ragged stage), a centroid with copies
    at ids 5, 21, 38, 69 and 76 and rows exactly on it."""
    K = 77
    for d in NS_D[ns]:
        assert pad_dim(d) // 16 == ns and pad_dim(d) <= 512, d
        n = block_rows(d) + 16 + 3
        for kind in KINDS:
            rng = _rng("inst", ns, metric, d, kind)
            cent, X = _tied_case(rng, kind, K, d, n)
            index = _index(faiss, cent, metric)
            D_ref, I_ref = _ref(cent, X, metric)
            if metric == L2:
                assert (I_ref[[0, n // 2, n - 1], 0] == 5).all() and (D_ref[[0, n // 2, n - 1], 0] == 0).all()
            assert_knn_identical(*_assign(index, X), D_ref, I_ref, f"ns={ns} d={d} {kind}")
    assert NS_D[ns][0] % 4 != 0 and NS_D[ns][1] % 4 == 0


# ------------------------------------------------------------------------------------------ 2. row edges
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [13, 64, 192, 257])
def test_row_edges(faiss, d, metric):
    """n = 1, around one 16-row tile and around one block's rows, per XT class (d = 13 and 257 by the scalar load):
    the clamp min(r, n - 1) re-reads the last row for every slot behind n, and nothing is written behind n."""
    import torch

    R = block_rows(d)
    assert (d % 4 != 0) == (d in (13, 257)) and R == {13: 512, 64: 512, 192: 256, 257: 128}[d]
    K = 77
    for kind in ("small", "signed"):
        rng = _rng("rows", d, metric, kind)
        cent, X_all = _tied_case(rng, kind, K, d, R + 1)
        index = _index(faiss, cent, metric)
        D_ref, I_ref = _ref(cent, X_all, metric)
        x_dev = torch.from_numpy(X_all).cuda()
        for n in (1, 15, 16, 17, R - 1, R, R + 1):
            # outputs with a guard row behind n, through the C ABI: a write past n would land on it
            D = torch.full((n + 1, 1), -7.0, dtype=torch.float32, device="cuda")
            I = torch.full((n + 1, 1), -7, dtype=torch.int64, device="cuda")
            x = x_dev[:n].clone()  # its own allocation: the row behind n - 1 is not this test's
            _call(index, x, n, D, I)
            torch.cuda.synchronize()
            assert float(D[n, 0]) == -7.0 and int(I[n, 0]) == -7, f"n={n}: wrote behind n"
            assert_knn_identical(D[:n].cpu().numpy(), I[:n].cpu().numpy(), D_ref[:n], I_ref[:n], f"d={d} n={n} {kind}")


def _call(index, x, n, D, I):
    """ise_index_assign_device on the current stream; D may be None."""
    import torch

    from image_search_engine_amd import _native

    assert x.is_contiguous() and x.dtype == torch.float32
    st = torch.cuda.current_stream(x.device).cuda_stream
    _native.check(_native.lib.ise_index_assign_device(index._h, x.data_ptr(), n, None if D is None else D.data_ptr(),
                                                      I.data_ptr(), st))


# ---------------------------------------------------------------------------------------- 3. misaligned x
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [64, 192, 512])
def test_misaligned_rows_take_the_scalar_load(faiss, d, metric):
    """d % 4 == 0, but the rows start one float into a device buffer: contiguous, 4 bytes past a 16-byte boundary.
    The scalar load must answer exactly what the vector load answers for the aligned copy."""
    import torch

    n, K = block_rows(d) + 16 + 3, 77
    rng = _rng("misaligned", d, metric)
    cent, X = _tied_case(rng, "small", K, d, n)
    index = _index(faiss, cent, metric)
    D_ref, I_ref = _ref(cent, X, metric)
    buf = torch.zeros(n * d + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = buf[1:1 + n * d].view(n, d)
    x.copy_(torch.from_numpy(X))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    Dm, Im = index.assign_torch(x)
    Da, Ia = index.assign_torch(torch.from_numpy(X).cuda())
    assert torch.equal(Im, Ia) and torch.equal(Dm.view(torch.int32), Da.view(torch.int32))
    assert_knn_identical(Dm.cpu().numpy(), Im.cpu().numpy(), D_ref, I_ref, f"misaligned d={d}")


# ------------------------------------------------------------------------------------------ 4. stage edges
STAGE_D = {64: 61, 320: 320, 384: 383, 448: 448, 512: 449}  # dp -> d: both load paths among them
STAGE_CS = {64: 128, 320: 112, 384: 96, 448: 80, 512: 64}    # the issue's hand reading of assign_stage_rows


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("dp", sorted(STAGE_D))
def test_stage_edges(faiss, dp, metric):
    """K at 1, around one 16-centroid tile, around one LDS stage of CS centroids and just past two stages.  Some rows
    win at the last centroid of a stage, others at the first of the next (both stage boundaries where K reaches them):
    L2 rows are copies of that centroid; inner-product rows are one-hot in a column where only that centroid is not
    zero.  The remaining rows are random and win anywhere."""
    d = STAGE_D[dp]
    CS = assign_stage_rows(dp)
    assert pad_dim(d) == dp and CS == STAGE_CS[dp] and CS % 16 == 0 and CS >= 16
    n = 150
    # ("signed": scores below zero, which the zero rows that fill a ragged stage would beat if they were not masked)
    for K, kind in [(K, kind) for K in (1, 15, 16, 17, CS - 1, CS, CS + 1, 2 * CS + 1) for kind in ("small", "signed")]:
        rng = _rng("stage", dp, metric, K, kind)
        cent, X = int_data(kind, rng, K, d), int_data(kind, rng, n, d)
        targets = sorted({t for t in (0, 15, 16, CS - 1, CS, 2 * CS - 1, 2 * CS, K - 1) if t < K})
        for j, t in enumerate(targets):
            rows = [3 + j, 40 + j, n - 1 - j]
            if metric == L2:
                X[rows] = cent[t]
            else:
                cent[:, j] = 0.0
                cent[t, j] = 1.0
                X[rows] = 0.0
                X[rows, j] = 1.0
        index = _index(faiss, cent, metric)
        D_ref, I_ref = _ref(cent, X, metric)
        for j, t in enumerate(targets):  # the premise: those rows win where they were planted
            assert (I_ref[[3 + j, 40 + j, n - 1 - j], 0] == t).all(), (K, t)
        if K > CS:
            assert {CS - 1, CS} <= set(I_ref[:, 0].tolist())
        assert_knn_identical(*_assign(index, X), D_ref, I_ref, f"dp={dp} K={K} {kind}")


# ------------------------------------------------------------------------------- 5. a second slab per block
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [16, 192, 257])
def test_second_slab_per_block(faiss, d, metric):
    """n = 2 cu R + 77 rows (R: a block's rows per slab) against a grid of at most cu blocks: every block takes a
    second slab, some a third.  The rows are drawn, on the device, from a pool of 2048 integer rows, so the oracle's
    answer for the pool is the oracle's answer for every row; all n results are compared.  The outputs go in
    pre-filled, so a slab nobody took shows as the fill value and not as a stale answer."""
    import torch

    cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    R = block_rows(d)
    assert R == {16: 512, 192: 256, 257: 128}[d]
    n = 2 * cu * R + 77
    assert n > cu * R, "a grid of cu blocks must need a second slab"
    K, P = 33, 2048
    rng = _rng("slab", d, metric)
    cent, pool = int_data("small", rng, K, d), int_data("small", rng, P, d)
    plant_ties(cent, 2, [17, 18, 32])  # 18: the lane of id 2
    pool[:8] = cent[2]
    D_pool, I_pool = np.empty((P, 1), np.float32), np.empty((P, 1), np.int64)
    for i0 in range(0, P, 512):  # the oracle in row chunks
        D_pool[i0:i0 + 512], I_pool[i0:i0 + 512] = _ref(cent, pool[i0:i0 + 512], metric)
    if metric == L2:
        assert (I_pool[:8, 0] == 2).all()
    index = _index(faiss, cent, metric)
    idx = torch.from_numpy(rng.integers(0, P, n)).cuda()
    x = torch.from_numpy(pool).cuda()[idx].contiguous()
    assert x.shape == (n, d) and x.data_ptr() % 16 == 0
    D = torch.full((n, 1), -7.0, dtype=torch.float32, device="cuda")
    I = torch.full((n, 1), -7, dtype=torch.int64, device="cuda")
    _call(index, x, n, D, I)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()
    assert len(np.unique(idx[cu * R:])) > P // 2  # the later slabs see (nearly) the whole pool
    assert_knn_identical(D.cpu().numpy(), I.cpu().numpy(), D_pool[idx], I_pool[idx], f"d={d} n={n}")


# -------------------------------------------------------- 6. shifted L2 on real values off the vector path
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [17, 130, 257, 449])
def test_real_values_off_the_vector_path(faiss, d, metric, capsys):
    """The data and tolerance of tests/test_knn_gpu.py::test_assignment_kernel_matches_oracle (SIFT-valued rows,
    unit-norm centroids, the index's own shift) at row lengths that take the scalar load."""
    n, K = 2100, 130
    assert d % 4 != 0
    rng = np.random.default_rng(n + K + d + metric)
    cent = ko.normalize_rows(rng.standard_normal((K, d)).astype(np.float32))
    X = rng.integers(0, 256, (n, d)).astype(np.float32)
    index = _index(faiss, cent, metric, zero_shift=False)
    D, I = _assign(index, X)
    D_ref, I_ref = ko.knn_exact(cent, X, 1, metric)
    rel = np.abs(D.astype(np.float64) - D_ref) / np.maximum(1.0, np.abs(D_ref.astype(np.float64)))
    with capsys.disabled():
        print(f"\nassign d={d} metric={'L2' if metric == L2 else 'IP'}: largest relative error {rel.max():.3e} "
              f"(bound 2e-4), id mismatches {(I != I_ref).sum()}")
    assert_knn_matches(D, I, D_ref, I_ref, cent, X, metric, gap=ko.kth_gap(cent, X, 1, metric), rtol=2e-4)


# --------------------------------------------------------------------------------------- 7. D_dev == NULL
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [29, 192])
def test_null_distances(faiss, d, metric):
    """The ABI allows D_dev == NULL: the ids are those of the call with D."""
    import torch

    n, K = block_rows(d) + 16 + 3, 77
    rng = _rng("null", d, metric)
    cent, X = _tied_case(rng, "small", K, d, n)
    index = _index(faiss, cent, metric)
    D_ref, I_ref = _ref(cent, X, metric)
    x = torch.from_numpy(X).cuda()
    D, I = index.assign_torch(x)
    I0 = torch.full((n, 1), -7, dtype=torch.int64, device="cuda")
    _call(index, x, n, None, I0)
    torch.cuda.synchronize()
    assert torch.equal(I0, I)
    assert_knn_identical(D.cpu().numpy(), I0.cpu().numpy(), D_ref, I_ref, f"null D d={d}")


# ------------------------------------------------------------------------------------------- 8. routing
@pytest.mark.parametrize("metric", [IP, L2])
def test_search_routes_a_scalar_path_d(faiss, metric):
    """index.search(X, 1) with 2048 rows or more goes to the assignment kernel, 64 rows go to the general scan (the
    short-index kernel): both identical to the oracle at d = 45, which neither loads by vector."""
    d, K, n = 45, 256, 2100
    rng = _rng("route", metric)
    cent, X = _tied_case(rng, "small", K, d, n)
    index = _index(faiss, cent, metric)
    assert index._assign_applies(n, 1) and not index._assign_applies(64, 1)
    D_ref, I_ref = _ref(cent, X, metric)
    before = index.short_stats()["short_batches"]
    assert_knn_identical(*index.search(X, 1), D_ref, I_ref, "search, n >= ASSIGN_MIN_NQ")
    assert index.short_stats()["short_batches"] == before, "the assignment kernel answers large k = 1 batches"
    assert_knn_identical(*index.search(X[:64], 1), D_ref[:64], I_ref[:64], "search, 64 rows")
    assert index.short_stats()["short_batches"] == before + 1
