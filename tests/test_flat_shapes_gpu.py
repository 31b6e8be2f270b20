"""GPU tests of the flat index's range pass (csrc/ise_range.hpp, range_scan_kernel; csrc/ise_flat_range.hip, range_batch)
and its selector-filtered pass (csrc/ise_sel_scan.hpp, sel_scan_kernel; csrc/ise_flat_sel.hip, sel_chunk_enqueue) at every
row-length class, for float32 and bf16 rows: the register chunk ch = 1, 2, 4, scalar and vector query staging
(range_stage_queries), rows so long that a masked pass keeps fewer than 32 results (kp) and that the streaming plan
drops to 4 waves (16 threads per query row), the length the index refuses, range searches of more than 256 queries and
filtered searches of more than 64, and windows, indexes and bitmaps that end inside a tile.

The data are small integers (tests/knn_checks.py), so every score is exact in float32 and in bf16 in any summation
order.  Every expected result is a float64 brute force in numpy (tests/range_ref.py, tests/sel_ref.py) and never comes
from the index; every comparison is bit for bit, ties by ascending id.  The Python mirrors of the host's geometry only
choose inputs and assert that a case reaches the path it is meant for.  The builders of the cases (sweep_case, kp_case,
...) need no GPU: tests/test_flat_shapes.py checks on the CPU that the chosen radii and selectors are not vacuous."""
import contextlib
import zlib

import numpy as np
import pytest

from image_search_engine_amd import _native as native
from image_search_engine_amd import faiss_compat as faiss
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data, INT_KINDS
from tests.range_ref import (assert_range_identical, assert_range_shape, range_of_scores, scores_f64,
                             segment_hits_max)
from tests.sel_ref import IP, L2, knn_of_scores, pad_value, selector_census
from tests.test_assign_shapes_gpu import pad_dim, qs_stride_units
from tests.test_ivf_shapes_gpu import LDS_LIMIT, SEL_KPASS_MAX, kp_cap, range_lds_bytes

pytestmark = pytest.mark.gpu

FLAVOURS = [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")]
RANGE_NQ_CHUNK = 256  # csrc/ise_flat_range.hip: queries per range batch
SEL_NQ_CHUNK = 64     # csrc/ise_flat_sel.hip: queries per masked launch
N, NQ = 600, 17       # 37.5 tiles: a partial last tile; one full query tile and one query


# ------------------------------------------------------------------ mirrors of the host geometry (inputs and premises only)
def row_bytes(d, storage):
    """csrc/ise_geometry.hpp, pad_dim times the element size: whole 64-byte k-steps (16 floats, 32 bf16), in fours
    beyond four."""
    if storage == "f32":
        return pad_dim(d) * 4
    steps = -(-d // 32)
    return (steps if steps <= 4 else -(-steps // 4) * 4) * 64


def stride(d, storage):
    """csrc/ise_flat.hpp, qs_stride_for: the LDS query row stride in 4-byte units, from row_bytes / 4."""
    return qs_stride_units(row_bytes(d, storage) // 4)


def chunk_steps(d, storage):
    """chunk_steps_rb capped at 4, as range_batch and sel_chunk_enqueue cap it: k-steps per register chunk."""
    steps = row_bytes(d, storage) // 64
    return next((min(ch, 4) for ch in (8, 4, 2) if steps % ch == 0), 1)


def plan_waves(d, storage):
    """Waves of the one-tile streaming plan (csrc/ise_knn.hip, range_staging -> make_plan(h, 16, 1): T = 1, kb = 16, no
    shadow rows): 8 if lds_bytes(8, 1) = scan_lds_layout(S, 8, 1, 16) fits the 160 KiB, else 4, else 0 -- the refusal."""
    S = stride(d, storage)
    for w in (8, 4):
        if S * 4 + 16 * (S * 4 + 4 + 8 + 8 + w * 4 + 16 * 8 + w * 16 * 8) <= LDS_LIMIT:
            return w
    return 0


def vec_staging(d, storage):
    """csrc/ise_geometry.hpp, range_staging_rule: 32 threads per query row behind an 8-wave plan, else 16; float32
    rows d % 4 == 0 and (S >> 2) <= 8 tpr, bf16 rows d % 8 == 0 and (S >> 2) <= 4 tpr."""
    tpr = 32 if plan_waves(d, storage) >= 8 else 16
    S4 = stride(d, storage) >> 2
    return int(d % 4 == 0 and S4 <= 8 * tpr) if storage == "f32" else int(d % 8 == 0 and S4 <= 4 * tpr)


def klass(d, storage):
    return chunk_steps(d, storage), vec_staging(d, storage)


def flat_kp(d, storage):
    """Results per masked pass the wave lists' LDS holds beside the query rows (sel_chunk_enqueue), before the cap of
    32.  For float32 rows this is kp_cap of the inverted-list suite."""
    return int((LDS_LIMIT - range_lds_bytes(stride(d, storage))) / 1024)


def sel_passes(d, storage, k, nq):
    """Masked passes of one filtered search: per launch of up to 64 queries, one pass per kp results."""
    return -(-nq // SEL_NQ_CHUNK) * -(-k // min(k, SEL_KPASS_MAX, flat_kp(d, storage)))


# d -> (ch, vec_q).  1000 is a multiple of 4 and of 8 that the scalar path stages: its stride is past what the threads of
# a query row cover in 16-byte slots
SWEEP = {"f32": {1: (1, 0), 33: (1, 0), 48: (1, 1), 17: (2, 0), 32: (2, 1), 63: (4, 0), 65: (4, 0), 600: (4, 1),
                 1000: (4, 0)},
         "bf16": {17: (1, 0), 32: (1, 1), 33: (2, 0), 64: (2, 1), 100: (4, 0), 600: (4, 1), 1000: (4, 0)}}
SWEEP_CASES = [(m, s, d) for m, s in FLAVOURS for d in sorted(SWEEP[s])]
KP_HAND = {"f32": {1920: 31, 2048: 23, 2240: 10}, "bf16": {3840: 31, 4096: 23, 4480: 10}}
KP_CASES = [(m, s, d) for m, s in FLAVOURS for d in sorted(KP_HAND[s])]
D_MAX = {"f32": 2240, "bf16": 4480}
# The streaming plan has 4 waves, and range_staging_rule 16 threads per query row, where lds_bytes(8, 1) no longer fits:
# strides above 2126 units, that is padded rows of more than 8448 bytes.  tests/test_exact_l2_gpu.py,
# test_long_rows_four_wave_blocks, names the same windows; the d = 2177 .. 2240 of tests/test_half_filter_gpu.py,
# test_lds_limit_rows_keep_the_float32_filter, is the narrower window in which a SHADOW kernel's image does not fit.
FOUR_WAVES = {"f32": range(2113, 2241), "bf16": range(4225, 4481)}
SCALAR_D = {"f32": 33, "bf16": 17}  # one scalar-staged d per storage (query and edge cases)
KINDS = ("small", "binary")


def test_geometry_mirrors():
    """The constants the cases below are built on, as read off the host code."""
    for storage in ("f32", "bf16"):
        assert {klass(d, storage) for d in SWEEP[storage]} == {(ch, v) for ch in (1, 2, 4) for v in (0, 1)}
        assert all(klass(d, storage) == c for d, c in SWEEP[storage].items())
        assert {d: flat_kp(d, storage) for d in KP_HAND[storage]} == KP_HAND[storage]
        assert [d for d in range(1, 5000) if plan_waves(d, storage) == 4] == list(FOUR_WAVES[storage])
        assert plan_waves(D_MAX[storage], storage) == 4 and plan_waves(D_MAX[storage] + 1, storage) == 0
    assert all(flat_kp(d, "f32") == kp_cap(d) for d in (17, 1000, 1920, 2048, 2240))


# ------------------------------------------------------------------------------------------------ helpers
def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


class EveryThird(faiss.IDSelector):
    def is_member(self, i):
        return int(i) % 3 == 0

    def members(self, ids):
        return np.asarray(ids, dtype=np.int64) % 3 == 0


class Masked(faiss.IDSelector):
    """The rows a bool array names (lowered to a bitmap)."""

    def __init__(self, mask):
        self.mask = np.asarray(mask, dtype=bool)

    def members(self, ids):
        return self.mask[np.asarray(ids, dtype=np.int64)]


def sweep_selectors(n):
    return {"inside": faiss.IDSelectorRange(123, 411),  # starts and ends mid-tile
            "third": EveryThird(),
            "tenth": faiss.IDSelectorBatch(_rng("tenth", n).choice(n, n // 10, replace=False)),
            "two_pieces": faiss.IDSelectorNot(faiss.IDSelectorRange(100, 500)),
            "all": faiss.IDSelectorRange(0, n)}


def P(sel):
    return faiss.SearchParameters(sel=sel)


def make_index(xb, metric, storage):
    idx = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    idx.add(xb)
    return idx


def few_radius(S, metric):
    """A half-integer radius at which every query keeps at least 1 and at most 50 rows, and whether one exists (the
    scores are integers).  Prefers a second score level where that still fits."""
    key = np.sort(S if metric == L2 else -S, axis=1)
    lo = key[:, 0].max()                                    # above every query's best score
    hi = key[:, 50].min() if key.shape[1] > 50 else np.inf  # at most every query's 51st
    r = np.floor(lo) + 0.5
    if r + 1 <= hi:
        r += 1
    return float(r if metric == L2 else -r), bool(r <= hi)


def sweep_radii(S, metric):
    """The four radii of a sweep case, chosen from the brute-force scores."""
    flat = np.sort(S.ravel())
    levels = np.unique(flat)
    # an attained score near the best quarter that has a better level, so that rows remain inside it
    q = max(flat[len(flat) // 4], levels[1]) if metric == L2 else min(flat[-(len(flat) // 4)], levels[-2])
    return {"none": float(S.min() - 0.5 if metric == L2 else S.max() + 0.5),
            "few": few_radius(S, metric)[0],
            "median": float(np.floor(np.median(S)) + 0.5),
            "attained": float(q)}  # strict comparison: the rows at exactly this score stay out


def similar_queries(kind, rng, d, nq):
    """nq queries of a pool of 24 nq whose entries sum to nearly the same: inner products grow with the query's
    length, and one radius keeps a few rows of every query only if the lengths are alike."""
    pool = int_data(kind, rng, 24 * nq, d)
    pool = pool[pool.sum(axis=1) > 0]  # an all-zero query scores every row 0: no radius keeps a few
    order = np.argsort(pool.sum(axis=1), kind="stable")
    mid = len(pool) // 2
    return np.ascontiguousarray(pool[rng.permutation(order[mid - nq // 2:mid - nq // 2 + nq])])


def sweep_case(metric, storage, d, kind, n=N, nq=NQ):
    """Rows, queries, the float64 scores and the radii of one sweep case.  Row 77 is query 0.  L2: every query has a
    copy and a row at distance 1 among the rows; inner product: queries of similar sums (similar_queries)."""
    rng = _rng("sweep", metric, storage, d, kind)
    xb = int_data(kind, rng, n, d)
    lo, hi = INT_KINDS[kind]
    if metric == L2:
        xq = int_data(kind, rng, nq, d)
        homes = rng.choice(np.setdiff1d(np.arange(n), [77]), 2 * nq, replace=False)
        xb[homes[:nq]] = xq
        xb[homes[nq:]] = xq
        xb[homes[nq:], 0] += np.where(xq[:, 0] < hi, 1, -1).astype(np.float32)
    else:
        xq = similar_queries(kind, rng, d, nq)
    xb[77] = xq[0]
    assert_exact_range(xb, xq)
    S = scores_f64(xb, xq, metric)
    return {"xb": xb, "xq": xq, "S": S, "radii": sweep_radii(S, metric)}


@contextlib.contextmanager
def stage_cap(monkeypatch, cap):
    """ISE_RANGE_STAGE_CAP for the calls inside, set and refreshed as tests/test_range_search_gpu.py does."""
    monkeypatch.setenv("ISE_RANGE_STAGE_CAP", str(cap))
    native.lib.ise_refresh_env_knobs()
    try:
        yield
    finally:
        monkeypatch.delenv("ISE_RANGE_STAGE_CAP")
        native.lib.ise_refresh_env_knobs()


def segments_are_tiles(n):
    """range_batch gives every block one tile while the tiles are no more than 4 per CU, and the block's wave 0 takes
    it: a wave segment is then one tile, 16 rows."""
    import torch

    return -(-n // 16) <= 4 * torch.cuda.get_device_properties(0).multi_processor_count


def checked_range(idx, xq, radius, want, what, sel=None, overflow=0):
    """range_search against the expected (lims, D, I), with the batch and overflow counters asserted."""
    rb, sb = idx.range_stats(), idx.sel_stats()
    got = idx.range_search(xq, radius) if sel is None else idx.range_search(xq, radius, params=P(sel))
    ra, sa = idx.range_stats(), idx.sel_stats()
    assert_range_shape(*got, len(xq), idx.ntotal)
    assert_range_identical(got, want, what)
    batches = -(-len(xq) // RANGE_NQ_CHUNK)
    assert ra["range_batches"] - rb["range_batches"] == (batches if sel is None else 0), what
    assert sa["sel_range_batches"] - sb["sel_range_batches"] == (0 if sel is None else batches), what
    assert ra["range_overflow_batches"] - rb["range_overflow_batches"] == overflow, what
    return got


def checked_search(idx, d, storage, xq, k, sel, want, what):
    """search(params=sel) against the expected (D, I), with one batch and ceil(k / kp) passes per chunk asserted."""
    before = idx.sel_stats()
    D, I = idx.search(xq, k, params=P(sel))
    after = idx.sel_stats()
    assert_knn_identical(D, I, *want, what)
    assert after["sel_batches"] - before["sel_batches"] == 1, what
    assert after["sel_passes"] - before["sel_passes"] == sel_passes(d, storage, k, len(xq)), what


def check_selector(idx, ds, members):
    info, want = ds.info(), selector_census(members)
    assert info["ntotal"] == idx.ntotal and info["selected"] == want["selected"]
    assert info["window"] == want["window"] and info["tiles"] == want["tiles"]


# ------------------------------------------------------------------------------------ 1. row-length sweep
@pytest.mark.parametrize("metric,storage,d", SWEEP_CASES)
def test_row_length_sweep(metric, storage, d, monkeypatch):
    """600 rows, 1 and 17 queries.  Unfiltered range search at four radii, the same with a staging capacity of 1 (the
    second pass wherever a tile holds two hits of a query), and range search and search under five selectors."""
    assert klass(d, storage) == SWEEP[storage][d]
    assert min(SEL_KPASS_MAX, flat_kp(d, storage)) == 32 and segments_are_tiles(N)
    sels = sweep_selectors(N)
    for kind in KINDS:
        c = sweep_case(metric, storage, d, kind)
        xq, S = c["xq"], c["S"]
        idx = make_index(c["xb"], metric, storage)
        calls = [(name, r, nq) for name, r in c["radii"].items() for nq in (1, NQ)]
        wants = {(name, nq): range_of_scores(S[:nq], r, metric) for name, r, nq in calls}
        for name, r, nq in calls:
            checked_range(idx, xq[:nq], r, wants[name, nq], f"d={d} {kind} {name} nq={nq}")
        with stage_cap(monkeypatch, 1):
            for name, r, nq in calls:
                checked_range(idx, xq[:nq], r, wants[name, nq], f"d={d} {kind} {name} nq={nq} cap=1",
                              overflow=int(segment_hits_max(wants[name, nq]) >= 2))
        for sname, sel in sels.items():
            m = sel.members(np.arange(N))
            ds = idx.make_selector(sel)
            check_selector(idx, ds, m)
            for name, r, nq in calls:
                checked_range(idx, xq[:nq], r, range_of_scores(S[:nq], r, metric, m), f"d={d} {kind} {sname} {name} nq={nq}",
                              sel=ds)
            Dw, Iw = knn_of_scores(S, m, 70, metric)
            for nq in (1, NQ):
                for k in (1, 10, 33, 70):
                    checked_search(idx, d, storage, xq[:nq], k, ds, (Dw[:nq, :k], Iw[:nq, :k]),
                                   f"d={d} {kind} {sname} nq={nq} k={k}")
            want = range_of_scores(S, c["radii"]["median"], metric, m)
            with stage_cap(monkeypatch, 1):  # the masked second pass
                checked_range(idx, xq, c["radii"]["median"], want, f"d={d} {kind} {sname} median cap=1", sel=ds,
                              overflow=int(segment_hits_max(want) >= 2))


# --------------------------------------------------------------------------------------- 2. shrinking kp
TIES = 40


def kp_case(metric, storage, d):
    """300 binary rows: 40 all-ones rows at ids 0 .. 39 tie at the top for the all-ones query (and for query 1, which
    has one zero), every other row has four zeros at least.  Selectors: every second member of the tie group masked
    out -- ties skipped by mask, not by score -- and all rows."""
    n = 300
    rng = _rng("kp", metric, storage, d)
    xb = (rng.random((n, d)) < 0.6).astype(np.float32)
    xb[:, :4] = 0.0
    xb[:TIES] = 1.0
    xq = (rng.random((NQ, d)) < 0.6).astype(np.float32)
    xq[0] = 1.0
    xq[1] = 1.0
    xq[1, 0] = 0.0  # still ranks the group first: distance 1, score d - 1
    assert_exact_range(xb, xq)
    half = np.ones(n, bool)
    half[1:TIES:2] = False
    S = scores_f64(xb, xq, metric)
    radii = {"ties": 0.5 if metric == L2 else d - 0.5,  # admits exactly the tie group, for query 0 alone
             "median": float(np.floor(np.median(S)) + 0.5)}
    return {"xb": xb, "xq": xq, "S": S, "radii": radii, "masks": {"half": half, "all": np.ones(n, bool)}}


@pytest.mark.parametrize("metric,storage,d", KP_CASES)
def test_shrinking_kp(metric, storage, d, monkeypatch):
    """Rows so long that a masked pass keeps fewer than 32 results per query: the wave lists, the block fold's i / kp
    and i % kp and the floor-keyed later passes all run at that kp, and with k beyond kp the second pass's floor falls
    inside the tie group.  The longest d of each storage is where the plan's 4 waves stage with 16 threads per query
    row (FOUR_WAVES; no statistic of the index exposes the plan's waves, so the mirror is all there is to assert)."""
    kp = flat_kp(d, storage)
    assert kp == KP_HAND[storage][d] and TIES > kp and klass(d, storage) == (4, 0)
    assert (d in FOUR_WAVES[storage]) == (d == D_MAX[storage])
    assert [sel_passes(d, storage, k, NQ) for k in (1, kp, kp + 1, 2 * kp + 1)] == [1, 1, 2, 3]
    c = kp_case(metric, storage, d)
    xq, S = c["xq"], c["S"]
    n = len(c["xb"])
    assert segments_are_tiles(n)
    idx = make_index(c["xb"], metric, storage)
    for mname, m in c["masks"].items():
        ds = idx.make_selector(Masked(m))
        check_selector(idx, ds, m)
        Dw, Iw = knn_of_scores(S, m, 2 * kp + 1, metric)
        for nq in (1, NQ):
            for k in (1, kp, kp + 1, 2 * kp + 1):
                checked_search(idx, d, storage, xq[:nq], k, ds, (Dw[:nq, :k], Iw[:nq, :k]), f"d={d} {mname} nq={nq} k={k}")
        for name, r in c["radii"].items():
            for nq in (1, NQ):
                checked_range(idx, xq[:nq], r, range_of_scores(S[:nq], r, metric, m), f"d={d} {mname} {name} nq={nq}", sel=ds)
                if mname == "all":
                    checked_range(idx, xq[:nq], r, range_of_scores(S[:nq], r, metric), f"d={d} unmasked {name} nq={nq}")
        want = range_of_scores(S, c["radii"]["ties"], metric, m)
        with stage_cap(monkeypatch, 1):
            checked_range(idx, xq, c["radii"]["ties"], want, f"d={d} {mname} ties cap=1", sel=ds, overflow=1)


# ------------------------------------------------------------------------------------ 3. the length limit
@pytest.mark.parametrize("metric,storage", FLAVOURS)
def test_rows_too_long_are_refused_by_the_plan(metric, storage):
    """One column past the longest row: adding and make_selector succeed (neither plans a pass), and range_search,
    range_search(params=) and search(params=) all raise make_plan's "d too large" from range_staging -- before
    sel_chunk_enqueue's own kp < 1 test, which no flat index reaches.  The index is left as it was."""
    d = D_MAX[storage] + 1
    assert plan_waves(d, storage) == 0 and flat_kp(d, storage) >= 1
    rng = _rng("refusal", metric, storage)
    xb, xq = int_data("binary", rng, 50, d), int_data("binary", rng, 3, d)
    idx = make_index(xb, metric, storage)
    ds = idx.make_selector(faiss.IDSelectorRange(5, 40))
    check_selector(idx, ds, (np.arange(50) >= 5) & (np.arange(50) < 40))
    for call in (lambda: idx.range_search(xq, 10.0),
                 lambda: idx.range_search(xq, 10.0, params=P(ds)),
                 lambda: idx.search(xq, 1, params=P(ds)),
                 lambda: idx.search(xq, 10, params=P(faiss.IDSelectorRange(5, 40)))):
        with pytest.raises(native.IseError, match="d too large"):
            call()
    assert idx.ntotal == 50 and np.array_equal(idx.reconstruct_n(0, 50), xb)
    idx.add(xb[:5])
    assert idx.ntotal == 55 and np.array_equal(idx.reconstruct_n(50, 5), xb[:5])


# -------------------------------------------------------------------------------------- 4. query-count edges
def two_batch_case(metric, storage, nq):
    d = 17
    rng = _rng("two batches", metric, storage, nq)
    xb, xq = int_data("small", rng, N, d), int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    S = scores_f64(xb, xq, metric)
    flat = np.sort(S.ravel())
    radii = {"tenth": float(np.floor(flat[len(flat) // 10] if metric == L2 else flat[-(len(flat) // 10)]) + 0.5),
             "median": float(np.floor(np.median(S)) + 0.5)}
    return {"xb": xb, "xq": xq, "S": S, "radii": radii}


@pytest.mark.parametrize("metric,storage", FLAVOURS)
@pytest.mark.parametrize("nq", [256, 257, 300])
def test_range_search_of_two_batches(nq, metric, storage):
    """More than 256 queries are two batches joined on the host: the lims base, the appended D / I, and -- the second
    time round on one index -- a batch that reuses the workspaces the larger one grew."""
    assert klass(17, storage)[1] == 0
    c = two_batch_case(metric, storage, nq)
    idx = make_index(c["xb"], metric, storage)
    assert -(-nq // RANGE_NQ_CHUNK) == {256: 1, 257: 2, 300: 2}[nq]
    third = EveryThird().members(np.arange(N))
    for turn in (0, 1):
        for name, r in c["radii"].items():
            checked_range(idx, c["xq"], r, range_of_scores(c["S"], r, metric), f"nq={nq} {name} turn {turn}")
        r = c["radii"]["median"]
        checked_range(idx, c["xq"], r, range_of_scores(c["S"], r, metric, third), f"nq={nq} third turn {turn}",
                      sel=EveryThird())


def mixed_overflow_case(storage):
    """300 queries, radius 0.5 (L2: exact copies only).  Rows 200 .. 207 -- one tile -- are copies of query 5: 8 hits in
    one segment.  Queries 260 and 299 of the second batch have single copies in tiles of their own."""
    d, nq = 17, 300
    rng = _rng("mixed overflow", storage)
    xb, xq = int_data("small", rng, N, d), int_data("small", rng, nq, d)
    xb[200:208] = xq[5]
    xb[50] = xq[260]
    xb[300] = xq[299]
    xb[420] = xq[299]
    assert_exact_range(xb, xq)
    return {"xb": xb, "xq": xq, "S": scores_f64(xb, xq, L2)}


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_range_batches_mixed_overflow(storage, monkeypatch):
    """Staging capacity 4: the first batch overflows (8 hits of query 5 in one tile) and takes the second pass, the
    second batch has hits but no tile with more than one and takes the compaction."""
    c = mixed_overflow_case(storage)
    want = range_of_scores(c["S"], 0.5, L2)
    lims = want[0].astype(np.int64)
    assert segment_hits_max(want) == 8 and lims[6] - lims[5] == 8
    tail = (want[0][RANGE_NQ_CHUNK:] - want[0][RANGE_NQ_CHUNK], want[1][lims[RANGE_NQ_CHUNK]:], want[2][lims[RANGE_NQ_CHUNK]:])
    assert segment_hits_max(tail) == 1 and len(tail[2]) >= 3
    idx = make_index(c["xb"], L2, storage)
    assert segments_are_tiles(N)
    with stage_cap(monkeypatch, 4):
        checked_range(idx, c["xq"], 0.5, want, "mixed overflow", overflow=1)


def sel_chunks_case(metric, storage, nq):
    d = SCALAR_D["f32"]  # 33: scalar-staged for both storages
    rng = _rng("sel chunks", metric, storage, nq)
    xb, xq = int_data("small", rng, N, d), int_data("small", rng, nq, d)
    rows = np.flatnonzero(EveryThird().members(np.arange(N)))

    def nearest(x):
        return int(knn_of_scores(scores_f64(xb[rows], x[None], metric), np.ones(len(rows), bool), 1, metric)[1][0, 0])

    for q in range(SEL_NQ_CHUNK, nq):  # query q + 64 is drawn again until its nearest selected row is not query q's
        while nearest(xq[q]) == nearest(xq[q - SEL_NQ_CHUNK]):
            xq[q] = int_data("small", rng, 1, d)[0]
    assert_exact_range(xb, xq)
    return {"xb": xb, "xq": xq, "S": scores_f64(xb, xq, metric), "d": d}


@pytest.mark.parametrize("metric,storage", FLAVOURS)
@pytest.mark.parametrize("nq", [64, 65, 130])
def test_filtered_search_of_several_launches(nq, metric, storage):
    """More than 64 queries take several masked launches through one slot's buffers.  Queries q and q + 64 have
    different nearest rows (asserted on the reference), so a result left over from the launch before shows up."""
    c = sel_chunks_case(metric, storage, nq)
    d = c["d"]
    assert klass(d, storage)[1] == 0
    m = EveryThird().members(np.arange(N))
    Dw, Iw = knn_of_scores(c["S"], m, 40, metric)
    assert (Iw[SEL_NQ_CHUNK:, 0] != Iw[:-SEL_NQ_CHUNK, 0]).all()
    chunks = -(-nq // SEL_NQ_CHUNK)
    assert chunks == {64: 1, 65: 2, 130: 3}[nq]
    assert [sel_passes(d, storage, k, nq) for k in (10, 40)] == [chunks, 2 * chunks]
    idx = make_index(c["xb"], metric, storage)
    ds = idx.make_selector(EveryThird())
    for k in (10, 40):
        checked_search(idx, d, storage, c["xq"], k, ds, (Dw[:, :k], Iw[:, :k]), f"nq={nq} k={k}")


# --------------------------------------------------------------------------------- 5. window and tile edges
WINDOWS = {"one tile": (32, 48), "one row": (77, 78), "last partial tile": (592, 600), "rows 15..16": (15, 17)}


def edge_case(metric, storage, n):
    d = SCALAR_D[storage]
    rng = _rng("edges", metric, storage, n)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, NQ, d)
    assert_exact_range(xb, xq)
    S = scores_f64(xb, xq, metric)
    return {"xb": xb, "xq": xq, "S": S, "d": d, "median": float(np.floor(np.median(S)) + 0.5)}


def check_mask(idx, c, metric, storage, sel, m, what):
    """search at k = 1, 10, 33 and range_search at the median radius, at the radii that keep everything and nothing,
    and at NaN, all under one selector."""
    d, S, xq = c["d"], c["S"], c["xq"]
    Dw, Iw = knn_of_scores(S, m, 33, metric)
    for nq in (1, NQ):
        for k in (1, 10, 33):
            checked_search(idx, d, storage, xq[:nq], k, sel, (Dw[:nq, :k], Iw[:nq, :k]), f"{what} nq={nq} k={k}")
        for r in (c["median"], np.inf, -np.inf, np.nan):
            checked_range(idx, xq[:nq], r, range_of_scores(S[:nq], r, metric, m), f"{what} nq={nq} radius {r}", sel=sel)
    everything = np.inf if metric == L2 else -np.inf
    assert np.array_equal(idx.range_search(xq[:1], everything, params=P(sel))[2], np.flatnonzero(m)), what


@pytest.mark.parametrize("metric,storage", FLAVOURS)
def test_windows_inside_and_across_tiles(metric, storage):
    c = edge_case(metric, storage, N)
    assert klass(c["d"], storage)[1] == 0
    idx = make_index(c["xb"], metric, storage)
    for what, (a, b) in WINDOWS.items():
        m = (np.arange(N) >= a) & (np.arange(N) < b)
        ds = idx.make_selector(faiss.IDSelectorRange(a, b))
        check_selector(idx, ds, m)
        check_mask(idx, c, metric, storage, ds, m, what)


@pytest.mark.parametrize("metric,storage", FLAVOURS)
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_indexes_of_a_tile_or_less(n, metric, storage):
    c = edge_case(metric, storage, n)
    idx = make_index(c["xb"], metric, storage)
    for what, m in (("all", np.ones(n, bool)), ("last row", np.arange(n) == n - 1), ("even", np.arange(n) % 2 == 0)):
        ds = idx.make_selector(Masked(m))
        check_selector(idx, ds, m)
        check_mask(idx, c, metric, storage, ds, m, f"n={n} {what}")
    for r in (c["median"], np.inf, -np.inf):
        checked_range(idx, c["xq"], r, range_of_scores(c["S"], r, metric), f"n={n} unmasked radius {r}")


def bitmap_words(m, garbage):
    """The bitmap of the bool mask m with every bit at or beyond len(m) of its last word set where ``garbage``."""
    words = faiss._bitmap_words(m).copy()
    if garbage and len(m) % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (len(m) % 32)) & 0xFFFFFFFF)
    return words


@pytest.mark.parametrize("metric,storage", FLAVOURS)
@pytest.mark.parametrize("n", [17, N])
def test_bitmap_bits_beyond_ntotal_are_cleared(n, metric, storage):
    """A caller's bitmap (ise_selector_create_bitmap) with every bit from ntotal to the end of its last word set: the
    census clears them, so the selector counts, and the passes return, real rows only -- the last tile's included."""
    c = edge_case(metric, storage, n)
    idx = make_index(c["xb"], metric, storage)
    for what, m in (("third", EveryThird().members(np.arange(n))), ("last row", np.arange(n) == n - 1),
                    ("none", np.zeros(n, bool))):
        words = bitmap_words(m, True)
        assert int(words[-1]) >> (n % 32) == (1 << (32 - n % 32)) - 1
        ds = faiss.DeviceSelector(idx, ("bitmap", words))
        check_selector(idx, ds, m)
        if m.any():
            check_mask(idx, c, metric, storage, ds, m, f"n={n} {what}")
        else:
            D, I = idx.search(c["xq"], 3, params=P(ds))
            assert (I == -1).all() and (D == pad_value(metric)).all()
            assert idx.range_search(c["xq"], c["median"], params=P(ds))[0].tolist() == [0] * (NQ + 1)
