"""GPU tests of the selector-filtered search and range search (csrc/ise_sel_scan.hpp).  Every comparison is bit for
bit, against (A) the complete ranking of the unfiltered index filtered on the host, or (B) a fresh index of the
selected rows (tests/sel_ref.py)."""
import threading

import numpy as np
import pytest

from image_search_engine_amd import _native
from image_search_engine_amd import faiss_compat as faiss
from oracle import knn_oracle as ko
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data, plant_ties, poison
from tests.range_ref import assert_range_identical, assert_range_shape
from tests.sel_ref import IP, L2, filter_range, filter_ranking, pad_value, selector_census, sub_index_search

pytestmark = pytest.mark.gpu

STORAGES = [(L2, "f32"), (IP, "f32"), (L2, "bf16"), (IP, "bf16")]
N = 600  # 37.5 tiles: a partial last tile


class EveryThird(faiss.IDSelector):
    def is_member(self, i):
        return int(i) % 3 == 0

    def members(self, ids):
        return np.asarray(ids, dtype=np.int64) % 3 == 0


def P(sel):
    return faiss.SearchParameters(sel=sel)


def make_index(xb, metric, storage):
    idx = faiss.IndexFlat(xb.shape[1], metric, storage=storage)
    idx.add(xb)
    return idx


def selectors(n, rng):
    return {
        "all": faiss.IDSelectorRange(0, n),
        "one": faiss.IDSelectorRange(5, 6),
        "inside": faiss.IDSelectorRange(123, 411),
        "batch10": faiss.IDSelectorBatch(rng.choice(n, n // 10, replace=False)),
        "not_one": faiss.IDSelectorNot(faiss.IDSelectorBatch([77])),
        "two_pieces": faiss.IDSelectorNot(faiss.IDSelectorRange(100, 500)),
        "third": EveryThird(),
        "empty": faiss.IDSelectorRange(7, 7),
        "outside": faiss.IDSelectorBatch([-3, n, n + 40, 1 << 40]),
    }


def data(metric, storage, n, d, nq, seed):
    rng = np.random.default_rng(seed)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    if metric == IP and storage == "bf16":
        faiss.normalize_L2(xb)
        faiss.normalize_L2(xq)
    return xb, xq


@pytest.mark.parametrize("metric,storage", STORAGES)
@pytest.mark.parametrize("d", [20, 128])
def test_parity_sweep(metric, storage, d):
    xb, xq = data(metric, storage, N, d, 40, 100 + d)
    idx = make_index(xb, metric, storage)
    sels = selectors(N, np.random.default_rng(5))
    full = {nq: idx.search(xq[:nq], N) for nq in (1, 16, 17, 40)}  # (A): the complete ranking, computed once
    for name, sel in sels.items():
        m = sel.members(np.arange(N))
        ds = idx.make_selector(sel)
        info = ds.info()
        want = selector_census(m)
        assert info["ntotal"] == N and info["selected"] == want["selected"] and info["tiles"] == want["tiles"], name
        assert info["window"] == want["window"], name
        before = idx.sel_stats()
        calls = 0
        for nq in (1, 16, 17, 40):
            for k in (1, 10, 33, 70):
                D, I = idx.search(xq[:nq], k, params=P(ds))
                Dw, Iw = filter_ranking(*full[nq], sel.members, k, metric)
                assert_knn_identical(D, I, Dw, Iw, f"{name} nq={nq} k={k}")
                calls += 1
        assert idx.sel_stats()["sel_batches"] - before["sel_batches"] == calls
        if name in ("empty", "outside"):  # an empty selection launches no pass
            assert idx.sel_stats()["sel_passes"] == before["sel_passes"]
        # the per-call route (the selector is built and destroyed inside the call), and (B) on a subset
        D, I = idx.search(xq[:17], 10, params=P(sel))
        assert_knn_identical(D, I, *filter_ranking(*full[17], sel.members, 10, metric), f"{name} per call")
        if name in ("inside", "batch10", "third", "two_pieces", "empty"):
            Db, Ib = sub_index_search(lambda rows: make_index(rows, metric, storage), xb, m, xq[:17], 10, metric)
            assert_knn_identical(D, I, Db, Ib, f"{name} sub-index")


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_fewer_selected_rows_than_k(metric, storage):
    xb, xq = data(metric, storage, N, 64, 5, 9)
    idx = make_index(xb, metric, storage)
    sel = faiss.IDSelectorBatch([3, 590, 599, 17, 200])
    for k in (8, 40):
        D, I = idx.search(xq, k, params=P(sel))
        assert (I[:, 5:] == -1).all() and (D[:, 5:] == pad_value(metric)).all()
        assert all(sorted(r.tolist()) == [3, 17, 200, 590, 599] for r in I[:, :5])
        assert_knn_identical(D, I, *filter_ranking(*idx.search(xq, N), sel.members, k, metric), f"k={k}")


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_tie_order(metric, storage):
    """Tie groups that straddle a wave's sub-slab and a block's slab (512 rows = 32 tiles: 4 blocks of 8 tiles, a
    tile per wave), every other member masked out: equal scores come back in ascending id."""
    rng = np.random.default_rng(21)
    n, d = 512, 16
    xb = int_data("binary", rng, n, d)
    xq = int_data("binary", rng, 16, d)
    # disjoint groups: 10..39 crosses two wave sub-slabs, 120..135 the block edge at 128, 63 | 64 a wave edge, 383 | 384
    # a block edge
    groups = [list(range(10, 40)), list(range(120, 136)), list(range(250, 262)) + [300, 301, 511],
              [0, 63, 64, 383, 384, 400]]
    assert sum(len(g) for g in groups) == len({r for g in groups for r in g})
    for gi, g in enumerate(groups):
        xb[g[0]] = xq[gi]  # the group ties at the best score of one query
        plant_ties(xb, g[0], g[1:])
    idx = make_index(xb, metric, storage)
    idx.set_shift(np.zeros(d, np.float32)) if (metric, storage) == (L2, "f32") else None
    mask = np.ones(n, bool)
    for g in groups:
        mask[g[1::2]] = False  # every other member of a group is masked out

    class Masked(faiss.IDSelector):
        def members(self, ids):
            return mask[np.asarray(ids, dtype=np.int64)]

    full = idx.search(xq, n)
    for k in (1, 10, 33):
        D, I = idx.search(xq, k, params=P(Masked()))
        assert_knn_identical(D, I, *filter_ranking(*full, Masked().members, k, metric), f"k={k}")
    D, I = idx.search(xq, 10, params=P(Masked()))
    for gi, g in enumerate(groups):
        kept = [r for r in g if mask[r]][:10]
        if metric == L2:  # distance 0: nothing ranks before the group
            assert I[gi, :len(kept)].tolist() == kept


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_nonfinite_rows(metric, storage):
    rng = np.random.default_rng(33)
    n, d = N, 24
    xb = int_data("small", rng, n, d)
    xq = int_data("small", rng, 17, d)
    bad = np.array([0, 15, 16, 130, 299, 300, 584, 599])
    poison(xb, bad[:3], "nan")
    poison(xb, bad[3:5], "inf", col=3)
    poison(xb, bad[5:6], "all_nan")
    xb[bad[6:], 1] = np.float32(3e38)
    idx = make_index(xb, metric, storage)
    mk = lambda rows: make_index(rows, metric, storage)
    clean = np.ones(n, bool)
    clean[bad] = False
    # poisoned rows masked OUT: as if they were not there
    for sel in (faiss.IDSelectorNot(faiss.IDSelectorBatch(bad)),):
        for k in (10, 40):
            D, I = idx.search(xq, k, params=P(sel))
            assert_knn_identical(D, I, *sub_index_search(mk, xb, clean, xq, k, metric), f"masked out k={k}")
    # poisoned rows selected: as search treats them
    m = np.zeros(n, bool)
    m[bad] = True
    m[100:400:7] = True
    for k in (10, 70):
        D, I = idx.search(xq, k, params=P(faiss.IDSelectorBatch(np.flatnonzero(m))))
        assert_knn_identical(D, I, *sub_index_search(mk, xb, m, xq, k, metric), f"selected k={k}")


def test_shift_independence():
    xb, xq = data(L2, "f32", N, 128, 17, 4)
    idx = make_index(xb, L2, "f32")
    sel = faiss.IDSelectorRange(123, 411)
    ref = idx.search(xq, 33, params=P(sel))
    for mu in (np.full(128, 1000.0, np.float32), np.linspace(-300, 300, 128).astype(np.float32)):
        idx.set_shift(mu)
        assert_knn_identical(*idx.search(xq, 33, params=P(sel)), *ref, "pinned shift")
        assert_knn_identical(*idx.search(xq, 33, params=P(EveryThird())),
                             *filter_ranking(*idx.search(xq, N), EveryThird().members, 33, L2), "pinned shift, third")


def test_long_index_with_shadows():
    rng = np.random.default_rng(8)
    n, d = 270_000, 32  # above the 262144-row shadow threshold
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((16, d)).astype(np.float32)
    idx = make_index(xb, L2, "f32")
    idx.search(xq, 10)  # builds the shadows
    rnd = np.zeros(n, bool)
    rnd[rng.choice(n, n // 100, replace=False)] = True

    class Rnd(faiss.IDSelector):
        def members(self, ids):
            return rnd[np.asarray(ids, dtype=np.int64)]

    row = int(idx.search(xq[:1], 1)[1][0, 0])  # exclude the best row of query 0
    half, byte, st = idx.half_stats(), idx.byte_stats(), idx.sel_stats()
    got = [idx.search(xq, 10, params=P(s)) for s in
           (faiss.IDSelectorRange(81_000, 108_000), Rnd(), faiss.IDSelectorNot(faiss.IDSelectorBatch([row])))]
    assert idx.half_stats() == half and idx.byte_stats() == byte
    assert idx.sel_stats()["sel_batches"] == st["sel_batches"] + 3 and idx.sel_stats()["sel_passes"] == st["sel_passes"] + 3
    mk = lambda rows: make_index(rows, L2, "f32")
    a = np.arange(n)
    for (D, I), m, what in zip(got, ((a >= 81_000) & (a < 108_000), rnd, a != row), ("range", "random", "not one")):
        assert_knn_identical(D, I, *sub_index_search(mk, xb, m, xq, 10, L2), what)
    assert row not in got[2][1][0]


@pytest.mark.parametrize("metric,storage", STORAGES)
def test_range_search_params(metric, storage):
    xb, xq = data(metric, storage, N, 128, 40, 12)
    idx = make_index(xb, metric, storage)
    Ds, _ = idx.search(xq, N)
    for r in (float(np.quantile(Ds, 0.05)), float(np.quantile(Ds, 0.5)), np.inf, -np.inf, np.nan):
        base = idx.range_search(xq, r)
        for sel in (faiss.IDSelectorRange(123, 411), EveryThird(), faiss.IDSelectorRange(7, 7)):
            before = idx.sel_stats()["sel_range_batches"]
            got = idx.range_search(xq, r, params=P(sel))
            assert idx.sel_stats()["sel_range_batches"] == before + 1
            assert_range_shape(*got, len(xq), N)
            assert_range_identical(got, filter_range(base, sel.members), f"radius {r} {type(sel).__name__}")


def test_range_search_params_overflow_pass(monkeypatch):
    xb, xq = data(L2, "f32", N, 64, 17, 13)
    idx = make_index(xb, L2, "f32")
    base = idx.range_search(xq, np.inf)
    monkeypatch.setenv("ISE_RANGE_STAGE_CAP", "1")
    _native.lib.ise_refresh_env_knobs()
    try:
        before = idx.range_stats()["range_overflow_batches"]
        got = idx.range_search(xq, np.inf, params=P(EveryThird()))
        assert idx.range_stats()["range_overflow_batches"] == before + 1
    finally:
        monkeypatch.delenv("ISE_RANGE_STAGE_CAP")
        _native.lib.ise_refresh_env_knobs()
    assert_range_identical(got, filter_range(base, EveryThird().members), "overflow pass")


def test_index_id_map():
    rng = np.random.default_rng(14)
    xb, xq = data(L2, "f32", N, 32, 5, 15)
    ext = rng.permutation(10_000)[:N].astype(np.int64) + 1_000_000
    idm = faiss.IndexIDMap(faiss.IndexFlatL2(32))
    idm.add_with_ids(xb, ext)
    sel = faiss.IDSelectorBatch(ext[50:300:2])

    def check(what):
        full = idm.search(xq, idm.ntotal)
        for s in (sel, faiss.IDSelectorNot(sel), faiss.IDSelectorRange(1_002_000, 1_005_000)):
            D, I = idm.search(xq, 12, params=P(s))
            assert_knn_identical(D, I, *filter_ranking(*full, s.members, 12, L2), what)
            got = idm.range_search(xq, float(np.median(full[0])), params=P(s))
            assert_range_identical(got, filter_range(idm.range_search(xq, float(np.median(full[0]))), s.members), what)

    check("before")
    assert idm.remove_ids(ext[40:120]) == 80
    check("after remove_ids")


def test_device_selector_lifetime():
    import torch

    xb, xq = data(L2, "f32", N, 32, 17, 16)
    idx, other = make_index(xb, L2, "f32"), make_index(xb, L2, "f32")
    sel = faiss.IDSelectorRange(123, 411)
    want = filter_ranking(*idx.search(xq, N), sel.members, 10, L2)
    ds = idx.make_selector(sel)
    assert_knn_identical(*idx.search(xq, 10, params=P(ds)), *want, "first")
    assert_knn_identical(*idx.search(xq, 10, params=P(ds)), *want, "second")
    Dt, It = idx.search_torch(torch.from_numpy(xq).cuda(), 10, params=P(ds))
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), *want, "search_torch")
    Dt, It = idx.search_torch(torch.from_numpy(xq).cuda(), 10, params=P(sel))
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), *want, "search_torch, per call")
    with pytest.raises(_native.IseError, match="another index"):
        other.search(xq, 10, params=P(ds))
    with pytest.raises(_native.IseError, match="another index"):
        other.range_search(xq, 1.0, params=P(ds))
    idx.add(xb[:3])
    with pytest.raises(_native.IseError, match="ntotal"):
        idx.search(xq, 10, params=P(ds))
    ds = idx.make_selector(sel)
    assert idx.remove_ids(faiss.IDSelectorRange(N, N + 3)) == 3  # ntotal is back, the row epoch is not
    assert_knn_identical(*idx.search(xq, 10, params=P(sel)), *want, "after add + remove")
    with pytest.raises(_native.IseError, match="epoch"):
        idx.search(xq, 10, params=P(ds))
    with pytest.raises(_native.IseError, match="epoch"):
        idx.search_torch(torch.from_numpy(xq).cuda(), 10, params=P(ds))
    ds = idx.make_selector(sel)
    assert_knn_identical(*idx.search(xq, 10, params=P(ds)), *want, "fresh selector")
    full = idx.search(xq, 10)
    idx.reset()
    with pytest.raises(_native.IseError):
        idx.search(xq, 10, params=P(ds))
    idx.add(xb)
    with pytest.raises(_native.IseError, match="epoch"):
        idx.search(xq, 10, params=P(ds))
    assert_knn_identical(*idx.search(xq, 10), *full, "unfiltered search after failed calls")
    with pytest.raises(_native.IseError):
        idx.search(xq, 4000, params=P(sel))  # k out of range


def test_five_streams_share_four_slots():
    """The masked pass has four workspace slots: a stream keeps its slot, and the fifth stream takes the least recently
    taken one behind its event and grows it.  Five streams, growing batches (the last two need two passes and so the
    keys buffer), the first stream once more, nothing waited for in between; every result has the bits of the host
    search with the same selector."""
    import torch

    rng = np.random.default_rng(900)
    n, d = 900, 20
    xb = int_data("small", rng, n, d)
    idx = make_index(xb, L2, "f32")
    ds = idx.make_selector(faiss.IDSelectorRange(5, 777))  # cuts a tile at both ends
    dev = torch.device("cuda", idx.device)
    pairs = [(2, 3), (5, 10), (9, 10), (17, 33), (40, 40)]
    xqs = [int_data("small", rng, nq, d) for nq, _ in pairs]
    for xq in xqs:
        assert_exact_range(xb, xq)
    xts = [torch.from_numpy(xq).to(dev) for xq in xqs]
    torch.cuda.synchronize(dev)  # the inputs are there: no stream waits for another through torch
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(device=dev) for _ in range(4)]
    got = []
    for st, xt, (_, k) in zip(streams + streams[:1], xts + xts[:1], pairs + pairs[:1]):
        with torch.cuda.stream(st):
            got.append(idx.search_torch(xt, k, params=P(ds)))
    torch.cuda.synchronize(dev)
    for j, ((Dt, It), xq, (nq, k)) in enumerate(zip(got, xqs + xqs[:1], pairs + pairs[:1])):
        assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), *idx.search(xq, k, params=P(ds)), f"call {j}: nq={nq} k={k}")


def test_host_search_of_more_than_one_staging_batch():
    """A filtered host search stages 1024 queries at a time through its context's device buffers: 1030 queries are two
    batches, and the second one's queries and results sit at an offset in the caller's arrays.  Integer data, so the
    oracle's answer over the selected rows is the only correct one, bit for bit."""
    rng = np.random.default_rng(1030)
    xb, xq = int_data("small", rng, 2000, 32), int_data("small", rng, 1030, 32)
    assert_exact_range(xb, xq)
    idx = make_index(xb, L2, "f32")
    D, I = idx.search(xq, 5, params=P(faiss.IDSelectorRange(100, 1500)))
    assert_knn_identical(D, I, *ko.knn_exact(xb[100:1500], xq, 5, L2, id_offset=100), "nq=1030")


def test_threads_mixed_with_unfiltered():
    xb, xq = data(L2, "f32", 2000, 64, 8 * 6, 17)
    idx = make_index(xb, L2, "f32")
    sels = [faiss.IDSelectorRange(100, 1500), EveryThird(), None, faiss.IDSelectorNot(faiss.IDSelectorBatch([11]))]
    jobs = [(xq[i:i + 1 + i % 3], 10, sels[i % 4]) for i in range(len(xq) - 3)]
    serial = [idx.search(x, k, params=P(s)) if s is not None else idx.search(x, k) for x, k, s in jobs]
    before = idx.host_stats()["combined_calls"]
    out = [None] * len(jobs)
    errs = []

    def work(t):
        try:
            for j in range(t, len(jobs), 8):
                x, k, s = jobs[j]
                out[j] = idx.search(x, k, params=P(s)) if s is not None else idx.search(x, k)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for j, (got, want) in enumerate(zip(out, serial)):
        assert_knn_identical(*got, *want, f"job {j}")
    unfiltered = sum(1 for _, _, s in jobs if s is None)
    assert idx.host_stats()["combined_calls"] - before <= unfiltered
