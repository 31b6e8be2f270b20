"""GPU tests of IndexIVFFlat (include/ise_knn.h, ise_ivf_*; csrc/ise_ivf.hpp).  Every comparison is bit for bit:
against the complete ranking of an IndexFlat over the same rows cut to the members of each query's probed lists, or
(integer data) against a float64 brute force over those members (tests/ivf_ref.py)."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data
from tests.sel_ref import IP, L2, pad_value

pytestmark = pytest.mark.gpu

N, NLIST = 600, 7
SIZES = [16, 1, 0, 100, 200, 150, 133]  # exactly one tile, one row, empty, 6 tiles + 4 rows, ...
CHUNKS = [250, 1, 349]                  # the three add calls
assert sum(SIZES) == N and sum(CHUNKS) == N


def flat(d, metric):
    return faiss.IndexFlatIP(d) if metric == IP else faiss.IndexFlatL2(d)


def clustered(d, seed, nq=40):
    """Hand-made centroids 30 apart from the origin in orthogonal directions, N Gaussian rows around them in the
    proportions SIZES at shuffled ids, queries half around centroids (the empty list's too) and half anywhere."""
    rng = np.random.default_rng(seed)
    cent = (30.0 * np.linalg.qr(rng.standard_normal((d, d)))[0][:NLIST]).astype(np.float32)
    plan = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
    xb = (cent[plan] + rng.standard_normal((N, d))).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32) * 4
    xq[::2] += cent[rng.integers(0, NLIST, len(xq[::2]))]
    return cent, plan, xb, xq


def build(cent, xb, metric, qmetric, chunks=CHUNKS):
    qz = flat(cent.shape[1], qmetric)
    qz.add(cent)
    ivf = faiss.IndexIVFFlat(qz, cent.shape[1], len(cent), metric)
    assert ivf.is_trained and ivf.ntotal == 0 and ivf.nprobe == 1 and ivf.quantizer is qz
    ivf.train(xb)  # a no-op: the quantiser is full
    assert qz.ntotal == len(cent)
    i0 = 0
    for c in chunks:
        ivf.add(xb[i0:i0 + c])
        i0 += c
        assert ivf.ntotal == i0
    return qz, ivf


def check_list_shapes(ivf, assign):
    sizes = [ivf.list_size(l) for l in range(ivf.nlist)]
    assert sizes == np.bincount(assign, minlength=ivf.nlist).tolist()
    assert 0 in sizes and 16 in sizes and 1 in sizes and any(s % 16 for s in sizes if s > 16)
    return sizes


def test_lists():
    cent, plan, xb, _ = clustered(20, 1)
    qz, ivf = build(cent, xb, L2, L2)
    assign = qz.search(xb, 1)[1].reshape(-1)
    assert np.array_equal(assign, plan)  # the data are what they were made to be
    check_list_shapes(ivf, assign)
    for rep in range(2):  # before and after the rebuild a search triggers
        for l, want in enumerate(ivf_ref.list_members(assign, NLIST)):
            ids, rows = ivf.get_list(l)
            assert ids.dtype == np.int64 and rows.dtype == np.float32 and rows.shape == (len(want), 20)
            assert np.array_equal(ids, want) and (np.diff(ids) > 0).all()
            assert np.array_equal(rows.view(np.uint32), xb[want].view(np.uint32))
        ivf.search(xb[:3], 2)
    # rows added after a rebuild go behind the rows of their list
    ivf.add(xb[:40])
    assign2 = np.concatenate([assign, assign[:40]])
    for l, want in enumerate(ivf_ref.list_members(assign2, NLIST)):
        ids, rows = ivf.get_list(l)
        assert np.array_equal(ids, want)
        assert np.array_equal(rows.view(np.uint32), np.concatenate([xb, xb[:40]])[want].view(np.uint32))
    assert ivf.ntotal == N + 40
    ivf.reset()
    assert ivf.ntotal == 0 and ivf.is_trained and qz.ntotal == NLIST
    assert [ivf.list_size(l) for l in range(NLIST)] == [0] * NLIST
    D, I = ivf.search(xb[:2], 3)
    assert (I == -1).all() and (D == pad_value(L2)).all()
    ivf.add(xb[:5])
    assert ivf.ntotal == 5 and sorted(np.concatenate([ivf.get_list(l)[0] for l in range(NLIST)]).tolist()) == [0, 1, 2, 3, 4]


def sweep(ivf, qz, fl, xq, assign, metric, nqs=(1, 16, 17, 40), ks=(1, 10, 33, 70), nprobes=(1, 3, 7)):
    n = fl.ntotal
    for nq in nqs:
        full = fl.search(xq[:nq], n)  # the complete ranking, computed once
        for nprobe in nprobes:
            ivf.nprobe = nprobe
            probes = qz.search(xq[:nq], min(nprobe, ivf.nlist))[1]
            members = ivf_ref.probed_members(probes, assign, ivf.nlist)
            for k in ks:
                D, I = ivf.search(xq[:nq], k)
                Dw, Iw = ivf_ref.expected_from_ranking(*full, members, k, metric)
                assert_knn_identical(D, I, Dw, Iw, f"nq={nq} nprobe={nprobe} k={k}")
                if nprobe >= ivf.nlist:
                    assert_knn_identical(D, I, *fl.search(xq[:nq], k), f"all lists: nq={nq} k={k}")


@pytest.mark.parametrize("metric,qmetric", [(L2, L2), (IP, L2), (IP, IP)])
@pytest.mark.parametrize("d", [20, 128])
def test_parity_sweep(metric, qmetric, d):
    cent, plan, xb, xq = clustered(d, 100 + d)
    qz, ivf = build(cent, xb, metric, qmetric)
    assign = qz.search(xb, 1)[1].reshape(-1)
    sizes = check_list_shapes(ivf, assign)
    fl = flat(d, metric)
    fl.add(xb)
    before = ivf.ivf_stats()
    sweep(ivf, qz, fl, xq, assign, metric)
    after = ivf.ivf_stats()
    assert after["batches"] - before["batches"] == 4 * 3 * 4
    # a launch serves up to 64 queries (4 groups of 16).  k <= 32: one pass; k = 33: two; k = 70: three
    assert after["passes"] - before["passes"] == 4 * 3 * (1 + 1 + 2 + 3)
    # padding where the probed lists hold fewer than k rows
    ivf.nprobe = 1
    one = int(np.flatnonzero(np.asarray(sizes) == 1)[0])
    D, I = ivf.search_preassigned(xq[:2], 10, np.full((2, 1), one))
    assert (I[:, 0] == ivf.get_list(one)[0][0]).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == pad_value(metric)).all()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", ["binary", "signed"])
def test_ties(metric, kind):
    """Integer rows at d = 20: dense tie groups whose members sit in several lists."""
    rng = np.random.default_rng(31)
    n, d, nq, nlist = 500, 20, 24, 5
    xb, xq = int_data(kind, rng, n, d), int_data(kind, rng, nq, d)
    assert_exact_range(xb, xq)
    cent = int_data(kind, rng, nlist, d) * np.float32(0.75)
    qz, ivf = build(cent, xb, metric, L2, chunks=[100, 399, 1])
    assign = qz.search(xb, 1)[1].reshape(-1)
    assert (np.bincount(assign, minlength=nlist) > 0).sum() >= 3
    for nprobe in (1, 2, 5):
        ivf.nprobe = nprobe
        members = ivf_ref.probed_members(qz.search(xq, nprobe)[1], assign, nlist)
        for k in (1, 10, 33, 70):
            D, I = ivf.search(xq, k)
            Dw, Iw = ivf_ref.expected_brute(xb, xq, members, k, metric)
            assert_knn_identical(D, I, Dw, Iw, f"{kind} nprobe={nprobe} k={k}")
            if metric == L2 and k == 33 and kind == "binary":  # the groups are dense: whole runs of equal distances
                assert (np.diff(D[:, :20], axis=1) == 0).mean() > 0.5


@pytest.mark.parametrize("metric", [L2, IP])
def test_tie_across_lists_smaller_id_in_later_slot(metric):
    """Every row is one-hot, so every row is at distance 1 from the zero query (score 1 for the all-ones query).  The
    rows of the first add call go to list 1, those of the second to list 0: list 0's slots come first in the row array
    and carry the LARGER ids.  Ties go by ascending id, so the answer is the first call's rows, in order."""
    d = 20
    cent = np.zeros((2, d), np.float32)
    cent[0, 10:] = 0.5
    cent[1, :10] = 0.5
    first = np.eye(d, dtype=np.float32)[np.arange(24) % 10]        # ones in columns 0..9: nearest to centroid 1
    second = np.eye(d, dtype=np.float32)[10 + np.arange(40) % 10]  # ones in columns 10..19: nearest to centroid 0
    xb = np.concatenate([first, second])
    qz, ivf = build(cent, xb, metric, L2, chunks=[24, 40])
    assign = qz.search(xb, 1)[1].reshape(-1)
    assert (assign[:24] == 1).all() and (assign[24:] == 0).all()
    assert ivf.get_list(0)[0].min() > ivf.get_list(1)[0].max()
    xq = np.zeros((3, d), np.float32) if metric == L2 else np.ones((3, d), np.float32)
    assert_exact_range(xb, xq)
    ivf.nprobe = 2
    for k in (1, 5, 24, 33, 64, 70):
        D, I = ivf.search(xq, k)
        want = np.where(np.arange(k) < 64, np.arange(k), -1)
        assert np.array_equal(I, np.tile(want, (3, 1))), (k, I[0].tolist())
        assert (D[:, :min(k, 64)] == 1.0).all()
        members = ivf_ref.probed_members(np.tile([0, 1], (3, 1)), assign, 2)
        assert_knn_identical(D, I, *ivf_ref.expected_brute(xb, xq, members, k, metric), f"k={k}")


def test_torch_preassigned_and_odd_probes():
    import torch

    d = 20
    cent, plan, xb, xq = clustered(d, 7)
    qz, ivf = build(cent, xb, L2, L2)
    assign = qz.search(xb, 1)[1].reshape(-1)
    fl = flat(d, L2)
    fl.add(xb)
    dev = torch.device("cuda", ivf.device)
    xq_t = torch.from_numpy(xq).to(dev)
    for nprobe, k in ((1, 10), (3, 33), (7, 5), (50, 5)):  # nprobe beyond nlist is clipped
        ivf.nprobe = nprobe
        D, I = ivf.search(xq, k)
        Dt, It = ivf.search_torch(xq_t, k)
        assert Dt.is_cuda and It.dtype == torch.int64
        assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D, I, f"torch nprobe={nprobe}")
        probes = qz.search(xq, min(nprobe, NLIST))[1]
        assert_knn_identical(*ivf.search_preassigned(xq, k, probes), D, I, f"preassigned nprobe={nprobe}")
    # duplicate, -1 and out-of-range probe entries
    empty = int(np.flatnonzero(np.bincount(assign, minlength=NLIST) == 0)[0])
    probes = np.array([[3, 3, 3, 3], [-1, -1, -1, -1], [4, -1, 4, 0], [empty, -1, empty, -1], [6, 5, 6, 5]] * 4, np.int64)[:17]
    members = ivf_ref.probed_members(probes, assign, NLIST)
    full = fl.search(xq[:17], N)
    for k in (1, 10, 40):
        D, I = ivf.search_preassigned(xq[:17], k, probes)
        assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(*full, members, k, L2), f"odd probes k={k}")
        assert (I[1] == -1).all() and (I[3] == -1).all()
        for q in range(17):
            real = I[q][I[q] >= 0]
            assert len(set(real.tolist())) == len(real)  # a list named twice delivers its rows once
    # add_torch files rows like add
    qz2, ivf2 = build(cent, xb[:0], L2, L2, chunks=[])
    ivf2.add_torch(torch.from_numpy(xb[:300]).to(dev))
    ivf2.add_torch(torch.from_numpy(xb[300:]).to(dev))
    ivf2.nprobe = 3
    ivf.nprobe = 3
    assert_knn_identical(*ivf2.search(xq, 10), *ivf.search(xq, 10), "add_torch")
    for l in range(NLIST):
        assert np.array_equal(ivf2.get_list(l)[0], ivf.get_list(l)[0])
    # a NaN query returns all padding
    bad = xq[:3].copy()
    bad[1, 4] = np.nan
    D, I = ivf.search(bad, 5)
    assert (I[1] == -1).all() and (D[1] == pad_value(L2)).all() and (I[0] >= 0).all() and (I[2] >= 0).all()
    Dt, It = ivf.search_torch(torch.from_numpy(bad).to(dev), 5)
    assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D, I, "NaN query, torch")
    # a NaN row in add raises and leaves ntotal unchanged
    rows = xb[:6].copy()
    rows[4, 0] = np.nan
    with pytest.raises(ValueError, match="row 4"):
        ivf.add(rows)
    with pytest.raises(ValueError, match="row 4"):
        ivf.add_torch(torch.from_numpy(rows).to(dev))
    assert ivf.ntotal == N
    assert_knn_identical(*ivf.search(xq, 10), *ivf2.search(xq, 10), "after the refused add")
    # a list number out of range is refused by the library, and nothing of the call is added
    from image_search_engine_amd import _native as n

    lists = np.array([0, 1, NLIST, 2], np.int64)
    assert n.lib.ise_ivf_add_host(ivf._h, xb[:4].ctypes.data, lists.ctypes.data, 4) == n.E_INVALID
    assert b"nothing was added" in n.lib.ise_last_error() and ivf.ntotal == N
    # what is not provided
    with pytest.raises(NotImplementedError):
        ivf.search(xq, 3, params=faiss.SearchParameters())
    with pytest.raises(NotImplementedError):
        ivf.range_search(xq, 1.0)
    with pytest.raises(NotImplementedError):
        ivf.remove_ids([1])
    with pytest.raises(NotImplementedError):
        faiss.write_index(ivf, "/nonexistent/never-written")
    with pytest.raises(NotImplementedError):
        faiss.IndexIDMap(ivf2)
    untrained = faiss.IndexIVFFlat(flat(d, L2), d, 4)
    assert not untrained.is_trained
    with pytest.raises(RuntimeError):
        untrained.add(xb[:4])
    with pytest.raises(RuntimeError):
        untrained.train(xb[:3])  # fewer rows than lists


def test_one_handle_from_two_streams():
    """Adds and searches on one handle from the default stream and a side stream, nothing waited for in between: the
    side stream's search (two chunks of two k-passes, more queries and a larger k than the call before) has to grow
    every workspace while the first search may still be in flight.  Every result is the host form's, bit for bit."""
    import torch

    d, n, nlist = 40, 900, 6
    rng = np.random.default_rng(31)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, 70, d)
    cent = xb[[1, 2, 3, 5, 8, 13]]
    qz, ivf = build(cent, xb, L2, L2, chunks=[n])
    qz2, twin = build(cent, xb[:0], L2, L2, chunks=[])
    ivf.nprobe = twin.nprobe = 3
    want = {(nq, k): ivf.search(xq[:nq], k) for nq, k in ((3, 10), (70, 33))}
    dev = torch.device("cuda", twin.device)
    side = torch.cuda.Stream(device=dev)
    xb_t, xq_t = torch.from_numpy(xb).to(dev), torch.from_numpy(xq).to(dev)
    torch.cuda.synchronize(dev)
    twin.add_torch(xb_t[:300])
    with torch.cuda.stream(side):
        twin.add_torch(xb_t[300:])
    assert twin.ntotal == n and [twin.list_size(l) for l in range(nlist)] == [ivf.list_size(l) for l in range(nlist)]
    first = twin.search_torch(xq_t[:3], 10)  # rebuilds the lists
    with torch.cuda.stream(side):
        second = twin.search_torch(xq_t, 33)
    third = twin.search_torch(xq_t[:3], 10)
    torch.cuda.synchronize(dev)
    for name, got, key in (("first", first, (3, 10)), ("side stream", second, (70, 33)), ("third", third, (3, 10))):
        assert_knn_identical(got[0].cpu().numpy(), got[1].cpu().numpy(), *want[key], name)
    for key, (D, I) in want.items():
        assert_knn_identical(*twin.search(xq[:key[0]], key[1]), D, I, f"the twin's host form {key}")
    assert twin.ntotal == n
    for l in range(nlist):
        (ids, rows), (ids2, rows2) = ivf.get_list(l), twin.get_list(l)
        assert np.array_equal(ids, ids2) and np.array_equal(rows.view(np.uint32), rows2.view(np.uint32))


def test_add_torch_and_search_torch_from_two_threads():
    """One thread adds the same 16 rows 20 times with ``add_torch``, another searches with ``search_torch`` meanwhile;
    both go through the index's lock.  Afterwards the index holds 16 * 20 rows and answers as a fresh index that was
    given them in one call: the lock changes no result."""
    import threading

    import torch

    d, nlist, n, rounds = 8, 3, 16, 20
    rng = np.random.default_rng(53)
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, 5, d)
    cent = xb[[0, 5, 11]]
    _, ivf = build(cent, xb[:0], L2, L2, chunks=[])
    _, fresh = build(cent, np.tile(xb, (rounds, 1)), L2, L2, chunks=[n * rounds])
    ivf.nprobe = fresh.nprobe = 2
    dev = torch.device("cuda", ivf.device)
    xb_t, xq_t = torch.from_numpy(xb).to(dev), torch.from_numpy(xq).to(dev)
    torch.cuda.synchronize(dev)
    errors = []

    def run(call):
        try:
            for _ in range(rounds):
                call()
            torch.cuda.synchronize(dev)
        except Exception as e:  # reported by the asserting thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(lambda: ivf.add_torch(xb_t),)),
               threading.Thread(target=run, args=(lambda: ivf.search_torch(xq_t, 4),))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert ivf.ntotal == n * rounds
    D, I = ivf.search_torch(xq_t, 10)
    assert_knn_identical(D.cpu().numpy(), I.cpu().numpy(), *fresh.search(xq, 10), "after the two threads")


def test_work_is_proportional_to_the_probes():
    d = 20
    cent, plan, xb, xq = clustered(d, 3)
    qz, ivf = build(cent, xb, L2, L2)
    assign = qz.search(xb, 1)[1].reshape(-1)
    sizes = np.bincount(assign, minlength=NLIST)
    ivf.search(xq[:1], 1)  # the rebuild is behind us
    for l in range(NLIST):  # nq = 1, nprobe = 1: exactly that list's tiles
        for k in (1, 32):
            t0 = ivf.ivf_stats()["tiles_loaded"]
            ivf.search_preassigned(xq[:1], k, np.array([[l]]))
            assert ivf.ivf_stats()["tiles_loaded"] - t0 == ivf_ref.tiles_of([sizes[l]]), (l, k)
    ivf.nprobe = 3
    probes = qz.search(xq[:16], 3)[1]
    t0 = ivf.ivf_stats()["tiles_loaded"]
    ivf.search(xq[:16], 10)
    got = ivf.ivf_stats()["tiles_loaded"] - t0
    lo = ivf_ref.tiles_of(sizes[np.unique(probes[probes >= 0])])
    hi = ivf_ref.tiles_of(sizes[probes[probes >= 0]])
    assert lo <= got <= hi, (lo, got, hi)


def test_train_and_the_reference_call():
    from image_search_engine_amd.utils import create_search_index

    rng = np.random.default_rng(5)
    x = rng.standard_normal((2000, 32)).astype(np.float32)
    xq = rng.standard_normal((17, 32)).astype(np.float32)
    qz = faiss.IndexFlatL2(32)
    ivf = faiss.IndexIVFFlat(qz, 32, 8)
    assert not ivf.is_trained
    ivf.train(x)
    assert ivf.is_trained and qz.ntotal == 8
    cents = qz.reconstruct_n(0, 8)
    ivf.train(x)  # trained: a no-op
    assert np.array_equal(qz.reconstruct_n(0, 8), cents)
    ivf.add(x)
    assert ivf.ntotal == 2000
    assign = qz.search(x, 1)[1].reshape(-1)
    fl = faiss.IndexFlatL2(32)
    fl.add(x)
    sweep(ivf, qz, fl, xq, assign, L2, nqs=(17,), ks=(10, 33), nprobes=(3,))
    # the reference's call (backend/utils.py:311-325 without the product quantiser)
    index = create_search_index(x.copy(), "cell-probe-flat")
    assert isinstance(index, faiss.IndexIVFFlat) and index.nprobe == 5 and index.nlist == 8 and index.ntotal == 2000
    assert index.quantizer.metric_type == L2 and index.quantizer.ntotal == 8
    assign = index.quantizer.search(x, 1)[1].reshape(-1)
    sweep(index, index.quantizer, fl, xq, assign, L2, nqs=(17,), ks=(10,), nprobes=(5,))
    # spherical training behind an inner-product quantiser
    ivf_ip = faiss.IndexIVFFlat(faiss.IndexFlatIP(32), 32, 8, IP)
    ivf_ip.cp.niter = 2
    ivf_ip.train(x)
    assert np.allclose(np.linalg.norm(ivf_ip.quantizer.reconstruct_n(0, 8), axis=1), 1.0, atol=1e-5)


# ---- more tiles than 8 x blocks: every wave of a pass visits several tiles, of several lists
NBIG = 150_000  # 9375+ tiles at 16 rows: at least two per wave of the largest grid (1024 blocks of 8 waves = 8192 waves)


def pass_blocks(tiles, device):
    """The grid of a pass (csrc/ise_ivf.hip, ivf_chunk_enqueue): a tile per wave, two blocks per CU, the merge's lists."""
    import torch

    cu = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(-(-tiles // 8), 2 * cu, 1024))


def assert_waves_cross_tiles(ivf):
    """Fails if the index is so short that a wave gets one tile only (the round-robin deal has stride 8 x blocks)."""
    tiles = ivf_ref.tiles_of([ivf.list_size(l) for l in range(ivf.nlist)])
    blocks = pass_blocks(tiles, ivf.device)
    assert tiles >= 2 * 8 * blocks, (tiles, blocks)
    return tiles


@pytest.mark.parametrize("metric", [L2, IP])
def test_wave_meets_larger_ids_first_at_an_equal_bound(metric):
    """All rows are the all-ones row and so is the query: mu is the row itself, every norm, every dot product around mu
    and every lower bound is exactly 0, and so is every distance -- lo == tau the moment a list is full.  The first add
    call's rows (ids below n0) are filed in list 1, the second's in list 0, whose tiles come first: with 9376 tiles over
    at most 8192 waves a wave meets a list-0 tile (larger ids) and then a list-1 tile (smaller ids, equal distance, equal
    bound).  Pruning at lo >= tau, or comparing distances instead of full keys, loses the smaller ids."""
    from image_search_engine_amd import _native as n

    d, n0 = 20, NBIG // 2
    qz = flat(d, L2)
    qz.add(np.stack([np.zeros(d, np.float32), np.ones(d, np.float32)]))
    ivf = faiss.IndexIVFFlat(qz, d, 2, metric)
    xb = np.ones((n0, d), np.float32)
    for l in (1, 0):  # list numbers by hand, as the C ABI takes them
        lists = np.full(n0, l, np.int64)
        n.check(n.lib.ise_ivf_add_host(ivf._h, xb.ctypes.data, lists.ctypes.data, n0))
    assert [ivf.list_size(0), ivf.list_size(1)] == [n0, n0] and ivf.ntotal == 2 * n0
    tiles = assert_waves_cross_tiles(ivf)
    xq = np.ones((3, d), np.float32)
    assert_exact_range(xb[:4], xq)
    for probes in ([0, 1], [1, 0]):
        for k in (1, 10, 33):
            D, I = ivf.search_preassigned(xq, k, np.tile(probes, (3, 1)))
            assert np.array_equal(I, np.tile(np.arange(k), (3, 1))), (k, I[0].tolist())
            assert (D == (0.0 if metric == L2 else float(d))).all()
    assert ivf.get_list(0)[0][0] == n0 and ivf.get_list(1)[0][-1] == n0 - 1
    t0 = ivf.ivf_stats()["tiles_loaded"]
    ivf.search_preassigned(xq[:1], 5, np.array([[0, 1]]))
    assert ivf.ivf_stats()["tiles_loaded"] - t0 == tiles  # every tile of every wave's deal was visited


@pytest.mark.parametrize("metric", [L2, IP])
def test_multi_tile_parity_with_the_flat_search(metric):
    """Gaussian rows around seven centroids, long enough that a wave visits tiles of several lists: with every list
    probed the result is the flat search's, bit for bit."""
    d = 20
    rng = np.random.default_rng(77)
    cent = (30.0 * np.linalg.qr(rng.standard_normal((d, d)))[0][:NLIST]).astype(np.float32)
    plan = rng.integers(0, NLIST - 1, NBIG)  # the last list stays empty
    xb = (cent[plan] + rng.standard_normal((NBIG, d))).astype(np.float32)
    xq = (cent[rng.integers(0, NLIST, 17)] + rng.standard_normal((17, d)) * 2).astype(np.float32)
    qz, ivf = build(cent, xb, metric, L2, chunks=[60_000, 1, NBIG - 60_001])
    assert ivf.list_size(NLIST - 1) == 0
    assert_waves_cross_tiles(ivf)
    fl = flat(d, metric)
    fl.add(xb)
    ivf.nprobe = NLIST
    for nq in (1, 17):
        for k in (10, 33):
            assert_knn_identical(*ivf.search(xq[:nq], k), *fl.search(xq[:nq], k), f"nq={nq} k={k}")
    # fewer lists: the complete ranking of the probed rows is out of the flat index's reach (k <= 2048), so the members'
    # own flat index answers
    ivf.nprobe = 2
    assign = qz.search(xb, 1)[1].reshape(-1)
    probes = qz.search(xq[:3], 2)[1]
    members = ivf_ref.probed_members(probes, assign, NLIST)
    D, I = ivf.search(xq[:3], 33)
    for q in range(3):
        sub = flat(d, metric)
        sub.add(np.ascontiguousarray(xb[members[q]]))
        Ds, Is = sub.search(xq[q:q + 1], 33)
        assert_knn_identical(D[q:q + 1], I[q:q + 1], Ds, np.where(Is >= 0, members[q][np.maximum(Is, 0)], -1), f"query {q}")


@pytest.mark.parametrize("metric", [L2, IP])
def test_multi_tile_ties(metric):
    """150 000 binary rows at d = 20: at most 21 distinct distances, so the k best are one long tie group spread over
    every list and every wave; the float64 brute force over the members decides, ids ascending."""
    rng = np.random.default_rng(41)
    d, nlist, nq = 20, 5, 6
    xb, xq = int_data("binary", rng, NBIG, d), int_data("binary", rng, nq, d)
    assert_exact_range(xb, xq)
    cent = int_data("binary", rng, nlist, d) * np.float32(0.75)
    qz, ivf = build(cent, xb, metric, L2, chunks=[100_000, NBIG - 100_000])
    assign = qz.search(xb, 1)[1].reshape(-1)
    assert (np.bincount(assign, minlength=nlist) > 0).sum() >= 3
    assert_waves_cross_tiles(ivf)
    for nprobe in (1, 3, 5):
        ivf.nprobe = nprobe
        members = ivf_ref.probed_members(qz.search(xq, nprobe)[1], assign, nlist)
        for k in (10, 33):
            D, I = ivf.search(xq, k)
            assert_knn_identical(D, I, *ivf_ref.expected_brute(xb, xq, members, k, metric), f"nprobe={nprobe} k={k}")
