"""The deep plan of the byte shadow scan on the GPU (make_plan / search_enqueue, csrc/ise_knn.hip; the one-request
exchange read, csrc/ise_scan.hpp ROWS_I8_ONE; arithmetic: tests/test_scan_depth.py).  The plan changes
which block holds which keys and how wide the exchange bound is, never the merged keys: at every depth D and I are the
bits of depth 1 and of the fp16 and float32 filters, the byte route is asserted (_three), ise_index_depth_stats moves in
the right column, and the byte route sends no more queries to the exact scan -- which would hide a broken list -- than
the larger of the other two routes.

Nothing allocated after reserve(): no accessor shows a slot's pointers, so that is checked in the C code (the slots are
sized by the depth-1 grid and make_plan refuses a deep plan with more blocks; tests/test_scan_depth.py restates the
block counts); here a deep and an isolated batch follow reserve() in either order with the right bits."""
import threading
import zlib

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.knn_checks import assert_knn_identical, brute_knn, int_data, plant_ties
from tests.test_byte_filter_gpu import _three
from tests.test_exact_l2_gpu import env_knob, no_direct
from tests.test_scan_depth import block_row0, block_tiles, deep_plan, seeded

pytestmark = pytest.mark.gpu
L2 = ko.METRIC_L2
N, N_MIXED, D = 500_000, 350_000, 64
WINDOW = 256  # rows of a seeded block's boot window
KB = 32       # block-list slots of the byte route (kc = 32)
DEPTHS = (1, 2, 4)


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _index(faiss, xb):
    index = faiss.IndexFlatL2(xb.shape[1])
    index.add(xb)
    return index


def _plan(n, depth):
    import torch

    return deep_plan(n, depth, torch.cuda.get_device_properties(0).multi_processor_count)


def depth_knob(depth):
    return env_knob("ISE_SCAN_DEPTH", depth)


def _depth_counts(index):
    st = index.depth_stats()
    return st["isolated_batches"], st["deep_batches"]


def _three_at(index, n, xq, k, depth):
    """_three with the depth forced; asserts that its one byte batch was counted in the column the plan says."""
    i0, d0 = _depth_counts(index)
    with depth_knob(depth), no_direct():
        Dk, Ik, exact = _three(index, xq, k, "byte")
    i1, d1 = _depth_counts(index)
    deep = _plan(n, depth)["depth"] > 1
    assert (i1 - i0, d1 - d0) == ((0, 1) if deep else (1, 0)), (n, depth, i1 - i0, d1 - d0)
    return Dk, Ik, exact


def _same_bits(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: ids differ"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: distances differ"


def _no_more_exact_scans(exact, what):
    xb8, xh, xf = exact
    assert xb8 <= max(xh, xf), f"{what}: exact scans byte {xb8}, fp16 {xh}, float32 {xf}"


@pytest.fixture(scope="module")
def uniform(faiss):
    out = {}
    for n in (N, N_MIXED):
        xb = _rng("sd", "uniform", n).random((n, D), dtype=np.float32)
        out[n] = (_index(faiss, xb), xb)
    return out


def test_shapes_on_this_device():
    """The cases below are what they are meant to be on the device they run on."""
    for n in (N, N_MIXED):
        for depth in (2, 4):
            p = _plan(n, depth)
            assert p["depth"] == depth and p["blocks"] <= 256 and seeded(p, 0), (n, depth, p)
    p = _plan(N, 2)
    assert not seeded(p, p["blocks"] - 1) and block_tiles(p, p["blocks"] - 1) >= 1  # a short last block: the cut
    assert not seeded(_plan(N_MIXED, 1), 0) and seeded(_plan(N_MIXED, 2), 0)  # depth changes which boot runs


@pytest.mark.parametrize("n", [N, N_MIXED])
@pytest.mark.parametrize("k", [1, 10])
def test_same_bits_at_every_depth(uniform, n, k):
    """1. uniform rows: at depths 1, 2 and 4 the three routes' bits, equal to depth 1's, nothing sent to the exact scan."""
    index, xb = uniform[n]
    rng = _rng("sd", "q", n, k)
    for nq in (1, 2, 7, 15, 16):
        xq = rng.random((nq, D), dtype=np.float32)
        ref = None
        for depth in DEPTHS:
            Dk, Ik, exact = _three_at(index, n, xq, k, depth)
            assert exact == [0, 0, 0], (n, k, nq, depth, exact)
            ref = ref or (Dk, Ik)
            _same_bits((Dk, Ik), ref, f"n {n} k {k} nq {nq} depth {depth} against depth 1")


def test_neighbours_planted_at_deep_block_boundaries(faiss):
    """2. the ten true neighbours of a query sit, by the deep plans' block boundaries (depths 2 and 4): inside one deep
    block's boot window, across the window's end, in a deep block's last tile, in the last block (a short one at
    depth 2), and in the index's last (partial) tile.  Planted at squared distances below 1e-3 among uniform rows
    (nearest ~ 3): the float32 route certifies them alone."""
    n, k = N - 5, 10
    rng = _rng("sd", "plant")
    xb = rng.random((n, D), dtype=np.float32)
    starts = [n - k]
    for depth in (2, 4):
        p = _plan(n, depth)
        assert n % 16 and p["depth"] == depth
        last = p["blocks"] - 1
        starts += [block_row0(p, 3 + depth) + 40, block_row0(p, 5 + depth) + WINDOW - k // 2,
                   block_row0(p, 9 + depth) + 16 * p["tpb"] - k, block_row0(p, last) + 20]
    assert len(set(s // 16 for s in starts)) == len(starts) <= 16
    xq = rng.random((len(starts), D), dtype=np.float32)
    want = []
    for j, s in enumerate(starts):
        order = rng.permutation(k)  # distance rank of the rows s .. s + k - 1
        for i in range(k):
            xb[s + i] = xq[j] + np.float32(0.001 * (1 + order[i])) * rng.standard_normal(D).astype(np.float32)
        want.append(np.arange(s, s + k))
    index = _index(faiss, xb)
    for kk in (1, k):
        D_ref, I_ref = brute_knn(xb, xq, kk, L2)
        ref = None
        for depth in DEPTHS:
            Dk, Ik, exact = _three_at(index, n, xq, kk, depth)
            _no_more_exact_scans(exact, f"planted, k = {kk}, depth {depth}")
            assert np.array_equal(Ik, I_ref), (kk, depth)
            for j in range(len(starts)):
                assert set(Ik[j]) <= set(want[j]), (j, Ik[j], want[j])
            ref = ref or (Dk, Ik)
            _same_bits((Dk, Ik), ref, f"planted, k = {kk}, depth {depth} against depth 1")


def test_more_window_keys_under_the_bound_than_the_list_holds(faiss):
    """3. adversarial, integer data (ties are exact): 100 copies of a near row inside one deep block's boot window (more
    than kb: the block cuts exactly), exactly kb copies, and copies spread over two deep blocks' windows."""
    n, k = N, 10
    rng = _rng("sd", "overflow")
    xb = int_data("small", rng, n, D)
    p = _plan(n, 2)
    srcs = [block_row0(p, 4) + 3, block_row0(p, 8) + 100, block_row0(p, 12) + 200]
    xb[srcs] += np.float32(16)  # three rows apart from the rest and from each other
    xb[srcs[1], :8] += np.float32(5)
    xb[srcs[2], 8:16] += np.float32(5)
    plant_ties(xb, srcs[0], srcs[0] + 1 + np.arange(100))
    plant_ties(xb, srcs[1], srcs[1] + 1 + np.arange(KB - 1))
    plant_ties(xb, srcs[2], np.concatenate([srcs[2] + 1 + np.arange(50), block_row0(p, 13) + 5 + np.arange(60)]))
    xq = xb[srcs].copy()
    index = _index(faiss, xb)
    D_ref, I_ref = brute_knn(xb, xq, k, L2)
    assert (D_ref == 0).all()
    for kk in (1, k):
        for depth in DEPTHS:
            Dk, Ik, exact = _three_at(index, n, xq, kk, depth)
            _no_more_exact_scans(exact, f"copies, k = {kk}, depth {depth}")
            assert_knn_identical(Dk, Ik, D_ref[:, :kk], I_ref[:, :kk], f"copies in a deep boot window, k = {kk}, depth {depth}")


def _on_streams(index, tq, k, streams, order):
    """One batch per entry of `order` on streams[entry]; returns the outputs and the (isolated, deep) counts of each."""
    import torch

    outs, moves = [], []
    for j in order:
        c0 = _depth_counts(index)
        with torch.cuda.stream(streams[j]):
            outs.append(index.search_torch(tq, k))
        c1 = _depth_counts(index)
        moves.append((c1[0] - c0[0], c1[1] - c0[1]))
    torch.cuda.synchronize()
    return [(Do.cpu().numpy(), Io.cpu().numpy()) for Do, Io in outs], moves


def test_which_batches_go_deep(uniform):
    """4. the rule: a batch on another stream than the index's previous search takes the deep plan, one on the same
    stream and every batch with the depth forced to 1 the isolated one.  Same bits each time."""
    import torch

    index, xb = uniform[N]
    k = 10
    xq = _rng("sd", "rule").random((16, D), dtype=np.float32)
    ref = index.search(xq, k)
    tq = torch.from_numpy(xq).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    index.reserve(16, k)
    # two streams used alternately: every batch after the first is counted deep (the first follows index.search,
    # which ran on a stream of the library's own: deep as well)
    outs, moves = _on_streams(index, tq, k, streams, [0, 1, 0, 1, 0])
    assert moves == [(0, 1)] * 5, moves
    # one stream: the first batch follows one on the other stream, the rest are isolated
    outs1, moves = _on_streams(index, tq, k, streams, [1, 1, 1, 1])
    assert moves == [(0, 1)] + [(1, 0)] * 3, moves
    # an isolated batch, then a deep one, then an isolated one, in the slots reserve() sized
    outs2, moves = _on_streams(index, tq, k, streams, [1, 0, 0])
    assert moves == [(1, 0), (0, 1), (1, 0)], moves
    with depth_knob(1):
        outs3, moves = _on_streams(index, tq, k, streams, [0, 1, 0, 1])
    assert moves == [(1, 0)] * 4, moves
    with depth_knob(4):
        outs4, moves = _on_streams(index, tq, k, streams, [1, 1])
    assert moves == [(0, 1)] * 2, moves
    for o in outs + outs1 + outs2 + outs3 + outs4:
        _same_bits(o, ref, "a batch on a stream against the sequential reference")


def test_sixteen_streams_six_batches_with_both_plans(uniform):
    """5. 16 threads x 6 batches on their own streams over the six workspace slots, near and far batches alternating:
    the two plans lay the exchange entries out differently in the same slot, an entry of another launch carries another
    sequence and counts as absent whichever layout wrote it.  A thread's first batch follows another stream's and is
    deep; which of the others are depends on the interleaving.  A list emptied by a foreign bound would fail the
    certificate and come back with the right bits from the exact scan, so the count of queries sent there is bounded
    as in tests/test_boot_seed_gpu.py."""
    import torch

    index, xb = uniform[N]
    k = 10
    rng = _rng("sd", "conc")
    qs = [(xb[rng.integers(0, N, 16)] + np.float32(0.001)).astype(np.float32) if i % 2 else
          rng.random((16, D), dtype=np.float32) * np.float32(3.0) for i in range(16)]
    refs, other = [], [0, 0]
    for q in qs:  # sequential, isolated: the byte route asserted, the three routes' bits equal, each route's exact scans
        Dr, Ir, (xb8, xh, xf) = _three(index, q, k, "byte")
        assert xb8 <= max(xh, xf), f"sequential batch: exact scans byte {xb8}, fp16 {xh}, float32 {xf}"
        refs.append((Dr, Ir))
        other[0] += xh
        other[1] += xf
    (i0, d0), e0 = _depth_counts(index), index.exact_stats()["exact_scan"]
    errors = []

    def work(i):
        try:
            st = torch.cuda.Stream()
            tq = torch.from_numpy(qs[i]).cuda()
            with torch.cuda.stream(st):
                outs = [index.search_torch(tq, k) for _ in range(6)]
            st.synchronize()
            for Do, Io in outs:
                assert np.array_equal(Io.cpu().numpy(), refs[i][1]), i
                assert np.array_equal(Do.cpu().numpy().view(np.uint32), refs[i][0].view(np.uint32)), i
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(16)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    i1, d1 = _depth_counts(index)
    assert (i1 - i0) + (d1 - d0) == 16 * 6 and d1 - d0 >= 16, (i1 - i0, d1 - d0)
    sent = index.exact_stats()["exact_scan"] - e0
    assert sent <= 6 * max(other), f"threaded byte batches sent {sent} queries to the exact scan, fp16 / float32 {other}"
