"""GPU tests of the 8-bit scan (csrc/ise_sq.hpp, sq_scan_body) where tests/test_sq_gpu.py and tests/test_ivfsq_gpu.py do
not reach: step counts that do not divide the ring of four, the d at which QT switches (and the largest LDS footprint),
waves that stream three tiles or more and cut their buffers under live thresholds on rows of several steps, a second
staging chunk at QT = 8, the query's power of two, and every kind of query that gets padding.  Parts A to E use the
integer construction of tests/sq_ref.py: every comparison is bit for bit, no tolerance, and every case asserts the range
in which float32 is exact and the scan's own condition 128 sum |w_j| < 2^24.  Part F runs real-valued data whose trained
range an outlier stretches and asserts the error bound DESIGN.md 4.15 derives (``sq_ref.score_bound``)."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref, sq_ref
from tests.knn_checks import (HUGE, assert_exact_range, assert_knn_identical, assert_knn_matches, brute_knn, int_data,
                              true_scores)
from tests.sel_ref import IP, L2, pad_value
from tests.test_ivfsq_gpu import check_lists, force_add, new_index, search_pre, sizes_of, sq_index
from tests.test_sq_gpu import CHUNKS, QTYPES, check_searches, integer_index

pytestmark = pytest.mark.gpu

SQ = faiss.ScalarQuantizer


def assert_scan_exact(xq, t, d, qtype, metric):
    """The scan's own condition: with the weights w_j = s_j (x_j - o_j) (L2) or s_j x_j (inner product), o_j = vmin_j +
    s_j / 2, the accumulators hold 2^sh times partial sums of w_j (c_j - 128), integers of magnitude at most
    128 sum_j |w_j|: below 2^24 every one of them is an exact float32."""
    vmin, vdiff = sq_ref.expand(t, d, qtype)
    s = vdiff.astype(np.float64) / 255.0  # 1 or 2 on the integer construction: exact
    o = vmin.astype(np.float64) + s / 2.0
    x = np.asarray(xq, np.float64)
    w = s[None, :] * (x - o[None, :]) if metric == L2 else s[None, :] * x
    assert np.array_equal(w, np.rint(w)), "integer weights expected"
    held = 128.0 * np.abs(w).sum(1)
    assert (held < 1 << 24).all(), f"the accumulators leave float32's exact integer range: {held.max():.0f}"


def counted_search(index, xq, k):
    """search, with the counters checked: one batch, ceil(nq / QT) * ceil(k / 32) passes."""
    before = index.sq_stats()
    D, I = index.search(xq, k)
    after = index.sq_stats()
    assert after["search_batches"] - before["search_batches"] == 1
    assert after["scan_passes"] - before["scan_passes"] == sq_ref.passes_of(index.d, len(xq), k)
    return D, I


def check_stored(index, t, xb, base):
    """The stored bytes and the decoded rows are the construction's (stride - d pad bytes lie behind every row)."""
    vmin, vdiff = sq_ref.expand(t, index.d, index.qtype)
    got = index.codes
    assert got.dtype == np.uint8 and got.shape == base.shape and np.array_equal(got, base)
    assert np.array_equal(sq_ref.encode(xb, vmin, vdiff), base)
    rec = index.reconstruct_n()
    assert rec.dtype == np.float32 and np.array_equal(rec.view(np.uint32), sq_ref.decode(base, vmin, vdiff).view(np.uint32))
    assert np.array_equal(rec.view(np.uint32), xb.view(np.uint32))


# ---------------------------------------------------------------- A. step counts that do not divide the ring
ODD_D = [130, 192, 193, 320, 448, 576]  # 3, 3, 4, 5, 7 and 9 steps of 64 entries


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("d", ODD_D)
def test_odd_step_counts(d, qtype, metric):
    """600 rows, grid 2: the waves of block 0 take two tiles (two of them a ragged second one), those of block 1 one:
    the ring slot at which a tile ends moves from tile to tile."""
    n = 600
    assert sq_ref.grid_of(n, d, 256) == 2
    index, t, xb, base, xq = integer_index(d, qtype, metric, n, 5000 + 7 * d + qtype, nq=17)
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, qtype, metric)
    check_stored(index, t, xb, base)
    check_searches(index, xq, xb, metric, (1, 16, 17), (1, 10, 33, 70), d)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("n", [63, 65])
@pytest.mark.parametrize("d", [130, 320])
def test_odd_step_counts_at_tile_edges(d, n, qtype, metric):
    index, t, xb, base, xq = integer_index(d, qtype, metric, n, 5100 + 7 * d + n + qtype, nq=17)
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, qtype, metric)
    check_stored(index, t, xb, base)
    check_searches(index, xq, xb, metric, (1, 16, 17), (1, 10, 33, 70), d)


def check_lists_against_flat(index, sqi, xq, xb, assign, tables, nqs, ks, metric):
    """Every probe table, nq and k: the brute force over the probed members, and the flat index's bits."""
    n, nlist = len(xb), index.nlist
    full = sq_ref.expected(xq, xb, n, metric)  # the complete rankings, computed once
    full_sq = sqi.search(xq, n)
    assert_knn_identical(*full_sq, *full, "the flat scalar-quantised index")
    for probes in tables:
        members = ivf_ref.probed_members(probes, assign, nlist)
        for nq in nqs:
            for k in ks:
                what = f"probes {probes[0].tolist()}.. nq={nq} k={k}"
                D, I = search_pre(index, xq[:nq], k, probes[:nq])
                assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full[0][:nq], full[1][:nq], members[:nq], k, metric), what)
                assert_knn_identical(D, I, *ivf_ref.expected_from_ranking(full_sq[0][:nq], full_sq[1][:nq], members[:nq], k, metric),
                                     "IndexScalarQuantizer's bits " + what)
                if probes.shape[1] == nlist:
                    assert_knn_identical(D, I, *sqi.search(xq[:nq], k), "all lists " + what)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("d", ODD_D)
def test_odd_step_counts_in_lists(d, qtype, metric):
    n, sizes, nq = 600, [0, 1, 64, 65, 470], 17
    rng = np.random.default_rng(5200 + 7 * d + qtype)
    t, m, s = sq_ref.integer_trained(rng, d, qtype)
    xb, base = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, qtype, metric)
    assign = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    qz, index = new_index(d, qtype, metric, rng.standard_normal((len(sizes), d)), t)
    i0 = 0
    for c in CHUNKS:
        force_add(index, xb[i0:i0 + c], assign[i0:i0 + c])
        i0 += c
    assert sizes_of(index) == sizes and index.ntotal == n
    check_lists(index, assign, base)
    every = np.tile(np.arange(len(sizes)), (nq, 1))
    two = np.stack([np.arange(nq) % 5, (np.arange(nq) + 2) % 5], axis=1)  # the empty list and the list of one among them
    check_lists_against_flat(index, sq_index(d, qtype, metric, t, xb), xq, xb, assign, (every, two), (1, 16, 17), (1, 10, 33, 70),
                             metric)


# ---------------------------------------------------------------- B. the QT switch
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [1472, 1473])
def test_qt_switch(d, metric):
    """d = 1472: 16 queries per pass and the largest dynamic LDS request there is; d = 1473: 8 queries per pass, the
    MFMA's columns 8 .. 15 mirrors of 0 .. 7.  A launch that fails raises RuntimeError."""
    n, nq, nlist = 300, 17, 3
    assert sq_ref.qt_of(d) == (16 if d == 1472 else 8)
    assert sq_ref.lds_bytes(d) == (160_512 if d == 1472 else 82_304) and sq_ref.lds_bytes(d) <= sq_ref.LDS_LIMIT
    index, t, xb, base, xq = integer_index(d, SQ.QT_8bit, metric, n, 1400 + d, nq=nq, kind="binary", qkind="binary")
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, SQ.QT_8bit, metric)
    check_stored(index, t, xb, base)
    check_searches(index, xq, xb, metric, (1, 8, 9, 16, 17), (1, 33), d)
    # three lists; queries 8 .. 15 probe another list than 0 .. 7 and the last query a third
    rng = np.random.default_rng(1500 + d)
    assign = np.repeat(np.arange(nlist), [100, 130, 70])
    qz, ivf = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    force_add(ivf, xb, assign)
    check_lists(ivf, assign, base)
    every = np.tile(np.arange(nlist), (nq, 1))
    one = np.array([[0]] * 8 + [[1]] * 8 + [[2]], np.int64)
    check_lists_against_flat(ivf, index, xq, xb, assign, (every, one), (1, 8, 9, 16, 17), (1, 33), metric)


# ---------------------------------------------------------------- C. a long index: the stream after a cut
def num_cu(device) -> int:
    import torch

    return int(torch.cuda.get_device_properties(device).multi_processor_count)


def pointing_at(code, m, s, metric):
    """The query whose best rows are exactly those with the binary code ``code``: L2, the decoded row (distance 0);
    inner product, +1 where the code is 1 and -1 where it is 0 (changing code byte j costs s_j under either metric)."""
    return (m + s * code).astype(np.float32) if metric == L2 else (2.0 * code - 1.0).astype(np.float32)


@pytest.mark.parametrize("metric", [L2, IP])
def test_long_index_streams_cuts_and_worst_case_order(metric):
    """d = 260: five steps, one block per CU.  Every wave streams three tiles or more, so keys are turned away by a live
    threshold, appended behind the keys a cut kept, and cut again; the floors of passes two and three fall inside streams
    that cut.  Query 0 sees the worst-case order (every row beats or ties all before it: a cut after every tile from the
    second on), the others a random order.  Wave 0 of block 0 streams tiles 0, 4 G, 8 G, 12 G: the best row for query 1
    is row 0 and its runner-up the LAST row of tile 8 G, which has to get in below the threshold of the first cut; one
    tie group sits in tile 0, in tile 4 G and in the last tile (3 rows)."""
    d, nq, qtype = 260, 17, SQ.QT_8bit
    index = faiss.IndexScalarQuantizer(d, qtype, metric)
    cus = num_cu(index.device)
    per_cu = max(1, sq_ref.LDS_LIMIT // sq_ref.lds_bytes(d))
    assert per_cu == 1 and sq_ref.qt_of(d) == 16
    gcap = min(per_cu * cus, sq_ref.MERGE_LISTS_MAX)
    n = 64 * 12 * gcap + 3
    G = sq_ref.grid_of(n, d, cus)
    tpw = -(-n // 64) // (4 * G)  # the fewest tiles a wave takes
    print(f"d={d}: {cus} CUs, grid {G}, {n} rows, tiles per wave {tpw} (wave 0 of block 0: {tpw + 1})")
    assert G == gcap and tpw >= 3
    runner = 8 * G * 64 + 63
    tie = [5, 64 * 4 * G + 1, n - 1]
    assert tie[1] < runner < n - 3

    rng = np.random.default_rng(2600 + metric)
    t, m, s = sq_ref.integer_trained(rng, d, qtype)
    index.sq.set_trained(t)
    j1 = int(np.flatnonzero(s == 1)[0])  # the byte whose change costs least
    best, group = rng.integers(0, 2, d).astype(np.uint8), rng.integers(0, 2, d).astype(np.uint8)
    xq = int_data("small", rng, nq, d)
    xq[1], xq[-1] = pointing_at(best, m, s, metric), pointing_at(group, m, s, metric)
    assert_exact_range((np.abs(m) + s)[None, :].astype(np.float32), xq)  # |m_j + s_j c_j| <= |m_j| + s_j for c_j in {0, 1}
    assert_scan_exact(xq, t, d, qtype, metric)
    codes = rng.integers(0, 2, (n, d), dtype=np.uint8)
    S = sq_ref.scores_from_codes(codes, m, s, xq, metric)
    order = np.argsort(-S[:, 0] if metric == L2 else S[:, 0], kind="stable")  # query 0: every row beats or ties its predecessors
    codes, S = codes[order], S[order]
    codes[0] = best
    codes[runner] = best
    codes[runner, j1] ^= 1
    codes[tie] = group
    planted = [0, runner] + tie
    S[planted] = sq_ref.scores_from_codes(codes[planted], m, s, xq, metric)
    ids = np.arange(n, dtype=np.int64)
    tops = [sq_ref.top_of_scores(np.ascontiguousarray(S[:, q]), ids, 70, metric) for q in range(nq)]
    Dw, Iw = np.stack([tp[0] for tp in tops]), np.stack([tp[1] for tp in tops])
    assert Iw[1, :2].tolist() == [0, runner] and Iw[-1, :3].tolist() == tie  # the data are what they were built to be

    index._add_codes(codes)
    assert index.ntotal == n and np.array_equal(index.codes, codes)
    flat = {}
    for k in (1, 32, 33, 70):
        flat[k] = counted_search(index, xq, k)
        assert_knn_identical(*flat[k], Dw[:, :k], Iw[:, :k], f"k={k}")
    # the first 70 000 rows again, through the encoder: its row terms, where the index above has the row-term kernel's
    n2 = 70_000
    twin = faiss.IndexScalarQuantizer(d, qtype, metric)
    twin.sq.set_trained(t)
    twin.add((m[None, :] + s[None, :] * codes[:n2]).astype(np.float32))
    assert twin.ntotal == n2 and np.array_equal(twin.codes, codes[:n2])
    D2, I2 = counted_search(twin, xq, 33)
    for q in range(nq):
        Dq, Iq = sq_ref.top_of_scores(np.ascontiguousarray(S[:n2, q]), ids[:n2], 33, metric)
        assert_knn_identical(D2[q:q + 1], I2[q:q + 1], Dq[None, :], Iq[None, :], f"the encoded copy, q={q}")
    # the same rows in three lists by contiguous thirds, every list probed
    third = n // 3
    lists = np.repeat(np.arange(3), [third, third, n - 2 * third])
    qz, ivf = new_index(d, qtype, metric, rng.standard_normal((3, d)), t)
    ivf._add_codes(codes, lists)
    assert ivf.ntotal == n and sizes_of(ivf) == [third, third, n - 2 * third]
    every = np.tile(np.arange(3), (nq, 1))
    for k in (1, 32, 33, 70):
        D, I = search_pre(ivf, xq, k, every)
        assert_knn_identical(D, I, *flat[k], f"lists against the flat index, k={k}")
        assert_knn_identical(D[:2], I[:2], Dw[:2, :k], Iw[:2, :k], f"lists against the exact top, k={k}")


@pytest.mark.parametrize("d", [130, 1473])  # QT = 16, 8
def test_one_block_cut_then_short_lists(d):
    """512 rows are eight tiles in one block (``sq_ref.one_block_case``): wave 0 streams tiles 0 and 4 and cuts after the
    second, every wave folds.  The rows lie in descending distance to query 0 (every key of the second tile passes),
    k = 33 runs the floor-keyed second pass and the merge's floor write.  The last three queries are far from all rows --
    an entry of 2^64: finite weights, every distance rounds to inf -- so their lists end without a key in either pass,
    beside queries whose lists are full.  The same case through two inverted lists: tests/test_ivfsq_gpu.py."""
    qtype = SQ.QT_8bit
    assert sq_ref.grid_of(512, d, 256) == 1 and sq_ref.qt_of(d) == (16 if d == 130 else 8)
    t, xb, base, plain, xq, Dw, Iw = sq_ref.one_block_case(d)
    assert_scan_exact(plain, t, d, qtype, L2)
    index = sq_index(d, qtype, L2, t, xb)
    check_stored(index, t, xb, base)
    D, I = counted_search(index, xq, 33)
    assert_knn_identical(D, I, Dw, Iw, f"the flat index, d={d}")
    assert (D[13:] == pad_value(L2)).all()


# ---------------------------------------------------------------- D. a second staging chunk at QT = 8
@pytest.mark.parametrize("metric", [L2, IP])
def test_chunk_reuse_at_qt8(metric):
    """73 queries at d = 1473: a full chunk of 64 (eight passes), then a pass of eight and a pass of one whose records
    take the first chunk's place in the one buffer."""
    import torch

    d, n, nq = 1473, 130, 73
    assert sq_ref.qt_of(d) == 8
    index, t, xb, base, xq = integer_index(d, SQ.QT_8bit, metric, n, 7300, nq=nq, kind="binary", qkind="binary")
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, SQ.QT_8bit, metric)
    check_searches(index, xq, xb, metric, (nq,), (1, 33), d)
    xq_t = torch.from_numpy(xq).to(torch.device("cuda", index.device))
    for k in (1, 33):
        D, I = index.search(xq, k)
        Dt, It = index.search_torch(xq_t, k)
        assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D, I, f"search_torch k={k}")
        for a, b in ((64, 73), (70, 71)):
            assert_knn_identical(*counted_search(index, xq[a:b], k), D[a:b], I[a:b], f"queries {a}..{b} alone, k={k}")
            Dt, It = index.search_torch(xq_t[a:b], k)
            assert_knn_identical(Dt.cpu().numpy(), It.cpu().numpy(), D[a:b], I[a:b], f"search_torch of queries {a}..{b}, k={k}")


# ---------------------------------------------------------------- E. the query's scale, and what gets padding
@pytest.mark.parametrize("d", [24, 130])
def test_inner_product_follows_the_query_scale(d):
    """A query times 2^e: the same ids, and D times 2^e bit for bit -- the staging scales the weights by the query's own
    power of two, and nothing overflows or goes subnormal at these e."""
    index, t, xb, base, xq = integer_index(d, SQ.QT_8bit, IP, 600, 8000 + d, nq=20, qkind="signed")
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, SQ.QT_8bit, IP)
    D0, I0 = counted_search(index, xq, 33)
    assert_knn_identical(D0, I0, *sq_ref.expected(xq, xb, 33, IP), "unscaled")
    for e in (-120, -20, 40, 100):
        scaled = np.ldexp(xq, e).astype(np.float32)
        assert np.isfinite(scaled).all() and np.array_equal(np.ldexp(scaled.astype(np.float64), -e), xq)
        want = np.ldexp(D0.astype(np.float64), e).astype(np.float32)
        assert np.array_equal(np.ldexp(want.astype(np.float64), -e), D0) and np.isfinite(want).all()
        D, I = counted_search(index, scaled, 33)
        assert_knn_identical(D, I, want, I0, f"queries times 2^{e}")
        assert_knn_identical(D, I, *sq_ref.expected(scaled, xb, 33, IP), f"the reference at 2^{e}")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [24, 130])
def test_all_zero_query(d, metric):
    """amax = 0, sh = 0.  Inner product: every score +0, so ids 0 .. k - 1; L2: the ranking by |y|^2."""
    n = 600
    index, t, xb, base, xq = integer_index(d, SQ.QT_8bit, metric, n, 8100 + d, nq=20, qkind="signed")
    zeros = [0, 7, 16, 19]
    xq[zeros] = 0.0
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, SQ.QT_8bit, metric)
    norms = (xb.astype(np.float64) ** 2).sum(1)
    by_norm = np.lexsort((np.arange(n), norms))
    for k in (1, 10, 33):
        D, I = counted_search(index, xq, k)
        assert_knn_identical(D, I, *sq_ref.expected(xq, xb, k, metric), f"k={k}")
        for q in zeros:
            if metric == IP:
                assert I[q].tolist() == list(range(k)) and (D[q] == 0).all() and not np.signbit(D[q]).any()
            else:
                assert I[q].tolist() == by_norm[:k].tolist() and np.array_equal(D[q], norms[by_norm[:k]].astype(np.float32))
        assert_knn_identical(*index.search(xq[:1], k), D[:1], I[:1], f"the zero query alone, k={k}")


BAD_AT = [0, 15, 16, 19]  # of 20 queries: the first, both sides of the pass edge, the last
BAD_KINDS = [(kind, metric) for metric in (L2, IP) for kind in ("nan", "inf", "-inf", "overflow")] + [("huge", L2)]


def spoil(xq, kind, s):
    """Queries BAD_AT get one entry (at another column each) that is NaN, +inf, -inf, 3e38 under a step of 2 (the weight
    overflows) or 2^64 (finite weights; every L2 score rounds to inf)."""
    d = xq.shape[1]
    twos = np.flatnonzero(s == 2)
    assert twos.size >= len(BAD_AT)
    bad = xq.copy()
    for i, q in enumerate(BAD_AT):
        col = int(twos[i]) if kind == "overflow" else (0, d - 1, d // 2, 5)[i]
        bad[q, col] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "overflow": np.float32(3e38), "huge": HUGE}[kind]
    return bad


@pytest.mark.parametrize("kind,metric", BAD_KINDS)
@pytest.mark.parametrize("d", [24, 130])
def test_bad_queries_get_padding(d, kind, metric):
    n, nq, nlist = 600, 20, 3
    index, t, xb, base, xq = integer_index(d, SQ.QT_8bit, metric, n, 8200 + d, nq=nq)
    assert_exact_range(xb, xq)
    assert_scan_exact(xq, t, d, SQ.QT_8bit, metric)
    vmin, vdiff = sq_ref.expand(t, d, SQ.QT_8bit)
    bad = spoil(xq, kind, sq_ref.step_of(vdiff))
    good = [q for q in range(nq) if q not in BAD_AT]
    if kind == "overflow":
        with np.errstate(over="ignore"):
            assert np.isfinite(bad).all() and np.isinf(sq_ref.staged_weights(bad[BAD_AT], vmin, vdiff, metric)[1]).any(1).all()
    if kind == "huge":  # finite weights: what the reference's gate gives decides -- no score is below FLT_MAX
        assert np.isfinite(sq_ref.staged_weights(bad[BAD_AT], vmin, vdiff, metric)[1]).all()
        assert (brute_knn(xb, bad[BAD_AT], 33, metric)[1] == -1).all()
    rng = np.random.default_rng(8300 + d)
    assign = rng.integers(0, nlist, n)
    qz, ivf = new_index(d, SQ.QT_8bit, metric, rng.standard_normal((nlist, d)), t)
    force_add(ivf, xb, assign)
    every = np.tile(np.arange(nlist), (nq, 1))
    for k in (1, 33):
        D, I = counted_search(index, bad, k)
        assert (I[BAD_AT] == -1).all() and (D[BAD_AT] == pad_value(metric)).all(), f"k={k}"
        assert_knn_identical(D[good], I[good], *index.search(xq[good], k), f"beside the bad queries, k={k}")
        assert_knn_identical(D[good], I[good], *sq_ref.expected(xq[good], xb, k, metric), f"the reference, k={k}")
        assert_knn_identical(*search_pre(ivf, bad, k, every), D, I, f"the lists, k={k}")


# ---------------------------------------------------------------- F. the error bound on stretched ranges
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("family", [30, 100, 900, "offset", "relu"])
@pytest.mark.parametrize("d", [64, 512])
def test_error_bound_on_stretched_ranges(d, family, qtype, metric):
    """Rows and queries near one end of a trained range that an outlier stretches (``sq_ref.stretched_case``): the
    weights and the centred codes keep one sign, the float32 accumulators hold 128 sum |w_j|, far above the score.
    Asserted: |D - D64| <= the derived worst case (``sq_ref.score_bound``), elementwise, against float64
    over the decoded rows, and ranks that are right up to that bound.  The measured error is printed, not asserted."""
    n, nq, k = 600, 8, 10
    train, xb, xq = sq_ref.stretched_case(family, d, qtype, n=n, nq=nq)
    index = faiss.IndexScalarQuantizer(d, qtype, metric)
    index.train(train)
    index.add(xb)
    t = index.sq.trained
    assert np.array_equal(t.view(np.uint32), sq_ref.train_minmax(train, qtype).view(np.uint32))
    vmin, vdiff = sq_ref.expand(t, d, qtype)
    codes = index.codes
    rec = index.reconstruct_n()
    assert np.array_equal(rec.view(np.uint32), sq_ref.decode(codes, vmin, vdiff).view(np.uint32))
    D, I = counted_search(index, xq, k)
    Iw = brute_knn(rec, xq, k, metric)[1]
    D64 = true_scores(rec, xq, Iw, metric)
    E, parts = sq_ref.score_bound(xq, codes, vmin, vdiff, metric)
    bound = E[:, None] * (1 + sq_ref.U) + sq_ref.U * np.abs(D64)
    err = np.abs(D.astype(np.float64) - D64)
    rel = err / np.maximum(1.0, np.abs(D64))
    emu = np.abs(np.take_along_axis(sq_ref.emulate_scores(xq, codes, vmin, vdiff, metric).astype(np.float64), I, axis=1)
                 - D.astype(np.float64)).max()
    print(f"d={d} family={family} qtype={qtype} metric={metric}: largest |D - D64| = {err.max():.3e}, / max(1, |D64|) = "
          f"{rel.max():.3e}; largest error / bound = {(err / bound).max():.3e} (bound / max(1, |D64|) up to "
          f"{(bound / np.maximum(1.0, np.abs(D64))).max():.3e}); largest |D - emulation| = {emu:.3e}")
    assert (err <= bound).all(), f"largest error / bound = {(err / bound).max():.3e}"
    assert_knn_matches(D, I, D64, Iw, rec, xq, metric, rtol=float((bound / np.maximum(1.0, np.abs(D64))).max()),
                       atol=float(bound.max()), near=2.0 * bound.max(1))
    if metric == L2:
        assert (D >= 0).all()
