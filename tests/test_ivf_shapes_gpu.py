"""GPU tests of the inverted-list scan (csrc/ise_ivf.hpp, ivf_scan_kernel; csrc/ise_ivf.hip, ivf_chunk_enqueue) at every
row-length class: the register chunk ch = 1, 2, 4, scalar and vector query staging, rows so long that the wave lists'
LDS holds fewer than 32 results per pass (kp), the length at which the search is refused, launches of more than 64
queries with probes that differ per launch, and more lists than rows.

Rows are filed under list numbers the test names (ise_ivf_add_host) and searched with search_preassigned, so no coarse
quantiser takes part.  The data are small integers (tests/knn_checks.py): every result must equal the float64 brute
force over each query's probed members (tests/ivf_ref.py) bit for bit, ties by ascending id.  The Python mirrors of the
host's geometry only choose inputs and assert that a case reaches the path it is meant for."""
import zlib

import numpy as np
import pytest

from image_search_engine_amd import _native as native
from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref
from tests.knn_checks import assert_exact_range, assert_knn_identical, int_data
from tests.sel_ref import IP, L2, pad_value
from tests.test_assign_shapes_gpu import pad_dim, qs_stride_units

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ mirrors of the host geometry (inputs and premises only)
LDS_LIMIT = 160 * 1024   # csrc/ise_scan_params.hpp
SEL_W = 8                # csrc/ise_sel_scan.hpp: waves per block
SEL_KPASS_MAX = 32       # most results per query of one pass
IVF_NQ_CHUNK = 64        # csrc/ise_ivf.hip: queries per launch


def chunk_steps(d):
    """csrc/ise_geometry.hpp, chunk_steps_rb, capped at 4 as ivf_chunk_enqueue does: k-steps per register chunk."""
    steps = pad_dim(d) * 4 // 64
    return next((min(ch, 4) for ch in (8, 4, 2) if steps % ch == 0), 1)


def vec_staging(d):
    """csrc/ise_geometry.hpp, range_staging_rule for float32 rows and the pass's 8 waves (32 threads per query row)."""
    tpr = 32 if SEL_W >= 8 else 16
    return int(d % 4 == 0 and (qs_stride_units(pad_dim(d)) >> 2) <= tpr * 8)


def range_lds_bytes(S):
    """csrc/ise_range.hpp: mus [S] | qs [16][S] | xn [16]."""
    return S * 4 + 16 * S * 4 + 16 * 4


def kp_cap(d):
    """Results per pass the wave lists' LDS holds beside the query rows (ivf_chunk_enqueue): below 1 is a refusal."""
    left = LDS_LIMIT - range_lds_bytes(qs_stride_units(pad_dim(d)))
    return int(left / (SEL_W * 16 * 8))  # C's division: towards zero


def kpass(d, k):
    return min(k, SEL_KPASS_MAX, kp_cap(d))


def passes_of(d, k, nq):
    """Scan passes of one search: per launch of up to 64 queries, one pass per kp results."""
    return -(-nq // IVF_NQ_CHUNK) * -(-k // kpass(d, k))


def test_geometry_mirrors():
    """The constants the cases below are built on, as read off the host code."""
    assert [kp_cap(d) for d in (17, 1024, 1920, 2048, 2368)] == [155, 91, 31, 23, 2]
    assert qs_stride_units(2048) == 2056 and qs_stride_units(2368) == 2376
    assert kp_cap(2369) < 1 and pad_dim(2369) == 2432
    assert {(chunk_steps(d), vec_staging(d)) for d in SWEEP} == {(ch, v) for ch in (1, 2, 4) for v in (0, 1)}


# ------------------------------------------------------------------------------------------------ helpers
def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def new_ivf(d, nlist, metric):
    """An index whose quantiser stays empty: rows come with their list numbers, searches with their probes."""
    return faiss.IndexIVFFlat(faiss.IndexFlatL2(d), d, nlist, metric)


def force_add(ivf, x, lists):
    x = np.ascontiguousarray(x, dtype=np.float32)
    lists = np.ascontiguousarray(lists, dtype=np.int64)
    native.check(native.lib.ise_ivf_add_host(ivf._h, x.ctypes.data, lists.ctypes.data, len(x)))


def filed(d, nlist, metric, xb, assign, chunks):
    ivf = new_ivf(d, nlist, metric)
    i0 = 0
    for c in chunks:
        force_add(ivf, xb[i0:i0 + c], assign[i0:i0 + c])
        i0 += c
    assert i0 == len(xb) and ivf.ntotal == len(xb)
    assert [ivf.list_size(l) for l in range(nlist)] == np.bincount(assign, minlength=nlist).tolist()
    return ivf


def counted(ivf, d, xq, k, probes):
    """search_preassigned, with its batch and pass counts asserted -> (D, I)."""
    before = ivf.ivf_stats()
    D, I = ivf.search_preassigned(xq, k, probes)
    after = ivf.ivf_stats()
    assert after["batches"] - before["batches"] == 1
    assert after["passes"] - before["passes"] == passes_of(d, k, len(xq)), (d, k, len(xq))
    return D, I


def check(ivf, d, metric, xb, xq, assign, probes, ks, what):
    """Every k of ks against the brute force over the probed members (computed once, at the largest k)."""
    members = ivf_ref.probed_members(probes, assign, ivf.nlist)
    Dw, Iw = ivf_ref.expected_brute(xb, xq, members, max(ks), metric)
    for k in ks:
        D, I = counted(ivf, d, xq, k, probes)
        assert_knn_identical(D, I, Dw[:, :k], Iw[:, :k], f"{what} k={k}")


# ------------------------------------------------------------------------------------ 1. row-length sweep
N, NLIST = 600, 7
SIZES = [16, 1, 0, 100, 200, 150, 133]  # exactly one tile, one row, empty, 6 tiles + 4 rows, ...
CHUNKS = [250, 1, 349]
# d -> (ch, vec_q).  32 and 48 complete the (ch, vec_q) combinations: a row without padding, staged by vector
SWEEP = {1: (1, 0), 3: (1, 0), 17: (2, 0), 32: (2, 1), 33: (1, 0), 48: (1, 1), 63: (4, 0), 65: (4, 0), 130: (4, 0),
         257: (4, 0), 600: (4, 1), 1024: (4, 0)}


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", sorted(SWEEP))
def test_row_length_sweep(d, metric):
    """600 rows in seven lists (one empty, one of a single row, one of exactly a tile), 1 and 17 queries, k up to three
    passes, one, three and all lists probed -- per query different ones."""
    assert (chunk_steps(d), vec_staging(d)) == SWEEP[d]
    assert kpass(d, 70) == 32
    for kind in ("small", "binary"):
        rng = _rng("sweep", d, metric, kind)
        xb, xq = int_data(kind, rng, N, d), int_data(kind, rng, 17, d)
        xq[0] = xb[77]
        assert_exact_range(xb, xq)
        assign = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
        ivf = filed(d, NLIST, metric, xb, assign, CHUNKS)
        q = np.arange(17)
        for name, probes in (("one", (q % NLIST)[:, None]),
                             ("three", np.stack([q % NLIST, (q + 2) % NLIST, (q + 3) % NLIST], axis=1)),
                             ("all", np.tile(np.arange(NLIST), (17, 1)))):
            for nq in (1, 17):
                check(ivf, d, metric, xb, xq[:nq], assign, probes[:nq], (1, 10, 33, 70), f"d={d} {kind} {name} nq={nq}")


# --------------------------------------------------------------------------------------- 2. shrinking kp
KP_HAND = {1920: 31, 2048: 23, 2368: 2}  # 2048 and 2368: the hand derivation this file was asked to confirm


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", sorted(KP_HAND))
def test_shrinking_kp(d, metric):
    """Rows so long that a pass keeps fewer than 32 results per query: the wave lists, the block fold's i / kp and
    i % kp, wave_select and the floor of the later passes all run at that kp.  300 binary rows in three lists; 40
    all-ones rows at ids 0 .. 39 tie at the top for the all-ones query, the smaller ids in the LATER lists, and every
    other row has four zeros at least: with k beyond kp the second pass's floor falls inside the group."""
    kp = kp_cap(d)
    assert kp == KP_HAND[d] and pad_dim(d) == d and chunk_steps(d) == 4
    n, nlist, ties = 300, 3, 40
    assert ties > kp
    rng = _rng("kp", d, metric)
    xb = (rng.random((n, d)) < 0.6).astype(np.float32)
    xb[:, :4] = 0.0
    xb[:ties] = 1.0
    xq = (rng.random((17, d)) < 0.6).astype(np.float32)
    xq[0] = 1.0
    xq[1] = 1.0
    xq[1, 0] = 0.0  # still ranks the group first: distance 1, score d - 1
    assert_exact_range(xb, xq)
    assign = np.concatenate([2 - np.arange(ties) // 14, rng.integers(0, nlist, n - ties)])
    ivf = filed(d, nlist, metric, xb, assign, [120, 180])
    assert ivf.get_list(2)[0][0] == 0 and ivf.get_list(0)[0][0] == 28
    ks = sorted({1, kp, kp + 1, 2 * kp + 1} | ({70} if kp >= 23 else set()))
    assert [passes_of(d, k, 17) for k in (1, kp, kp + 1, 2 * kp + 1)] == [1, 1, 2, 3]
    for probes in (np.tile(np.arange(nlist), (17, 1)), np.tile([2, 0], (17, 1))):
        for nq in (1, 17):
            check(ivf, d, metric, xb, xq[:nq], assign, probes[:nq], ks, f"d={d} probes={probes[0].tolist()} nq={nq}")
    D, I = ivf.search_preassigned(xq[:2], ties, np.tile(np.arange(nlist), (2, 1)))
    assert (I == np.arange(ties)).all() and (D[0] == (0.0 if metric == L2 else d)).all()


# ------------------------------------------------------------------------------------------- 3. refusal
@pytest.mark.parametrize("metric", [L2, IP])
def test_rows_too_long_are_refused_by_the_search(metric):
    """The smallest d at which not one result per pass fits beside the query rows: adding succeeds, a search raises and
    leaves the index as it was."""
    d = next(d for d in range(1, 4096) if kp_cap(d) < 1)
    assert d == 2369 and pad_dim(d) == 2432 and kp_cap(d - 1) == 2
    rng = _rng("refusal", metric)
    xb, xq = int_data("binary", rng, 50, d), int_data("binary", rng, 3, d)
    assign = rng.integers(0, 2, 50)
    ivf = filed(d, 2, metric, xb, assign, [50])
    for k in (1, 10):
        with pytest.raises(native.IseError, match="rows too long for the inverted-list search"):
            ivf.search_preassigned(xq, k, np.tile([0, 1], (3, 1)))
    assert ivf.ntotal == 50
    assert [ivf.list_size(l) for l in range(2)] == np.bincount(assign, minlength=2).tolist()
    for l in range(2):
        ids, rows = ivf.get_list(l)
        assert np.array_equal(ids, np.flatnonzero(assign == l)) and np.array_equal(rows, xb[ids])
    force_add(ivf, xb[:5], assign[:5])
    assert ivf.ntotal == 55


# -------------------------------------------------------------------------------------------- 4. chunks
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [64, 65, 130])
def test_launches_of_64_queries_with_their_own_probes(nq, metric):
    """More than 64 queries take several launches that share one mask array.  Every query probes ONE list, and query
    q + 64 never the list of query q: a mask left over from the launch before would hand out rows of a list the query
    does not probe."""
    d = 17
    rng = _rng("chunks", nq, metric)
    xb, xq = int_data("small", rng, N, d), int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    assign = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
    ivf = filed(d, NLIST, metric, xb, assign, CHUNKS)
    q = np.arange(nq)
    probes = ((rng.integers(0, NLIST, IVF_NQ_CHUNK)[q % IVF_NQ_CHUNK] + q // IVF_NQ_CHUNK) % NLIST)[:, None]
    assert (probes[IVF_NQ_CHUNK:] != probes[:-IVF_NQ_CHUNK]).all()
    chunks = -(-nq // IVF_NQ_CHUNK)
    assert chunks == {64: 1, 65: 2, 130: 3}[nq]
    assert [passes_of(d, k, nq) for k in (10, 40)] == [chunks, 2 * chunks]
    check(ivf, d, metric, xb, xq, assign, probes, (10, 40), f"nq={nq}")


# ------------------------------------------------------------------------------- 5. more lists than rows
@pytest.mark.parametrize("metric", [L2, IP])
def test_more_lists_than_rows(metric):
    """300 lists, 600 rows in 40 of them: the probe tables name empty lists, -1 and list numbers beyond nlist.  One
    query loads exactly the tiles of the non-empty lists it names, each once."""
    d, nlist, used = 33, 300, 40
    rng = _rng("sparse", metric)
    xb, xq = int_data("small", rng, N, d), int_data("small", rng, 17, d)
    assert_exact_range(xb, xq)
    homes = np.sort(rng.choice(nlist, used, replace=False))
    assign = homes[rng.integers(0, used, N)]
    sizes = np.bincount(assign, minlength=nlist)
    empty = np.flatnonzero(sizes == 0)
    assert (sizes > 0).sum() == used and len(empty) == nlist - used
    ivf = filed(d, nlist, metric, xb, assign, CHUNKS)
    probes = np.empty((17, 8), np.int64)
    for i in range(17):
        probes[i] = [homes[i % used], empty[i], -1, nlist, homes[(3 * i + 1) % used], nlist + 7, homes[i % used], empty[-1 - i]]
    probes[5] = [empty[0], -1, nlist, empty[1], -1, -1, 2 ** 40, empty[2]]  # names no row at all
    for nq in (1, 17):
        check(ivf, d, metric, xb, xq[:nq], assign, probes[:nq], (1, 10, 40), f"nq={nq}")
    D, I = ivf.search_preassigned(xq[5:6], 3, probes[5:6])
    assert (I == -1).all() and (D == pad_value(metric)).all()
    for i in (0, 5, 9):
        named = np.unique(probes[i][(probes[i] >= 0) & (probes[i] < nlist)])
        t0 = ivf.ivf_stats()["tiles_loaded"]
        ivf.search_preassigned(xq[i:i + 1], 10, probes[i:i + 1])
        assert ivf.ivf_stats()["tiles_loaded"] - t0 == ivf_ref.tiles_of(sizes[named]), i
