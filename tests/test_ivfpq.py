"""CPU tests of IndexIVFPQ's host side (no GPU): the numpy reference against a brute force, the "IwPQ" file layout and
the refusals that need no device."""
import struct

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref, ivfpq_ref, ivfsq_ref, pq_ref
from tests.knn_checks import assert_knn_identical, int_data
from tests.sel_ref import IP, L2


def small_case(seed, M=4, dsub=2, n=300, nq=9, nlist=5):
    rng = np.random.default_rng(seed)
    d = M * dsub
    C = int_data("signed", rng, M * 256, dsub).reshape(M, 256, dsub)
    xb, xq = int_data("signed", rng, n, d), int_data("signed", rng, nq, d)
    assign = rng.integers(0, nlist - 1, n)  # the last list stays empty
    return d, C, xb, xq, assign


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_matches_a_brute_force_over_the_members(metric):
    nlist = 5
    d, C, xb, xq, assign = small_case(11)
    codes = pq_ref.encode(xb, C)
    dec = pq_ref.decode(codes, C)
    probes = np.array([[0, 1], [4, 4], [-1, 2], [nlist, 3], [1, 1], [0, 3], [2, -1], [-1, -1], [3, 0]], np.int64)
    members = ivf_ref.probed_members(probes, assign, nlist)
    assert len(members[1]) == 0 and len(members[7]) == 0  # the empty list, and a row that names nothing
    for k in (1, 7, 40, 200):
        D, I = ivfpq_ref.expected(xq, C, codes, probes, assign, nlist, k, metric)
        assert_knn_identical(D, I, *ivf_ref.expected_brute(dec, xq, members, k, metric), f"k={k}")
        # on integer data the table-lookup sum is the same number
        assert_knn_identical(D, I, *ivfpq_ref.expected_adc(xq, C, codes, probes, assign, nlist, k, metric), f"adc k={k}")
        for q, mem in enumerate(members):
            assert (I[q, len(mem):] == -1).all() and np.isin(I[q, :min(k, len(mem))], mem).all()


def test_stats_reference():
    sizes = [0, 1, 63, 64, 65, 128, 129]  # tiles 0 1 1 1 2 2 3
    # M = 16: QT = 4.  Five queries: one group of four, one of one
    probes = np.array([[1], [2], [2], [-1], [6]])
    assert ivfpq_ref.pass_tile_counts(probes, sizes, 16) == [2, 3]
    assert ivfpq_ref.stats_of(probes, sizes, 16, 33, 5) == {"batches": 1, "passes": 4, "tiles_loaded": 10, "table_builds": 1}
    # M = 64: QT = 2; 130 queries are three chunks of 64, 64 and 2: 65 groups
    probes = np.tile(np.arange(7), (130, 1))
    want = {"batches": 1, "passes": 65, "tiles_loaded": 65 * ivfsq_ref.tiles_of(sizes), "table_builds": 3}
    assert ivfpq_ref.stats_of(probes, sizes, 64, 32, 130) == want
    # M = 4: QT = 16; a group whose queries probe disjoint lists visits their union once
    probes = np.array([[l] for l in (1, 4, 6, 6)])
    assert ivfpq_ref.stats_of(probes, sizes, 4, 1, 4)["tiles_loaded"] == 1 + 2 + 3


# ---------------------------------------------------------------- the file layout
def image_case():
    nlist = 5
    d, C, xb, xq, assign = small_case(12)
    codes = pq_ref.encode(xb, C)
    lists = [(ids, codes[ids]) for ids in ivf_ref.list_members(assign, nlist)]
    cent = np.arange(nlist * d, dtype=np.float32).reshape(nlist, d)
    return d, C, cent, lists, nlist


def test_serialize_parse_round_trip():
    d, C, cent, lists, nlist = image_case()
    buf = faiss.serialize_ivfpq(d, IP, nlist, 3, L2, cent, C, lists)
    assert buf[:4] == b"IwPQ"
    p = faiss.parse_ivfpq(buf)
    assert len(p) == 11
    pd, metric, pnlist, nprobe, qmetric, pcent, M, nbits, pqc, plists, by_residual = p
    assert (pd, metric, pnlist, nprobe, qmetric, M, nbits, by_residual) == (d, IP, nlist, 3, L2, C.shape[0], 8, False)
    assert pcent.dtype == np.float32 and np.array_equal(pcent, cent)
    assert pqc.dtype == np.float32 and pqc.shape == C.shape and np.array_equal(pqc.view(np.uint32), C.view(np.uint32))
    assert len(plists) == nlist
    for (ids, codes), (pids, pcodes) in zip(lists, plists):
        assert pids.dtype == np.int64 and pcodes.dtype == np.uint8 and pcodes.shape == (len(ids), M)
        assert np.array_equal(pids, ids) and np.array_equal(pcodes, codes)
    # the order of the fields behind the quantiser's image and the empty direct map: by_residual, code_size, d, M, nbits
    at = buf.index(b"IxF2") + len(faiss.serialize_flat(d, L2, cent)) + 9
    assert struct.unpack_from("<BQqqq", buf, at) == (0, M, d, M, 8)
    # an untrained quantiser and empty lists
    empty = [(np.zeros(0, np.int64), np.zeros((0, M), np.uint8))] * nlist
    p = faiss.parse_ivfpq(faiss.serialize_ivfpq(d, L2, nlist, 1, L2, np.zeros((0, d), np.float32), C, empty))
    assert p[5].shape == (0, d) and all(len(ids) == 0 for ids, _ in p[9])


def test_damaged_images():
    d, C, cent, lists, nlist = image_case()
    M = C.shape[0]
    buf = faiss.serialize_ivfpq(d, L2, nlist, 3, L2, cent, C, lists)
    for cut in (3, 20, 60, len(buf) // 2, len(buf) - 1):
        with pytest.raises(RuntimeError, match="truncated IndexIVFPQ file"):
            faiss.parse_ivfpq(buf[:cut])
    with pytest.raises(RuntimeError, match="not an IndexIVFPQ"):
        faiss.parse_ivfpq(b"IwSq" + buf[4:])
    at = buf.index(b"IxF2") + len(faiss.serialize_flat(d, L2, cent)) + 9  # by_residual, code_size, d, M, nbits
    four_bits = bytearray(buf)
    struct.pack_into("<q", four_bits, at + 9 + 16, 4)
    with pytest.raises(RuntimeError, match="8-bit"):
        faiss.parse_ivfpq(bytes(four_bits))
    wide = bytearray(buf)
    struct.pack_into("<Q", wide, at + 1, M + 1)
    with pytest.raises(RuntimeError, match="code_size"):
        faiss.parse_ivfpq(bytes(wide))
    residual = bytearray(buf)
    residual[at] = 1
    p = faiss.parse_ivfpq(bytes(residual))  # it parses; reading it into an index raises (tests/test_ivfpq_gpu.py)
    assert p[10] is True and p[6] == M
    assert faiss.parse_ivfpq(faiss.serialize_ivfpq(d, L2, nlist, 3, L2, cent, C, lists, by_residual=True))[10] is True
    short = list(lists)
    short[0] = (short[0][0][:-1], short[0][1][:-1])
    bad = bytearray(faiss.serialize_ivfpq(d, L2, nlist, 3, L2, cent, C, short))
    struct.pack_into("<q", bad, 8, sum(len(ids) for ids, _ in lists))  # ntotal of the header no longer the lists' sum
    with pytest.raises(RuntimeError, match="do not add up"):
        faiss.parse_ivfpq(bytes(bad))


def test_read_index_refuses_a_residual_file_before_the_device(tmp_path):
    d, C, cent, lists, nlist = image_case()
    path = tmp_path / "residual.index"
    path.write_bytes(faiss.serialize_ivfpq(d, L2, nlist, 3, L2, cent, C, lists, by_residual=True))
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.read_index(path)


# ---------------------------------------------------------------- refusals
def test_residual_codes_are_refused_by_name():
    from image_search_engine_amd import utils

    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFPQ()
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFPQ(None, 16, 8, 16, 8)
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFPQ(None, 16, 8, 16, 4)  # before anything else is looked at
    with pytest.raises(NotImplementedError, match="by_residual"):
        faiss.IndexIVFPQ(quantizer=None, d=16, nlist=8, M=16, by_residual=True)
    with pytest.raises(NotImplementedError, match="nbits"):
        faiss.IndexIVFPQ(None, 16, 8, 16, 4, by_residual=False)
    with pytest.raises(NotImplementedError, match="by_residual.*cell-probe-pq"):
        utils.create_search_index(np.zeros((4, 16), np.float32), "cell-probe")


def test_cell_probe_pq_is_a_known_key():
    from image_search_engine_amd import utils

    with pytest.raises(ValueError, match="unknown index_type"):
        utils.create_search_index(np.zeros((4, 16), np.float32), "cell-probe-pqx")
    try:
        utils.create_search_index(np.zeros((4, 16), np.float32), "cell-probe-pq")
    except ValueError as e:  # (without a GPU the quantiser's constructor raises; with one, training needs more rows)
        assert "unknown index_type" not in str(e)
    except Exception:
        pass
