"""The byte shadow rows stored tile-blocked (csrc/ise_byte_layout.hpp).

Every consumer of xq8 -- the builder, the scan, the growth copy, remove_ids and the debug read -- goes through one
address map.  The stored codes are read back row by row (ise_index_byte_row_codes) and compared with the numpy
restatement of byte_rows_kernel, after the first search, after growth with and without a reallocation and after
removals that start and end mid-tile, so a consumer that missed the layout cannot pass; the results keep the bits of
the fp16 and float32 filters on both plans of the byte scan."""
import zlib

import numpy as np
import pytest

from tests import byte_filter_ref as br
from tests.test_byte_filter_gpu import _three
from tests.test_exact_l2_gpu import env_knob, no_direct

pytestmark = pytest.mark.gpu
N0 = 262_144  # the shadows' threshold


@pytest.fixture(scope="module")
def faiss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import image_search_engine_amd.faiss_compat as fc

    return fc


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _rows_to_check(n, *more):
    seeded = _rng("bb", "rows", n).choice(n, 200, replace=False)
    rows = np.concatenate([seeded, np.arange(33), np.arange(n - 33, n)] + [np.asarray(m) for m in more])
    return np.unique(rows[(rows >= 0) & (rows < n)])


def _check_codes(index, xb, rows, zero_until=None):
    """Rows `rows` of the index hold the reference codes of xb's rows; rows [n, zero_until) read zero (default: the
    rest of n's tile)."""
    n, d = xb.shape
    assert index.ntotal == n
    mu = np.asarray(index.get_shift(), np.float32)
    q_ref = br.byte_rows(xb[rows], mu)[0]
    dpb = br.dpb_for(d)
    for i, q in zip(rows, q_ref):
        got = index.byte_row_codes(int(i))
        assert got.shape == (dpb,) and got.dtype == np.int8
        assert np.array_equal(got[:d], q), f"codes of row {i} of {n} x {d} differ"
        assert not got[d:].any(), f"pad columns of row {i} are not zero"
    for i in range(n, max((n + 15) // 16 * 16, zero_until or 0)):
        assert not index.byte_row_codes(i).any(), f"row {i} beyond n = {n} does not read zero"


def _check_results(index, d, tag):
    """nq = 16, k = 10 and nq = 3, k = 1 through the byte route: the bits of both other filters, no exact scan."""
    rng = _rng("bb", "q", tag)
    for nq, k in ((16, 10), (3, 1)):
        xq = rng.random((nq, d), dtype=np.float32)
        with no_direct():
            _, _, exact = _three(index, xq, k, "byte")
        assert exact == [0, 0, 0], ("exact scans (byte, fp16, float32)", tag, nq, k, exact)


def _index(faiss, xb):
    index = faiss.IndexFlatL2(xb.shape[1])
    index.add(xb)
    return index


SHAPES = [(dn, d) for d in (64, 100, 512) for dn in (1, 15, 16, 17)] + [(17, 1000)]


@pytest.mark.parametrize("dn,d", SHAPES)
def test_stored_codes_and_results(faiss, dn, d):
    """1 and 4: dpb 64, 128, 512, 1024 = 1, 2, 8, 16 k-steps; a last tile of 1, 15, 16 and 1 rows."""
    n = N0 + dn
    xb = _rng("bb", "xb", n, d).random((n, d), dtype=np.float32)
    index = _index(faiss, xb)
    index.search(xb[:16], 10)  # the first search builds the shadows
    _check_codes(index, xb, _rows_to_check(n))
    _check_results(index, d, (n, d))
    _check_codes(index, xb, _rows_to_check(n)[::16])  # searching leaves the rows alone


@pytest.mark.parametrize("d", [100, 512])
def test_codes_after_growth(faiss, d):
    """2 (and 4 again): 270 000 rows, then 20 005 more -- a reallocation, and a tile continued mid-way."""
    n1, n2 = 270_000, 290_005
    xb = _rng("bb", "grow", d).random((n2, d), dtype=np.float32)
    index = _index(faiss, xb[:n1])
    index.search(xb[:16], 10)
    edge = np.arange(269_990, 270_021)
    _check_codes(index, xb[:n1], _rows_to_check(n1, edge))
    index.add(xb[n1:])
    index.search(xb[:16], 10)
    _check_codes(index, xb, _rows_to_check(n2, edge))
    _check_results(index, d, ("grow", d))


@pytest.mark.parametrize("d", [100, 512])
def test_codes_after_remove_ids(faiss, d):
    """3 (and 4 again): a run inside a tile; a run over three tiles that starts and ends mid-tile; the last 5 rows
    plus every 1000th row.  The kept rows' codes, in order; the tail reads zero up to the old row count."""
    n = N0 + 17 + 1000  # stays above the shadows' threshold through all three removals
    xb = _rng("bb", "rm", d).random((n, d), dtype=np.float32)
    index = _index(faiss, xb)
    index.search(xb[:16], 10)
    removals = [np.arange(1003, 1009),                                        # inside tile 62
                np.arange(16 * 5000 + 7, 16 * 5002 + 11),                      # three tiles, mid-tile at both ends
                None]                                                          # the last 5 + every 1000th, below
    for r, ids in enumerate(removals):
        n_old = xb.shape[0]
        if ids is None:
            ids = np.unique(np.concatenate([np.arange(n_old - 5, n_old), np.arange(0, n_old, 1000)]))
        assert index.remove_ids(ids.astype(np.int64)) == ids.size
        xb = np.delete(xb, ids, axis=0)
        near = np.concatenate([np.arange(ids[0] - 20, ids[0] + 40), np.arange(ids[-1] - 40, ids[-1] + 20)])
        _check_codes(index, xb, _rows_to_check(xb.shape[0], near), zero_until=n_old)
        _check_results(index, d, ("rm", d, r))


def _depth_counts(index):
    st = index.depth_stats()
    return st["isolated_batches"], st["deep_batches"]


def test_both_plans_same_bits(faiss):
    """5: 300 000 x 512 on one stream (the isolated plan: non-temporal loads) and alternately on two streams (the
    deep plan, the one-request kernel: plain loads): the same bits, and those of the float32 filter."""
    import torch

    n, d, k = 300_000, 512, 10
    xb = _rng("bb", "plans").random((n, d), dtype=np.float32)
    index = _index(faiss, xb)
    xq = _rng("bb", "plans", "q").random((16, d), dtype=np.float32)
    with env_knob("ISE_NO_HALF_FILTER"):
        D_ref, I_ref = index.search(xq, k)
    tq = torch.from_numpy(xq).cuda()
    index.reserve(16, k)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run(order):
        outs, moves = [], []
        for j in order:
            c0 = _depth_counts(index)
            with torch.cuda.stream(streams[j]):
                outs.append(index.search_torch(tq, k))
            c1 = _depth_counts(index)
            moves.append((c1[0] - c0[0], c1[1] - c0[1]))
        torch.cuda.synchronize()
        return [(Do.cpu().numpy(), Io.cpu().numpy()) for Do, Io in outs], moves

    b0 = index.byte_stats()["byte_batches"]
    one, moves = run([0, 0, 0, 0])
    assert moves[1:] == [(1, 0)] * 3, moves  # the first follows a search on another stream
    two, moves = run([1, 0, 1, 0])
    assert moves == [(0, 1)] * 4, moves
    assert index.byte_stats()["byte_batches"] - b0 == 8
    for Do, Io in one + two:
        assert np.array_equal(Io, I_ref), "ids differ between the plans or from the float32 filter"
        assert np.array_equal(Do.view(np.uint32), D_ref.view(np.uint32)), "distances differ"
