"""GPU tests of what the three inverted-list kinds share (csrc/ise_ivf_lists.hpp: IvfCore, ivf_reset; the methods of
``_IndexIVF`` in faiss_compat.py): ``reset`` followed by ``add`` and a ``search_torch`` on another stream, for each kind
against the flat index over the same rows, and the Python surface of ``IndexBinaryIVF``, whose ``add``, ``add_torch``,
``get_list``, ``search``, ``search_preassigned`` and ``search_torch`` are ``_IndexIVF``'s."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import binary_ref, sq_ref
from tests.knn_checks import assert_exact_range, int_data
from tests.sel_ref import L2

pytestmark = pytest.mark.gpu

SQ = faiss.ScalarQuantizer
INT32_MAX = binary_ref.INT32_MAX


def assert_identical(got, want, what):
    """Bit for bit: float32 or int32 D, int64 I."""
    (D, I), (Dw, Iw) = got, want
    assert D.dtype == Dw.dtype and D.dtype.itemsize == 4 and I.dtype == Iw.dtype == np.int64, (what, D.dtype, I.dtype)
    assert D.shape == Dw.shape and I.shape == Iw.shape, (what, D.shape, Dw.shape)
    bad = np.flatnonzero((D.view(np.uint32) != Dw.view(np.uint32)).any(axis=1) | (I != Iw).any(axis=1))
    assert bad.size == 0, f"{what}: query {bad[0]}: D {D[bad[0]][:8]} I {I[bad[0]][:8]}, want D {Dw[bad[0]][:8]} I {Iw[bad[0]][:8]}"


def kind_case(kind: str):
    """-> (index over nlist lists, flat(rows) -> the flat index of the same rows, rows [n], queries [nq]) on data whose
    every distance is exact, so that the two indexes agree bit for bit with every list probed."""
    rng = np.random.default_rng(sorted(kind.encode()))
    nlist, n, nq = 7, 900, 40
    if kind == "binary":
        cs = 9
        C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
        xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
        xq = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
        qz = faiss.IndexBinaryFlat(cs * 8)
        qz.add(C)
        index = faiss.IndexBinaryIVF(qz, cs * 8, nlist)

        def flat(rows):
            f = faiss.IndexBinaryFlat(cs * 8)
            f.add(rows)
            return f
        return index, flat, xb, xq
    d = 24
    t, m, s = sq_ref.integer_trained(rng, d, SQ.QT_8bit)
    xb, _ = sq_ref.integer_rows(rng, n, d, m, s)
    xq = int_data("small", rng, nq, d)
    assert_exact_range(xb, xq)
    qz = faiss.IndexFlatL2(d)
    qz.add(np.ascontiguousarray(xb[rng.choice(n, nlist, replace=False)]))
    if kind == "float":
        index = faiss.IndexIVFFlat(qz, d, nlist, L2)

        def flat(rows):
            f = faiss.IndexFlatL2(d)
            f.add(rows)
            return f
        return index, flat, xb, xq
    index = faiss.IndexIVFScalarQuantizer(qz, d, nlist, SQ.QT_8bit, L2, by_residual=False)
    index.sq.set_trained(t)

    def flat(rows):
        f = faiss.IndexScalarQuantizer(d, SQ.QT_8bit, L2)
        f.sq.set_trained(t)
        f.add(rows)
        return f
    return index, flat, xb, xq


@pytest.mark.parametrize("kind", ["float", "sq", "binary"])
def test_reset_then_add_and_search_on_another_stream(kind):
    """A search on one stream, ``reset`` (it drains the device and forgets the search's end: there is nothing left to
    order a call behind), other rows added, a search on a second stream and one on the default stream, nothing waited
    for in between: every result is the flat index's over the rows added since the reset, whose ids start again at 0."""
    import torch

    index, flat, xb, xq = kind_case(kind)
    assert index.is_trained
    index.nprobe = index.nlist
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    xb_t, xq_t = torch.from_numpy(xb).cuda(), torch.from_numpy(xq).cuda()
    torch.cuda.synchronize()
    index.add_torch(xb_t[:600])
    with torch.cuda.stream(first):
        before = index.search_torch(xq_t, 40)  # two passes a group: the floors and every workspace are in use
    index.reset()
    assert index.ntotal == 0 and [index.list_size(l) for l in range(index.nlist)] == [0] * index.nlist
    with torch.cuda.stream(second):
        empty = index.search_torch(xq_t[:3], 5)
    index.add_torch(xb_t[500:])
    assert index.ntotal == 400
    with torch.cuda.stream(second):
        after = index.search_torch(xq_t, 40)
    again = index.search_torch(xq_t[:17], 3)
    torch.cuda.synchronize()
    host = lambda r: (r[0].cpu().numpy(), r[1].cpu().numpy())
    assert_identical(host(before), flat(xb[:600]).search(xq, 40), f"{kind}: before the reset")
    assert (host(empty)[1] == -1).all()
    want = flat(xb[500:])
    assert_identical(host(after), want.search(xq, 40), f"{kind}: on the second stream after the reset")
    assert_identical(host(again), want.search(xq[:17], 3), f"{kind}: on the default stream after the reset")
    assert_identical(index.search(xq, 40), want.search(xq, 40), f"{kind}: the host form after the reset")


def test_binary_ivf_surface_of_the_shared_methods():
    """dtypes, shapes and refusals of the six methods ``IndexBinaryIVF`` has from ``_IndexIVF``: int32 D, int64 I, uint8
    lists of ``code_size`` bytes a row; a wrong dtype, width, device or probe table is an assertion."""
    import torch

    d, cs, nlist, n = 72, 9, 4, 300
    rng = np.random.default_rng(72)
    C = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (5, cs), dtype=np.uint8)
    qz = faiss.IndexBinaryFlat(d)
    qz.add(C)
    index = faiss.IndexBinaryIVF(qz, d, nlist)
    assert (index.d, index.code_size, index.nlist, index.nprobe, index.device) == (d, cs, nlist, 1, qz.device)
    assert index.quantizer is qz and isinstance(index.cp, faiss.ClusteringParameters) and index.is_trained
    xb_t, xq_t = torch.from_numpy(xb).cuda(), torch.from_numpy(xq).cuda()
    # add, add_torch
    assert index.add(xb[:100]) is None and index.add(xb[:0]) is None and index.ntotal == 100
    assert index.add_torch(xb_t[100:]) is None and index.add_torch(xb_t[:0]) is None and index.ntotal == n
    for bad in (xb.astype(np.float32), xb.astype(np.int8), xb[:, :8], xb[0]):
        with pytest.raises(AssertionError):
            index.add(bad)
    for bad in (xb_t.float(), xb_t[:, :8], xb_t.cpu(), xb_t[0]):
        with pytest.raises(AssertionError):
            index.add_torch(bad)
    assert index.ntotal == n
    # get_list
    assign = qz.search(xb, 1)[1].reshape(-1)
    total = 0
    for l in range(nlist):
        ids, codes = index.get_list(l)
        assert ids.dtype == np.int64 and codes.dtype == np.uint8 and ids.shape == (index.list_size(l),)
        assert codes.shape == (len(ids), cs) and np.array_equal(ids, np.flatnonzero(assign == l)) and np.array_equal(codes, xb[ids])
        total += len(ids)
    assert total == n
    # search, search_preassigned
    index.nprobe = nlist
    want = binary_ref.search(xb, xq, 6)
    probes = np.tile(np.arange(nlist), (5, 1))
    for D, I in (index.search(xq, 6), index.search_preassigned(xq, 6, probes), index.search_preassigned(xq, 6, probes.astype(np.int32))):
        assert D.dtype == np.int32 and I.dtype == np.int64 and D.shape == I.shape == (5, 6)
        assert np.array_equal(D, want[0]) and np.array_equal(I, want[1])
    D, I = index.search_preassigned(xq, 3, np.full((5, 2), -1))  # nothing probed: padding
    assert D.dtype == np.int32 and (D == INT32_MAX).all() and I.dtype == np.int64 and (I == -1).all()
    for D, I in (index.search(xq[:0], 3), index.search_preassigned(xq[:0], 3, np.zeros((0, 1), np.int64))):
        assert D.dtype == np.int32 and I.dtype == np.int64 and D.shape == I.shape == (0, 3)
    for bad in (xq.astype(np.float32), xq.astype(np.int8), xq[:, :8], xq[0]):
        with pytest.raises(AssertionError):
            index.search(bad, 1)
        with pytest.raises(AssertionError):
            index.search_preassigned(bad, 1, probes)
    for bad in (probes[:3], probes[:, :0], probes[0]):
        with pytest.raises(AssertionError):
            index.search_preassigned(xq, 1, bad)
    with pytest.raises(AssertionError):
        index.search_preassigned(xq, 0, probes)
    with pytest.raises(NotImplementedError):
        index.search(xq, 1, params=faiss.SearchParameters())
    # search_torch
    D, I = index.search_torch(xq_t, 6)
    assert D.dtype == torch.int32 and I.dtype == torch.int64 and D.is_cuda and I.is_cuda and D.shape == I.shape == (5, 6)
    assert np.array_equal(D.cpu().numpy(), want[0]) and np.array_equal(I.cpu().numpy(), want[1])
    D, I = index.search_torch(xq_t[:0], 3)
    assert D.dtype == torch.int32 and I.dtype == torch.int64 and D.shape == I.shape == (0, 3)
    for bad in (xq_t.float(), xq_t[:, :8], xq_t.cpu(), xq_t[0]):
        with pytest.raises(AssertionError):
            index.search_torch(bad, 1)
    with pytest.raises(NotImplementedError):
        index.search_torch(xq_t, 1, params=faiss.SearchParameters())
    untrained = faiss.IndexBinaryIVF(faiss.IndexBinaryFlat(d), d, nlist)
    for call in (lambda: untrained.add(xb), lambda: untrained.add_torch(xb_t), lambda: untrained.search(xq, 1),
                 lambda: untrained.search_torch(xq_t, 1)):
        with pytest.raises(RuntimeError, match="before train"):
            call()
