"""Faiss-shaped surface over the gfx950 kNN library.

Exactly the names the reference uses from ``faiss`` on its hot path
(SURVEY.md 8b), so a maintainer can write
``import image_search_engine_amd.faiss_compat as faiss`` in
backend/utils.py:12, backend/engine.py:13, backend/indexer.py:9,
backend/kmeans_faiss.py:1 and backend/siamese/test_index.py:

    IndexFlatL2(d) / IndexFlatIP(d)      backend/utils.py:302,306
    index.add(x) / .ntotal / .d          backend/utils.py:327-328, backend/engine.py:117
    index.search(x, k) -> (D, I)         backend/engine.py:55, backend/kmeans_faiss.py:49
    index.range_search(x, radius)        Faiss's (lims, D, I); not called by the reference (its DHASH
                                         method's "every match" request, backend/engine.py:82-91)
    index.remove_ids(sel or ids) -> int  Faiss IndexFlatCodes::remove_ids with IDSelectorRange / Batch / Array /
                                         Not: the other rows keep their order and are renumbered (in-place
                                         compaction on the device, csrc/ise_remove.hpp); never called by the reference
    IndexIDMap(index).add_with_ids       Faiss's id-mapping wrapper, so that ids handed out earlier survive a removal
    SearchParameters(sel=sel)            ``search`` / ``range_search`` / ``search_torch(..., params=)``: only the rows an
                                         IDSelector names (for IndexIDMap: external ids) -- one masked pass per 16
                                         queries that skips tiles without a selected row (csrc/ise_sel_scan.hpp); never
                                         called by the reference.  ``index.make_selector(sel)`` (extension) keeps the
                                         device bitmap for reuse
    normalize_L2(x)                      backend/utils.py:303, backend/engine.py:53
    write_index / read_index             backend/indexer.py:59, backend/engine.py:116 (IndexFlat and IndexIDMap)
    Kmeans(...).index / .centroids       backend/kmeans_faiss.py:29-44 (assignment only)
    IndexBinaryFlat(d)                   Faiss's exact Hamming index over d-bit codes: ``add`` / ``search`` (int32 D) /
                                         ``range_search`` / ``reconstruct_n`` / ``reset`` (csrc/ise_binary_scan.hpp); the
                                         near-duplicate search the reference's DHASH method (backend/engine.py:82-91)
                                         answers with a dict lookup of bit-identical hashes; never called by the reference
    index.remove_ids / params=           the binary index takes the same ``remove_ids`` arguments and the same
                                         ``SearchParameters(sel=...)`` on ``search`` / ``range_search`` / ``search_torch`` as
                                         the float index: a masked Hamming pass that skips 64-row tiles without a selected
                                         row, an in-place compaction of the code rows (csrc/ise_binary_scan.hpp)
    IndexBinaryIDMap(index)              Faiss's id-mapping wrapper over a binary index: ``add_with_ids``, external ids in
                                         results, selectors and ``remove_ids``
    IndexIVFFlat(quantizer, d, nlist)    Faiss's cell-probe index WITHOUT compression (the "IndexIVFFlat" the comment at
                                         backend/utils.py:312 points to): ``train`` / ``add`` / ``search`` with ``nprobe`` /
                                         ``search_preassigned``; rows scattered into inverted lists on the device, one
                                         pass over the probed lists only (csrc/ise_ivf.hpp); never called by the reference
    IndexPQ(d, M, nbits=8)               Faiss's product-quantised index: rows kept as M code bytes, one of 256 centroids per
                                         sub-vector; ``train`` (one k-means per sub-quantiser) / ``add`` / ``search`` by
                                         lookup tables over the codes (csrc/ise_pq.hpp), ``reconstruct_n``, ``sa_encode`` /
                                         ``sa_decode``, ``index.pq`` (``centroids``, ``set_centroids``, ``compute_codes``,
                                         ``decode``), ``write_index`` / ``read_index`` ("IxPq"); the compression half of
                                         the reference's "cell-probe" index (backend/utils.py:311-325), IndexIVFPQ below
    IndexScalarQuantizer(d, qtype)       Faiss's scalar-quantised index with ``ScalarQuantizer.QT_8bit`` / ``QT_8bit_uniform``:
                                         rows kept as one byte per entry (a quarter of float32) between a trained
                                         per-dimension (or single) minimum and maximum; ``train`` (min / max) / ``add`` /
                                         ``search`` by a byte-row scan on the matrix cores (csrc/ise_sq.hpp),
                                         ``reconstruct_n``, ``sa_encode`` / ``sa_decode``, ``index.sq`` (``trained``,
                                         ``set_trained``, ``compute_codes``, ``decode``), ``write_index`` / ``read_index``
                                         ("IxSQ"); the other quantiser types raise; never called by the reference
    IndexIVFScalarQuantizer(quantizer, d, nlist, qtype, metric, by_residual=False)
                                         Faiss's cell-probe index over scalar-quantised rows: ``IndexIVFFlat``'s lists holding
                                         ``IndexScalarQuantizer``'s bytes (the same codec for the same ``sq.trained``);
                                         ``train`` (k-means, then min / max) / ``add`` / ``search`` with ``nprobe`` /
                                         ``search_preassigned`` / ``search_torch``, ``get_list``, ``index.sq``,
                                         ``write_index`` / ``read_index`` ("IwSq"); a pass reads the 64-row tiles of the
                                         probed lists only (csrc/ise_ivfsq.hpp) and D has ``IndexScalarQuantizer``'s bits;
                                         ``by_residual=True`` (Faiss's default) raises
    IndexIVFPQ(quantizer, d, nlist, M, nbits=8, metric, by_residual=False)
                                         the reference's "cell-probe" index (backend/utils.py:311-325) over codes of the rows
                                         themselves: ``IndexIVFFlat``'s lists holding ``IndexPQ``'s code rows (the same codec
                                         for the same ``pq.centroids``); ``train`` (k-means, then the codebook) / ``add`` /
                                         ``search`` with ``nprobe`` / ``search_preassigned`` / ``search_torch``, ``get_list``,
                                         ``index.pq``, ``sa_encode`` / ``sa_decode``, ``write_index`` / ``read_index``
                                         ("IwPQ"); a pass gathers from the queries' lookup tables over the 64-row tiles of
                                         the probed lists only (csrc/ise_ivfpq.hpp) and D has ``IndexPQ``'s bits;
                                         ``by_residual=True`` (Faiss's default, and the reference's call) raises
    IndexRefineFlat(base_index)          Faiss's exact re-ranking of an approximate index: ``search`` asks ``base_index`` (an
                                         ``IndexPQ``, an ``IndexScalarQuantizer``, an ``IndexIVFFlat``, an
                                         ``IndexIVFScalarQuantizer``, an ``IndexIVFPQ`` or an ``IndexFlat`` of
                                         either storage) for
                                         ``k * k_factor`` labels and returns the k best of them by their exact distance to
                                         float32 rows kept beside it (csrc/ise_subset.hpp: a gather-and-score pass spread
                                         over the device, then one sort per query); ``IndexRefine(base, refine_index)``,
                                         ``IndexRefineSearchParameters(k_factor=, base_index_params=)``,
                                         ``IndexFlat.search_subset`` / ``compute_distance_subset`` (the pass on its own),
                                         ``write_index`` / ``read_index`` ("IxRF"); never called by the reference
    write_index_binary / read_index_binary   Faiss's names for IndexBinaryFlat ("IBxF"), IndexBinaryIDMap ("IBMp") and
                                         IndexBinaryIVF ("IBwF") files
    IndexBinaryIVF(quantizer, d, nlist)  Faiss's cell-probe index over bit codes: an ``IndexBinaryFlat`` of ``nlist`` centroid
                                         codes in front of inverted lists of ``d``-bit codes; ``train`` (k-means on the
                                         bits as +-1, binarised) / ``add`` / ``search`` with ``nprobe`` /
                                         ``search_preassigned`` / ``search_torch``, ``get_list``; a Hamming pass reads the
                                         64-row tiles of the probed lists only (csrc/ise_binary_ivf.hpp), and with
                                         ``nprobe == nlist`` the result is ``IndexBinaryFlat.search``'s bit for bit; what
                                         near-duplicate search by hash (backend/engine.py:82-91) needs once one
                                         brute-force pass over the collection is too much; never called by the reference
    IndexPreTransform(ltrans, index)     Faiss's transform chain in front of any index kind here: ``PCAMatrix`` (mean,
                                         float64 covariance, ``eigen_power`` for whitening), ``OPQMatrix`` (the
                                         non-parametric OPQ rotation for an ``IndexPQ``), ``RandomRotationMatrix``,
                                         ``LinearTransform`` (``A``, ``b``), ``NormalizationTransform``,
                                         ``CenteringTransform``; ``train`` / ``add`` / ``search`` / ``search_torch`` /
                                         ``reconstruct`` / ``apply_chain``, ``SearchParametersPreTransform``,
                                         ``write_index`` / ``read_index`` ("IxPT"); y = A x + b is a HIP kernel whose bits
                                         depend on ``d_in`` alone (csrc/ise_linear.hpp), so a stored row sent as a query is
                                         at distance 0; ``IndexRefineFlat`` takes one as its base; never called by the
                                         reference

All arithmetic runs on the MI355X through ``include/ise_knn.h``; there is no
CPU path here.  Without the HIP library or without a GPU the constructors and
``normalize_L2`` raise.
"""
from __future__ import annotations

import ctypes
import struct
import threading
from collections import namedtuple

import numpy as np

from . import _native as _n

METRIC_INNER_PRODUCT = _n.METRIC_INNER_PRODUCT
METRIC_L2 = _n.METRIC_L2

_FLT_MAX = float(np.finfo(np.float32).max)


def _as_rows(x, d=None) -> np.ndarray:
    """Coerce like the Faiss SWIG wrapper: C-contiguous float32 (n, d).
    ``np.matrix`` (what ``.todense()`` yields, backend/engine.py:96) is accepted."""
    x = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
    assert x.ndim == 2, "expected a 2-D array"
    if d is not None:
        assert x.shape[1] == d, f"dimension mismatch: got {x.shape[1]}, index has d={d}"
    return x


def _default_device() -> int:
    import torch

    return torch.cuda.current_device() if torch.cuda.is_available() else 0


# ---------------------------------------------------------------- what the index kinds share
class _AbiFamily:
    """An object behind one family of entry points of include/ise_knn.h: ``_ABI`` is the family's prefix, ``_fn(name)``
    looks ``<prefix>_<name>`` up.  For removal, statistics, selector and range paths; the search paths name their entry
    point outright (no string lookup per call)."""

    _ABI = ""

    def _fn(self, name: str):
        return getattr(_n.lib, f"{self._ABI}_{name}")


class _IndexHandle(_AbiFamily):
    """The lifetime of an index's library handle ``_h``."""

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._fn("destroy")(h)
            except Exception:  # interpreter shutdown: module globals may already be gone
                pass
            h.value = None


def _counters(fn, h, keys: tuple) -> dict:
    """``len(keys)`` uint64 counters from the statistics entry point ``fn(handle, out)``, by name."""
    out = (ctypes.c_uint64 * len(keys))()
    _n.check(fn(h, out))
    return {key: int(v) for key, v in zip(keys, out)}


def _ntotal_property(info, nargs: int, pos: int) -> property:
    """``ntotal`` over a family's ``*_info`` entry point: ``nargs`` arguments, the handle first, the ``pos``-th (from 0)
    the ``int64_t*`` that receives the row count; the others are passed as NULL."""
    before, after = (None,) * (pos - 1), (None,) * (nargs - pos - 1)

    def ntotal(self) -> int:
        n = ctypes.c_int64(0)
        _n.check(info(self._h, *before, ctypes.byref(n), *after))
        return int(n.value)

    return property(ntotal)


def _read_range_result(res, d_dtype, get, destroy):
    """A ``*_range_result`` handle -> (lims uint64 (nq + 1,), D ``d_dtype``, I int64) as fresh arrays; the handle is
    destroyed, also when reading it fails."""
    try:
        n = ctypes.c_int64()
        lp, dp_, ip = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _n.check(get(res, ctypes.byref(n), ctypes.byref(lp), ctypes.byref(dp_), ctypes.byref(ip)))
        lims = np.ctypeslib.as_array(ctypes.cast(lp, ctypes.POINTER(ctypes.c_int64)), (n.value + 1,))
        lims = lims.astype(np.uint64)
        total = int(lims[-1])
        D = np.empty(total, dtype=d_dtype)
        I = np.empty(total, dtype=np.int64)
        if total:
            ctypes.memmove(D.ctypes.data, dp_.value, D.nbytes)
            ctypes.memmove(I.ctypes.data, ip.value, I.nbytes)
    finally:
        destroy(res)
    return lims, D, I


def _torch_io(x, dtype, width: int, k: int, d_dtype):
    """The check-and-allocate step of the torch paths: ``x`` is a CUDA (n, width) tensor of ``dtype`` -> (x contiguous,
    D ``d_dtype`` (n, k), I int64 (n, k), the handle of x's device's current stream); D and I are uninitialised."""
    import torch

    assert x.is_cuda and x.dtype == dtype and x.dim() == 2 and x.shape[1] == width
    x = x.contiguous()
    D = torch.empty((x.shape[0], k), dtype=d_dtype, device=x.device)
    I = torch.empty((x.shape[0], k), dtype=torch.int64, device=x.device)
    return x, D, I, torch.cuda.current_stream(x.device).cuda_stream


# ---------------------------------------------------------------- id selectors (faiss.IDSelector*)
def _ids_array(ids) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)


def _runs_of_sorted(ids: np.ndarray) -> np.ndarray:
    """Sorted unique ids -> (T, 2) int64 runs (start, len), maximal (no two runs adjacent)."""
    if ids.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    brk = np.flatnonzero(np.diff(ids) != 1) + 1
    starts = np.concatenate(([0], brk))
    ends = np.concatenate((brk, [ids.size]))
    return np.stack([ids[starts], ends - starts], axis=1).astype(np.int64)


class IDSelector:
    """What ``remove_ids`` takes: ``is_member(i)``; ``runs(n)`` -- the selected ids inside [0, n) as sorted, disjoint,
    non-adjacent (start, len) runs, (T, 2) int64; ``members(ids)`` -- ``is_member`` over an int64 array."""

    def is_member(self, i: int) -> bool:
        raise NotImplementedError

    def runs(self, n: int) -> np.ndarray:
        raise NotImplementedError

    def members(self, ids) -> np.ndarray:
        return np.fromiter((self.is_member(int(i)) for i in _ids_array(ids)), dtype=bool, count=len(_ids_array(ids)))


class IDSelectorRange(IDSelector):
    """ids in [imin, imax); never materialised."""

    def __init__(self, imin: int, imax: int):
        self.imin, self.imax = int(imin), int(imax)

    def is_member(self, i: int) -> bool:
        return self.imin <= int(i) < self.imax

    def runs(self, n: int) -> np.ndarray:
        a, b = max(self.imin, 0), min(self.imax, int(n))
        return np.array([[a, b - a]], dtype=np.int64) if a < b else np.zeros((0, 2), dtype=np.int64)

    def members(self, ids) -> np.ndarray:
        ids = _ids_array(ids)
        return (ids >= self.imin) & (ids < self.imax)


class IDSelectorBatch(IDSelector):
    """The given ids, in any order, duplicates allowed; ids that name no row select nothing."""

    def __init__(self, ids):
        self.ids = np.unique(_ids_array(ids))  # sorted

    def is_member(self, i: int) -> bool:
        p = int(np.searchsorted(self.ids, int(i)))
        return p < self.ids.size and int(self.ids[p]) == int(i)

    def runs(self, n: int) -> np.ndarray:
        return _runs_of_sorted(self.ids[(self.ids >= 0) & (self.ids < int(n))])

    def members(self, ids) -> np.ndarray:
        return np.isin(_ids_array(ids), self.ids)


class IDSelectorArray(IDSelectorBatch):
    """Faiss's linear-scan form of IDSelectorBatch: the same members."""


class IDSelectorNot(IDSelector):
    """Every id ``sel`` does not select."""

    def __init__(self, sel: IDSelector):
        self.sel = sel

    def is_member(self, i: int) -> bool:
        return not self.sel.is_member(i)

    def runs(self, n: int) -> np.ndarray:
        n = int(n)
        r = self.sel.runs(n)
        starts = np.concatenate(([0], r[:, 0] + r[:, 1]))
        ends = np.concatenate((r[:, 0], [n]))
        keep = ends > starts
        return np.stack([starts[keep], (ends - starts)[keep]], axis=1).astype(np.int64)

    def members(self, ids) -> np.ndarray:
        return ~self.sel.members(ids)


class SearchParameters:
    """faiss.SearchParameters: ``sel`` is an ``IDSelector`` (or a ``DeviceSelector`` made by ``IndexFlat.make_selector``
    / a ``BinaryDeviceSelector`` made by ``IndexBinaryFlat.make_selector``, extensions), or None for an unfiltered
    search."""

    def __init__(self, sel=None):
        if sel is not None and not isinstance(sel, (IDSelector, DeviceSelector)):
            raise TypeError(f"SearchParameters.sel must be an IDSelector or a DeviceSelector, not {type(sel).__name__}")
        self.sel = sel


def _params_sel(params):
    """The selector of a ``params=`` argument, or None for today's unfiltered path."""
    if params is None:
        return None
    if not isinstance(params, SearchParameters):
        raise TypeError(f"params must be a SearchParameters, not {type(params).__name__}")
    return params.sel


class IndexRefineSearchParameters(SearchParameters):
    """faiss.IndexRefineSearchParameters: ``k_factor`` replaces the index's own for one ``IndexRefine.search`` call,
    ``base_index_params`` goes to the base index's ``search``."""

    def __init__(self, k_factor: float = 1.0, base_index_params=None):
        super().__init__()
        if not float(k_factor) >= 1.0:
            raise ValueError(f"k_factor must be >= 1, got {k_factor!r}")
        self.k_factor = float(k_factor)
        self.base_index_params = base_index_params


def _bitmap_words(members: np.ndarray) -> np.ndarray:
    """bool (n,) -> uint32 words, bit ``r & 31`` of word ``r >> 5``, ceil(n / 32) of them."""
    members = np.asarray(members, dtype=bool).reshape(-1)
    nw = (members.size + 31) // 32
    by = np.zeros(4 * nw, dtype=np.uint8)
    packed = np.packbits(members, bitorder="little")
    by[:packed.size] = packed
    return by.view("<u4")


def lower_selector(sel: IDSelector, ntotal: int):
    """How a selector reaches the device (include/ise_knn.h): ``("range", imin, imax)``, ``("ids", ids, invert)`` -- the
    ids travel, not a bitmap -- or ``("bitmap", words)`` for everything else."""
    if isinstance(sel, IDSelectorRange):
        return ("range", sel.imin, sel.imax)
    if isinstance(sel, IDSelectorBatch):
        return ("ids", sel.ids, 0)
    if isinstance(sel, IDSelectorNot) and isinstance(sel.sel, IDSelectorBatch):
        return ("ids", sel.sel.ids, 1)
    if not isinstance(sel, IDSelector):
        raise TypeError(f"expected an IDSelector, not {type(sel).__name__}")
    return ("bitmap", _bitmap_words(sel.members(np.arange(int(ntotal), dtype=np.int64))))


class DeviceSelector(_AbiFamily):
    """A selector on an index's device (``IndexFlat.make_selector``; an extension, Faiss has no counterpart): the
    bitmap, its row window and counts.  Valid while the index keeps its rows: after ``add``, ``remove_ids`` or
    ``reset`` a search with it raises ``IseError``."""

    _ABI = "ise_selector"  # "tiles" of ``info`` are 16-row tiles

    def __init__(self, index, lowered):
        self.index = index
        self._s = ctypes.c_void_p()
        kind = lowered[0]
        if kind == "range":
            _n.check(self._fn("create_range")(index._h, int(lowered[1]), int(lowered[2]), ctypes.byref(self._s)))
        elif kind == "ids":
            ids = _ids_array(lowered[1])
            _n.check(self._fn("create_ids")(index._h, ids.ctypes.data, ids.size, int(lowered[2]), ctypes.byref(self._s)))
        else:
            words = np.ascontiguousarray(lowered[1], dtype="<u4")
            _n.check(self._fn("create_bitmap")(index._h, words.ctypes.data, words.size, ctypes.byref(self._s)))

    def close(self) -> None:
        s = getattr(self, "_s", None)
        if s is not None and s.value:
            try:
                self._fn("destroy")(s)
            except Exception:  # interpreter shutdown
                pass
            s.value = None

    __del__ = close

    def info(self) -> dict:
        out = (ctypes.c_int64 * 5)()
        _n.check(self._fn("info")(self._s, out))
        return {"ntotal": int(out[0]), "selected": int(out[1]), "window": (int(out[2]), int(out[3])),
                "tiles": int(out[4])}


class BinaryDeviceSelector(DeviceSelector):
    """``IndexBinaryFlat.make_selector``: the same object over a binary index (ise_binary_selector_*); "tiles" of
    ``info`` are the non-empty 64-row tiles, the unit the masked Hamming pass skips.  It serves the binary index it
    was made from only; a float index refuses it, and a binary index refuses a float index's ``DeviceSelector``."""

    _ABI = "ise_binary_selector"


def _runs_to_ids(runs: np.ndarray) -> np.ndarray:
    if len(runs) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(a, a + m, dtype=np.int64) for a, m in runs])


class _RemovableIndex(_IndexHandle):
    """What ``IndexFlat`` and ``IndexBinaryFlat`` share above their handles: ``reset``, ``remove_ids`` and the selector
    plumbing of ``params=``.  A subclass names its family of entry points (``_ABI``), the class of its device selectors
    (``_SELECTOR``) and what it says to a selector of another family (``_FOREIGN_SELECTOR``)."""

    _SELECTOR = DeviceSelector
    _FOREIGN_SELECTOR = ""

    def reset(self) -> None:
        _n.check(self._fn("reset")(self._h))

    def remove_ids(self, sel) -> int:
        """faiss ``index.remove_ids``: remove the rows an ``IDSelector`` names -- or an int64 array-like, taken as an
        ``IDSelectorBatch`` as the Faiss wrapper does -- and return how many went.  The other rows keep their order
        and are renumbered densely (``IndexIDMap`` / ``IndexBinaryIDMap`` keep external ids).  In place on the device:
        the rows and what is kept beside them (a float index's norms and shadows) move, nothing is re-uploaded
        (include/ise_knn.h, ise_index_remove_ids_host / ise_binary_index_remove_ids_host)."""
        out = ctypes.c_int64(0)
        if isinstance(sel, IDSelectorRange):
            _n.check(self._fn("remove_range")(self._h, sel.imin, sel.imax, ctypes.byref(out)))
            return int(out.value)
        if isinstance(sel, IDSelectorBatch):
            ids = sel.ids
        elif isinstance(sel, IDSelector):  # Not, or a user's selector: complemented / evaluated against ntotal here
            ids = _runs_to_ids(sel.runs(self.ntotal))
        else:
            ids = _ids_array(sel)
        if ids.size:
            _n.check(self._fn("remove_ids_host")(self._h, ids.ctypes.data, ids.size, ctypes.byref(out)))
        return int(out.value)

    def remove_stats(self) -> dict:
        """Removals since the index was created (include/ise_knn.h, ise_index_remove_stats /
        ise_binary_index_remove_stats): calls that removed something, rows removed, rows that moved to a new
        position."""
        return _counters(self._fn("remove_stats"), self._h, ("remove_calls", "rows_removed", "rows_moved"))

    # -- selector-filtered search (faiss.SearchParameters(sel=...))
    def make_selector(self, sel) -> DeviceSelector:
        """Extension (not in Faiss): ``sel`` lowered to a device object that can be reused across ``search``,
        ``range_search`` and ``search_torch`` calls through ``SearchParameters(sel=...)`` until the index changes."""
        return self._SELECTOR(self, lower_selector(sel, self.ntotal))

    def _with_selector(self, sel, fn):
        """``fn(handle)`` with the device selector of ``sel``; one built here is destroyed before returning.  A device
        selector of another family of entry points is refused by its type, before any handle is touched."""
        if isinstance(sel, DeviceSelector):
            if sel._ABI != self._SELECTOR._ABI:
                raise TypeError(self._FOREIGN_SELECTOR)
            return fn(sel._s)
        ds = self.make_selector(sel)
        try:
            return fn(ds._s)
        finally:
            ds.close()

    def sel_stats(self) -> dict:
        """Filtered search batches, masked passes launched (a binary index: one per 16 queries and per 32 results),
        filtered range batches (include/ise_knn.h, ise_index_sel_stats / ise_binary_index_sel_stats)."""
        return _counters(self._fn("sel_stats"), self._h, ("sel_batches", "sel_passes", "sel_range_batches"))


class IndexFlat(_RemovableIndex):
    """Exhaustive-search index owning a device copy of its rows.

    Mirrors faiss.IndexFlat as the reference touches it: ``d``, ``ntotal``,
    ``is_trained``, ``metric_type``, ``add``, ``search``, ``reset``,
    ``reconstruct_n``.  Thread-safe for concurrent ``search`` callers (Flask
    request threads, backend/engine.py:137; joblib threads,
    backend/descriptors.py:125); the GIL is released while the device works.
    """

    _ABI = "ise_index"
    _FOREIGN_SELECTOR = "a binary index's selector cannot filter a float index"

    def __init__(self, d: int, metric: int = METRIC_L2, device: int | None = None, storage: str = "f32"):
        """``storage="bf16"`` (extension, not a Faiss IndexFlat feature) keeps rows as bf16 and
        rounds queries to bf16 too: approximate results at half the HBM traffic (BASELINE config 5)."""
        self.d = int(d)
        self.metric_type = int(metric)
        self.is_trained = True
        self.storage = storage
        self.device = _default_device() if device is None else int(device)
        self._h = ctypes.c_void_p()
        self._lock = threading.Lock()
        store = {"f32": _n.STORE_F32, "bf16": _n.STORE_BF16}[storage]
        _n.check(_n.lib.ise_index_create_ex(ctypes.byref(self._h), self.d, self.metric_type, self.device, store))

    ntotal = _ntotal_property(_n.lib.ise_index_info, 5, 3)

    def exact_stats(self) -> dict:
        """Counters of the exact float32 L2 path (include/ise_knn.h, ise_index_stats): queries
        re-ranked, queries the certificate sent to the exact direct-difference scan, refreshes of the
        shift vector."""
        return _counters(_n.lib.ise_index_stats, self._h, ("reranked", "exact_scan", "shift_updates", "gemm_chunks"))

    def gemm_stats(self) -> dict:
        """The large-batch path (include/ise_knn.h, ise_index_gemm_stats): query chunks that took it, and queries of
        the flavours without a re-rank (float32 inner product, bf16 rows) whose candidates it left incomplete, so that
        the streaming passes rewrote their chunk."""
        return _counters(_n.lib.ise_index_gemm_stats, self._h, ("gemm_chunks", "gemm_lost_queries"))

    def host_stats(self) -> dict:
        """Combining of concurrent ``search`` calls (include/ise_knn.h, ise_index_host_stats): how many
        shared batches ran and how many calls they served; and how many queries the direct small-batch
        scan answered (float32 L2, at most 4 queries, k <= 32)."""
        return _counters(_n.lib.ise_index_host_stats, self._h, ("combined_batches", "combined_calls", "direct_queries"))

    def short_stats(self) -> dict:
        """Batches scanned by the short-index kernel (include/ise_knn.h, ise_index_short_stats)."""
        return _counters(_n.lib.ise_index_short_stats, self._h, ("short_batches",))

    def half_stats(self) -> dict:
        """Batches whose filter read shadow rows, fp16 or byte (include/ise_knn.h, ise_index_half_stats)."""
        return _counters(_n.lib.ise_index_half_stats, self._h, ("half_batches",))

    def byte_stats(self) -> dict:
        """Batches whose filter read the byte shadow rows, and whether the index's byte route is open (include/ise_knn.h,
        ise_index_byte_stats)."""
        c = _counters(_n.lib.ise_index_byte_stats, self._h, ("byte_batches", "byte_route"))
        c["byte_route"] = bool(c["byte_route"])
        return c

    def depth_stats(self) -> dict:
        """Byte-shadow batches scanned with the isolated plan and with a deep one (include/ise_knn.h,
        ise_index_depth_stats)."""
        return _counters(_n.lib.ise_index_depth_stats, self._h, ("isolated_batches", "deep_batches"))

    def byte_row(self, i: int) -> tuple:
        """(c_r, e_r) of byte shadow row i (include/ise_knn.h, ise_index_byte_row)."""
        out = (ctypes.c_float * 2)()
        _n.check(_n.lib.ise_index_byte_row(self._h, int(i), out))
        return float(out[0]), float(out[1])

    def byte_row_codes(self, i: int):
        """The int8 codes of byte shadow row i in column order, its dpb padded columns (include/ise_knn.h,
        ise_index_byte_row_codes)."""
        steps = (self.d + 63) // 64  # dpb as the library pads it: whole 64-byte k-steps, in fours beyond four
        out = np.zeros((steps if steps <= 4 else (steps + 3) // 4 * 4) * 64, dtype=np.int8)
        _n.check(_n.lib.ise_index_byte_row_codes(self._h, int(i), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def shadow_row(self, i: int) -> tuple:
        """(|u~|^2, e_r, s_r) of shadow row i (include/ise_knn.h, ise_index_shadow_row)."""
        out = (ctypes.c_float * 3)()
        _n.check(_n.lib.ise_index_shadow_row(self._h, int(i), out))
        return float(out[0]), float(out[1]), int(out[2])

    def stage_query_debug(self, q: "torch.Tensor", route: str) -> dict:
        """One float32 device query through the staging of the "half" or "byte" shadow filter, on its own (tests only;
        include/ise_knn.h, ise_index_stage_query_debug): hi / lo limbs of the padded row (int8, or fp16), sh, |v|^2,
        e_q and whether the vector path ran.  The tensor's own pointer is used, so a slice keeps its alignment."""
        import torch
        assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 1 and q.is_contiguous() and q.numel() == self.d
        es = {"half": 2, "byte": 1}[route]
        buf = np.zeros(2 * 1024 * es, dtype=np.uint8)
        out, info = (ctypes.c_float * 2)(), (ctypes.c_int32 * 3)()
        torch.cuda.synchronize()
        _n.check(_n.lib.ise_index_stage_query_debug(self._h, q.data_ptr(), es == 1, buf.ctypes.data, buf.nbytes, out, info))
        P = int(info[2])
        limbs = buf[: 2 * P * es].view(np.int8 if es == 1 else np.float16).reshape(2, P)
        return {"hi": limbs[0].copy(), "lo": limbs[1].copy(), "sh": int(info[0]), "vec": bool(info[1]),
                "vn2": float(out[0]), "eq": float(out[1])}

    def range_stats(self) -> dict:
        """Range-search batches and those that needed the overflow pass (include/ise_knn.h, ise_index_range_stats)."""
        return _counters(_n.lib.ise_index_range_stats, self._h, ("range_batches", "range_overflow_batches"))

    def reserve(self, nq: int, k: int) -> None:
        """Size every internal workspace for batches of ``nq`` queries / ``k`` results now, so that the
        first search of that shape allocates nothing (serving loops, bench.py)."""
        _n.check(_n.lib.ise_index_reserve_workspaces(self._h, int(nq), int(k)))

    # float32 L2 indexes filter around a shift vector (see include/ise_knn.h); search results do not
    # depend on it.  The k = 1 assignment kernel (assign_torch, search with nq >= ASSIGN_MIN_NQ) scores in
    # the expanded form around it, so there its rounding can reorder near-ties and even exact ties between
    # distinct centroids (tests/test_tie_order_gpu.py::test_assignment_kernel_tie_order)
    def get_shift(self) -> np.ndarray:
        mu = np.zeros(self.d, dtype=np.float32)
        _n.check(_n.lib.ise_index_get_shift(self._h, mu.ctypes.data))
        return mu

    def set_shift(self, mu) -> None:
        mu = np.ascontiguousarray(mu, dtype=np.float32)
        assert mu.shape == (self.d,)
        _n.check(_n.lib.ise_index_set_shift(self._h, mu.ctypes.data))

    # -- build side
    def add(self, x) -> None:
        """Append rows (copied; the caller may mutate or free ``x`` afterwards)."""
        x = _as_rows(x, self.d)
        _n.check(_n.lib.ise_index_add_host(self._h, x.ctypes.data, x.shape[0]))

    def add_torch(self, x) -> None:
        """Append rows from a CUDA float32 tensor on this index's device (no host hop)."""
        import torch

        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.d
        x = x.contiguous()
        st = torch.cuda.current_stream(x.device).cuda_stream
        with self._lock:
            _n.check(_n.lib.ise_index_add_device(self._h, x.data_ptr(), x.shape[0], st))
        torch.cuda.current_stream(x.device).synchronize()  # x may be freed by the caller

    def remove_last_timing(self) -> tuple:
        """(milliseconds, bytes) of the last removal's slab launches (include/ise_knn.h, ise_index_remove_last_timing)."""
        ms, nb = ctypes.c_float(0), ctypes.c_uint64(0)
        _n.check(_n.lib.ise_index_remove_last_timing(self._h, ctypes.byref(ms), ctypes.byref(nb)))
        return float(ms.value), int(nb.value)

    def reconstruct_n(self, i0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.ntotal - i0 if n is None else n
        out = np.empty((n, self.d), dtype=np.float32)
        _n.check(_n.lib.ise_index_reconstruct_host(self._h, int(i0), int(n), out.ctypes.data))
        return out

    @staticmethod
    def _from_parts(parts, device):
        """The index a parsed "IxF2" / "IxFI" image describes (``parse_flat``)."""
        index = IndexFlat(parts.d, parts.metric, device)
        if parts.xb.shape[0]:
            index.add(parts.xb)
        return index

    # -- query side
    ASSIGN_MIN_NQ = 2048  # k = 1 searches with at least this many rows use the assignment kernel

    def _assign_applies(self, nq: int, k: int) -> bool:
        return (k == 1 and nq >= self.ASSIGN_MIN_NQ and self.storage == "f32" and self.d <= 512
                and 0 < self.ntotal <= 65536)

    def assign_torch(self, x):
        """Nearest index row of every row of ``x`` (CUDA float32 (n, d)): the k = 1 search of
        FaissKMeans.transform (backend/kmeans_faiss.py:49) as one MFMA-bound kernel.
        Returns CUDA (D float32 (n, 1), I int64 (n, 1))."""
        import torch

        x, D, I, st = _torch_io(x, torch.float32, self.d, 1, torch.float32)
        _n.check(_n.lib.ise_index_assign_device(self._h, x.data_ptr(), x.shape[0], D.data_ptr(), I.data_ptr(), st))
        return D, I

    def search(self, x, k: int, params=None):
        """(D float32 (nq,k), I int64 (nq,k)), fresh arrays.  L2: squared distance
        ascending; IP: descending; unfilled slots -1 / +-FLT_MAX.  ``params=SearchParameters(sel=...)``: among the
        rows the selector names only."""
        x = _as_rows(x, self.d)
        k = int(k)
        assert k > 0
        nq = x.shape[0]
        sel = _params_sel(params)
        if sel is not None:
            D = np.empty((nq, k), dtype=np.float32)
            I = np.empty((nq, k), dtype=np.int64)
            self._with_selector(sel, lambda s: _n.check(_n.lib.ise_index_search_sel_host(
                self._h, x.ctypes.data, nq, k, s, D.ctypes.data, I.ctypes.data)))
            return D, I
        if self._assign_applies(nq, k):
            import torch

            D = np.empty((nq, 1), dtype=np.float32)
            I = np.empty((nq, 1), dtype=np.int64)
            dev = torch.device("cuda", self.device)
            step = max(1, (1 << 28) // (4 * self.d))  # 256 MiB of rows per upload
            for i0 in range(0, nq, step):
                d_, i_ = self.assign_torch(torch.from_numpy(x[i0:i0 + step]).to(dev))
                D[i0:i0 + step] = d_.cpu().numpy()
                I[i0:i0 + step] = i_.cpu().numpy()
            return D, I
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        _n.check(_n.lib.ise_index_search_host(self._h, x.ctypes.data, nq, k, D.ctypes.data, I.ctypes.data))
        return D, I

    def range_search(self, x, radius: float, params=None):
        """(lims uint64 (nq+1,), D float32, I int64), fresh arrays, as Faiss returns them: query i's rows are
        ``I[lims[i]:lims[i+1]]`` in ascending id order, every row with D < radius (L2) or D > radius (inner
        product), D as ``search`` reports it.  ``params=SearchParameters(sel=...)``: among the selected rows only."""
        x = _as_rows(x, self.d)
        nq = x.shape[0]
        res = ctypes.c_void_p()
        sel = _params_sel(params)
        if sel is not None:
            self._with_selector(sel, lambda s: _n.check(_n.lib.ise_index_range_search_sel_host(
                self._h, x.ctypes.data, nq, ctypes.c_float(float(radius)), s, ctypes.byref(res))))
        else:
            _n.check(_n.lib.ise_index_range_search_host(self._h, x.ctypes.data, nq, ctypes.c_float(float(radius)),
                                                        ctypes.byref(res)))
        return _read_range_result(res, np.float32, _n.lib.ise_range_result_get, _n.lib.ise_range_result_destroy)

    def search_torch(self, xq, k: int, params=None):
        """Device-resident search: CUDA float32 (nq,d) in, CUDA (D, I) out, enqueued on
        the current torch stream (no host synchronisation).  ``params=SearchParameters(sel=...)`` as ``search``; a
        selector that is not a ``DeviceSelector`` is built and destroyed here, which waits for the device."""
        import torch

        # written out, not through _torch_io, here and in search_keys_torch: a latency path (host call
        # overhead) keeps its number of Python-level calls
        assert xq.is_cuda and xq.dtype == torch.float32 and xq.dim() == 2 and xq.shape[1] == self.d
        xq = xq.contiguous()
        nq = xq.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        st = torch.cuda.current_stream(xq.device).cuda_stream
        sel = _params_sel(params)
        if sel is not None:
            def run(s):
                with self._lock:
                    _n.check(_n.lib.ise_index_search_sel_device(self._h, xq.data_ptr(), nq, int(k), s, D.data_ptr(),
                                                                I.data_ptr(), st))
            self._with_selector(sel, run)
            return D, I
        with self._lock:
            _n.check(_n.lib.ise_index_search_device(self._h, xq.data_ptr(), nq, int(k), D.data_ptr(),
                                                    I.data_ptr(), st))
        return D, I

    # -- subset scoring (include/ise_knn.h, ise_index_search_subset_* / ise_index_distance_subset_*)
    @staticmethod
    def _subset_ids(ids, nq: int) -> np.ndarray:
        ids = np.ascontiguousarray(np.asarray(ids), dtype=np.int64)
        assert ids.ndim == 2 and ids.shape[0] == nq, f"ids are (nq, kc) = ({nq}, kc), got {ids.shape}"
        return ids

    def search_subset(self, x, k: int, ids):
        """The exact k best among the rows ``ids[q]`` names for query q -> (D float32 (nq,k), I int64 (nq,k)), with the
        D bits ``search`` reports for the same (query, row) pair.  ``ids``: int64 (nq, kc), kc <= 2048; entries outside
        [0, ntotal) (Faiss's -1 padding) are ignored, an id named twice counts once.  Float32 storage only."""
        x = _as_rows(x, self.d)
        k = int(k)
        nq = x.shape[0]
        ids = self._subset_ids(ids, nq)
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        _n.check(_n.lib.ise_index_search_subset_host(self._h, x.ctypes.data, nq, k, ids.ctypes.data, ids.shape[1],
                                                     D.ctypes.data, I.ctypes.data))
        return D, I

    def search_subset_torch(self, xq, k: int, ids):
        """``search_subset`` on CUDA tensors (``ids`` int64 (nq, kc)), enqueued on the current torch stream (no host
        synchronisation)."""
        import torch

        k = int(k)
        xq, D, I, st = _torch_io(xq, torch.float32, self.d, k, torch.float32)
        nq = xq.shape[0]
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[0] == nq
        ids = ids.contiguous()
        with self._lock:
            _n.check(_n.lib.ise_index_search_subset_device(self._h, xq.data_ptr(), nq, k, ids.data_ptr(), ids.shape[1],
                                                           D.data_ptr(), I.data_ptr(), st))
        return D, I

    def compute_distance_subset(self, x, ids) -> np.ndarray:
        """Faiss's ``compute_distance_subset``: float32 shaped like ``ids``, entry (q, j) the score of query q and row
        ``ids[q, j]`` as ``search`` reports it (a NaN stays a NaN); +FLT_MAX (L2) / -FLT_MAX (inner product) for an
        entry outside [0, ntotal)."""
        x = _as_rows(x, self.d)
        nq = x.shape[0]
        ids = self._subset_ids(ids, nq)
        out = np.empty(ids.shape, dtype=np.float32)
        _n.check(_n.lib.ise_index_distance_subset_host(self._h, x.ctypes.data, nq, ids.ctypes.data, ids.shape[1],
                                                       out.ctypes.data))
        return out

    def compute_distance_subset_torch(self, xq, ids):
        """``compute_distance_subset`` on CUDA tensors, enqueued on the current torch stream."""
        import torch

        assert xq.is_cuda and xq.dtype == torch.float32 and xq.dim() == 2 and xq.shape[1] == self.d
        xq = xq.contiguous()
        nq = xq.shape[0]
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[0] == nq
        ids = ids.contiguous()
        out = torch.empty(ids.shape, dtype=torch.float32, device=xq.device)
        st = torch.cuda.current_stream(xq.device).cuda_stream
        with self._lock:
            _n.check(_n.lib.ise_index_distance_subset_device(self._h, xq.data_ptr(), nq, ids.data_ptr(), ids.shape[1],
                                                             out.data_ptr(), st))
        return out

    def subset_stats(self) -> dict:
        """Subset batches, score launches, candidate entries inside [0, ntotal) that were scored (include/ise_knn.h,
        ise_index_subset_stats).  Waits for the device."""
        return _counters(_n.lib.ise_index_subset_stats, self._h, ("subset_batches", "score_launches", "rows_scored"))

    # -- allocation-free forms for latency-critical loops (bench.py, sharded search): the caller owns
    # every buffer and names the stream; nothing is checked beyond what the C ABI checks
    def search_into(self, xq, k: int, D, I, stream: int) -> None:
        with self._lock:
            _n.check(_n.lib.ise_index_search_device(self._h, xq.data_ptr(), xq.shape[0], int(k), D.data_ptr(),
                                                    I.data_ptr(), stream))

    def search_keys_into(self, xq, k: int, id_base: int, keys, stream: int) -> None:
        with self._lock:
            _n.check(_n.lib.ise_index_search_keys_device(self._h, xq.data_ptr(), xq.shape[0], int(k), int(id_base),
                                                         keys.data_ptr(), stream))

    def search_keys_torch(self, xq, k: int, id_base: int = 0):
        """Shard-local search for the multi-GPU path: packed uint64 candidates
        (as an int64 tensor (nq,k)), see include/ise_knn.h."""
        import torch

        assert xq.is_cuda and xq.dtype == torch.float32 and xq.dim() == 2 and xq.shape[1] == self.d
        xq = xq.contiguous()
        nq = xq.shape[0]
        keys = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        st = torch.cuda.current_stream(xq.device).cuda_stream
        with self._lock:
            _n.check(_n.lib.ise_index_search_keys_device(self._h, xq.data_ptr(), nq, int(k), int(id_base),
                                                         keys.data_ptr(), st))
        return keys

    def search_timed_torch(self, xq, k: int, iters: int):
        """bench.py hook: (D, I, scan_ms_avg, merge_ms_avg) with HIP events on the stream
        the kernels run on."""
        import torch

        xq = xq.contiguous()
        nq = xq.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
        st = torch.cuda.current_stream(xq.device).cuda_stream
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        with self._lock:
            _n.check(_n.lib.ise_index_search_timed_device(self._h, xq.data_ptr(), nq, int(k), D.data_ptr(),
                                                          I.data_ptr(), st, int(iters), ctypes.byref(a),
                                                          ctypes.byref(b)))
        return D, I, float(a.value), float(b.value)


class IndexFlatL2(IndexFlat):
    def __init__(self, d: int, device: int | None = None, storage: str = "f32"):
        super().__init__(d, METRIC_L2, device, storage)


class IndexFlatIP(IndexFlat):
    def __init__(self, d: int, device: int | None = None, storage: str = "f32"):
        super().__init__(d, METRIC_INNER_PRODUCT, device, storage)


class _RowMask(IDSelector):
    """Rows by a bool mask (IndexIDMap's external-id selectors, already evaluated against ``id_map``)."""

    def __init__(self, mask: np.ndarray):
        self.mask = np.asarray(mask, dtype=bool).reshape(-1)

    def is_member(self, i: int) -> bool:
        return 0 <= int(i) < self.mask.size and bool(self.mask[int(i)])

    def members(self, ids) -> np.ndarray:
        ids = _ids_array(ids)
        ok = (ids >= 0) & (ids < self.mask.size)
        out = np.zeros(ids.shape, dtype=bool)
        out[ok] = self.mask[ids[ok]]
        return out


class _IDMapBase:
    """Faiss's id-mapping wrapper over a flat index of either kind: rows carry the caller's 64-bit ids, which survive
    ``remove_ids`` (the sub-index renumbers its rows; ``id_map[row]`` follows).  The mapping is host numpy, off the hot
    path.  Selectors -- in ``remove_ids`` and in ``params=`` -- are over EXTERNAL ids.  A subclass says how rows are
    coerced (``_rows``) and forwards what its sub-index has beyond ``d``, ``is_trained`` and ``ntotal``; the messages
    carry its name."""

    def __init__(self, index):
        assert index.ntotal == 0, f"{type(self).__name__} wraps an empty index (Faiss: index is empty on input)"
        self.index = index
        self.id_map = np.zeros(0, dtype=np.int64)

    d = property(lambda self: self.index.d)
    is_trained = property(lambda self: self.index.is_trained)
    ntotal = property(lambda self: self.index.ntotal)

    def _rows(self, x) -> np.ndarray:
        raise NotImplementedError

    def add(self, x) -> None:
        raise RuntimeError(f"add does not work with {type(self).__name__}, call add_with_ids")  # Faiss throws the same

    def add_with_ids(self, x, ids) -> None:
        x = self._rows(x)
        ids = _ids_array(ids)
        assert ids.shape[0] == x.shape[0], "one id per row"
        self.index.add(x)
        self.id_map = np.concatenate((self.id_map, ids))

    def _map(self, I: np.ndarray) -> np.ndarray:
        out = np.full(I.shape, -1, dtype=np.int64)
        ok = I >= 0
        out[ok] = self.id_map[I[ok]]
        return out

    def _row_params(self, params):
        """A selector over EXTERNAL ids -> one over rows (a bitmap from ``sel.members(id_map)``)."""
        sel = _params_sel(params)
        if sel is None:
            return None
        if isinstance(sel, DeviceSelector):
            raise TypeError(f"{type(self).__name__} takes an IDSelector over external ids, not a DeviceSelector over "
                            "rows")
        return SearchParameters(sel=_RowMask(sel.members(self.id_map)))

    def search(self, x, k: int, params=None):
        D, I = self.index.search(x, k, params=self._row_params(params))
        return D, self._map(I)

    def range_search(self, x, radius: float, params=None):
        lims, D, I = self.index.range_search(x, radius, params=self._row_params(params))
        return lims, D, self._map(I)

    def remove_ids(self, sel) -> int:
        """``sel`` selects EXTERNAL ids (a selector, or an int64 array-like taken as a batch)."""
        if not isinstance(sel, IDSelector):
            sel = IDSelectorBatch(sel)
        gone = sel.members(self.id_map)
        rows = np.flatnonzero(gone).astype(np.int64)
        if rows.size == 0:
            return 0
        n = self.index.remove_ids(rows)
        assert n == rows.size
        self.id_map = self.id_map[~gone]
        return n

    def reset(self) -> None:
        self.index.reset()
        self.id_map = np.zeros(0, dtype=np.int64)


class IndexIDMap(_IDMapBase):
    """faiss.IndexIDMap over an ``IndexFlat``."""

    def __init__(self, index: IndexFlat):
        if isinstance(index, _IndexIVF):
            raise NotImplementedError(f"IndexIDMap over an {type(index).__name__} is not provided")
        if isinstance(index, IndexPQ):
            raise NotImplementedError("IndexIDMap over an IndexPQ is not provided")
        if isinstance(index, IndexScalarQuantizer):
            raise NotImplementedError("IndexIDMap over an IndexScalarQuantizer is not provided")
        if isinstance(index, IndexRefine):
            raise NotImplementedError("IndexIDMap over an IndexRefine is not provided")
        super().__init__(index)

    metric_type = property(lambda self: self.index.metric_type)

    def _rows(self, x) -> np.ndarray:
        return _as_rows(x, self.index.d)

    def _image(self) -> bytes:
        sub = self.index
        return serialize_idmap(sub.d, sub.metric_type, sub.reconstruct_n(0, sub.ntotal), self.id_map)

    @classmethod
    def _from_parts(cls, parts, device):
        """The index a parsed "IxMp" image describes (``parse_idmap``)."""
        index = cls(IndexFlat(parts.d, parts.metric, device))
        if parts.xb.shape[0]:
            index.add_with_ids(parts.xb, parts.ids)
        return index


def merge_keys_torch(keys, metric: int):
    """Merge all-gathered candidate lists: ``keys`` int64 CUDA (n_lists, nq, k) ->
    (D float32 (nq,k), I int64 (nq,k)) on the same device."""
    import torch

    assert keys.is_cuda and keys.dtype == torch.int64 and keys.dim() == 3
    keys = keys.contiguous()
    n_lists, nq, k = keys.shape
    D = torch.empty((nq, k), dtype=torch.float32, device=keys.device)
    I = torch.empty((nq, k), dtype=torch.int64, device=keys.device)
    st = torch.cuda.current_stream(keys.device).cuda_stream
    _n.check(_n.lib.ise_merge_keys_device(keys.data_ptr(), n_lists, nq, k, int(metric), D.data_ptr(), I.data_ptr(),
                                          keys.device.index, st))
    return D, I


def merge_keys_into(keys, metric: int, D, I, stream: int) -> None:
    """Allocation-free form of ``merge_keys_torch``: keys int64 CUDA (n_lists, nq, k) contiguous."""
    n_lists, nq, k = keys.shape
    _n.check(_n.lib.ise_merge_keys_device(keys.data_ptr(), n_lists, nq, k, int(metric), D.data_ptr(), I.data_ptr(),
                                          keys.device.index, stream))


def normalize_L2(x) -> None:
    """In-place row L2 normalisation (faiss.normalize_L2): float32 C-contiguous (n, d)
    required, returns None, zero rows untouched.  Runs on the GPU."""
    import torch

    if isinstance(x, torch.Tensor):
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
        st = torch.cuda.current_stream(x.device).cuda_stream
        _n.check(_n.lib.ise_normalize_rows_device(x.data_ptr(), x.shape[0], x.shape[1], x.device.index, st))
        return None
    assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 2 and x.flags.c_contiguous, \
        "normalize_L2 needs a C-contiguous float32 (n, d) array"
    _n.check(_n.lib.ise_normalize_rows_host(x.ctypes.data, x.shape[0], x.shape[1], _default_device()))
    return None


# ---------------------------------------------------------------- persistence
class _Cursor:
    """A read position in a file image, for the ``_parse_*_at`` readers below: each reads the image that starts at the
    cursor and leaves the cursor behind it, so that an image inside another file is read where it lies.  An operation
    names the message of the RuntimeError it raises when bytes are missing; ``truncated``, where the cursor was made
    with one, replaces them all (an image inside an "IwSq", "IwPQ" or "IxRF" file is cut short with its file)."""

    _COUNT = struct.Struct("<Q")

    def __init__(self, buf, truncated: str | None = None):
        self.buf, self.off, self.truncated = buf, 0, truncated

    def _advance(self, size: int, missing) -> int:
        at = self.off
        if len(self.buf) < at + size:
            raise RuntimeError(self.truncated or missing)
        self.off = at + size
        return at

    def take(self, st: struct.Struct, missing=None) -> tuple:
        return st.unpack_from(self.buf, self._advance(st.size, missing))

    def fourcc(self, missing=None) -> bytes:
        at = self._advance(4, missing)
        return bytes(self.buf[at:at + 4])

    def peek(self, missing=None) -> bytes:
        """The fourcc at the cursor, which stays there."""
        fourcc = self.fourcc(missing)
        self.off -= 4
        return fourcc

    def expect(self, fourcc: bytes, what: str) -> None:
        """A whole fourcc at the cursor that is not ``fourcc`` is a foreign file."""
        got = bytes(self.buf[self.off:self.off + 4])
        if len(got) == 4 and got != fourcc:
            raise RuntimeError(f"unsupported index type {got!r}: not an {what}")

    def array(self, dtype, count: int, missing=None) -> np.ndarray:
        """``count`` little-endian items of ``dtype``, as a fresh array."""
        dtype = np.dtype(dtype)
        at = self._advance(count * dtype.itemsize, missing)
        return np.frombuffer(self.buf, dtype=dtype.newbyteorder("<"), count=count, offset=at).astype(dtype)

    def vector(self, dtype, expect, miscounted: str, missing=None, count_missing=None) -> np.ndarray:
        """A counted vector: uint64 count, then count items.  RuntimeError(``miscounted``) when the count is not
        ``expect`` (a number, or a predicate); ``count_missing`` where the count's own bytes have another message."""
        (count,) = self.take(self._COUNT, count_missing or missing)
        if not (expect(count) if callable(expect) else count == expect):
            raise RuntimeError(miscounted)
        return self.array(dtype, count, missing)


def _pack_vector(a: np.ndarray) -> bytes:
    """A counted vector as every layout here writes it: uint64 count, then the items."""
    return struct.pack("<Q", a.size) + a.tobytes()


# Faiss on-disk IndexFlat layout [upstream-faiss index_write.cpp, restated from
# the published format; no sample .faiss file exists in the reference, so byte
# compatibility with real Faiss files is UNPINNED]:
#   fourcc "IxF2" (L2) / "IxFI" (IP); int32 d; int64 ntotal; int64 1<<20;
#   int64 1<<20; uint8 is_trained; int32 metric_type; uint64 count (= N*d
#   float32 words); count float32.
# IndexIDMap [upstream-faiss index_write.cpp, restated from the published format and UNPINNED like row 8f-1]:
#   fourcc "IxMp"; the same index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type); the sub-index as
#   written above; then the id vector: uint64 count (= ntotal); count int64.
_FOURCC = {METRIC_L2: b"IxF2", METRIC_INNER_PRODUCT: b"IxFI"}
_FOURCC_IDMAP = b"IxMp"
_HDR = struct.Struct("<4siqqqBi")
_FlatParts = namedtuple("_FlatParts", "d metric xb")
_IDMapParts = namedtuple("_IDMapParts", "d metric xb ids")


def serialize_flat(d: int, metric: int, xb: np.ndarray) -> bytes:
    xb = np.ascontiguousarray(xb, dtype="<f4")
    n = xb.shape[0] if xb.size else 0
    head = _HDR.pack(_FOURCC[metric], d, n, 1 << 20, 1 << 20, 1, metric)
    return head + struct.pack("<Q", n * d) + xb.tobytes()


def _pack_id_vector(ids, n: int) -> bytes:
    """The tail of both id-map files: uint64 count (= ntotal), count int64."""
    ids = np.ascontiguousarray(ids, dtype="<i8").reshape(-1)
    assert ids.size == n, "one id per row"
    return _pack_vector(ids)


def serialize_idmap(d: int, metric: int, xb: np.ndarray, ids) -> bytes:
    n = xb.shape[0] if np.size(xb) else 0
    head = _HDR.pack(_FOURCC_IDMAP, d, n, 1 << 20, 1 << 20, 1, metric)
    return head + serialize_flat(d, metric, xb) + _pack_id_vector(ids, n)


def _parse_idmap_at(cur: _Cursor) -> _IDMapParts:
    fourcc, d, n, _, _, _, metric = cur.take(_HDR, "truncated index file")
    if fourcc != _FOURCC_IDMAP:
        raise RuntimeError(f"unsupported index type {fourcc!r}: not an IndexIDMap")
    d2, metric, xb = _parse_flat_at(cur)
    if d2 != d or xb.shape[0] != n:
        raise RuntimeError("corrupt IndexIDMap: the sub-index does not match the header")
    truncated = "truncated IndexIDMap id vector"  # also what this format says to a count that is not ntotal
    return _IDMapParts(d, metric, xb, cur.vector(np.int64, n, truncated, truncated))


def parse_idmap(buf: bytes):
    """-> (d, metric, xb float32 (n, d), ids int64 (n,)); raises RuntimeError on a foreign or truncated file."""
    return tuple(_parse_idmap_at(_Cursor(buf)))


def _flat_image(index) -> bytes:
    """An ``IndexFlat`` -- or whatever has its ``d``, ``metric_type``, ``ntotal`` and ``reconstruct_n`` -- as a file."""
    return serialize_flat(index.d, index.metric_type, index.reconstruct_n(0, index.ntotal))


def _parse_flat_at(cur: _Cursor) -> _FlatParts:
    fourcc, d, n, _, _, _, metric = cur.take(_HDR, "truncated index file")
    if fourcc not in (b"IxF2", b"IxFI", b"IxFl"):
        raise RuntimeError(f"unsupported index type {fourcc!r}: only flat indexes are readable")
    if fourcc == b"IxF2":
        metric = METRIC_L2
    elif fourcc == b"IxFI":
        metric = METRIC_INNER_PRODUCT
    corrupt = "corrupt flat index payload"  # also what this format says to missing rows
    return _FlatParts(d, metric, cur.vector(np.float32, n * d, corrupt, corrupt, "truncated index file").reshape(n, d))


def parse_flat(buf: bytes):
    """-> (d, metric, xb float32 (n, d)); raises RuntimeError on a foreign file."""
    return tuple(_parse_flat_at(_Cursor(buf)))


# IndexPQ [upstream-faiss index_write.cpp write_index / write_ProductQuantizer, restated from memory of the published
# format and UNPINNED like the four layouts here: there is no sample file]:
#   fourcc "IxPq"; the index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type); the product quantiser: int64 d;
#   int64 M; int64 nbits; the centroid vector: uint64 count (= M * 256 * dsub), count float32; the code vector: uint64
#   count (= ntotal * M), count uint8; then the polysemous fields: int32 search_type (0, "exhaustive ADC search"),
#   uint8 encode_signs (0), int32 polysemous_ht (0).
_FOURCC_PQ = b"IxPq"
_PQ_DIMS = struct.Struct("<qqq")
_PQ_TAIL = struct.Struct("<iBi")
_PQParts = namedtuple("_PQParts", "d M nbits metric centroids codes")


def serialize_pq(d: int, metric: int, centroids, codes) -> bytes:
    """``centroids`` float32 (M, 256, dsub), ``codes`` uint8 (n, M) (any n, also 0)."""
    c = np.ascontiguousarray(centroids, dtype="<f4")
    assert c.ndim == 3 and c.shape[1] == 256 and c.shape[0] * c.shape[2] == int(d), "centroids are (M, 256, d / M)"
    M = c.shape[0]
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, M)
    head = _HDR.pack(_FOURCC_PQ, int(d), codes.shape[0], 1 << 20, 1 << 20, 1, int(metric))
    return head + _PQ_DIMS.pack(int(d), M, 8) + _pack_vector(c) + _pack_vector(codes) + _PQ_TAIL.pack(0, 0, 0)


def _parse_pq_at(cur: _Cursor) -> _PQParts:
    cur.expect(_FOURCC_PQ, "IndexPQ")
    _, d, n, _, _, _, metric = cur.take(_HDR, "truncated IndexPQ file")
    d2, M, nbits = cur.take(_PQ_DIMS, "truncated IndexPQ file")
    if d <= 0 or d2 != d or M <= 0 or d % M != 0 or nbits != 8 or n < 0:
        raise RuntimeError("corrupt IndexPQ header (only 8-bit product quantisers are readable)")
    centroids = cur.vector(np.float32, 256 * d, "corrupt IndexPQ: the centroid vector does not hold M * 256 * dsub floats",
                           "truncated IndexPQ centroids", "truncated IndexPQ file").reshape(M, 256, d // M)
    codes = cur.vector(np.uint8, n * M, "corrupt IndexPQ: the code vector does not hold ntotal * M bytes",
                       "truncated IndexPQ codes", "truncated IndexPQ centroids").reshape(n, M)
    cur.take(_PQ_TAIL, "truncated IndexPQ codes")
    return _PQParts(d, M, nbits, metric, centroids, codes)


def parse_pq(buf: bytes):
    """-> (d, M, nbits, metric, centroids float32 (M, 256, dsub), codes uint8 (n, M)); raises RuntimeError on a foreign,
    truncated or miscounted file."""
    return tuple(_parse_pq_at(_Cursor(buf)))


# IndexScalarQuantizer [upstream-faiss index_write.cpp write_index / write_ScalarQuantizer, restated from memory of the
# published format and UNPINNED like the layouts above: there is no sample file]:
#   fourcc "IxSQ"; the index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type); the scalar quantiser: int32
#   qtype; int32 rangestat; float32 rangestat_arg; uint64 d; uint64 code_size; the trained vector: uint64 count (= 2 d,
#   or 2 for the uniform type), count float32; then the code vector: uint64 count (= ntotal * code_size), count uint8.
_FOURCC_SQ = b"IxSQ"
_SQ_HEAD = struct.Struct("<iifQQ")
_SQ_QTYPES = (0, 2)  # QT_8bit, QT_8bit_uniform: the types that are readable
_SQParts = namedtuple("_SQParts", "d metric qtype rangestat rangestat_arg trained codes")


def _pack_sq_block(d: int, qtype: int, trained, rangestat: int, rangestat_arg: float) -> bytes:
    """The scalar quantiser block of "IxSQ" and "IwSq": ``_SQ_HEAD``, then the trained vector."""
    assert qtype in _SQ_QTYPES, "only QT_8bit and QT_8bit_uniform are written"
    t = np.ascontiguousarray(trained, dtype="<f4").reshape(-1)
    assert t.size == (2 if qtype == 2 else 2 * d), "the trained vector is [vmin.., vdiff..]"
    return _SQ_HEAD.pack(qtype, int(rangestat), float(rangestat_arg), d, d) + _pack_vector(t)


def _parse_sq_block_at(cur: _Cursor, d: int, what: str, mismatch: str, missing=None, missing_trained=None):
    """-> (qtype, rangestat, rangestat_arg, trained) of the block at the cursor, in a file of a ``what``."""
    qtype, rangestat, rangestat_arg, d2, code_size = cur.take(_SQ_HEAD, missing)
    if qtype not in _SQ_QTYPES:
        raise RuntimeError(f"unsupported scalar quantiser type {qtype}: only QT_8bit (0) and QT_8bit_uniform (2) are readable")
    if d2 != d or code_size != d:
        raise RuntimeError(mismatch)
    trained = cur.vector(np.float32, 2 if qtype == 2 else 2 * d,
                         f"corrupt {what}: the trained vector does not hold vmin and vdiff", missing_trained, missing)
    return qtype, rangestat, float(rangestat_arg), trained


def serialize_sq(d: int, metric: int, qtype: int, trained, codes, rangestat: int = 0, rangestat_arg: float = 0.0) -> bytes:
    """``trained`` float32 (2 d,) or (2,) for the uniform type, ``codes`` uint8 (n, d) (any n, also 0)."""
    d, qtype = int(d), int(qtype)
    block = _pack_sq_block(d, qtype, trained, rangestat, rangestat_arg)
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, d)
    return _HDR.pack(_FOURCC_SQ, d, codes.shape[0], 1 << 20, 1 << 20, 1, int(metric)) + block + _pack_vector(codes)


def _parse_sq_at(cur: _Cursor) -> _SQParts:
    cur.expect(_FOURCC_SQ, "IndexScalarQuantizer")
    corrupt = "corrupt IndexScalarQuantizer header"
    _, d, n, _, _, _, metric = cur.take(_HDR, "truncated IndexScalarQuantizer file")
    qtype, rangestat, rangestat_arg, trained = _parse_sq_block_at(
        cur, d, "IndexScalarQuantizer", corrupt, "truncated IndexScalarQuantizer file",
        "truncated IndexScalarQuantizer trained vector")
    if d <= 0 or n < 0:
        raise RuntimeError(corrupt)
    codes = cur.vector(np.uint8, n * d, "corrupt IndexScalarQuantizer: the code vector does not hold ntotal * d bytes",
                       "truncated IndexScalarQuantizer codes", "truncated IndexScalarQuantizer trained vector").reshape(n, d)
    return _SQParts(d, metric, qtype, rangestat, rangestat_arg, trained, codes)


def parse_sq(buf: bytes):
    """-> (d, metric, qtype, rangestat, rangestat_arg, trained float32, codes uint8 (n, d)); raises RuntimeError on a
    foreign, truncated or miscounted file and on a quantiser type other than the two 8-bit ones."""
    return tuple(_parse_sq_at(_Cursor(buf)))


# IndexIVFScalarQuantizer [upstream-faiss index_write.cpp write_index / write_ivf_header / write_InvertedLists, restated
# from memory of the published format and UNPINNED like the layouts above: there is no sample file]:
#   fourcc "IwSq"; the index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type); uint64 nlist; uint64 nprobe; the
#   quantiser as its own "IxF2" / "IxFI" image; the direct map, empty: uint8 type (0, none), uint64 count (0); the scalar
#   quantiser block of "IxSQ": int32 qtype; int32 rangestat; float32 rangestat_arg; uint64 d; uint64 code_size; uint64
#   count (= 2 d, or 2 for the uniform type), count float32; then uint64 code_size; uint8 by_residual; the inverted lists:
#   fourcc "ilar"; uint64 nlist; uint64 code_size; the sizes -- fourcc "full", uint64 count (= nlist), count uint64 (what is
#   written here), or fourcc "sprs", uint64 count (= 2 x the lists that hold rows), count uint64 as (list, size) pairs
#   (Faiss writes it when fewer than half of the lists hold rows; readable) -- then, per list that holds rows: size x
#   code_size uint8, size int64 ids.
_FOURCC_IVFSQ = b"IwSq"
_IVF_DIMS = struct.Struct("<QQ")
_IVF_DIRECT_MAP = struct.Struct("<BQ")
_IVF_CODE = struct.Struct("<QB")
_TRUNCATED_IVFSQ = "truncated IndexIVFScalarQuantizer file"
_IVFSQParts = namedtuple("_IVFSQParts", "d metric nlist nprobe qmetric centroids qtype trained lists rangestat "
                                        "rangestat_arg by_residual")


def serialize_ivfsq(d: int, metric: int, nlist: int, nprobe: int, qmetric: int, centroids, qtype: int, trained, lists,
                    rangestat: int = 0, rangestat_arg: float = 0.0, by_residual: bool = False) -> bytes:
    """``centroids`` float32 (nlist, d) (or (0, d): an untrained quantiser) under the quantiser's metric ``qmetric``;
    ``trained`` as for ``serialize_sq``; ``lists``: ``nlist`` pairs (ids int64 (m,), codes uint8 (m, d)), any m, also 0."""
    d, qtype, nlist = int(d), int(qtype), int(nlist)
    block = _pack_sq_block(d, qtype, trained, rangestat, rangestat_arg)
    assert len(lists) == nlist, "one (ids, codes) pair per list"
    pairs = [(np.ascontiguousarray(ids, dtype="<i8").reshape(-1), np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, d))
             for ids, codes in lists]
    assert all(ids.size == codes.shape[0] for ids, codes in pairs), "one id per code row"
    head = [_HDR.pack(_FOURCC_IVFSQ, d, sum(ids.size for ids, _ in pairs), 1 << 20, 1 << 20, 1, int(metric)),
            _IVF_DIMS.pack(nlist, int(nprobe)),
            serialize_flat(d, int(qmetric), np.asarray(centroids, dtype=np.float32).reshape(-1, d)), _IVF_DIRECT_MAP.pack(0, 0),
            block, _IVF_CODE.pack(d, 1 if by_residual else 0)]
    return b"".join(head) + _pack_ivf_lists(pairs, nlist, d)


def _pack_ivf_lists(pairs, nlist: int, code_size: int) -> bytes:
    """The inverted lists of "IwSq" and "IwPQ": fourcc "ilar", nlist, code_size, the sizes in the "full" form, then per
    list that holds rows its codes and its ids.  ``pairs``: ``nlist`` pairs (ids "<i8" (m,), codes uint8 (m, code_size))."""
    sizes = np.array([ids.size for ids, _ in pairs], dtype="<u8")
    out = [b"ilar", _IVF_DIMS.pack(nlist, code_size), b"full", _pack_vector(sizes)]
    for ids, codes in pairs:
        if ids.size:
            out += [codes.tobytes(), ids.tobytes()]
    return b"".join(out)


def _parse_ivf_lists_at(cur: _Cursor, nlist: int, code_size: int, n: int, what: str) -> list:
    """-> [(ids int64 (m,), codes uint8 (m, code_size))] * nlist of the inverted lists at the cursor, in a file of a
    ``what`` whose header says ``nlist`` lists, ``code_size`` bytes a row and ``n`` rows."""
    corrupt = f"corrupt {what}: "
    lists = cur.fourcc()
    if lists != b"ilar":
        raise RuntimeError(f"unsupported inverted lists {lists!r}: only array lists (\"ilar\") are readable")
    if cur.take(_IVF_DIMS) != (nlist, code_size):
        raise RuntimeError(corrupt + "the inverted lists do not match the header")
    form = cur.fourcc()
    sizes = np.zeros(nlist, dtype=np.int64)
    if form == b"full":
        sizes[:] = cur.vector(np.uint64, nlist, corrupt + "the size vector does not hold nlist entries").astype(np.int64)
    elif form == b"sprs":
        pairs = cur.vector(np.uint64, lambda count: count % 2 == 0 and count <= 2 * nlist,
                           corrupt + "the sparse size vector does not hold (list, size) pairs").astype(np.int64).reshape(-1, 2)
        if pairs.size and (pairs[:, 0].min() < 0 or pairs[:, 0].max() >= nlist):
            raise RuntimeError(corrupt + "a list number outside [0, nlist)")
        sizes[pairs[:, 0]] = pairs[:, 1]
    else:
        raise RuntimeError(f"unsupported list size form {form!r} in an {what} file")
    if sizes.min() < 0 or int(sizes.sum()) != n:
        raise RuntimeError(corrupt + "the list sizes do not add up to ntotal")
    lists = []
    for m in (int(s) for s in sizes):
        codes = cur.array(np.uint8, m * code_size).reshape(m, code_size)
        lists.append((cur.array(np.int64, m), codes))
    return lists


def _parse_ivfsq_at(cur: _Cursor) -> _IVFSQParts:
    """(Every missing byte is ``_TRUNCATED_IVFSQ``: the cursor is made with it.)"""
    corrupt = "corrupt IndexIVFScalarQuantizer: "
    cur.expect(_FOURCC_IVFSQ, "IndexIVFScalarQuantizer")
    _, d, n, _, _, _, metric = cur.take(_HDR)
    nlist, nprobe = cur.take(_IVF_DIMS)
    if d <= 0 or n < 0 or nlist <= 0:
        raise RuntimeError("corrupt IndexIVFScalarQuantizer header")
    quantizer = cur.peek()
    if quantizer not in (b"IxF2", b"IxFI"):
        raise RuntimeError(f"unsupported quantiser type {quantizer!r} in an IndexIVFScalarQuantizer file: "
                           "only flat quantisers are readable")
    d2, qmetric, centroids = _parse_flat_at(cur)
    if d2 != d or centroids.shape[0] not in (0, nlist):
        raise RuntimeError(corrupt + "the quantiser does not hold nlist centroids of dimension d")
    if cur.take(_IVF_DIRECT_MAP) != (0, 0):
        raise RuntimeError("an IndexIVFScalarQuantizer file with a direct map is not readable")
    qtype, rangestat, rangestat_arg, trained = _parse_sq_block_at(
        cur, d, "IndexIVFScalarQuantizer", corrupt + "the scalar quantiser does not match the header")
    code_size, by_residual = cur.take(_IVF_CODE)
    if code_size != d:
        raise RuntimeError(corrupt + "the inverted lists do not match the header")
    lists = _parse_ivf_lists_at(cur, nlist, d, n, "IndexIVFScalarQuantizer")
    return _IVFSQParts(d, metric, int(nlist), int(nprobe), qmetric, centroids, qtype, trained, lists, rangestat,
                       rangestat_arg, bool(by_residual))


def parse_ivfsq(buf: bytes):
    """-> (d, metric, nlist, nprobe, qmetric, centroids float32 (nlist or 0, d), qtype, trained float32, lists [(ids int64
    (m,), codes uint8 (m, d))] * nlist, rangestat, rangestat_arg, by_residual): ``serialize_ivfsq``'s arguments.  Raises
    RuntimeError on a foreign, truncated or miscounted file and on a quantiser type other than the two 8-bit ones."""
    return tuple(_parse_ivfsq_at(_Cursor(buf, _TRUNCATED_IVFSQ)))


# IndexIVFPQ [upstream-faiss index_write.cpp write_index / write_ivf_header / write_ProductQuantizer /
# write_InvertedLists, restated from memory of the published format and UNPINNED like the layouts above: there is no
# sample file]:
#   fourcc "IwPQ"; the IVF header of "IwSq": the index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type), uint64
#   nlist, uint64 nprobe, the quantiser as its own "IxF2" / "IxFI" image, the direct map, empty: uint8 type (0), uint64
#   count (0); then uint8 by_residual; uint64 code_size (= M); the product quantiser block of "IxPq": int64 d, int64 M,
#   int64 nbits, the centroid vector (uint64 count = M * 256 * dsub, count float32); then the inverted lists as in "IwSq"
#   with code_size = M.
_FOURCC_IVFPQ = b"IwPQ"
_IVFPQ_CODE = struct.Struct("<BQ")
_TRUNCATED_IVFPQ = "truncated IndexIVFPQ file"
_IVFPQParts = namedtuple("_IVFPQParts", "d metric nlist nprobe qmetric centroids M nbits pq_centroids lists by_residual")


def serialize_ivfpq(d: int, metric: int, nlist: int, nprobe: int, qmetric: int, centroids, pq_centroids, lists,
                    by_residual: bool = False) -> bytes:
    """``centroids`` float32 (nlist, d) (or (0, d): an untrained quantiser) under the quantiser's metric ``qmetric``;
    ``pq_centroids`` float32 (M, 256, d / M); ``lists``: ``nlist`` pairs (ids int64 (m,), codes uint8 (m, M)), any m, also 0."""
    d, nlist = int(d), int(nlist)
    c = np.ascontiguousarray(pq_centroids, dtype="<f4")
    assert c.ndim == 3 and c.shape[1] == 256 and c.shape[0] * c.shape[2] == d, "the codebook is (M, 256, d / M)"
    M = c.shape[0]
    assert len(lists) == nlist, "one (ids, codes) pair per list"
    pairs = [(np.ascontiguousarray(ids, dtype="<i8").reshape(-1), np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, M))
             for ids, codes in lists]
    assert all(ids.size == codes.shape[0] for ids, codes in pairs), "one id per code row"
    head = [_HDR.pack(_FOURCC_IVFPQ, d, sum(ids.size for ids, _ in pairs), 1 << 20, 1 << 20, 1, int(metric)),
            _IVF_DIMS.pack(nlist, int(nprobe)),
            serialize_flat(d, int(qmetric), np.asarray(centroids, dtype=np.float32).reshape(-1, d)), _IVF_DIRECT_MAP.pack(0, 0),
            _IVFPQ_CODE.pack(1 if by_residual else 0, M), _PQ_DIMS.pack(d, M, 8), _pack_vector(c)]
    return b"".join(head) + _pack_ivf_lists(pairs, nlist, M)


def _parse_ivfpq_at(cur: _Cursor) -> _IVFPQParts:
    """(Every missing byte is ``_TRUNCATED_IVFPQ``: the cursor is made with it.)"""
    corrupt = "corrupt IndexIVFPQ: "
    cur.expect(_FOURCC_IVFPQ, "IndexIVFPQ")
    _, d, n, _, _, _, metric = cur.take(_HDR)
    nlist, nprobe = cur.take(_IVF_DIMS)
    if d <= 0 or n < 0 or nlist <= 0:
        raise RuntimeError("corrupt IndexIVFPQ header")
    quantizer = cur.peek()
    if quantizer not in (b"IxF2", b"IxFI"):
        raise RuntimeError(f"unsupported quantiser type {quantizer!r} in an IndexIVFPQ file: only flat quantisers are readable")
    d2, qmetric, centroids = _parse_flat_at(cur)
    if d2 != d or centroids.shape[0] not in (0, nlist):
        raise RuntimeError(corrupt + "the quantiser does not hold nlist centroids of dimension d")
    if cur.take(_IVF_DIRECT_MAP) != (0, 0):
        raise RuntimeError("an IndexIVFPQ file with a direct map is not readable")
    by_residual, code_size = cur.take(_IVFPQ_CODE)
    d3, M, nbits = cur.take(_PQ_DIMS)
    if d3 != d or M <= 0 or d % M != 0 or nbits != 8:
        raise RuntimeError(corrupt + "the product quantiser does not match the header (only 8-bit product quantisers are "
                           "readable)")
    if code_size != M:
        raise RuntimeError(corrupt + "code_size is not M")
    pq_centroids = cur.vector(np.float32, 256 * d, corrupt + "the centroid vector does not hold M * 256 * dsub floats"
                              ).reshape(M, 256, d // M)
    lists = _parse_ivf_lists_at(cur, nlist, M, n, "IndexIVFPQ")
    return _IVFPQParts(d, metric, int(nlist), int(nprobe), qmetric, centroids, int(M), int(nbits), pq_centroids, lists,
                       bool(by_residual))


def parse_ivfpq(buf: bytes):
    """-> (d, metric, nlist, nprobe, qmetric, centroids float32 (nlist or 0, d), M, nbits, pq_centroids float32 (M, 256,
    d / M), lists [(ids int64 (m,), codes uint8 (m, M))] * nlist, by_residual).  Raises RuntimeError on a foreign,
    truncated or miscounted file and on sub-quantisers of other than 8 bits; a file with ``by_residual`` set parses (reading
    it into an index raises)."""
    return tuple(_parse_ivfpq_at(_Cursor(buf, _TRUNCATED_IVFPQ)))


# IndexRefineFlat [upstream-faiss index_write.cpp, restated from memory of the published format and UNPINNED like the
# layouts above: there is no sample file]:
#   fourcc "IxRF"; the index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type); the base index as its own file
#   image; the refine index as an "IxF2" / "IxFI" image; float32 k_factor.
_FOURCC_REFINE = b"IxRF"
_TRUNCATED_REFINE = "truncated IndexRefineFlat file"
_RefineParts = namedtuple("_RefineParts", "d metric base_kind base xb k_factor")
_K_FACTOR = struct.Struct("<f")
_SUB_IMAGES = {b"IxF2": ("flat", _parse_flat_at), b"IxFI": ("flat", _parse_flat_at), _FOURCC_PQ: ("pq", _parse_pq_at),
               _FOURCC_SQ: ("sq", _parse_sq_at), _FOURCC_IVFPQ: ("ivfpq", _parse_ivfpq_at)}


def _sub_image(cur: _Cursor):
    """-> (kind "flat" | "pq" | "sq" | "ivfpq", the reader of the sub-index image at the cursor)."""
    fourcc = cur.peek(_TRUNCATED_REFINE)
    if fourcc not in _SUB_IMAGES:
        raise RuntimeError(f"unsupported sub-index type {fourcc!r} in an IndexRefineFlat file")
    return _SUB_IMAGES[fourcc]


def serialize_refine(base_image: bytes, d: int, metric: int, xb: np.ndarray, k_factor: float) -> bytes:
    """``base_image``: the base index as ``serialize_flat``, ``serialize_pq``, ``serialize_sq`` or ``serialize_ivfpq`` writes it;
    ``xb`` float32 (n, d): the refine index's rows."""
    n = xb.shape[0] if np.size(xb) else 0
    head = _HDR.pack(_FOURCC_REFINE, int(d), n, 1 << 20, 1 << 20, 1, int(metric))
    return head + bytes(base_image) + serialize_flat(int(d), int(metric), xb) + _K_FACTOR.pack(float(k_factor))


def _parse_refine_at(cur: _Cursor) -> _RefineParts:
    """(Every missing byte is ``_TRUNCATED_REFINE``: the cursor is made with it.)"""
    cur.expect(_FOURCC_REFINE, "IndexRefineFlat")
    _, d, n, _, _, _, metric = cur.take(_HDR)
    kind, read = _sub_image(cur)
    base = read(cur)
    rkind, read = _sub_image(cur)
    if rkind != "flat":
        raise RuntimeError("corrupt IndexRefineFlat: the refine index is not a flat index")
    d2, metric2, xb = read(cur)
    base_n = sum(len(ids) for ids, _ in base.lists) if kind == "ivfpq" else (base.xb if kind == "flat" else base.codes).shape[0]
    if d2 != d or base.d != d or xb.shape[0] != n or base_n != n or metric2 != metric:
        raise RuntimeError("corrupt IndexRefineFlat: the sub-indexes do not match the header")
    (k_factor,) = cur.take(_K_FACTOR)
    return _RefineParts(d, metric, kind, base, xb, float(k_factor))


def parse_refine(buf: bytes):
    """-> (d, metric, base_kind "flat" | "pq" | "sq" | "ivfpq", base as ``parse_flat`` / ``parse_pq`` / ``parse_sq`` /
    ``parse_ivfpq`` return it, xb float32 (n, d), k_factor); raises RuntimeError on a foreign, truncated or inconsistent file."""
    parts = _parse_refine_at(_Cursor(buf, _TRUNCATED_REFINE))
    return tuple(parts._replace(base=tuple(parts.base)))


def write_index(index, path) -> None:
    if isinstance(index, IndexIVFFlat):
        raise NotImplementedError("write_index of an IndexIVFFlat is not provided")
    # the image first: a kind that refuses (an untrained index) leaves what is at ``path`` as it is
    image = index._image() if isinstance(index, (_CodedIndex, _IndexIVF, IndexRefine, IndexIDMap, IndexPreTransform)) \
        else _flat_image(index)
    with open(str(path), "wb") as f:
        f.write(image)


def read_index(path, device: int | None = None):
    """-> IndexFlat, IndexIDMap, IndexPQ, IndexScalarQuantizer, IndexIVFScalarQuantizer, IndexIVFPQ, IndexRefineFlat or
    IndexPreTransform, as the file was written; the stored rows and codes are added as they are, nothing is encoded again."""
    with open(str(path), "rb") as f:
        buf = f.read()
    if buf[:4] in (b"IwFl", b"IwF2"):  # Faiss's fourccs of IndexIVFFlat files
        raise NotImplementedError("read_index of an IndexIVFFlat file is not provided")
    cls, read, truncated = _INDEX_FILES.get(bytes(buf[:4]), _FLAT_FILE)  # (a foreign file is the flat reader's to refuse)
    return cls()._from_parts(read(_Cursor(buf, truncated)), device)


# fourcc -> (the class of its index, late: the classes follow; the reader of its image; the cursor's message)
_FLAT_FILE = (lambda: IndexFlat, _parse_flat_at, None)
_INDEX_FILES = {_FOURCC_IDMAP: (lambda: IndexIDMap, _parse_idmap_at, None),
                _FOURCC_PQ: (lambda: IndexPQ, _parse_pq_at, None),
                _FOURCC_SQ: (lambda: IndexScalarQuantizer, _parse_sq_at, None),
                _FOURCC_IVFSQ: (lambda: IndexIVFScalarQuantizer, _parse_ivfsq_at, _TRUNCATED_IVFSQ),
                _FOURCC_IVFPQ: (lambda: IndexIVFPQ, _parse_ivfpq_at, _TRUNCATED_IVFPQ),
                _FOURCC_REFINE: (lambda: IndexRefineFlat, _parse_refine_at, _TRUNCATED_REFINE)}

# ---------------------------------------------------------------- binary flat index (faiss.IndexBinaryFlat)
_INT32_MAX = int(np.iinfo(np.int32).max)


def _as_codes(x, code_size=None) -> np.ndarray:
    """C-contiguous uint8 (n, code_size); a wrong dtype or width is an assertion, as in ``_as_rows``."""
    x = np.asarray(x)
    assert x.dtype == np.uint8, f"binary codes are uint8, got {x.dtype}"
    x = np.ascontiguousarray(x)
    assert x.ndim == 2, "expected a 2-D array"
    if code_size is not None:
        assert x.shape[1] == code_size, f"code size mismatch: got {x.shape[1]} bytes, index has {code_size}"
    return x


class IndexBinaryFlat(_RemovableIndex):
    """faiss.IndexBinaryFlat(d): exact brute-force search over ``d``-bit codes (uint8 rows of ``d / 8`` bytes) under the
    Hamming distance, on the device (include/ise_knn.h, ise_binary_index_*).  Distances are int32, ascending; ties go
    by ascending id, always (Faiss promises no order among equal distances); unfilled slots are -1 / INT32_MAX.  No
    CPU path: the constructor raises without a GPU."""

    _ABI = "ise_binary_index"
    _SELECTOR = BinaryDeviceSelector
    _FOREIGN_SELECTOR = "a float index's selector cannot filter a binary index"

    def __init__(self, d: int, device: int | None = None):
        self.d = int(d)
        self.code_size = self.d // 8
        self.is_trained = True
        self.device = _default_device() if device is None else int(device)
        self._h = ctypes.c_void_p()
        self._lock = threading.Lock()
        _n.check(_n.lib.ise_binary_index_create(ctypes.byref(self._h), self.d, self.device))

    ntotal = _ntotal_property(_n.lib.ise_binary_index_info, 4, 2)

    def binary_stats(self) -> dict:
        """Search batches, scan passes launched (one per 16 queries and per 32 results), range batches
        (include/ise_knn.h, ise_binary_index_stats)."""
        return _counters(_n.lib.ise_binary_index_stats, self._h, ("search_batches", "scan_passes", "range_batches"))

    def add(self, x) -> None:
        """Append codes (copied): uint8 (n, d / 8)."""
        x = _as_codes(x, self.code_size)
        _n.check(_n.lib.ise_binary_index_add_host(self._h, x.ctypes.data, x.shape[0]))

    def add_torch(self, x) -> None:
        """Append codes from a CUDA uint8 tensor on this index's device (no host hop)."""
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[1] == self.code_size
        x = x.contiguous()
        st = torch.cuda.current_stream(x.device).cuda_stream
        with self._lock:
            _n.check(_n.lib.ise_binary_index_add_device(self._h, x.data_ptr(), x.shape[0], st))
        torch.cuda.current_stream(x.device).synchronize()  # x may be freed by the caller

    def reconstruct_n(self, i0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.ntotal - i0 if n is None else n
        out = np.empty((n, self.code_size), dtype=np.uint8)
        _n.check(_n.lib.ise_binary_index_reconstruct_host(self._h, int(i0), int(n), out.ctypes.data))
        return out

    def reconstruct(self, i: int) -> np.ndarray:
        return self.reconstruct_n(int(i), 1)[0]

    def make_selector(self, sel) -> BinaryDeviceSelector:  # the shared method, with this index's return type
        return super().make_selector(sel)

    def search(self, x, k: int, params=None):
        """(D int32 (nq, k), I int64 (nq, k)), fresh arrays: Hamming distance ascending, ties by ascending id.
        ``params=SearchParameters(sel=...)``: among the rows the selector names only."""
        x = _as_codes(x, self.code_size)
        k = int(k)
        assert k > 0
        nq = x.shape[0]
        D = np.empty((nq, k), dtype=np.int32)
        I = np.empty((nq, k), dtype=np.int64)
        sel = _params_sel(params)
        if sel is not None:
            self._with_selector(sel, lambda s: _n.check(_n.lib.ise_binary_index_search_sel_host(
                self._h, x.ctypes.data, nq, k, s, D.ctypes.data, I.ctypes.data)))
            return D, I
        _n.check(_n.lib.ise_binary_index_search_host(self._h, x.ctypes.data, nq, k, D.ctypes.data, I.ctypes.data))
        return D, I

    def search_torch(self, xq, k: int, params=None):
        """Device-resident search: CUDA uint8 (nq, d / 8) in, CUDA (D int32, I int64) out, enqueued on the current
        torch stream (no host synchronisation).  ``params=SearchParameters(sel=...)`` as ``search``; a selector that is
        not a ``BinaryDeviceSelector`` is built and destroyed here, which waits for the device."""
        import torch

        xq, D, I, st = _torch_io(xq, torch.uint8, self.code_size, int(k), torch.int32)
        nq = xq.shape[0]
        sel = _params_sel(params)
        if sel is not None:
            def run(s):
                with self._lock:
                    _n.check(_n.lib.ise_binary_index_search_sel_device(self._h, xq.data_ptr(), nq, int(k), s,
                                                                       D.data_ptr(), I.data_ptr(), st))
            self._with_selector(sel, run)
            return D, I
        with self._lock:
            _n.check(_n.lib.ise_binary_index_search_device(self._h, xq.data_ptr(), nq, int(k), D.data_ptr(),
                                                           I.data_ptr(), st))
        return D, I

    def range_search(self, x, radius: int, params=None):
        """(lims uint64 (nq + 1,), D int32, I int64), fresh arrays: query i's rows are ``I[lims[i]:lims[i+1]]`` in
        ascending id order, every row with distance < radius (strict, as Faiss's hamming_range_search), D the numbers
        ``search`` reports.  Faiss's Python wrapper may hand D out as float32; here it stays int32.
        ``params=SearchParameters(sel=...)``: among the selected rows only."""
        x = _as_codes(x, self.code_size)
        nq = x.shape[0]
        res = ctypes.c_void_p()
        sel = _params_sel(params)
        if sel is not None:
            self._with_selector(sel, lambda s: _n.check(_n.lib.ise_binary_index_range_search_sel_host(
                self._h, x.ctypes.data, nq, int(radius), s, ctypes.byref(res))))
        else:
            _n.check(_n.lib.ise_binary_index_range_search_host(self._h, x.ctypes.data, nq, int(radius),
                                                               ctypes.byref(res)))
        return _read_range_result(res, np.int32, _n.lib.ise_binary_range_result_get,
                                  _n.lib.ise_binary_range_result_destroy)


# Faiss on-disk IndexBinaryFlat layout [upstream-faiss index_write.cpp write_index_binary, restated from the published
# format; no sample file exists in the reference, so byte compatibility with real Faiss files is UNPINNED like the two
# layouts above]:
#   fourcc "IBxF"; int32 d; int32 code_size; int64 ntotal; uint8 is_trained; int32 metric_type (1); uint64 count
#   (= ntotal * code_size); count bytes.
_FOURCC_BINARY = b"IBxF"
_BHDR = struct.Struct("<4siiqBi")
_BinaryFlatParts = namedtuple("_BinaryFlatParts", "d xb")
_BinaryIDMapParts = namedtuple("_BinaryIDMapParts", "d xb ids")


def serialize_binary_flat(d: int, xb) -> bytes:
    d = int(d)
    assert d > 0 and d % 8 == 0, "d must be a positive multiple of 8"
    cs = d // 8
    xb = np.asarray(xb, dtype=np.uint8)
    xb = _as_codes(xb.reshape(-1, cs), cs)
    return _BHDR.pack(_FOURCC_BINARY, d, cs, xb.shape[0], 1, 1) + _pack_vector(xb)


def _parse_binary_flat_at(cur: _Cursor) -> _BinaryFlatParts:
    cur.expect(_FOURCC_BINARY, "IndexBinaryFlat")
    _, d, cs, n, _, _ = cur.take(_BHDR, "truncated binary index file")
    # the count is part of the header check: a header that is wrong in itself has no right count
    expect = n * cs if d > 0 and d % 8 == 0 and cs == d // 8 and n >= 0 else -1
    xb = cur.vector(np.uint8, expect, "corrupt binary flat index header", "truncated binary flat index payload",
                    "truncated binary index file")
    return _BinaryFlatParts(d, xb.reshape(n, cs))


def parse_binary_flat(buf: bytes):
    """-> (d, xb uint8 (n, d / 8)); raises RuntimeError on a foreign or truncated file."""
    return tuple(_parse_binary_flat_at(_Cursor(buf)))


class IndexBinaryIDMap(_IDMapBase):
    """faiss.IndexBinaryIDMap over an ``IndexBinaryFlat``."""

    # two shared methods under this class's own annotations: the sub-index's type, a radius that is a Hamming distance
    def __init__(self, index: IndexBinaryFlat):
        if isinstance(index, _IndexIVF):
            raise NotImplementedError(f"IndexBinaryIDMap over an {type(index).__name__} is not provided")
        super().__init__(index)

    def range_search(self, x, radius: int, params=None):
        return super().range_search(x, radius, params)

    code_size = property(lambda self: self.index.code_size)

    def _rows(self, x) -> np.ndarray:
        return _as_codes(x, self.index.code_size)


# IndexBinaryIDMap [upstream-faiss index_write.cpp write_index_binary, restated from memory of the published format and
# UNPINNED like the three layouts above]:
#   fourcc "IBMp"; the binary header (int32 d; int32 code_size; int64 ntotal; uint8 is_trained; int32 metric_type); the
#   sub-index as "IBxF" writes it; then the id vector: uint64 count (= ntotal); count int64.
_FOURCC_BINARY_IDMAP = b"IBMp"


def serialize_binary_idmap(d: int, xb, ids) -> bytes:
    sub = serialize_binary_flat(d, xb)
    _, _, cs, n, _, _ = _BHDR.unpack_from(sub, 0)
    return _BHDR.pack(_FOURCC_BINARY_IDMAP, int(d), cs, n, 1, 1) + sub + _pack_id_vector(ids, n)


def _parse_binary_idmap_at(cur: _Cursor) -> _BinaryIDMapParts:
    cur.expect(_FOURCC_BINARY_IDMAP, "IndexBinaryIDMap")
    _, d, cs, n, _, _ = cur.take(_BHDR, "truncated binary index file")
    d2, xb = _parse_binary_flat_at(cur)
    if d2 != d or xb.shape[1] != cs or xb.shape[0] != n:
        raise RuntimeError("corrupt IndexBinaryIDMap: the sub-index does not match the header")
    ids = cur.vector(np.int64, n, "corrupt IndexBinaryIDMap: the id vector does not have one id per row",
                     "truncated IndexBinaryIDMap id vector")
    return _BinaryIDMapParts(d, xb, ids)


def parse_binary_idmap(buf: bytes):
    """-> (d, xb uint8 (n, d / 8), ids int64 (n,)); raises RuntimeError on a foreign or truncated file."""
    return tuple(_parse_binary_idmap_at(_Cursor(buf)))


# IndexBinaryIVF [upstream-faiss index_write.cpp write_index_binary / write_binary_ivf_header / write_InvertedLists,
# restated from memory of the published format and UNPINNED like the layouts above: there is no sample file]:
#   fourcc "IBwF"; the binary header (int32 d; int32 code_size; int64 ntotal; uint8 is_trained; int32 metric_type);
#   uint64 nlist; uint64 nprobe; the quantiser as its own "IBxF" image; the direct map, empty: uint8 type (0, none),
#   uint64 count (0); the inverted lists as in an "IwSq" file with code_size = d / 8 bytes per row: fourcc "ilar"; uint64
#   nlist; uint64 code_size; the sizes -- fourcc "full", uint64 count (= nlist), count uint64 (what is written here), or
#   fourcc "sprs", uint64 count, count uint64 as (list, size) pairs (readable) -- then, per list that holds rows: size x
#   code_size uint8, size int64 ids.
_FOURCC_BINARY_IVF = b"IBwF"
_TRUNCATED_BINARY_IVF = "truncated IndexBinaryIVF file"
_BinaryIVFParts = namedtuple("_BinaryIVFParts", "d nlist nprobe centroids lists")


def serialize_binary_ivf(d: int, nlist: int, nprobe: int, centroids, lists) -> bytes:
    """``centroids`` uint8 (nlist, d / 8) (or (0, d / 8): an untrained quantiser); ``lists``: ``nlist`` pairs (ids int64
    (m,), codes uint8 (m, d / 8)), any m, also 0."""
    d, nlist = int(d), int(nlist)
    assert d > 0 and d % 8 == 0, "d must be a positive multiple of 8"
    cs = d // 8
    assert len(lists) == nlist, "one (ids, codes) pair per list"
    pairs = [(np.ascontiguousarray(ids, dtype="<i8").reshape(-1), np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, cs))
             for ids, codes in lists]
    assert all(ids.size == codes.shape[0] for ids, codes in pairs), "one id per code row"
    sizes = np.array([ids.size for ids, _ in pairs], dtype="<u8")
    centroids = np.asarray(centroids, dtype=np.uint8).reshape(-1, cs)
    out = [_BHDR.pack(_FOURCC_BINARY_IVF, d, cs, int(sizes.sum()), 1 if centroids.shape[0] == nlist else 0, 1),
           _IVF_DIMS.pack(nlist, int(nprobe)), serialize_binary_flat(d, centroids), _IVF_DIRECT_MAP.pack(0, 0), b"ilar",
           _IVF_DIMS.pack(nlist, cs), b"full", _pack_vector(sizes)]
    for ids, codes in pairs:
        if ids.size:
            out += [codes.tobytes(), ids.tobytes()]
    return b"".join(out)


def _parse_binary_ivf_at(cur: _Cursor) -> _BinaryIVFParts:
    """(Every missing byte is ``_TRUNCATED_BINARY_IVF``: the cursor is made with it.)"""
    corrupt = "corrupt IndexBinaryIVF: "
    cur.expect(_FOURCC_BINARY_IVF, "IndexBinaryIVF")
    _, d, cs, n, _, _ = cur.take(_BHDR)
    nlist, nprobe = cur.take(_IVF_DIMS)
    if d <= 0 or d % 8 != 0 or cs != d // 8 or n < 0 or nlist <= 0:
        raise RuntimeError("corrupt IndexBinaryIVF header")
    quantizer = cur.peek()
    if quantizer != _FOURCC_BINARY:
        raise RuntimeError(f"unsupported quantiser type {quantizer!r} in an IndexBinaryIVF file: only a flat binary "
                           "quantiser is readable")
    d2, centroids = _parse_binary_flat_at(cur)
    if d2 != d or centroids.shape[0] not in (0, nlist):
        raise RuntimeError(corrupt + "the quantiser does not hold nlist codes of d bits")
    if cur.take(_IVF_DIRECT_MAP) != (0, 0):
        raise RuntimeError("an IndexBinaryIVF file with a direct map is not readable")
    lists = cur.fourcc()
    if lists != b"ilar":
        raise RuntimeError(f"unsupported inverted lists {lists!r}: only array lists (\"ilar\") are readable")
    if cur.take(_IVF_DIMS) != (nlist, cs):
        raise RuntimeError(corrupt + "the inverted lists do not match the header")
    form = cur.fourcc()
    sizes = np.zeros(nlist, dtype=np.int64)
    if form == b"full":
        sizes[:] = cur.vector(np.uint64, nlist, corrupt + "the size vector does not hold nlist entries").astype(np.int64)
    elif form == b"sprs":
        pairs = cur.vector(np.uint64, lambda count: count % 2 == 0 and count <= 2 * nlist,
                           corrupt + "the sparse size vector does not hold (list, size) pairs").astype(np.int64).reshape(-1, 2)
        if pairs.size and (pairs[:, 0].min() < 0 or pairs[:, 0].max() >= nlist):
            raise RuntimeError(corrupt + "a list number outside [0, nlist)")
        sizes[pairs[:, 0]] = pairs[:, 1]
    else:
        raise RuntimeError(f"unsupported list size form {form!r} in an IndexBinaryIVF file")
    if sizes.min() < 0 or int(sizes.sum()) != n:
        raise RuntimeError(corrupt + "the list sizes do not add up to ntotal")
    lists = []
    for m in (int(s) for s in sizes):
        codes = cur.array(np.uint8, m * cs).reshape(m, cs)
        lists.append((cur.array(np.int64, m), codes))
    return _BinaryIVFParts(d, int(nlist), int(nprobe), centroids, lists)


def parse_binary_ivf(buf: bytes):
    """-> (d, nlist, nprobe, centroids uint8 (nlist or 0, d / 8), lists [(ids int64 (m,), codes uint8 (m, d / 8))] *
    nlist): ``serialize_binary_ivf``'s arguments.  Raises RuntimeError on a foreign, truncated or miscounted file."""
    return tuple(_parse_binary_ivf_at(_Cursor(buf, _TRUNCATED_BINARY_IVF)))


def write_index_binary(index, path) -> None:
    if isinstance(index, IndexBinaryIVF):
        image = index._binary_image()
    elif isinstance(index, IndexBinaryIDMap):
        sub = index.index
        image = serialize_binary_idmap(sub.d, sub.reconstruct_n(0, sub.ntotal), index.id_map)
    else:
        image = serialize_binary_flat(index.d, index.reconstruct_n(0, index.ntotal))
    with open(str(path), "wb") as f:  # after the image, as ``write_index``
        f.write(image)


def read_index_binary(path, device: int | None = None):
    """-> IndexBinaryFlat, or IndexBinaryIDMap or IndexBinaryIVF for a file written from one."""
    with open(str(path), "rb") as f:
        buf = f.read()
    if buf[:4] == _FOURCC_BINARY_IVF:
        return IndexBinaryIVF._from_parts(_parse_binary_ivf_at(_Cursor(buf, _TRUNCATED_BINARY_IVF)), device)
    if buf[:4] == _FOURCC_BINARY_IDMAP:
        d, xb, ids = _parse_binary_idmap_at(_Cursor(buf))
        index = IndexBinaryIDMap(IndexBinaryFlat(d, device))
        if xb.shape[0]:
            index.add_with_ids(xb, ids)
        return index
    d, xb = _parse_binary_flat_at(_Cursor(buf))
    index = IndexBinaryFlat(d, device)
    if xb.shape[0]:
        index.add(xb)
    return index


class Kmeans:
    """``faiss.Kmeans`` as the reference drives it (backend/kmeans_faiss.py:29-44):
    ``Kmeans(d=, k=, niter=25, nredo=3, seed=42, spherical=True)``, ``.train(x, init_centroids=)``,
    then ``.index`` (the assignment index: inner product over unit centroids when spherical,
    L2 otherwise [upstream-faiss]), ``.centroids`` and ``.obj``.

    Assignment (``.index.search(X, 1)``) is the scoped hot path.  ``train`` is a
    "next" row and is provided as plain Lloyd iterations on the GPU: the assignment
    step is the MFMA assignment kernel, the centroid update a device scatter-add.  Faiss seeds its
    initial centroids from its own RNG, so trained centroids are not comparable run-for-run with
    Faiss's (parity unpinned).  ``init_centroids`` starts the iterations from a given codebook, as in
    Faiss; the reference reloads a saved model without training, by handing the index to
    ``FaissKMeans(index=...)`` (backend/bag_of_visual_words.py:207-216)."""

    def __init__(self, d, k, niter=25, nredo=1, seed=1234, spherical=False, verbose=False, **_):
        self.d, self.k = int(d), int(k)
        self.niter, self.nredo, self.seed = int(niter), int(nredo), int(seed)
        self.spherical, self.verbose = bool(spherical), bool(verbose)
        self.centroids = None
        self.index = None
        self.obj = np.zeros(0, dtype=np.float32)

    def _make_index(self, c: np.ndarray):
        index = IndexFlatIP(self.d) if self.spherical else IndexFlatL2(self.d)
        index.add(c)
        return index

    def _lloyd(self, x_dev, c0: np.ndarray, niter: int):
        import torch

        c = torch.from_numpy(c0).to(x_dev.device)
        obj = []
        n = x_dev.shape[0]
        # one assignment index for all iterations (its stream and buffers are created once): the centroids are
        # swapped in with reset() + add
        index = IndexFlat(self.d, METRIC_INNER_PRODUCT if self.spherical else METRIC_L2, x_dev.device.index)
        for _ in range(niter):
            if self.spherical:
                normalize_L2(c)
            index.reset()
            index.add_torch(c)
            D, I = index.assign_torch(x_dev) if index._assign_applies(n, 1) else index.search_torch(x_dev, 1)
            lab = I.view(-1).clamp_(min=0)
            obj.append(float(D.sum()))
            sums = torch.zeros_like(c).index_add_(0, lab, x_dev)
            cnt = torch.bincount(lab, minlength=self.k).to(c.dtype)
            empty = cnt == 0
            c = torch.where(empty[:, None], c, sums / cnt.clamp(min=1)[:, None])
            if bool(empty.any()):  # re-seed empty clusters from random rows
                g = torch.Generator(device="cpu").manual_seed(self.seed + len(obj))
                pick = torch.randint(0, n, (int(empty.sum()),), generator=g).to(x_dev.device)
                c[empty] = x_dev[pick]
        if self.spherical:
            normalize_L2(c)
        return c.cpu().numpy(), obj

    def train(self, x, init_centroids=None):
        import torch

        x = _as_rows(x, self.d)
        dev = torch.device("cuda", _default_device())
        best = None
        for redo in range(1 if init_centroids is not None else max(1, self.nredo)):
            if init_centroids is not None:
                c0 = _as_rows(init_centroids, self.d).copy()
                assert c0.shape[0] == self.k
            else:
                rs = np.random.RandomState(self.seed + redo)
                c0 = x[rs.choice(x.shape[0], self.k, replace=x.shape[0] < self.k)].copy()
            if self.niter > 0 and x.shape[0] > 0:
                c, obj = self._lloyd(torch.from_numpy(x).to(dev), c0, self.niter)
            else:
                c, obj = c0, [0.0]
                if self.spherical:
                    normalize_L2(c)
            # spherical k-means maximises the summed inner product, plain k-means minimises distance
            score = obj[-1] if self.spherical else -obj[-1]
            if best is None or score > best[0]:
                best = (score, c, obj)
        _, self.centroids, obj = best
        self.obj = np.asarray(obj, dtype=np.float32)
        self.index = self._make_index(self.centroids)
        return float(self.obj[-1])


# ---------------------------------------------------------------- inverted lists (faiss.IndexIVFFlat)
class ClusteringParameters:
    """The two fields of faiss.ClusteringParameters that ``IndexIVFFlat.train`` reads (``index.cp``)."""

    def __init__(self, niter: int = 10, seed: int = 1234):
        self.niter = int(niter)
        self.seed = int(seed)


class _IndexIVF(_IndexHandle):
    """What the inverted-list indexes share: the caller's coarse quantiser (an ``IndexFlat`` of ``nlist`` centroids),
    its clustering in ``train``, the assignment of rows to lists, ``add``, ``get_list``, ``nprobe`` and ``search`` as
    ``search_preassigned`` of the quantiser's answer.  A subclass creates its handle, says what ``is_trained`` is and
    names its family of entry points (``_ABI``), the two search calls outright (``_search_host``, ``_search_device``),
    its ``ntotal``, the dtype of a list's payload of (m, list width) entries (``_LIST_DTYPE``; the list width is the rows'
    unless ``_init_ivf`` is told another: a product quantiser stores ``M`` bytes for a row of ``d`` floats) and whether it
    encodes its rows (``_ENCODES``).  An index that does checks the rows of an ``add`` for NaN / inf entries, needs its training in
    ``search_preassigned`` too and answers an empty batch there itself, and has no lists to read while its codec is
    untrained.  An index over bit codes also names its quantiser's type (``_QUANTIZER``), how rows and queries are
    coerced (``_COERCE``: ``_as_rows`` or ``_as_codes``, to ``_width`` entries a row) and the dtypes of a row's entries
    and of a distance (``_ROW_DTYPE``, ``_DIST_DTYPE``: the name numpy and torch share)."""

    _QUANTIZER = IndexFlat
    _COERCE = staticmethod(_as_rows)
    _ROW_DTYPE = "float32"
    _DIST_DTYPE = "float32"
    _LIST_DTYPE = np.float32
    _ENCODES = False

    def _init_ivf(self, quantizer, d: int, nlist: int, metric: int | None, width: int | None = None,
                  list_width: int | None = None) -> None:
        """``metric``: None on an index without a ``metric_type``; ``width``: entries of a row where it is not ``d``;
        ``list_width``: entries of a STORED row where it is not ``width``."""
        assert isinstance(quantizer, self._QUANTIZER), f"the coarse quantiser is an {self._QUANTIZER.__name__}"
        assert quantizer.d == int(d), f"dimension mismatch: quantizer has d={quantizer.d}, index d={d}"
        self.quantizer = quantizer
        self.d = int(d)
        self._width = self.d if width is None else int(width)
        self._list_width = self._width if list_width is None else int(list_width)
        self.nlist = int(nlist)
        self.nprobe = 1
        if metric is not None:
            self.metric_type = int(metric)
        self.cp = ClusteringParameters()
        self.device = quantizer.device
        self._h = ctypes.c_void_p()
        self._lock = threading.Lock()

    def _train_quantizer(self, x) -> None:
        """Nothing when the quantiser already holds ``nlist`` centroids.  With an empty quantiser: ``Kmeans(d, nlist)``
        on ``x`` (spherical when the quantiser is an inner-product index), ``niter`` and ``seed`` from ``self.cp``, and
        the centroids are added to the quantiser."""
        if self.quantizer.ntotal == self.nlist:
            return
        if self.quantizer.ntotal != 0:
            raise RuntimeError(f"the quantizer holds {self.quantizer.ntotal} centroids, neither 0 nor nlist = {self.nlist}")
        x = _as_rows(x, self.d)
        if x.shape[0] < self.nlist:
            raise RuntimeError(f"{x.shape[0]} training rows for nlist = {self.nlist} centroids")
        km = Kmeans(self.d, self.nlist, niter=self.cp.niter, seed=self.cp.seed,
                    spherical=self.quantizer.metric_type == METRIC_INNER_PRODUCT)
        km.train(x)
        self.quantizer.add(km.centroids)

    def _require_trained(self, what: str) -> None:
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}.{what} before train")

    def _codec_trained(self) -> bool:
        return True

    def reset(self) -> None:
        """Drop the rows; the quantiser, a codec's trained state (and ``is_trained``) stay."""
        _n.check(self._fn("reset")(self._h))

    def _check_assignment(self, lists: np.ndarray) -> None:
        bad = np.flatnonzero(lists < 0)
        if bad.size:
            raise ValueError(f"row {int(bad[0])} has no nearest centroid (a NaN or inf entry?): nothing was added")

    def _assign(self, x: np.ndarray) -> np.ndarray:
        """int64 (n,): the list of every row, ``quantizer.search(x, 1)[1]``, checked."""
        lists = np.ascontiguousarray(self.quantizer.search(x, 1)[1].reshape(-1), dtype=np.int64)
        self._check_assignment(lists)
        return lists

    def _assign_torch(self, x):
        """The same on the device: the route ``quantizer.search(x, 1)`` takes for this many rows, so that the ids are the
        same (a quantiser over bit codes has the one route); the list numbers are read back to be checked."""
        qz = self.quantizer
        assign = hasattr(qz, "_assign_applies") and qz._assign_applies(x.shape[0], 1)
        lists = (qz.assign_torch(x) if assign else qz.search_torch(x, 1))[1].reshape(-1).contiguous()
        self._check_assignment(lists.cpu().numpy())
        return lists

    # -- build side
    def add(self, x) -> None:
        """Append rows (copied; encoded by an index that encodes); row i of the call goes to list
        ``quantizer.search(x, 1)[1][i]``.  On an index that encodes, a row with a NaN or inf entry raises ``ValueError``
        and nothing of the call is added."""
        self._require_trained("add")
        x = self._COERCE(x, self._width)
        if x.shape[0] == 0:
            return
        lists = self._assign(x)
        (_check_rows if self._ENCODES else _n.check)(
            self._fn("add_host")(self._h, x.ctypes.data, lists.ctypes.data, x.shape[0]))

    def add_torch(self, x) -> None:
        """``add`` from a CUDA tensor of the rows' dtype on this index's device (no host hop for the rows; the list
        numbers are read back to be checked, and an index that encodes waits for the encoder's verdict on non-finite
        entries).  Under the index's lock, like every device call that names a stream."""
        import torch

        self._require_trained("add")
        assert x.is_cuda and x.dtype == getattr(torch, self._ROW_DTYPE) and x.dim() == 2 and x.shape[1] == self._width
        x = x.contiguous()
        n = x.shape[0]
        if n == 0:
            return
        lists = self._assign_torch(x)
        st = torch.cuda.current_stream(x.device).cuda_stream
        with self._lock:
            (_check_rows if self._ENCODES else _n.check)(
                self._fn("add_device")(self._h, x.data_ptr(), lists.data_ptr(), n, st))

    # -- lists
    def list_size(self, l: int) -> int:
        sizes = np.zeros(self.nlist, dtype=np.int64)
        _n.check(self._fn("list_sizes_host")(self._h, sizes.ctypes.data))
        return int(sizes[int(l)])

    def get_list(self, l: int):
        """(ids int64 (m,), rows (m, list width) -- float32, or the uint8 codes of an index that encodes or holds bit
        codes) of list ``l``, in list order (ascending ids)."""
        m = self.list_size(l)
        ids = np.empty(m, dtype=np.int64)
        rows = np.empty((m, self._list_width), dtype=self._LIST_DTYPE)
        if self._codec_trained():
            _n.check(self._fn("list_host")(self._h, int(l), ids.ctypes.data, rows.ctypes.data))
        return ids, rows

    # -- query side
    def _nprobe(self) -> int:
        return max(1, min(int(self.nprobe), self.nlist))

    def _no_params(self, params) -> None:
        if params is not None:
            raise NotImplementedError(f"search parameters are not provided on {type(self).__name__}: set index.nprobe")

    def search(self, x, k: int, params=None):
        """(D (nq,k) float32 -- int32 over bit codes --, I int64 (nq,k)), fresh arrays: the k best among the rows of the
        ``nprobe`` lists nearest to each query (``quantizer.search(x, min(nprobe, nlist))[1]``)."""
        self._no_params(params)
        self._require_trained("search")
        x = self._COERCE(x, self._width)
        if x.shape[0] == 0:
            return np.empty((0, int(k)), dtype=self._DIST_DTYPE), np.empty((0, int(k)), dtype=np.int64)
        return self.search_preassigned(x, k, self.quantizer.search(x, self._nprobe())[1])

    def search_preassigned(self, x, k: int, probes):
        """``search`` with the probed lists given: ``probes`` int64 (nq, nprobe); -1 entries are ignored."""
        if self._ENCODES:
            self._require_trained("search")
        x = self._COERCE(x, self._width)
        k = int(k)
        assert k > 0
        nq = x.shape[0]
        probes = np.ascontiguousarray(np.asarray(probes), dtype=np.int64)
        assert probes.ndim == 2 and probes.shape[0] == nq and probes.shape[1] >= 1
        D = np.empty((nq, k), dtype=self._DIST_DTYPE)
        I = np.empty((nq, k), dtype=np.int64)
        if nq or not self._ENCODES:  # (the float family checks k and the probes of an empty batch too)
            _n.check(self._search_host(self._h, x.ctypes.data, nq, k, probes.ctypes.data, probes.shape[1],
                                       D.ctypes.data, I.ctypes.data))
        return D, I

    def search_torch(self, xq, k: int, params=None):
        """Device-resident search: CUDA (nq, width) of the rows' dtype in, CUDA (D, I) out; the quantiser's search and
        the scan are enqueued on the current torch stream, under the index's lock.  No host synchronisation, except
        that the first search after an ``add`` rebuilds the lists and waits for that."""
        import torch

        self._no_params(params)
        self._require_trained("search")
        k = int(k)
        xq, D, I, st = _torch_io(xq, getattr(torch, self._ROW_DTYPE), self._width, k, getattr(torch, self._DIST_DTYPE))
        nq = xq.shape[0]
        if nq == 0:
            return D, I
        probes = self.quantizer.search_torch(xq, self._nprobe())[1].contiguous()
        with self._lock:
            _n.check(self._search_device(self._h, xq.data_ptr(), nq, k, probes.data_ptr(), probes.shape[1], D.data_ptr(),
                                         I.data_ptr(), st))
        return D, I

    def range_search(self, *a, **kw):
        raise NotImplementedError(f"range_search is not provided on {type(self).__name__}")

    def remove_ids(self, *a, **kw):
        raise NotImplementedError(f"remove_ids is not provided on {type(self).__name__}")


class IndexIVFFlat(_IndexIVF):
    """faiss.IndexIVFFlat: a coarse quantiser (an ``IndexFlat`` of ``nlist`` centroids, the caller's object) in front of
    uncompressed float32 rows.  ``add`` puts every row into the inverted list of its nearest centroid; ``search`` visits
    the ``nprobe`` lists whose centroids are nearest to the query and returns the exact k best among THEIR rows -- D has
    the bits ``IndexFlat.search`` reports for the same (query, row) pair, ties go by ascending id, unfilled slots are
    -1 / +-FLT_MAX.  With ``nprobe == nlist`` the result is ``IndexFlat.search`` itself.

    For given centroids everything here is determined, and it is checked bit for bit against this package's own flat
    index; Faiss's own IVF (its k-means seeding, its scanning order among equal distances) is unpinned.

    The lists live on the device (include/ise_knn.h, ise_ivf_*): ``add`` appends to a pending buffer, the first search
    after an ``add`` rebuilds the lists, which moves the whole index once.  Not provided (they raise
    ``NotImplementedError``): ``range_search``, ``remove_ids``, ``params=``, ``write_index`` / ``read_index`` and
    ``IndexIDMap`` over this type."""

    _ABI = "ise_ivf"
    _search_host = staticmethod(_n.lib.ise_ivf_search_host)
    _search_device = staticmethod(_n.lib.ise_ivf_search_device)
    ntotal = _ntotal_property(_n.lib.ise_ivf_info, 6, 4)

    def __init__(self, quantizer: IndexFlat, d: int, nlist: int, metric: int = METRIC_L2):
        self._init_ivf(quantizer, d, nlist, metric)
        _n.check(_n.lib.ise_ivf_create(ctypes.byref(self._h), self.d, self.metric_type, self.nlist, self.device))
        self.is_trained = quantizer.ntotal == self.nlist

    def train(self, x) -> None:
        """A no-op when the quantiser already holds ``nlist`` centroids.  With an empty quantiser: ``Kmeans(d, nlist)``
        on ``x`` (spherical when the quantiser is an inner-product index), ``niter`` and ``seed`` from ``self.cp``, and
        the centroids are added to the quantiser.  ``cp.niter`` defaults to 10, Faiss's default for an IVF's clustering
        as restated from memory: unpinned, like the seeding of ``Kmeans`` itself."""
        self._train_quantizer(x)
        self.is_trained = True

    def ivf_stats(self) -> dict:
        """Search batches, scan passes launched, 16-row tiles of list rows the passes loaded (include/ise_knn.h,
        ise_ivf_stats).  Waits for the device."""
        return _counters(_n.lib.ise_ivf_stats, self._h, ("batches", "passes", "tiles_loaded"))


# ---------------------------------------------------------------- inverted lists over bit codes (faiss.IndexBinaryIVF)
def _bits_to_signs(x: np.ndarray, d: int) -> np.ndarray:
    """uint8 (n, d / 8) -> float32 (n, d) of +-1: bit i of a code is ``(byte[i >> 3] >> (i & 7)) & 1``, a set bit is +1."""
    bits = np.unpackbits(x, axis=1, bitorder="little")[:, :d]
    return np.ascontiguousarray(bits.astype(np.float32) * 2.0 - 1.0)


def _signs_to_bits(c: np.ndarray) -> np.ndarray:
    """float32 (n, d) -> uint8 (n, d / 8): a bit is set where the entry is > 0 (the inverse of ``_bits_to_signs``)."""
    return np.ascontiguousarray(np.packbits(c > 0, axis=1, bitorder="little"))


class IndexBinaryIVF(_IndexIVF):
    """faiss.IndexBinaryIVF(quantizer, d, nlist): a coarse quantiser (an ``IndexBinaryFlat`` of ``nlist`` codes, the
    caller's object) in front of ``d``-bit codes (uint8 rows of ``d / 8`` bytes).  ``add`` puts every code into the
    inverted list of its nearest centroid code (``quantizer.search(x, 1)[1]``: Hamming distance, ties by ascending id);
    ``search`` visits the ``nprobe`` lists whose centroids are nearest to the query and returns the exact k best among
    THEIR rows: D int32 Hamming distances ascending, ties by ascending id, unfilled slots INT32_MAX / -1.  With ``nprobe ==
    nlist`` the result is ``IndexBinaryFlat.search`` on the same rows, bit for bit.

    For given centroid codes everything here is determined, and it is checked exactly against this package's own flat
    binary index; Faiss's own binary IVF (its k-means seeding, its order among equal distances) is unpinned.

    Rows and queries are uint8 (n, d / 8), on the host or, in ``add_torch`` / ``search_torch``, as CUDA tensors; D is int32
    and I int64 (on the device too), unfilled slots are INT32_MAX / -1; ``get_list`` gives (ids int64 (m,), codes uint8
    (m, d / 8)).  In ``search_preassigned``'s probes, -1 and out-of-range entries are ignored and a list named twice
    counts once.

    The lists live on the device (include/ise_knn.h, ise_binary_ivf_*): ``add`` appends to a pending
    buffer, the first search after an ``add`` rebuilds the lists.  Not provided (they raise ``NotImplementedError``):
    ``range_search``, ``remove_ids``, ``params=`` and ``IndexBinaryIDMap`` over this type."""

    _ABI = "ise_binary_ivf"
    _search_host = staticmethod(_n.lib.ise_binary_ivf_search_host)
    _search_device = staticmethod(_n.lib.ise_binary_ivf_search_device)
    _QUANTIZER = IndexBinaryFlat
    _COERCE = staticmethod(_as_codes)
    _ROW_DTYPE = "uint8"
    _DIST_DTYPE = "int32"
    _LIST_DTYPE = np.uint8
    ntotal = _ntotal_property(_n.lib.ise_binary_ivf_info, 5, 3)

    def __init__(self, quantizer: IndexBinaryFlat, d: int, nlist: int):
        self.code_size = int(d) // 8
        self._init_ivf(quantizer, d, nlist, None, self.code_size)
        _n.check(_n.lib.ise_binary_ivf_create(ctypes.byref(self._h), self.d, self.nlist, self.device))
        self.is_trained = quantizer.ntotal == self.nlist

    # -- build side
    def train(self, x) -> None:
        """uint8 (n, d / 8).  A no-op when the quantiser already holds ``nlist`` codes; ``RuntimeError`` when it holds
        neither 0 nor ``nlist`` codes, or when ``n < nlist``.  Otherwise the bits are expanded to +-1 float32 (bit i of
        a code is ``(byte[i >> 3] >> (i & 7)) & 1``), ``Kmeans(d, nlist, niter=cp.niter, seed=cp.seed)`` runs on them, a
        centroid's bit is ``value > 0``, and the ``nlist`` codes are added to the quantiser.

        This is Faiss's scheme for a binary IVF restated from memory: the comparison with Faiss (its seeding, its
        ``cp.niter`` default, how it binarises) is unpinned, as for ``IndexIVFFlat.train``.

        Two centroids may binarise to the same code.  The quantiser breaks ties by ascending id, so the later of the two
        lists is never the nearest: it stays empty, and nothing else changes -- an empty list is probed and adds nothing."""
        if self.quantizer.ntotal != self.nlist:
            if self.quantizer.ntotal != 0:
                raise RuntimeError(f"the quantizer holds {self.quantizer.ntotal} codes, neither 0 nor nlist = {self.nlist}")
            x = _as_codes(x, self.code_size)
            if x.shape[0] < self.nlist:
                raise RuntimeError(f"{x.shape[0]} training rows for nlist = {self.nlist} centroids")
            km = Kmeans(self.d, self.nlist, niter=self.cp.niter, seed=self.cp.seed)
            km.train(_bits_to_signs(x, self.d))
            self.quantizer.add(_signs_to_bits(km.centroids))
        self.is_trained = True

    def binary_ivf_stats(self) -> dict:
        """Search batches, scan passes (one per 16 queries and 32 results), 64-row tiles of list rows the passes visited
        (include/ise_knn.h, ise_binary_ivf_stats).  Waits for the device."""
        return _counters(_n.lib.ise_binary_ivf_stats, self._h, ("batches", "passes", "tiles_loaded"))

    # -- files
    def _image(self) -> bytes:
        raise NotImplementedError("write_index of an IndexBinaryIVF is not provided: write_index_binary writes binary indexes")

    def _binary_image(self) -> bytes:
        qz = self.quantizer
        lists = [self.get_list(l) for l in range(self.nlist)]
        return serialize_binary_ivf(self.d, self.nlist, int(self.nprobe), qz.reconstruct_n(0, qz.ntotal), lists)

    @classmethod
    def _from_parts(cls, parts, device):
        """The index a parsed "IBwF" image describes (``parse_binary_ivf``); the stored codes are added as they are, in
        the order of their ids, which have to be the insertion numbers 0 .. ntotal - 1."""
        d, nlist, nprobe, centroids, lists = parts
        quantizer = IndexBinaryFlat(d, device)
        if centroids.shape[0]:
            quantizer.add(centroids)
        index = cls(quantizer, d, nlist)
        index.nprobe = nprobe
        ids = np.concatenate([ids for ids, _ in lists]) if lists else np.zeros(0, np.int64)
        if ids.size:
            order = np.argsort(ids, kind="stable")
            if not np.array_equal(ids[order], np.arange(ids.size)):
                raise RuntimeError("an IndexBinaryIVF file whose ids are not the insertion numbers 0 .. ntotal - 1 is not "
                                   "readable")
            codes = np.ascontiguousarray(np.concatenate([codes for _, codes in lists])[order])
            list_no = np.ascontiguousarray(np.repeat(np.arange(nlist, dtype=np.int64), [len(ids) for ids, _ in lists])[order])
            _n.check(_n.lib.ise_binary_ivf_add_host(index._h, codes.ctypes.data, list_no.ctypes.data, codes.shape[0]))
        return index


# ---------------------------------------------------------------- product quantisation (faiss.IndexPQ)
class ProductQuantizer:
    """``index.pq``: the view of an ``IndexPQ``'s (or ``IndexIVFPQ``'s) codec that faiss.ProductQuantizer gives -- ``d``,
    ``M``, ``nbits``, ``dsub``, ``ksub``, ``code_size``, ``cp`` (the clustering parameters of ``train``), ``centroids`` (a
    float32 (M, 256, dsub) copy), ``compute_codes`` and ``decode``.  ``set_centroids`` is an extension, in place of
    Faiss's ``copy_array_to_vector(c, pq.centroids)`` followed by ``index.is_trained = True``."""

    TRAIN_MAX_ROWS = 256 * 256  # Faiss's max_points_per_centroid x ksub

    def __init__(self, index):
        self._index = index
        self.cp = ClusteringParameters(niter=25)
        self.d, self.M, self.nbits = index.d, index.M, 8
        self.dsub, self.ksub, self.code_size = index.d // index.M, 256, index.M

    @property
    def centroids(self) -> np.ndarray:
        out = np.empty((self.M, self.ksub, self.dsub), dtype=np.float32)
        _n.check(self._index._fn("get_centroids_host")(self._index._h, out.ctypes.data))
        return out

    def train(self, x, cp=None) -> None:
        """One ``Kmeans(dsub, 256)`` per sub-quantiser on its columns of ``x`` (at most ``256 * 256`` rows, drawn with a
        generator seeded by ``cp.seed``), ``niter`` and ``seed`` from ``cp`` (``self.cp`` unless given), then
        ``set_centroids``."""
        cp = self.cp if cp is None else cp
        x = _as_rows(x, self.d)
        if x.shape[0] < 256:
            raise RuntimeError(f"{x.shape[0]} training rows for 256 centroids per sub-quantiser")
        if x.shape[0] > self.TRAIN_MAX_ROWS:
            pick = np.random.default_rng(cp.seed).choice(x.shape[0], self.TRAIN_MAX_ROWS, replace=False)
            x = x[np.sort(pick)]
        c = np.empty((self.M, 256, self.dsub), dtype=np.float32)
        for m in range(self.M):
            km = Kmeans(self.dsub, 256, niter=cp.niter, seed=cp.seed)
            km.train(np.ascontiguousarray(x[:, m * self.dsub:(m + 1) * self.dsub]))
            c[m] = km.centroids
        self.set_centroids(c)

    def set_centroids(self, c) -> None:
        """float32 (M, 256, dsub), finite; refused while the index holds rows (their codes belong to the centroids in
        place).  Marks the index trained."""
        c = np.ascontiguousarray(np.asarray(c), dtype=np.float32)
        assert c.shape == (self.M, self.ksub, self.dsub), f"centroids are {(self.M, self.ksub, self.dsub)}, got {c.shape}"
        if not np.isfinite(c).all():
            raise ValueError("a centroid has a NaN or inf entry")
        if self._index.ntotal > 0:
            raise RuntimeError("set_centroids on an index that holds rows: reset() first")
        _n.check(self._index._fn("set_centroids_host")(self._index._h, c.ctypes.data))
        self._index._trained_set()

    def compute_codes(self, x) -> np.ndarray:
        return self._index.sa_encode(x)

    def decode(self, codes) -> np.ndarray:
        return self._index.sa_decode(codes)


def _check_rows(rc: int) -> None:
    """The library's answer to rows with a NaN or inf entry is a ValueError here, as ``IndexIVFFlat.add`` gives."""
    if rc == _n.E_INVALID and b"NaN or inf" in _n.lib.ise_last_error():
        raise ValueError(_n.lib.ise_last_error().decode("utf-8", "replace"))
    _n.check(rc)


class _CodedIndex(_IndexHandle):
    """What ``IndexPQ`` and ``IndexScalarQuantizer`` share above their handles: float32 rows go in, ``code_size`` bytes per
    row are kept (``M`` for a product quantiser, ``d`` for a scalar one), and everything but ``train`` is the same call
    into the family of entry points ``_ABI`` names.  A subclass names its two search entry points outright
    (``_search_host``, ``_search_device``), its ``ntotal`` and what a ``params=`` argument cannot carry."""

    _NO_PARAMS = ""

    def reset(self) -> None:
        """Drop the rows; the codec's state (and ``is_trained``) stay."""
        _n.check(self._fn("reset")(self._h))

    def _require_trained(self, what: str) -> None:
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}.{what} before train")

    # -- build side
    def add(self, x) -> None:
        """Encode and append rows; a row with a NaN or inf entry raises ``ValueError`` and nothing of the call is
        added."""
        self._require_trained("add")
        x = _as_rows(x, self.d)
        _check_rows(self._fn("add_host")(self._h, x.ctypes.data, x.shape[0]))

    def add_torch(self, x) -> None:
        """``add`` from a CUDA float32 tensor on this index's device (no host hop for the rows; the call waits for the
        encoder's verdict on non-finite entries)."""
        import torch

        self._require_trained("add")
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.d
        x = x.contiguous()
        st = torch.cuda.current_stream(x.device).cuda_stream
        with self._lock:
            _check_rows(self._fn("add_device")(self._h, x.data_ptr(), x.shape[0], st))

    def _add_codes(self, codes: np.ndarray) -> None:
        codes = _as_codes(codes, self.code_size)
        _n.check(self._fn("add_codes_host")(self._h, codes.ctypes.data, codes.shape[0]))

    # -- readback and codec
    @property
    def codes(self) -> np.ndarray:
        """uint8 (ntotal, code_size), a copy."""
        out = np.empty((self.ntotal, self.code_size), dtype=np.uint8)
        _n.check(self._fn("codes_host")(self._h, 0, out.shape[0], out.ctypes.data))
        return out

    def reconstruct_n(self, i0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.ntotal - i0 if n is None else n
        out = np.empty((n, self.d), dtype=np.float32)
        _n.check(self._fn("reconstruct_host")(self._h, int(i0), int(n), out.ctypes.data))
        return out

    def reconstruct(self, i: int) -> np.ndarray:
        return self.reconstruct_n(int(i), 1)[0]

    def sa_code_size(self) -> int:
        return self.code_size

    def sa_encode(self, x) -> np.ndarray:
        """uint8 (n, code_size): the codes ``add`` would store."""
        self._require_trained("sa_encode")
        x = _as_rows(x, self.d)
        out = np.empty((x.shape[0], self.code_size), dtype=np.uint8)
        _check_rows(self._fn("encode_host")(self._h, x.ctypes.data, x.shape[0], out.ctypes.data))
        return out

    def sa_decode(self, codes) -> np.ndarray:
        """float32 (n, d): the rows the codes stand for -- the concatenation of the centroids a product quantiser's code
        names; entry j ``fmaf(codes[i, j] + 0.5, s_j, vmin_j)`` for a scalar quantiser."""
        self._require_trained("sa_decode")
        codes = _as_codes(codes, self.code_size)
        out = np.empty((codes.shape[0], self.d), dtype=np.float32)
        _n.check(self._fn("decode_host")(self._h, codes.ctypes.data, codes.shape[0], out.ctypes.data))
        return out

    # -- query side
    def search(self, x, k: int, params=None):
        """(D float32 (nq,k), I int64 (nq,k)), fresh arrays."""
        if params is not None:
            raise NotImplementedError(f"search parameters ({self._NO_PARAMS}) are not provided on {type(self).__name__}")
        self._require_trained("search")
        x = _as_rows(x, self.d)
        k = int(k)
        assert k > 0
        nq = x.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        if nq:
            _n.check(self._search_host(self._h, x.ctypes.data, nq, k, D.ctypes.data, I.ctypes.data))
        return D, I

    def search_torch(self, xq, k: int, params=None):
        """Device-resident search: CUDA float32 (nq,d) in, CUDA (D, I) out, enqueued on the current torch stream (no
        host synchronisation)."""
        import torch

        if params is not None:
            raise NotImplementedError(f"search parameters ({self._NO_PARAMS}) are not provided on {type(self).__name__}")
        self._require_trained("search")
        k = int(k)
        xq, D, I, st = _torch_io(xq, torch.float32, self.d, k, torch.float32)
        nq = xq.shape[0]
        if nq == 0:
            return D, I
        with self._lock:
            _n.check(self._search_device(self._h, xq.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), st))
        return D, I

    def range_search(self, *a, **kw):
        raise NotImplementedError(f"range_search is not provided on {type(self).__name__}")

    def remove_ids(self, *a, **kw):
        raise NotImplementedError(f"remove_ids is not provided on {type(self).__name__}")


class IndexPQ(_CodedIndex):
    """faiss.IndexPQ(d, M, nbits=8, metric): every row is kept as ``M`` bytes, byte m the number of the centroid (of 256,
    trained per sub-quantiser) nearest to the row's m-th sub-vector of ``d / M`` entries in squared L2, the lowest number
    among equals -- for inner-product indexes too, as in Faiss.  ``search`` scores a row from per-query lookup tables
    (asymmetric distance computation): D is the squared L2 distance or inner product of the query and the DECODED row
    (``reconstruct_n``), float32; L2 ascending, inner product descending, ties by ascending id, unfilled slots
    -1 / +-FLT_MAX.

    For a given codebook everything here is determined; Faiss's own training (its seeding, its iteration count) is
    unpinned.  On the device (include/ise_knn.h, ise_pq_*).  Not provided (they raise
    ``NotImplementedError``): ``nbits != 8``, ``range_search``, ``remove_ids``, ``params=``, polysemous search and
    ``IndexIDMap`` over this type."""

    _ABI = "ise_pq"
    TRAIN_MAX_ROWS = ProductQuantizer.TRAIN_MAX_ROWS
    _NO_PARAMS = "selectors, polysemous search"
    _search_host = staticmethod(_n.lib.ise_pq_search_host)
    _search_device = staticmethod(_n.lib.ise_pq_search_device)
    ntotal = _ntotal_property(_n.lib.ise_pq_info, 8, 5)

    def __init__(self, d: int, M: int, nbits: int = 8, metric: int = METRIC_L2, device: int | None = None):
        if int(nbits) != 8:
            raise NotImplementedError(f"IndexPQ with nbits = {nbits}: only 8-bit sub-quantisers are provided")
        self.d, self.M = int(d), int(M)
        self.metric_type = int(metric)
        self.code_size = self.M
        self.is_trained = False
        self.cp = ClusteringParameters(niter=25)
        self.device = _default_device() if device is None else int(device)
        self._h = ctypes.c_void_p()
        self._lock = threading.Lock()
        _n.check(_n.lib.ise_pq_create(ctypes.byref(self._h), self.d, self.M, 8, self.metric_type, self.device))
        self.pq = ProductQuantizer(self)
        self.pq.cp = self.cp

    def _trained_set(self) -> None:  # ProductQuantizer.set_centroids has set the codebook
        self.is_trained = True

    @classmethod
    def _from_parts(cls, parts, device, add_codes: bool = True):
        """The index a parsed "IxPq" image describes (``parse_pq``); the stored codes are added as they are."""
        index = cls(parts.d, parts.M, parts.nbits, parts.metric, device)
        index.pq.set_centroids(parts.centroids)
        if add_codes:
            index._add_codes(parts.codes)
        return index

    def _image(self) -> bytes:
        return serialize_pq(self.d, self.metric_type, self.pq.centroids, self.codes)

    def pq_stats(self) -> dict:
        """Search batches, scan passes (one per QT(M) queries and 32 results), table builds (one per 64 queries), bytes
        of code storage allocated on the device (include/ise_knn.h, ise_pq_stats)."""
        return _counters(_n.lib.ise_pq_stats, self._h, ("search_batches", "scan_passes", "table_builds", "code_bytes"))

    # -- build side
    def train(self, x) -> None:
        """A no-op when trained.  Otherwise one ``Kmeans(dsub, 256)`` per sub-quantiser on its columns of ``x`` (at most
        ``256 * 256`` rows, drawn with a generator seeded by ``cp.seed``), ``niter`` and ``seed`` from ``self.cp`` -- L2
        k-means for inner-product indexes too, as in Faiss.  ``cp.niter`` defaults to 25, Faiss's default for a product
        quantiser's clustering as restated from memory: unpinned, like the seeding of ``Kmeans`` itself."""
        if self.is_trained:
            return
        self.pq.train(x, self.cp)


# ---------------------------------------------------------------- scalar quantisation (faiss.IndexScalarQuantizer)
class ScalarQuantizer:
    """``index.sq``: the view of an ``IndexScalarQuantizer``'s (or ``IndexIVFScalarQuantizer``'s) codec that faiss.ScalarQuantizer gives -- ``d``, ``qtype``,
    ``code_size``, ``trained`` (a float32 copy: ``[vmin_0.., vdiff_0..]``, or ``[vmin, vdiff]`` for the uniform type),
    ``rangestat`` / ``rangestat_arg`` (only Faiss's ``RS_minmax`` with argument 0 trains), ``compute_codes`` and
    ``decode``.  The constants carry Faiss's enum values as restated from memory (unpinned, like the file layouts).
    ``set_trained`` is an extension, named like ``ProductQuantizer.set_centroids``."""

    QT_8bit, QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16, QT_8bit_direct, QT_6bit, QT_bf16, \
        QT_8bit_direct_signed = range(9)
    RS_minmax, RS_meanstd, RS_quantiles, RS_optim = range(4)
    _PROVIDED = (0, 2)

    def __init__(self, index):
        self._index = index
        self.d, self.qtype, self.code_size = index.d, index.qtype, index.d
        self.rangestat, self.rangestat_arg = self.RS_minmax, 0.0

    @property
    def _trained_size(self) -> int:
        return 2 if self.qtype == self.QT_8bit_uniform else 2 * self.d

    @property
    def trained(self) -> np.ndarray:
        if not self._index._codec_trained():
            return np.zeros(0, dtype=np.float32)
        out = np.empty(self._trained_size, dtype=np.float32)
        _n.check(self._index._fn("get_trained_host")(self._index._h, out.ctypes.data))
        return out

    def train(self, x) -> None:
        """Nothing when the state is set.  Otherwise vmin = the minimum and vdiff = maximum - minimum of the training
        rows, per dimension or (uniform) over everything: Faiss's ``RS_minmax`` with ``rangestat_arg = 0``; any other
        setting of ``rangestat`` / ``rangestat_arg`` raises ``NotImplementedError``.  A NaN or inf entry raises
        ``ValueError``."""
        if self._index._codec_trained():
            return
        if self.rangestat != self.RS_minmax or float(self.rangestat_arg) != 0.0:
            raise NotImplementedError("only rangestat = RS_minmax with rangestat_arg = 0 is provided")
        x = _as_rows(x, self.d)
        if x.shape[0] == 0:
            raise RuntimeError("no training rows")
        if not np.isfinite(x).all():
            raise ValueError("a training row has a NaN or inf entry")
        if self.qtype == self.QT_8bit_uniform:
            vmin, vmax = np.float32(x.min()), np.float32(x.max())
            t = np.array([vmin, vmax - vmin], dtype=np.float32)
        else:
            vmin = x.min(axis=0)
            t = np.concatenate([vmin, x.max(axis=0) - vmin]).astype(np.float32)
        if not np.isfinite(t).all():
            raise ValueError("the range of the training rows overflows float32")
        self.set_trained(t)

    def set_trained(self, t) -> None:
        """float32 ``[vmin.., vdiff..]``, finite, no negative ``vdiff``; refused while the index holds rows (their codes
        belong to the state in place).  Marks the index trained."""
        t = np.ascontiguousarray(np.asarray(t), dtype=np.float32).reshape(-1)
        assert t.size == self._trained_size, f"the trained vector holds {self._trained_size} floats, got {t.size}"
        if not np.isfinite(t).all():
            raise ValueError("the trained state has a NaN or inf entry")
        if (t[t.size // 2:] < 0).any():
            raise ValueError("the trained state has a negative vdiff")
        if self._index.ntotal > 0:
            raise RuntimeError("set_trained on an index that holds rows: reset() first")
        _n.check(self._index._fn("set_trained_host")(self._index._h, t.ctypes.data))
        self._index._trained_set()

    def compute_codes(self, x) -> np.ndarray:
        return self._index.sa_encode(x)

    def decode(self, codes) -> np.ndarray:
        return self._index.sa_decode(codes)


class IndexScalarQuantizer(_CodedIndex):
    """faiss.IndexScalarQuantizer(d, qtype, metric) for ``ScalarQuantizer.QT_8bit`` (a minimum and a range per dimension)
    and ``QT_8bit_uniform`` (one of each for all): every row is kept as ``d`` bytes, byte j =
    ``min(255, max(0, floor((x_j - vmin_j) / s_j)))`` with the step ``s_j = vdiff_j / 255`` (0 where the step is 0), all in
    float32 and for both metrics; it decodes to ``fmaf(c_j + 0.5, s_j, vmin_j)``.  ``search`` scores the query against
    the DECODED row (``reconstruct_n``): D is their squared L2 distance or inner product in float32, exact on integer
    data and within ``1e-4 * max(1, |D|)`` of the float64 value where the data fill their trained range (min/max
    training on the added rows, no outlier that stretches it; otherwise the error is bounded by the weights' sum, not
    by D: include/ise_knn.h); L2 ascending, inner product descending, ties
    by ascending id, unfilled slots -1 / +-FLT_MAX; a query with a NaN or inf entry gets padding only.

    On the device (include/ise_knn.h, ise_sq_*).  Not provided (they raise ``NotImplementedError``):
    the other quantiser types, range statistics other than ``RS_minmax`` with argument 0, ``range_search``,
    ``remove_ids``, ``params=`` and ``IndexIDMap`` over this type."""

    _ABI = "ise_sq"
    _NO_PARAMS = "selectors"
    _search_host = staticmethod(_n.lib.ise_sq_search_host)
    _search_device = staticmethod(_n.lib.ise_sq_search_device)
    ntotal = _ntotal_property(_n.lib.ise_sq_info, 7, 4)

    def __init__(self, d: int, qtype: int = ScalarQuantizer.QT_8bit, metric: int = METRIC_L2, device: int | None = None):
        if int(qtype) not in ScalarQuantizer._PROVIDED:
            raise NotImplementedError(f"IndexScalarQuantizer with qtype = {qtype}: only QT_8bit and QT_8bit_uniform are "
                                      "provided (IndexFlat(storage=\"bf16\") is the 2-byte route)")
        self.d, self.qtype = int(d), int(qtype)
        self.metric_type = int(metric)
        self.code_size = self.d
        self.is_trained = False
        self.device = _default_device() if device is None else int(device)
        self._h = ctypes.c_void_p()
        self._lock = threading.Lock()
        _n.check(_n.lib.ise_sq_create(ctypes.byref(self._h), self.d, self.qtype, self.metric_type, self.device))
        self.sq = ScalarQuantizer(self)

    def _codec_trained(self) -> bool:  # what ``sq`` asks its owner
        return self.is_trained

    def _trained_set(self) -> None:  # ScalarQuantizer.set_trained has set the state
        self.is_trained = True

    @classmethod
    def _from_parts(cls, parts, device, add_codes: bool = True):
        """The index a parsed "IxSQ" image describes (``parse_sq``); the stored codes are added as they are."""
        index = cls(parts.d, parts.qtype, parts.metric, device)
        index.sq.rangestat, index.sq.rangestat_arg = parts.rangestat, parts.rangestat_arg
        index.sq.set_trained(parts.trained)
        if add_codes:
            index._add_codes(parts.codes)
        return index

    def _image(self) -> bytes:
        self._require_trained("write_index")
        return serialize_sq(self.d, self.metric_type, self.qtype, self.sq.trained, self.codes, self.sq.rangestat,
                            self.sq.rangestat_arg)

    def sq_stats(self) -> dict:
        """Search batches, scan passes (one per QT(d) queries and 32 results), bytes of code storage allocated on the
        device (include/ise_knn.h, ise_sq_stats)."""
        return _counters(_n.lib.ise_sq_stats, self._h, ("search_batches", "scan_passes", "code_bytes"))

    def train(self, x) -> None:
        """A no-op when trained; otherwise ``sq.train``: vmin / vdiff from the rows' minimum and maximum."""
        self.sq.train(x)


# ---------------------------------------------------------------- inverted lists over 8-bit rows (faiss.IndexIVFScalarQuantizer)
class IndexIVFScalarQuantizer(_IndexIVF):
    """faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, qtype, metric, by_residual) for ``ScalarQuantizer.QT_8bit`` and
    ``QT_8bit_uniform`` with ``by_residual=False``: ``IndexIVFFlat``'s lists holding ``IndexScalarQuantizer``'s rows.  The
    codec is that index's -- the same trained state, code bytes and decoded rows for the same ``sq.trained``.  ``add``
    files row i under ``quantizer.search(x, 1)[1][i]``; ``search`` visits the ``nprobe`` lists nearest each query and
    returns the exact k best among their rows by the score against the DECODED row: D has the bits
    ``IndexScalarQuantizer.search`` reports for the same (query, row) pair, ties go by ascending id, unfilled slots are
    -1 / +-FLT_MAX, a query with a NaN or inf entry gets padding only.  With ``nprobe == nlist`` the result is
    ``IndexScalarQuantizer.search`` itself.

    ``by_residual=True`` -- Faiss's default, and this constructor's -- raises ``NotImplementedError``: a residual code
    makes the scan's operand differ per (query, list), which the byte-row pass does not provide.  Pass
    ``by_residual=False``.

    On the device (include/ise_knn.h, ise_ivfsq_*): ``add`` encodes into a pending buffer, the first
    search after an ``add`` rebuilds the lists.  Not provided (they raise ``NotImplementedError``): the other quantiser
    types, ``range_search``, ``remove_ids``, ``params=`` and ``IndexIDMap`` over this type."""

    _ABI = "ise_ivfsq"
    _search_device = staticmethod(_n.lib.ise_ivfsq_search_device)
    _search_host = staticmethod(_n.lib.ise_ivfsq_search_host)
    _LIST_DTYPE = np.uint8
    _ENCODES = True
    ntotal = _ntotal_property(_n.lib.ise_ivfsq_info, 8, 5)

    def __init__(self, quantizer: IndexFlat, d: int, nlist: int, qtype: int = ScalarQuantizer.QT_8bit, metric: int = METRIC_L2,
                 by_residual: bool = True):
        if by_residual:
            raise NotImplementedError("IndexIVFScalarQuantizer with by_residual = True (Faiss's default) is not provided: "
                                      "pass by_residual=False (codes of the rows themselves, not of their residuals)")
        if int(qtype) not in ScalarQuantizer._PROVIDED:
            raise NotImplementedError(f"IndexIVFScalarQuantizer with qtype = {qtype}: only QT_8bit and QT_8bit_uniform are "
                                      "provided")
        self._init_ivf(quantizer, d, nlist, metric)
        self.qtype = int(qtype)
        self.by_residual = False
        self.code_size = self.d
        self._sq_trained = False
        self._codec = None
        _n.check(_n.lib.ise_ivfsq_create(ctypes.byref(self._h), self.d, self.qtype, self.metric_type, self.nlist, self.device))
        self.sq = ScalarQuantizer(self)

    @property
    def is_trained(self) -> bool:
        return self._sq_trained and self.quantizer.ntotal == self.nlist

    def _codec_trained(self) -> bool:  # what ``sq`` asks its owner (the index is trained with its quantiser only)
        return self._sq_trained

    def _trained_set(self) -> None:  # ScalarQuantizer.set_trained has set the state
        self._sq_trained = True
        self._codec = None

    # -- build side
    def train(self, x) -> None:
        """The quantiser's k-means as ``IndexIVFFlat.train`` (nothing when it holds ``nlist`` centroids), then vmin /
        vdiff from the rows' minimum and maximum as ``IndexScalarQuantizer.train`` (nothing when the state is set)."""
        self._train_quantizer(x)
        self.sq.train(x)

    def _add_codes(self, codes: np.ndarray, lists: np.ndarray) -> None:
        codes = _as_codes(codes, self.d)
        lists = np.ascontiguousarray(lists, dtype=np.int64).reshape(-1)
        assert lists.size == codes.shape[0], "one list number per code row"
        _n.check(_n.lib.ise_ivfsq_add_codes_host(self._h, codes.ctypes.data, lists.ctypes.data, codes.shape[0]))

    # -- the codec: an empty IndexScalarQuantizer with the same trained state (ise_ivfsq_* has no encode / decode entry)
    def _codec_index(self):
        if not self._sq_trained:
            raise RuntimeError("IndexIVFScalarQuantizer's codec before train")
        if self._codec is None:
            codec = IndexScalarQuantizer(self.d, self.qtype, self.metric_type, self.device)
            codec.sq.set_trained(self.sq.trained)
            self._codec = codec
        return self._codec

    def sa_code_size(self) -> int:
        return self.code_size

    def sa_encode(self, x) -> np.ndarray:
        """uint8 (n, d): the codes ``add`` would store."""
        return self._codec_index().sa_encode(x)

    def sa_decode(self, codes) -> np.ndarray:
        return self._codec_index().sa_decode(codes)

    def ivfsq_stats(self) -> dict:
        """Search batches, scan passes (one per QT(d) queries and 32 results), 64-row tiles of list rows the passes
        visited (include/ise_knn.h, ise_ivfsq_stats).  Waits for the device."""
        return _counters(_n.lib.ise_ivfsq_stats, self._h, ("batches", "passes", "tiles_loaded"))

    # -- files
    def _image(self) -> bytes:
        self._require_trained("write_index")
        qz = self.quantizer
        lists = [self.get_list(l) for l in range(self.nlist)]
        return serialize_ivfsq(self.d, self.metric_type, self.nlist, int(self.nprobe), qz.metric_type,
                               qz.reconstruct_n(0, qz.ntotal), self.qtype, self.sq.trained, lists, self.sq.rangestat,
                               self.sq.rangestat_arg, False)

    @classmethod
    def _from_parts(cls, parts, device):
        """The index a parsed "IwSq" image describes (``parse_ivfsq``); the stored codes are added as they are, in the
        order of their ids, which have to be the insertion numbers 0 .. ntotal - 1."""
        d, metric, nlist, nprobe, qmetric, centroids, qtype, trained, lists, rangestat, rangestat_arg, by_residual = parts
        if by_residual:
            raise NotImplementedError("read_index of an IndexIVFScalarQuantizer file with by_residual = true is not provided")
        quantizer = IndexFlat(d, qmetric, device)
        if centroids.shape[0]:
            quantizer.add(centroids)
        index = cls(quantizer, d, nlist, qtype, metric, by_residual=False)
        index.nprobe = nprobe
        index.sq.rangestat, index.sq.rangestat_arg = rangestat, rangestat_arg
        index.sq.set_trained(trained)
        ids = np.concatenate([ids for ids, _ in lists]) if lists else np.zeros(0, np.int64)
        if ids.size:
            order = np.argsort(ids, kind="stable")
            if not np.array_equal(ids[order], np.arange(ids.size)):
                raise RuntimeError("an IndexIVFScalarQuantizer file whose ids are not the insertion numbers 0 .. ntotal - 1 "
                                   "is not readable")
            codes = np.concatenate([codes for _, codes in lists])
            list_no = np.repeat(np.arange(nlist, dtype=np.int64), [len(ids) for ids, _ in lists])
            index._add_codes(codes[order], list_no[order])
        return index


# ---------------------------------------------------------------- inverted lists over product-quantiser codes (faiss.IndexIVFPQ)
def _ivfpq_args(quantizer=None, d=0, nlist=0, M=0, nbits=8, metric=METRIC_L2, by_residual=True):
    """``IndexIVFPQ``'s constructor arguments, by position or by name."""
    return quantizer, d, nlist, M, nbits, metric, by_residual


class IndexIVFPQ(_IndexIVF):
    """faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits=8, metric=METRIC_L2, by_residual=False) with 8-bit sub-quantisers:
    ``IndexIVFFlat``'s lists holding ``IndexPQ``'s code rows -- the reference's "cell-probe" index (backend/utils.py:311-325)
    over codes of the rows themselves.  The codec is ``IndexPQ``'s: the same codebook ``[M][256][d / M]``, code bytes and
    decoded rows for the same ``pq.centroids``.  ``add`` files row i under ``quantizer.search(x, 1)[1][i]``; ``search``
    visits the ``nprobe`` lists nearest each query and returns the exact k best among their rows by the table-lookup
    score: D has the bits ``IndexPQ.search`` reports for the same (query, row) pair and codebook, ties go by ascending id,
    unfilled slots are -1 / +-FLT_MAX, a query with a NaN or inf entry gets padding only.  With ``nprobe == nlist`` the
    result is ``IndexPQ.search`` itself.

    ``by_residual=True`` -- Faiss's default, and this constructor's -- raises ``NotImplementedError`` before anything else
    is looked at, and so does assigning it afterwards: a residual code makes the lookup tables differ per (query, list),
    which needs a table builder and a scan of their own.  Pass ``by_residual=False``.  (The constructor
    takes its arguments as ``*a, **kw``, the signature it had while the type was not provided; they are the ones above.)

    ``cp`` holds the clustering parameters of the coarse quantiser (``niter`` 10), ``pq.cp`` those of the codebook
    (``niter`` 25): the same rows, ``pq.cp`` and seed give ``IndexPQ.train``'s codebook bit for bit.

    On the device (include/ise_knn.h, ise_ivfpq_*): ``add`` encodes into a pending buffer, the first search
    after an ``add`` rebuilds the lists.  Not provided (they raise ``NotImplementedError``): ``nbits != 8``, residual
    codes, ``range_search``, ``remove_ids``, ``params=``, ``add_with_ids`` and ``IndexIDMap`` over this type."""

    _ABI = "ise_ivfpq"
    _search_device = staticmethod(_n.lib.ise_ivfpq_search_device)
    _search_host = staticmethod(_n.lib.ise_ivfpq_search_host)
    _LIST_DTYPE = np.uint8
    _ENCODES = True
    ntotal = _ntotal_property(_n.lib.ise_ivfpq_info, 9, 6)

    def __init__(self, *a, **kw):
        quantizer, d, nlist, M, nbits, metric, by_residual = _ivfpq_args(*a, **kw)
        if by_residual:
            raise NotImplementedError("IndexIVFPQ with by_residual = True (Faiss's default) is not provided: pass "
                                      "by_residual=False (codes of the rows themselves, not of their residuals)")
        if int(nbits) != 8:
            raise NotImplementedError(f"IndexIVFPQ with nbits = {nbits}: only 8-bit sub-quantisers are provided")
        self.M = int(M)
        assert 1 <= self.M <= _n.PQ_MAX_M and int(d) % self.M == 0, f"1 <= M <= {_n.PQ_MAX_M}, and M divides d"
        self._init_ivf(quantizer, d, nlist, metric, list_width=self.M)
        self.code_size = self.M
        self._pq_trained = False
        self._codec = None
        _n.check(_n.lib.ise_ivfpq_create(ctypes.byref(self._h), self.d, self.M, 8, self.metric_type, self.nlist, self.device))
        self.pq = ProductQuantizer(self)

    @property
    def by_residual(self) -> bool:
        return False

    @by_residual.setter
    def by_residual(self, value) -> None:
        if value:
            raise NotImplementedError("IndexIVFPQ with by_residual = True is not provided (codes of the rows themselves only)")

    @property
    def is_trained(self) -> bool:
        return self._pq_trained and self.quantizer.ntotal == self.nlist

    def _codec_trained(self) -> bool:  # the index is trained with its quantiser only; the lists need the codec alone
        return self._pq_trained

    def _trained_set(self) -> None:  # ProductQuantizer.set_centroids has set the codebook
        self._pq_trained = True
        self._codec = None

    # -- build side
    def train(self, x) -> None:
        """The quantiser's k-means as ``IndexIVFFlat.train`` (nothing when it holds ``nlist`` centroids), then the
        codebook on the rows themselves as ``IndexPQ.train`` with ``pq.cp`` (nothing when the centroids are set)."""
        self._train_quantizer(x)
        if not self._pq_trained:
            self.pq.train(x)

    def _add_codes(self, codes: np.ndarray, lists: np.ndarray) -> None:
        codes = _as_codes(codes, self.M)
        lists = np.ascontiguousarray(lists, dtype=np.int64).reshape(-1)
        assert lists.size == codes.shape[0], "one list number per code row"
        _n.check(_n.lib.ise_ivfpq_add_codes_host(self._h, codes.ctypes.data, lists.ctypes.data, codes.shape[0]))

    # -- the codec: an empty IndexPQ with the same centroids (ise_ivfpq_* has no encode / decode entry)
    def _codec_index(self):
        if not self._pq_trained:
            raise RuntimeError("IndexIVFPQ's codec before train")
        if self._codec is None:
            codec = IndexPQ(self.d, self.M, 8, self.metric_type, self.device)
            codec.pq.set_centroids(self.pq.centroids)
            self._codec = codec
        return self._codec

    def sa_code_size(self) -> int:
        return self.code_size

    def sa_encode(self, x) -> np.ndarray:
        """uint8 (n, M): the codes ``add`` would store."""
        return self._codec_index().sa_encode(x)

    def sa_decode(self, codes) -> np.ndarray:
        return self._codec_index().sa_decode(codes)

    def ivfpq_stats(self) -> dict:
        """Search batches, scan passes (one per QT(M) queries and 32 results), 64-row tiles of list rows the passes
        visited, table builds (one per 64 queries) (include/ise_knn.h, ise_ivfpq_stats).  Waits for the device."""
        return _counters(_n.lib.ise_ivfpq_stats, self._h, ("batches", "passes", "tiles_loaded", "table_builds"))

    # -- files
    def _image(self) -> bytes:
        self._require_trained("write_index")
        qz = self.quantizer
        lists = [self.get_list(l) for l in range(self.nlist)]
        return serialize_ivfpq(self.d, self.metric_type, self.nlist, int(self.nprobe), qz.metric_type,
                               qz.reconstruct_n(0, qz.ntotal), self.pq.centroids, lists, False)

    def _add_lists(self, lists) -> None:
        """The stored codes of a parsed image, added as they are, in the order of their ids, which have to be the
        insertion numbers 0 .. ntotal - 1."""
        ids = np.concatenate([ids for ids, _ in lists]) if lists else np.zeros(0, np.int64)
        if ids.size:
            order = np.argsort(ids, kind="stable")
            if not np.array_equal(ids[order], np.arange(ids.size)):
                raise RuntimeError("an IndexIVFPQ file whose ids are not the insertion numbers 0 .. ntotal - 1 is not readable")
            codes = np.concatenate([codes for _, codes in lists])
            list_no = np.repeat(np.arange(self.nlist, dtype=np.int64), [len(ids) for ids, _ in lists])
            self._add_codes(codes[order], list_no[order])

    @classmethod
    def _from_parts(cls, parts, device, add_codes: bool = True):
        """The index a parsed "IwPQ" image describes (``parse_ivfpq``)."""
        if parts.by_residual:
            raise NotImplementedError("read_index of an IndexIVFPQ file with by_residual = true is not provided")
        quantizer = IndexFlat(parts.d, parts.qmetric, device)
        if parts.centroids.shape[0]:
            quantizer.add(parts.centroids)
        index = cls(quantizer, parts.d, parts.nlist, parts.M, parts.nbits, parts.metric, by_residual=False)
        index.nprobe = parts.nprobe
        index.pq.set_centroids(parts.pq_centroids)
        if add_codes:
            index._add_lists(parts.lists)
        return index


# ---------------------------------------------------------------- exact re-ranking (faiss.IndexRefine / IndexRefineFlat)
class IndexRefine:
    """faiss.IndexRefine(base_index, refine_index): ``search`` asks ``base_index`` -- an ``IndexFlat`` of either storage,
    an ``IndexPQ``, an ``IndexScalarQuantizer``, an ``IndexIVFFlat``, an ``IndexIVFScalarQuantizer`` or an ``IndexIVFPQ`` -- for
    ``int(k * k_factor)`` labels and returns the k best of them by the exact
    score ``refine_index`` (a float32 ``IndexFlat`` that holds the same rows) computes: D has the bits
    ``refine_index.search`` reports for the same (query, row) pair, ties go by ascending id, unfilled slots are
    -1 / +-FLT_MAX; -1 labels of the base are ignored.  With ``k * k_factor >= ntotal`` the result is
    ``refine_index.search`` itself.  ``k_factor`` defaults to 1 as in Faiss: the base's own id set in exact order.

    The re-ranking is one gather-and-score pass over the candidate rows and one sort per query on the device
    (``IndexFlat.search_subset``, csrc/ise_subset.hpp).  Not provided (they raise
    ``NotImplementedError``): ``range_search``, ``remove_ids`` and ``IndexIDMap`` over this type."""

    def __init__(self, base_index, refine_index):
        assert isinstance(base_index, (IndexFlat, IndexPQ, IndexScalarQuantizer, _IndexIVF, IndexPreTransform)), \
            "the base index is an IndexFlat, an IndexPQ, an IndexScalarQuantizer, an IndexIVFFlat, an IndexIVFScalarQuantizer, " \
            "an IndexIVFPQ or an IndexPreTransform over one of them"
        assert base_index.ntotal == 0, f"{type(self).__name__} wraps an empty index (Faiss: index is empty on input)"
        assert isinstance(refine_index, IndexFlat) and refine_index.storage == "f32", \
            "the refine index is a float32 IndexFlat"
        assert refine_index.d == base_index.d, f"dimension mismatch: base d={base_index.d}, refine d={refine_index.d}"
        assert refine_index.metric_type == base_index.metric_type, "the two indexes have different metrics"
        assert refine_index.device == base_index.device, "the two indexes live on different devices"
        assert refine_index.ntotal == base_index.ntotal, "the two indexes hold different numbers of rows"
        self.base_index = base_index
        self.refine_index = refine_index
        self.k_factor = 1.0
        self.d = base_index.d
        self.metric_type = base_index.metric_type
        self.device = base_index.device

    is_trained = property(lambda self: self.base_index.is_trained)
    ntotal = property(lambda self: self.refine_index.ntotal)

    # -- build side
    def train(self, x) -> None:
        if hasattr(self.base_index, "train"):  # an IndexFlat has nothing to train
            self.base_index.train(x)

    def add(self, x) -> None:
        """To the base first, then to the refine index: if the base refuses the rows (a NaN row on an ``IndexPQ`` base
        raises ``ValueError``) nothing is added anywhere."""
        x = _as_rows(x, self.d)
        self.base_index.add(x)
        self.refine_index.add(x)

    def add_torch(self, x) -> None:
        self.base_index.add_torch(x)
        self.refine_index.add_torch(x)

    def reset(self) -> None:
        self.base_index.reset()
        self.refine_index.reset()

    def reconstruct_n(self, i0: int = 0, n: int | None = None) -> np.ndarray:
        return self.refine_index.reconstruct_n(i0, n)

    def reconstruct(self, i: int) -> np.ndarray:
        return self.refine_index.reconstruct_n(int(i), 1)[0]

    # -- query side
    def _plan(self, k: int, params):
        """-> (k_base, the base index's params) of one search call, after the checks both forms share."""
        k_factor, base_params = self.k_factor, None
        if params is not None:
            if not isinstance(params, IndexRefineSearchParameters):
                raise TypeError(f"params must be an IndexRefineSearchParameters, not {type(params).__name__}")
            k_factor, base_params = params.k_factor, params.base_index_params
        if not float(k_factor) >= 1.0:
            raise ValueError(f"k_factor must be >= 1, got {k_factor!r}")
        k_base = int(k * k_factor)
        if k_base > _n.MAX_K:
            raise ValueError(f"k * k_factor = {k_base} candidates per query: at most {_n.MAX_K}")
        if self.base_index.ntotal != self.refine_index.ntotal:
            raise RuntimeError(f"the base index holds {self.base_index.ntotal} rows, the refine index "
                               f"{self.refine_index.ntotal}: rows were added to one of them alone")
        return k_base, base_params

    def search(self, x, k: int, params=None):
        """(D float32 (nq,k), I int64 (nq,k)), fresh arrays.  ``params=IndexRefineSearchParameters(k_factor=...,
        base_index_params=...)`` replaces ``self.k_factor`` for this call."""
        k = int(k)
        assert k > 0
        k_base, base_params = self._plan(k, params)
        x = _as_rows(x, self.d)
        labels = self.base_index.search(x, k_base, params=base_params)[1]
        return self.refine_index.search_subset(x, k, labels)

    def search_torch(self, xq, k: int, params=None):
        """Device-resident search: the base index's ``search_torch`` and the re-ranking are enqueued on the current
        torch stream; this method makes no host synchronisation of its own."""
        k = int(k)
        assert k > 0
        k_base, base_params = self._plan(k, params)
        labels = self.base_index.search_torch(xq, k_base, params=base_params)[1]
        return self.refine_index.search_subset_torch(xq, k, labels)

    def _image(self) -> bytes:
        base = self.base_index
        if isinstance(base, (_CodedIndex, IndexIVFPQ)):
            image = base._image()
        elif type(base) in (IndexFlat, IndexFlatL2, IndexFlatIP) and base.storage == "f32":
            image = _flat_image(base)
        else:
            raise NotImplementedError(f"write_index of an IndexRefine over {type(base).__name__} is not provided "
                                      "(float32 IndexFlat, IndexPQ, IndexScalarQuantizer and IndexIVFPQ bases are)")
        rf = self.refine_index
        return serialize_refine(image, self.d, self.metric_type, rf.reconstruct_n(0, rf.ntotal), self.k_factor)

    def range_search(self, *a, **kw):
        raise NotImplementedError("range_search is not provided on IndexRefine")

    def remove_ids(self, *a, **kw):
        raise NotImplementedError("remove_ids is not provided on IndexRefine")


class IndexRefineFlat(IndexRefine):
    """faiss.IndexRefineFlat(base_index): ``IndexRefine`` with a float32 ``IndexFlat`` of its own, of the base's ``d``
    and metric and on the base's device."""

    def __init__(self, base_index):
        super().__init__(base_index, IndexFlat(base_index.d, base_index.metric_type, device=base_index.device))

    @classmethod
    def _from_parts(cls, parts, device):
        """The index a parsed "IxRF" image describes (``parse_refine``); each side gets what is stored for it."""
        kind, stored = parts.base_kind, parts.base
        if kind == "flat":
            base = IndexFlat(parts.d, stored.metric, device)
        else:
            base = {"pq": IndexPQ, "sq": IndexScalarQuantizer, "ivfpq": IndexIVFPQ}[kind]._from_parts(stored, device, add_codes=False)
        index = cls(base)
        index.k_factor = parts.k_factor
        if parts.xb.shape[0]:
            if kind == "flat":
                base.add(stored.xb)
            elif kind == "ivfpq":
                base._add_lists(stored.lists)
            else:
                base._add_codes(stored.codes)
            index.refine_index.add(parts.xb)
        return index


# ---------------------------------------------------------------- vector transforms (faiss.VectorTransform, IndexPreTransform)
_U32 = 2.0 ** -24  # the unit roundoff of float32
# Rows that are orthonormal in exact arithmetic and then stored as float32: every entry moves by at most u |a_jk|, so
# a dot product of two stored rows (taken in float64) moves by at most sum_k (2 u + u^2) |a_ik a_jk| <= 2 u + u^2
# (Cauchy-Schwarz over unit rows).  4 u is twice that: the other half is for the float64 arithmetic (QR, eigh, SVD,
# a product of two rotations: d 2^-53 per entry) that made the rows.
_ORTHONORMAL_TOL = 4 * _U32


class _LinearHandle(_IndexHandle):
    """An ``ise_linear`` handle: the matrix as the kernels load it, on one device; immutable."""

    _ABI = "ise_linear"

    def __init__(self, A: np.ndarray, b, device: int):
        self.device = int(device)
        self._h = ctypes.c_void_p()
        d_out, d_in = A.shape
        _n.check(_n.lib.ise_linear_create(ctypes.byref(self._h), d_in, d_out, A.ctypes.data,
                                          None if b is None else b.ctypes.data, self.device))


class VectorTransform:
    """faiss.VectorTransform: ``d_in`` -> ``d_out``; ``train(x)``, ``apply(x)`` (numpy in, a fresh numpy array out;
    ``apply_py`` is the same), ``apply_torch(x)`` (CUDA float32 in and out, enqueued on the current torch stream, no host
    synchronisation), ``reverse_transform(y)`` where the transform has one."""

    _FOURCC = b""

    def __init__(self, d_in: int = 0, d_out: int = 0):
        self.d_in, self.d_out = int(d_in), int(d_out)
        self.is_trained = True

    def train(self, x) -> None:
        pass

    def _require_trained(self, what: str) -> None:
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}.{what} before train")

    def apply(self, x) -> np.ndarray:
        raise NotImplementedError

    def apply_py(self, x) -> np.ndarray:
        return self.apply(x)

    def apply_torch(self, x):
        raise NotImplementedError

    def reverse_transform(self, y) -> np.ndarray:
        raise RuntimeError(f"reverse_transform is not provided on {type(self).__name__}")

    def _record_body(self) -> bytes:
        return b""

    def _record(self) -> bytes:
        """This transform as a record of an "IxPT" file."""
        return self._FOURCC + self._record_body() + _VT_TAIL.pack(self.d_in, self.d_out, 1 if self.is_trained else 0)


class LinearTransform(VectorTransform):
    """faiss.LinearTransform(d_in, d_out, have_bias): y = A x + b with ``A`` float32 (d_out, d_in) and ``b`` float32
    (d_out,).  Assigning ``A`` (which also marks the transform trained) or ``b`` drops the device handle; the next
    ``apply`` / ``apply_torch`` makes it again (include/ise_knn.h, ise_linear_*), so everything else here needs no GPU.
    The bits of y are a function of ``d_in`` alone: a row transforms to the same float32 values alone
    or in a batch of a million.  ``d_in`` and ``d_out`` are at most 4096."""

    _FOURCC = b"LTra"

    def __init__(self, d_in: int = 0, d_out: int = 0, have_bias: bool = False):
        super().__init__(d_in, d_out)
        self.have_bias = bool(have_bias)
        self.is_trained = False
        self.is_orthonormal = False
        self._A = np.zeros((0, 0), dtype=np.float32)
        self._b = np.zeros(0, dtype=np.float32)
        self._lh = None
        self._hlock = threading.Lock()

    @property
    def A(self) -> np.ndarray:
        return self._A

    @A.setter
    def A(self, A) -> None:
        A = np.ascontiguousarray(np.asarray(A), dtype=np.float32)
        assert A.shape == (self.d_out, self.d_in), f"A is (d_out, d_in) = ({self.d_out}, {self.d_in}), got {A.shape}"
        self._A, self._lh = A, None
        self.is_trained = True
        self.is_orthonormal = False

    @property
    def b(self) -> np.ndarray:
        return self._b

    @b.setter
    def b(self, b) -> None:
        b = np.ascontiguousarray(np.asarray(b), dtype=np.float32).reshape(-1)
        assert b.size in (0, self.d_out), f"b holds d_out = {self.d_out} entries, got {b.size}"
        self._b, self._lh = b, None
        self.have_bias = b.size > 0

    def set_is_orthonormal(self) -> None:
        """``is_orthonormal``: d_out <= d_in and A A^T (in float64) is the identity within 4 * 2^-24 per entry (the
        derivation stands at ``_ORTHONORMAL_TOL``)."""
        self._require_trained("set_is_orthonormal")
        if self.d_out > self.d_in:
            self.is_orthonormal = False
            return
        A = self._A.astype(np.float64)
        self.is_orthonormal = bool(np.abs(A @ A.T - np.eye(self.d_out)).max() <= _ORTHONORMAL_TOL)

    def _handle(self, device: int) -> _LinearHandle:
        with self._hlock:
            lh = self._lh
            if lh is None or lh.device != device:
                lh = self._lh = _LinearHandle(self._A, self._b if self.have_bias else None, device)
            return lh

    def linear_stats(self) -> dict:
        """Calls, few-row launches and tiled launches of the current handle (include/ise_knn.h, ise_linear_stats)."""
        lh = self._lh
        keys = ("calls", "few_row_launches", "tiled_launches")
        return dict.fromkeys(keys, 0) if lh is None else _counters(_n.lib.ise_linear_stats, lh._h, keys)

    def apply(self, x) -> np.ndarray:
        self._require_trained("apply")
        x = _as_rows(x, self.d_in)
        y = np.empty((x.shape[0], self.d_out), dtype=np.float32)
        if x.shape[0]:
            lh = self._handle(_default_device())
            _n.check(_n.lib.ise_linear_apply_host(lh._h, x.ctypes.data, x.shape[0], y.ctypes.data))
        return y

    def apply_torch(self, x):
        import torch

        self._require_trained("apply")
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.d_in
        x = x.contiguous()
        y = torch.empty((x.shape[0], self.d_out), dtype=torch.float32, device=x.device)
        if x.shape[0]:
            lh = self._handle(x.device.index)
            st = torch.cuda.current_stream(x.device).cuda_stream
            _n.check(_n.lib.ise_linear_apply_device(lh._h, x.data_ptr(), x.shape[0], y.data_ptr(), st))
        return y

    def reverse_transform(self, y) -> np.ndarray:
        """x = (y - b) A on the host (float64, narrowed once): the inverse when the rows of A are orthonormal
        (``is_orthonormal``; ``set_is_orthonormal`` decides), otherwise a RuntimeError, as in Faiss."""
        self._require_trained("reverse_transform")
        if not self.is_orthonormal:
            raise RuntimeError("reverse transform not implemented for non-orthonormal matrices")
        y = _as_rows(y, self.d_out).astype(np.float64)
        if self.have_bias:
            y = y - self._b.astype(np.float64)[None, :]
        return (y @ self._A.astype(np.float64)).astype(np.float32)

    def _record_body(self) -> bytes:
        return struct.pack("<B", 1 if self.have_bias else 0) + _pack_vector(self._A.astype("<f4")) + \
            _pack_vector((self._b if self.have_bias else self._b[:0]).astype("<f4"))


class RandomRotationMatrix(LinearTransform):
    """faiss.RandomRotationMatrix(d_in, d_out): ``init(seed)`` takes the Q of the QR factorisation of a Gaussian matrix
    (float64 on the host, numpy's generator: unpinned against Faiss's own); rows orthonormal when d_out <= d_in,
    columns otherwise.  ``train`` is ``init(12345)``."""

    _FOURCC = b"rrot"

    def __init__(self, d_in: int = 0, d_out: int = 0):
        super().__init__(d_in, d_out, False)

    def init(self, seed: int) -> None:
        lo, hi = min(self.d_in, self.d_out), max(self.d_in, self.d_out)
        q, _ = np.linalg.qr(np.random.default_rng(int(seed)).standard_normal((hi, lo)))  # (hi, lo), orthonormal columns
        self.A = q.T if self.d_out <= self.d_in else q
        self.set_is_orthonormal()

    def train(self, x) -> None:
        self.init(12345)


def _moments(x: np.ndarray, gram: bool):
    """float32 (n, d) -> (mean float64 (d,), the centred (n, n) Gram matrix Xc Xc^T if ``gram`` else the (d, d) scatter
    matrix Xc^T Xc, float64 on the host); neither is divided by n.  Sums in float64, on the device when there is one
    (in pieces of 64k rows), else on the host."""
    import torch

    n, d = x.shape
    dev = torch.device("cuda", _default_device()) if torch.cuda.is_available() else torch.device("cpu")
    step = 1 << 16
    total = torch.zeros(d, dtype=torch.float64, device=dev)
    for i0 in range(0, n, step):
        total += torch.from_numpy(x[i0:i0 + step]).to(dev).double().sum(0)
    mean = total / n
    if gram:
        xc = torch.from_numpy(x).to(dev).double() - mean
        m = xc @ xc.T
    else:
        m = torch.zeros((d, d), dtype=torch.float64, device=dev)
        for i0 in range(0, n, step):
            xc = torch.from_numpy(x[i0:i0 + step]).to(dev).double() - mean
            m += xc.T @ xc
    return mean.cpu(), m.cpu()


class PCAMatrix(LinearTransform):
    """faiss.PCAMatrix(d_in, d_out, eigen_power, random_rotation): ``train`` takes the mean and the covariance (divided
    by n, as in Faiss) in float64 -- through the (n, n) Gram matrix when n < d_in -- and its eigenvectors by
    ``torch.linalg.eigh`` on the host in float64, eigenvalues descending: ``mean`` float32 (d_in,), ``eigenvalues``
    float32 (d_in,) (zeros behind the rank a Gram matrix can show), ``PCAMat`` float32 (r, d_in), eigenvectors as rows (r
    = d_in, or the Gram matrix's rank).  ``A`` is the first ``d_out`` rows times ``eigenvalue ** eigen_power``
    (-0.5: whitening), times a random rotation if asked; ``b = -A mean``.  Eigenvector signs, and so Faiss's LAPACK
    path, are unpinned."""

    _FOURCC = b"PcAm"
    max_points_per_d = 1000

    def __init__(self, d_in: int = 0, d_out: int = 0, eigen_power: float = 0, random_rotation: bool = False):
        super().__init__(d_in, d_out, True)
        self.eigen_power = float(eigen_power)
        self.random_rotation = bool(random_rotation)
        self.balanced_bins = 0
        self.mean = np.zeros(0, dtype=np.float32)
        self.eigenvalues = np.zeros(0, dtype=np.float32)
        self.PCAMat = np.zeros((0, self.d_in), dtype=np.float32)
        self._eig64 = None  # train's float64 results, which prepare_Ab prefers to their float32 copies
        self._gram = None   # tests: force the Gram (True) or the covariance (False) path; None: Gram when n < d_in

    def train(self, x) -> None:
        import torch

        x = _as_rows(x, self.d_in)
        n = x.shape[0]
        assert n >= 2, "PCA needs at least two rows"
        gram = n < self.d_in if self._gram is None else self._gram
        mean, m = _moments(x, gram)
        lam, vec = torch.linalg.eigh(m / n)
        lam, vec = lam.flip(0).numpy(), vec.flip(1).numpy()  # descending; eigenvectors in columns
        if gram:
            # Xc Xc^T / n = U L U^T  ->  the covariance Xc^T Xc / n has eigenvectors Xc^T u / sqrt(n l) for l > 0
            keep = lam > lam[0] * n * 2.0 ** -52
            xc = x.astype(np.float64) - mean.numpy()[None, :]
            rows = (xc.T @ vec[:, keep] / np.sqrt(n * lam[keep])[None, :]).T
            lam = np.concatenate((lam[keep], np.zeros(self.d_in - int(keep.sum()))))
        else:
            rows = vec.T
        if rows.shape[0] < self.d_out:
            raise RuntimeError(f"{n} training rows span {rows.shape[0]} principal directions, d_out = {self.d_out}")
        self._eig64 = (mean.numpy(), np.maximum(lam, 0.0), rows)
        self.mean = self._eig64[0].astype(np.float32)
        self.eigenvalues = self._eig64[1].astype(np.float32)
        self.PCAMat = np.ascontiguousarray(rows, dtype=np.float32)
        self.prepare_Ab()

    def prepare_Ab(self) -> None:
        """``A`` and ``b`` from ``mean``, ``eigenvalues`` and ``PCAMat`` (float64, narrowed once)."""
        mean, lam, rows = self._eig64 or (self.mean.astype(np.float64), self.eigenvalues.astype(np.float64),
                                          self.PCAMat.astype(np.float64))
        assert rows.shape[0] >= self.d_out and rows.shape[1] == self.d_in and mean.size == self.d_in
        A = rows[:self.d_out]
        if self.eigen_power != 0:
            if self.eigen_power < 0 and not (lam[:self.d_out] > 0).all():
                raise RuntimeError("a zero eigenvalue among the first d_out: a negative eigen_power cannot scale it")
            A = A * (lam[:self.d_out] ** self.eigen_power)[:, None]
        if self.random_rotation:
            r = RandomRotationMatrix(self.d_out, self.d_out)
            r.init(5)
            A = r.A.astype(np.float64) @ A
        self.A = A
        self.b = -(A @ mean)
        if self.eigen_power == 0:
            self.set_is_orthonormal()

    def _record_body(self) -> bytes:
        head = struct.pack("<fBi", self.eigen_power, 1 if self.random_rotation else 0, int(self.balanced_bins))
        return head + _pack_vector(self.mean.astype("<f4")) + _pack_vector(self.eigenvalues.astype("<f4")) + \
            _pack_vector(self.PCAMat.astype("<f4")) + super()._record_body()


class OPQMatrix(LinearTransform):
    """faiss.OPQMatrix(d, M, d2=-1): the non-parametric OPQ of Ge, He, Ke and Sun ("Optimized Product Quantization",
    2013).  ``train`` starts from a random rotation and repeats ``niter`` times: rotate the rows (``apply_torch``), train
    a product quantiser on them (one ``Kmeans`` per sub-quantiser of ``niter_pq`` iterations -- ``niter_pq_0`` the first
    time -- warm-started from the previous round's centroids), encode and decode through a scratch ``IndexPQ``, and take
    the rotation nearest to mapping the rows onto their decoded images: A^T = U V^T from the SVD of X^T Xhat, float64 on
    the host.  At most ``max_train_points`` rows, drawn with a seeded generator.  Written to a file as a plain
    ``LinearTransform`` ("LTra"), as in Faiss."""

    niter, niter_pq, niter_pq_0 = 50, 4, 40  # Faiss's defaults; set on an object before ``train``
    max_train_points = 256 * 256
    seed = 1234

    def __init__(self, d: int = 0, M: int = 1, d2: int = -1):
        super().__init__(d, d if int(d2) < 0 else int(d2), False)
        self.M = int(M)
        assert self.d_out <= self.d_in and self.d_out % self.M == 0, "d2 <= d, and M divides d2"

    def train(self, x) -> None:
        import torch

        x = _as_rows(x, self.d_in)
        if x.shape[0] < 256:
            raise RuntimeError(f"{x.shape[0]} training rows for 256 centroids per sub-quantiser")
        if x.shape[0] > self.max_train_points:
            pick = np.random.default_rng(self.seed).choice(x.shape[0], self.max_train_points, replace=False)
            x = x[np.sort(pick)]
        d2, dsub = self.d_out, self.d_out // self.M
        x64 = x.astype(np.float64)
        x_dev = torch.from_numpy(x).to(torch.device("cuda", _default_device()))
        rot = RandomRotationMatrix(self.d_in, d2)
        rot.init(self.seed)
        self.A = rot.A
        pq = IndexPQ(d2, self.M, 8)
        centroids = None
        for it in range(int(self.niter)):
            xr = self.apply_torch(x_dev).cpu().numpy()
            c = np.empty((self.M, 256, dsub), dtype=np.float32)
            for m in range(self.M):
                km = Kmeans(dsub, 256, niter=self.niter_pq_0 if it == 0 else self.niter_pq, seed=self.seed)
                km.train(np.ascontiguousarray(xr[:, m * dsub:(m + 1) * dsub]),
                         init_centroids=None if centroids is None else centroids[m])
                c[m] = km.centroids
            centroids = c
            pq.pq.set_centroids(c)
            xhat = pq.sa_decode(pq.sa_encode(xr)).astype(np.float64)
            u, _, vt = np.linalg.svd(x64.T @ xhat, full_matrices=False)  # (d, d2) = u (d, d2) s vt (d2, d2)
            self.A = (u @ vt).T
        self.set_is_orthonormal()


class NormalizationTransform(VectorTransform):
    """faiss.NormalizationTransform(d, norm=2.0): every row divided by its L2 norm, zero rows untouched --
    ``normalize_L2`` on a copy (include/ise_knn.h, ise_normalize_rows_*).  Only norm 2 is provided."""

    _FOURCC = b"VNrm"

    def __init__(self, d: int = 0, norm: float = 2.0):
        super().__init__(d, d)
        if float(norm) != 2.0:
            raise NotImplementedError(f"NormalizationTransform with norm = {norm}: only the L2 norm is provided")
        self.norm = float(norm)

    def apply(self, x) -> np.ndarray:
        y = _as_rows(x, self.d_in).copy()
        if y.shape[0]:
            normalize_L2(y)
        return y

    def apply_torch(self, x):
        import torch

        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.d_in
        y = x.contiguous().clone()
        if y.shape[0]:
            normalize_L2(y)
        return y

    def reverse_transform(self, y) -> np.ndarray:
        return _as_rows(y, self.d_out).copy()  # the norm is gone: Faiss hands the rows back as they are

    def _record_body(self) -> bytes:
        return struct.pack("<f", self.norm)


class CenteringTransform(VectorTransform):
    """faiss.CenteringTransform(d): y = x - mean, ``mean`` from ``train``.  It runs as a ``LinearTransform`` with the
    identity for A and -mean for b rather than through a kernel of its own: every chain is then x_j exactly (zeros and
    one product by 1), and the one rounding is that of -mean_j + x_j, the bits of x_j - mean_j.  (A row with an inf
    entry turns NaN throughout: 0 * inf.)  d is at most 4096."""

    _FOURCC = b"VCnt"

    def __init__(self, d: int = 0):
        super().__init__(d, d)
        self.is_trained = False
        self._mean = np.zeros(0, dtype=np.float32)
        self._lt = None

    @property
    def mean(self) -> np.ndarray:
        return self._mean

    @mean.setter
    def mean(self, mean) -> None:
        mean = np.ascontiguousarray(np.asarray(mean), dtype=np.float32).reshape(-1)
        assert mean.size == self.d_in, f"mean holds d = {self.d_in} entries, got {mean.size}"
        self._mean, self._lt = mean, None
        self.is_trained = True

    def train(self, x) -> None:
        self.mean = _as_rows(x, self.d_in).astype(np.float64).mean(axis=0)

    def _linear(self) -> LinearTransform:
        self._require_trained("apply")
        if self._lt is None:
            lt = LinearTransform(self.d_in, self.d_in, True)
            lt.A = np.eye(self.d_in, dtype=np.float32)
            lt.b = -self._mean
            self._lt = lt
        return self._lt

    def apply(self, x) -> np.ndarray:
        return self._linear().apply(x)

    def apply_torch(self, x):
        return self._linear().apply_torch(x)

    def reverse_transform(self, y) -> np.ndarray:
        self._require_trained("reverse_transform")
        return _as_rows(y, self.d_out) + self._mean[None, :]

    def _record_body(self) -> bytes:
        return _pack_vector(self._mean.astype("<f4"))


class SearchParametersPreTransform(SearchParameters):
    """faiss.SearchParametersPreTransform(index_params=): ``index_params`` goes to the sub-index."""

    def __init__(self, index_params=None):
        super().__init__()
        self.index_params = index_params


class IndexPreTransform:
    """faiss.IndexPreTransform(ltrans, index) / IndexPreTransform(index) + ``prepend_transform(vt)``: the rows and the
    queries pass through ``chain`` (first transform first) before they reach ``index`` -- any index kind of this
    package with ``add`` and ``search``.  ``train`` trains each untrained transform on the rows as transformed so far,
    then the sub-index; ``search`` / ``search_torch`` return what the sub-index returns for ``apply_chain(x)``, bit for
    bit.  ``range_search``, ``remove_ids``, ``add_with_ids`` and ``params=`` (``SearchParametersPreTransform`` is
    unwrapped) go straight to the sub-index, which raises where it does not provide them; ``reconstruct`` goes back
    through every ``reverse_transform``."""

    def __init__(self, *args):
        assert len(args) in (1, 2), "IndexPreTransform(index) or IndexPreTransform(ltrans, index)"
        self.index = args[-1]
        assert hasattr(self.index, "search") and hasattr(self.index, "add"), "the sub-index has add and search"
        self.chain = []
        if len(args) == 2:
            self.prepend_transform(args[0])

    d = property(lambda self: self.chain[0].d_in if self.chain else self.index.d)
    metric_type = property(lambda self: self.index.metric_type)
    ntotal = property(lambda self: self.index.ntotal)
    device = property(lambda self: self.index.device)
    is_trained = property(lambda self: all(t.is_trained for t in self.chain) and bool(self.index.is_trained))

    def prepend_transform(self, vt: VectorTransform) -> None:
        assert isinstance(vt, VectorTransform), "a VectorTransform"
        assert vt.d_out == self.d, f"dimension mismatch: the transform gives d_out={vt.d_out}, what follows takes d={self.d}"
        self.chain.insert(0, vt)

    def apply_chain(self, x):
        """numpy rows -> numpy rows (``apply``), a CUDA tensor -> a CUDA tensor (``apply_torch``)."""
        if isinstance(x, np.ndarray) or not hasattr(x, "is_cuda"):
            x = _as_rows(x, self.d)
            for t in self.chain:
                x = t.apply(x)
            return x
        assert x.dim() == 2 and x.shape[1] == self.d, f"dimension mismatch: got {tuple(x.shape)}, index has d={self.d}"
        for t in self.chain:
            x = t.apply_torch(x)
        return x

    @staticmethod
    def _sub_params(params):
        return params.index_params if isinstance(params, SearchParametersPreTransform) else params

    # -- build side
    def train(self, x) -> None:
        x = _as_rows(x, self.d)
        for t in self.chain:
            if not t.is_trained:
                t.train(x)
            x = t.apply(x)
        if hasattr(self.index, "train"):
            self.index.train(x)

    def add(self, x) -> None:
        self.index.add(self.apply_chain(_as_rows(x, self.d)))

    def add_with_ids(self, x, ids) -> None:
        self.index.add_with_ids(self.apply_chain(_as_rows(x, self.d)), ids)

    def add_torch(self, x) -> None:
        self.index.add_torch(self.apply_chain(x))

    def reset(self) -> None:
        self.index.reset()

    def remove_ids(self, sel) -> int:
        return self.index.remove_ids(sel)

    def reconstruct_n(self, i0: int = 0, n: int | None = None) -> np.ndarray:
        x = self.index.reconstruct_n(i0, self.ntotal - i0 if n is None else n)
        for t in reversed(self.chain):
            x = t.reverse_transform(x)
        return x

    def reconstruct(self, i: int) -> np.ndarray:
        return self.reconstruct_n(int(i), 1)[0]

    # -- query side
    def search(self, x, k: int, params=None):
        return self.index.search(self.apply_chain(_as_rows(x, self.d)), k, params=self._sub_params(params))

    def search_torch(self, xq, k: int, params=None):
        """The transforms and the sub-index's ``search_torch``, enqueued on the current torch stream."""
        return self.index.search_torch(self.apply_chain(xq), k, params=self._sub_params(params))

    def range_search(self, x, radius: float, params=None):
        return self.index.range_search(self.apply_chain(_as_rows(x, self.d)), radius, params=self._sub_params(params))

    def _image(self) -> bytes:
        sub = self.index
        if isinstance(sub, IndexIVFFlat):
            raise NotImplementedError("write_index of an IndexIVFFlat is not provided")
        image = sub._image() if hasattr(sub, "_image") else _flat_image(sub)
        return serialize_pretransform(self.chain, image, self.d, self.metric_type, self.ntotal, self.is_trained)

    @classmethod
    def _from_parts(cls, parts, device):
        """The index a parsed "IxPT" image describes (``parse_pretransform``)."""
        sub_cls, _, _ = _INDEX_FILES.get(parts.sub_fourcc, _FLAT_FILE)
        index = cls(sub_cls()._from_parts(parts.sub, device))
        for t in reversed(parts.chain):
            index.prepend_transform(t)
        return index


# IndexPreTransform [upstream-faiss index_write.cpp write_index / write_VectorTransform, restated from memory of the
# published format and UNPINNED like the layouts above: there is no sample file]:
#   fourcc "IxPT"; the index header (d, ntotal, 1<<20, 1<<20, is_trained, metric_type); int32 count; count transform
#   records, the first to apply first; the sub-index as its own file image.
#   A transform record: fourcc "rrot" (RandomRotationMatrix), "PcAm" (PCAMatrix), "LTra" (LinearTransform, OPQMatrix),
#   "VNrm" (NormalizationTransform) or "VCnt" (CenteringTransform); for "PcAm" first: float32 eigen_power, uint8
#   random_rotation, int32 balanced_bins, the vectors mean, eigenvalues, PCAMat; for the three linear kinds: uint8
#   have_bias, the vectors A ([d_out][d_in]) and b; for "VNrm": float32 norm; for "VCnt": the vector mean; then for
#   every kind int32 d_in, int32 d_out, uint8 is_trained.  (A vector: uint64 count, count float32.)
_FOURCC_PRETRANSFORM = b"IxPT"
_TRUNCATED_PRETRANSFORM = "truncated IndexPreTransform file"
_VT_TAIL = struct.Struct("<iiB")
_VT_COUNT = struct.Struct("<i")
_VT_PCA_HEAD = struct.Struct("<fBi")
_VT_BYTE = struct.Struct("<B")
_VT_FLOAT = struct.Struct("<f")
_VT_KINDS = {b"rrot": RandomRotationMatrix, b"PcAm": PCAMatrix, b"LTra": LinearTransform, b"VNrm": NormalizationTransform,
             b"VCnt": CenteringTransform}
_PreTransformParts = namedtuple("_PreTransformParts", "d metric chain sub_fourcc sub")


def serialize_pretransform(chain, sub_image: bytes, d: int, metric: int, ntotal: int, is_trained: bool = True) -> bytes:
    """``chain``: the ``VectorTransform`` objects, the first to apply first; ``sub_image``: the sub-index as one of the
    writers here writes it."""
    head = _HDR.pack(_FOURCC_PRETRANSFORM, int(d), int(ntotal), 1 << 20, 1 << 20, 1 if is_trained else 0, int(metric))
    return head + _VT_COUNT.pack(len(chain)) + b"".join(t._record() for t in chain) + bytes(sub_image)


def _parse_transform_at(cur: _Cursor) -> VectorTransform:
    corrupt = "corrupt IndexPreTransform: a transform record's sizes do not agree"
    fourcc = cur.fourcc()
    if fourcc not in _VT_KINDS:
        raise RuntimeError(f"unsupported vector transform {fourcc!r} in an IndexPreTransform file")

    def floats():
        return cur.vector(np.float32, lambda count: True, corrupt)

    pca = lin = norm = mean = None
    if fourcc == b"PcAm":
        pca = cur.take(_VT_PCA_HEAD) + (floats(), floats(), floats())
    if fourcc in (b"rrot", b"PcAm", b"LTra"):
        lin = cur.take(_VT_BYTE) + (floats(), floats())
    elif fourcc == b"VNrm":
        (norm,) = cur.take(_VT_FLOAT)
    else:
        mean = floats()
    d_in, d_out, is_trained = cur.take(_VT_TAIL)
    if d_in <= 0 or d_out <= 0:
        raise RuntimeError(corrupt)
    if lin is not None:
        have_bias, A, b = lin
        t = _VT_KINDS[fourcc](d_in, d_out)
        if A.size not in (0, d_in * d_out) or b.size != (d_out if have_bias and A.size else 0) or bool(A.size) != bool(is_trained):
            raise RuntimeError(corrupt)
        if pca is not None:
            t.eigen_power, t.random_rotation, t.balanced_bins = float(pca[0]), bool(pca[1]), int(pca[2])
            if A.size and (pca[3].size != d_in or pca[4].size != d_in or pca[5].size % d_in or pca[5].size < d_in * d_out):
                raise RuntimeError(corrupt)
            t.mean, t.eigenvalues, t.PCAMat = pca[3], pca[4], pca[5].reshape(-1, d_in)
        t.have_bias = bool(have_bias)
        if A.size:
            t.A = A.reshape(d_out, d_in)
            if have_bias:
                t.b = b
            t.set_is_orthonormal()
    elif norm is not None:
        if d_in != d_out or norm != 2.0:
            raise RuntimeError("unsupported NormalizationTransform in an IndexPreTransform file: only the L2 norm is readable")
        t = NormalizationTransform(d_in, norm)
    else:
        if d_in != d_out or mean.size != (d_in if is_trained else 0):
            raise RuntimeError(corrupt)
        t = CenteringTransform(d_in)
        if is_trained:
            t.mean = mean
    return t


def _parse_pretransform_at(cur: _Cursor) -> _PreTransformParts:
    """(Every missing byte is ``_TRUNCATED_PRETRANSFORM``: the cursor is made with it.)"""
    cur.expect(_FOURCC_PRETRANSFORM, "IndexPreTransform")
    _, d, n, _, _, _, metric = cur.take(_HDR)
    (count,) = cur.take(_VT_COUNT)
    if d <= 0 or n < 0 or not 0 <= count <= 64:
        raise RuntimeError("corrupt IndexPreTransform header")
    chain = [_parse_transform_at(cur) for _ in range(count)]
    for t, after in zip(chain, chain[1:]):
        if t.d_out != after.d_in:
            raise RuntimeError("corrupt IndexPreTransform: the transforms do not chain")
    sub_fourcc = cur.peek()
    if sub_fourcc in (b"IwFl", b"IwF2"):
        raise NotImplementedError("read_index of an IndexIVFFlat file is not provided")
    if sub_fourcc == _FOURCC_PRETRANSFORM:
        raise RuntimeError("unsupported sub-index type b'IxPT' in an IndexPreTransform file")
    _, read, _ = _INDEX_FILES.get(sub_fourcc, _FLAT_FILE)
    sub = read(cur)
    if cur.off != len(cur.buf):
        raise RuntimeError("corrupt IndexPreTransform: bytes behind the sub-index")
    if (chain[0].d_in if chain else sub.d) != d or (chain and chain[-1].d_out != sub.d):
        raise RuntimeError("corrupt IndexPreTransform: the dimensions do not match the header")
    return _PreTransformParts(d, metric, chain, sub_fourcc, sub)


def parse_pretransform(buf: bytes):
    """-> (d, metric, chain: the ``VectorTransform`` objects, sub_fourcc, the sub-index as its own parser returns it);
    raises RuntimeError on a foreign, truncated or inconsistent file."""
    parts = _parse_pretransform_at(_Cursor(buf, _TRUNCATED_PRETRANSFORM))
    return tuple(parts._replace(sub=tuple(parts.sub)))


_INDEX_FILES[_FOURCC_PRETRANSFORM] = (lambda: IndexPreTransform, _parse_pretransform_at, _TRUNCATED_PRETRANSFORM)
