"""Every reader method of image_search_engine_amd.faiss_compat once, on the three index kinds: the exact keys and the
Python type of every value.  The keys are literals, copied from the module as it stood before its index kinds began to
share their Python code (tests/test_compat_surface.py pins the signatures; this pins what the readers return)."""
import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss

pytestmark = pytest.mark.gpu

_SELECTOR_INFO = {"ntotal": int, "selected": int, "window": tuple, "tiles": int}


def _check(got: dict, want: dict) -> None:
    """``want``: key -> type, in order.  bool is an int to ``isinstance``, so the types are compared outright."""
    assert tuple(got) == tuple(want), got
    for key, kind in want.items():
        assert type(got[key]) is kind, (key, got[key])


def test_every_reader_returns_its_keys_and_types():
    rng = np.random.default_rng(5)
    xb = rng.random((200, 32), dtype=np.float32)
    codes = rng.integers(0, 256, (200, 8), dtype=np.uint8)

    flat = faiss.IndexFlatL2(32)
    flat.add(xb)
    D, I = flat.search(xb[:3], 4)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (3, 4)
    assert I[:, 0].tolist() == [0, 1, 2]
    lims, Dr, Ir = flat.range_search(xb[:3], 1.0)
    assert lims.dtype == np.uint64 and Dr.dtype == np.float32 and Ir.dtype == np.int64
    assert lims.shape == (4,) and lims[0] == 0 and Dr.shape == Ir.shape == (int(lims[-1]),)
    assert all(q in Ir[int(lims[q]):int(lims[q + 1])] for q in range(3))

    binary = faiss.IndexBinaryFlat(64)
    binary.add(codes)
    D, I = binary.search(codes[:3], 4)
    assert D.dtype == np.int32 and I.dtype == np.int64 and D.shape == I.shape == (3, 4)
    assert D[:, 0].tolist() == [0, 0, 0]
    lims, Dr, Ir = binary.range_search(codes[:3], 20)
    assert lims.dtype == np.uint64 and Dr.dtype == np.int32 and Ir.dtype == np.int64
    assert lims.shape == (4,) and lims[0] == 0 and Dr.shape == Ir.shape == (int(lims[-1]),)
    assert all(q in Ir[int(lims[q]):int(lims[q + 1])] for q in range(3))

    quantizer = faiss.IndexFlatL2(32)
    quantizer.add(xb[:4])
    ivf = faiss.IndexIVFFlat(quantizer, 32, 4)
    ivf.add(xb)
    D, I = ivf.search(xb[:3], 4)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (3, 4)
    assert I[:, 0].tolist() == [0, 1, 2]
    assert (flat.ntotal, binary.ntotal, ivf.ntotal) == (200, 200, 200)

    _check(flat.exact_stats(), {"reranked": int, "exact_scan": int, "shift_updates": int, "gemm_chunks": int})
    _check(flat.gemm_stats(), {"gemm_chunks": int, "gemm_lost_queries": int})
    _check(flat.host_stats(), {"combined_batches": int, "combined_calls": int, "direct_queries": int})
    _check(flat.short_stats(), {"short_batches": int})
    _check(flat.half_stats(), {"half_batches": int})
    _check(flat.byte_stats(), {"byte_batches": int, "byte_route": bool})
    _check(flat.depth_stats(), {"isolated_batches": int, "deep_batches": int})
    _check(flat.range_stats(), {"range_batches": int, "range_overflow_batches": int})
    assert flat.range_stats()["range_batches"] >= 1  # the one range_search above
    timing = flat.remove_last_timing()
    assert type(timing) is tuple and len(timing) == 2 and type(timing[0]) is float and type(timing[1]) is int
    _check(binary.binary_stats(), {"search_batches": int, "scan_passes": int, "range_batches": int})
    assert binary.binary_stats()["search_batches"] >= 1 and binary.binary_stats()["range_batches"] >= 1
    _check(ivf.ivf_stats(), {"batches": int, "passes": int, "tiles_loaded": int})
    assert ivf.ivf_stats()["batches"] >= 1
    for index, selector_class in ((flat, faiss.DeviceSelector), (binary, faiss.BinaryDeviceSelector)):
        _check(index.remove_stats(), {"remove_calls": int, "rows_removed": int, "rows_moved": int})
        _check(index.sel_stats(), {"sel_batches": int, "sel_passes": int, "sel_range_batches": int})
        ds = index.make_selector(faiss.IDSelectorRange(10, 50))
        assert type(ds) is selector_class
        info = ds.info()
        _check(info, _SELECTOR_INFO)
        assert info["ntotal"] == 200 and info["selected"] == 40 and info["window"] == (10, 50)
        assert all(type(v) is int for v in info["window"])
        ds.close()
