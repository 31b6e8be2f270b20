"""CPU tests of the inverted-list index's host side: the new entry points' argument errors through the C ABI (no
device is touched), the numpy reference of the GPU tests, and what stays unprovided."""
import ctypes

import numpy as np
import pytest

from image_search_engine_amd import faiss_compat as faiss
from tests import ivf_ref
from tests.knn_checks import assert_knn_identical, brute_knn, int_data
from tests.sel_ref import IP, L2


def test_argument_errors_through_abi():
    from image_search_engine_amd import _native as n

    h = ctypes.c_void_p()
    for args, word in (((0, n.METRIC_L2, 4, 0), b"d must"), ((-3, n.METRIC_L2, 4, 0), b"d must"),
                       ((8, n.METRIC_L2, 0, 0), b"nlist"), ((8, n.METRIC_L2, -1, 0), b"nlist"), ((8, 7, 4, 0), b"metric")):
        assert n.lib.ise_ivf_create(ctypes.byref(h), *args) == n.E_INVALID, args
        assert word in n.lib.ise_last_error(), (args, n.lib.ise_last_error())
        assert h.value is None
    assert n.lib.ise_ivf_create(None, 8, n.METRIC_L2, 4, 0) == n.E_INVALID
    assert b"NULL" in n.lib.ise_last_error()
    assert n.lib.ise_ivf_destroy(None) == 0
    assert n.lib.ise_ivf_reset(None) == n.E_INVALID
    assert n.lib.ise_ivf_info(None, None, None, None, None, None) == n.E_INVALID
    x = np.zeros((2, 8), np.float32)
    lists = np.zeros(2, np.int64)
    out = np.zeros(4, np.int64)
    D, I = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int64)
    # NULL buffers
    assert n.lib.ise_ivf_add_host(None, None, lists.ctypes.data, 2) == n.E_INVALID
    assert b"pointer is NULL" in n.lib.ise_last_error()
    assert n.lib.ise_ivf_add_host(None, x.ctypes.data, None, 2) == n.E_INVALID
    assert b"pointer is NULL" in n.lib.ise_last_error()
    assert n.lib.ise_ivf_add_device(None, None, None, 2, None) == n.E_INVALID
    assert n.lib.ise_ivf_add_host(None, x.ctypes.data, lists.ctypes.data, -1) == n.E_INVALID
    assert n.lib.ise_ivf_add_host(None, x.ctypes.data, lists.ctypes.data, 2) == n.E_INVALID
    assert b"handle" in n.lib.ise_last_error()
    assert n.lib.ise_ivf_list_sizes_host(None, out.ctypes.data) == n.E_INVALID
    assert n.lib.ise_ivf_list_host(None, 0, None, None) == n.E_INVALID
    # k outside 1 .. ISE_MAX_K, nprobe, NULL buffers: before the handle is looked at
    for search, tail in ((n.lib.ise_ivf_search_host, ()), (n.lib.ise_ivf_search_device, (None,))):
        for k in (0, -1, n.MAX_K + 1):
            assert search(None, x.ctypes.data, 2, k, lists.ctypes.data, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
            assert b"k must" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 0, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"nprobe" in n.lib.ise_last_error()
        assert search(None, None, 2, 3, lists.ctypes.data, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"pointer is NULL" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, None, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"pointer is NULL" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 1, None, I.ctypes.data, *tail) == n.E_INVALID
        assert b"output pointer" in n.lib.ise_last_error()
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 1, D.ctypes.data, None, *tail) == n.E_INVALID
        assert search(None, x.ctypes.data, 2, 3, lists.ctypes.data, 1, D.ctypes.data, I.ctypes.data, *tail) == n.E_INVALID
        assert b"handle" in n.lib.ise_last_error()
    assert n.lib.ise_ivf_stats(None, (ctypes.c_uint64 * 3)()) == n.E_INVALID


def test_reference_members():
    """Duplicate probes, -1 probes, out-of-range probes and an empty list."""
    assign = np.array([2, 0, 2, 3, 0, 2, 3], np.int64)  # list 1 is empty
    lists = ivf_ref.list_members(assign, 4)
    assert [l.tolist() for l in lists] == [[1, 4], [], [0, 2, 5], [3, 6]]
    probes = np.array([[2, 2, 2], [-1, -1, -1], [1, -1, 1], [3, 0, 3], [0, 7, -1], [1, 2, 3]], np.int64)
    got = [m.tolist() for m in ivf_ref.probed_members(probes, assign, 4)]
    assert got == [[0, 2, 5], [], [], [1, 3, 4, 6], [1, 4], [0, 2, 3, 5, 6]]
    assert all(m.dtype == np.int64 for m in ivf_ref.probed_members(probes, assign, 4))
    assert ivf_ref.tiles_of([0, 1, 16, 17, 100]) == 0 + 1 + 1 + 2 + 7
    with pytest.raises(AssertionError):
        ivf_ref.list_members(np.array([0, 4]), 4)


@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_results(metric):
    """The two expected-result forms agree with each other on integer data, padding included."""
    rng = np.random.default_rng(11)
    n, d, nq, nlist = 200, 12, 6, 5
    xb, xq = int_data("small", rng, n, d), int_data("small", rng, nq, d)
    assign = rng.integers(0, nlist - 1, n)  # the last list stays empty
    assign[7] = 3
    probes = np.array([[0, 1], [4, 4], [3, -1], [2, 2], [-1, -1], [1, 0]], np.int64)
    members = ivf_ref.probed_members(probes, assign, nlist)
    assert members[1].size == 0 and members[4].size == 0
    D_full, I_full = brute_knn(xb, xq, n, metric)
    for k in (1, 10, 150):
        Da, Ia = ivf_ref.expected_from_ranking(D_full, I_full, members, k, metric)
        Db, Ib = ivf_ref.expected_brute(xb, xq, members, k, metric)
        assert_knn_identical(Da, Ia, Db, Ib, f"k={k}")
        assert (Ia[1] == -1).all() and (Ia[4] == -1).all()


def test_what_stays_unprovided(tmp_path):
    from image_search_engine_amd import utils

    with pytest.raises(NotImplementedError):
        utils.create_search_index(np.zeros((4, 16), np.float32), "cell-probe")
    with pytest.raises(NotImplementedError):
        faiss.IndexIVFPQ()
    p = tmp_path / "ivf.index"
    p.write_bytes(b"IwFl" + bytes(64))
    with pytest.raises(NotImplementedError, match="IndexIVFFlat"):
        faiss.read_index(str(p))
    for name in ("range_search", "remove_ids"):
        with pytest.raises(NotImplementedError):
            getattr(faiss.IndexIVFFlat, name)(None)
    cp = faiss.ClusteringParameters()
    assert (cp.niter, cp.seed) == (10, 1234)


def test_rebuild_bookkeeping_standalone(tmp_path):
    """csrc/ise_ivf_plan.hpp (the stable counting sort behind a rebuild) in a stand-alone host program with its own
    main, under the address and undefined-behaviour sanitizers (linked statically: the program then runs whatever
    else the environment loads first).  A missing compiler or sanitizer runtime fails the test."""
    import os
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone check (it is a tool of the build, not hardware)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "ivf_plan_check.cpp")
    exe = str(tmp_path / "ivf_plan_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized build failed (no unsanitized fallback):\n" + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
