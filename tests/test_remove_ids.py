"""CPU tests of remove_ids: the numpy restatement of the source map and slab schedule (tests/remove_ref.py), the host
planning itself (csrc/ise_remove_plan.hpp) in a stand-alone sanitized program, the id selectors against brute-force
sets, the IndexIDMap file layout and engine.remove_images over a fake index."""
import json

import numpy as np
import pytest

from tests import remove_ref as rr


def _cases():
    rng = np.random.default_rng(5)
    cases = []
    for n in (1, 2, 17, 100):
        cases += [(n, []), (n, [0]), (n, [n - 1]), (n, list(range(n))), (n, list(range(1, n))), (n, [n // 2])]
    cases += [(100, list(range(10, 60))), (100, list(range(10, 20)) + list(range(20, 30))),   # long run, adjacent runs
              (100, [3, 4, 5, 7, 8, 50, 99]), (100, list(range(0, 100, 2))), (64, list(range(0, 5)) + [63])]
    for _ in range(300):
        n = int(rng.integers(1, 200))
        p = rng.choice([0.01, 0.1, 0.5, 0.9])
        removed = np.flatnonzero(rng.random(n) < p).tolist()
        if rng.random() < 0.3 and n > 5:  # a long run on top
            a = int(rng.integers(0, n - 3))
            removed += list(range(a, min(n, a + int(rng.integers(2, 40)))))
        cases.append((n, removed))
    return cases


CASES = _cases()


def test_source_map_equals_np_delete():
    assert len(CASES) > 300
    for n, removed in CASES:
        runs = rr.runs_of(removed, n)
        src = rr.source_map(n, runs)
        want = np.delete(np.arange(n), np.unique(np.asarray(removed, dtype=np.int64)))
        assert np.array_equal(src, want), (n, removed)
        if len(src):
            assert (np.diff(src) > 0).all() and (src >= np.arange(len(src))).all()
        first = runs[0][0] if runs else n
        assert np.array_equal(src[:first], np.arange(min(first, len(src))))  # rows below the first removed one stay


def test_runs_are_sorted_disjoint_and_maximal():
    for n, removed in CASES:
        runs = rr.runs_of(removed + [-3, n, n + 7], n)
        ends = [s + m for s, m in runs]
        assert all(m > 0 for _, m in runs)
        assert all(runs[t + 1][0] > ends[t] for t in range(len(runs) - 1))  # a gap between runs: never adjacent
        assert sum(m for _, m in runs) == len(set(i for i in removed if 0 <= i < n))


@pytest.mark.parametrize("slab", [1, 7, 48, None])
def test_slab_schedule_never_reads_an_overwritten_row(slab):
    for n, removed in CASES:
        runs = rr.runs_of(removed, n)
        written = np.zeros(n, dtype=bool)
        for reads, writes in rr.slab_schedule(n, runs, slab or n):
            assert not written[reads].any(), (n, removed, slab)
            written[writes] = True
        # ... and running it reproduces np.delete, with the tail zeroed
        x = np.arange(1, n + 1, dtype=np.int64) * 10
        got, n_new = rr.compact(x, runs, slab or n)
        keep = np.delete(x, np.unique(np.asarray(removed, dtype=np.int64)))
        assert n_new == len(keep) and np.array_equal(got[:n_new], keep) and not got[n_new:].any()
        first = runs[0][0] if runs else n
        assert int(written.sum()) == n_new - min(first, n_new)  # rows moved


def test_remove_planning_standalone(tmp_path):
    """csrc/ise_remove_plan.hpp (ids -> runs -> g / cend tables, the slab rule: what tests/remove_ref.py restates) in a
    stand-alone host program with its own main, against a brute-force erase, under the address and undefined-behaviour
    sanitizers (linked statically: the program then runs whatever else the environment loads first).  A missing
    compiler or sanitizer runtime fails the test."""
    import os
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone check (it is a tool of the build, not hardware)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "remove_plan_check.cpp")
    exe = str(tmp_path / "remove_plan_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized build failed (no unsanitized fallback):\n" + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ selectors
def _selectors(faiss):
    rng = np.random.default_rng(9)
    raw = [np.array([5, 3, 3, 9, -4, 10**12, 40, 41, 42, 0, 199, 200, 250]),   # unsorted, duplicates, out of range
           rng.integers(-20, 260, 120), np.array([], dtype=np.int64), np.arange(200)]
    sels = []
    for ids in raw:
        want = set(int(i) for i in ids)
        sels.append((faiss.IDSelectorBatch(ids), want))
        sels.append((faiss.IDSelectorArray(list(ids)), want))
    for lo, hi in ((10, 20), (-5, 3), (190, 400), (7, 7), (9, 2), (0, 200)):
        sels.append((faiss.IDSelectorRange(lo, hi), set(range(lo, hi))))
    return sels


def _expand(runs):
    return [i for a, m in np.asarray(runs).reshape(-1, 2).tolist() for i in range(a, a + m)]


def test_selectors_against_brute_force_sets():
    import image_search_engine_amd.faiss_compat as faiss

    probe = list(range(-30, 270)) + [10**12]
    for sel, want in _selectors(faiss):
        for n in (0, 1, 200, 230):
            for s, member in ((sel, lambda i: i in want), (faiss.IDSelectorNot(sel), lambda i: i not in want),
                              (faiss.IDSelectorNot(faiss.IDSelectorNot(sel)), lambda i: i in want)):
                assert [s.is_member(i) for i in probe] == [member(i) for i in probe]
                assert s.members(np.asarray(probe)).tolist() == [member(i) for i in probe]
                runs = np.asarray(s.runs(n)).reshape(-1, 2)
                assert _expand(runs) == [i for i in range(n) if member(i)]
                assert (runs[:, 1] > 0).all()
                assert (runs[1:, 0] > runs[:-1, 0] + runs[:-1, 1]).all()  # sorted, disjoint, never adjacent


def test_range_selector_never_materialises():
    import image_search_engine_amd.faiss_compat as faiss

    sel = faiss.IDSelectorRange(5, 1 << 62)
    assert sel.runs(1 << 40).tolist() == [[5, (1 << 40) - 5]]
    assert faiss.IDSelectorNot(sel).runs(1 << 40).tolist() == [[0, 5]]


# ------------------------------------------------------------------------------------------------ file layout
def test_idmap_file_round_trip_and_errors():
    import struct

    import image_search_engine_amd.faiss_compat as faiss

    rng = np.random.default_rng(3)
    for metric in (faiss.METRIC_L2, faiss.METRIC_INNER_PRODUCT):
        for n in (0, 1, 37):
            xb = rng.standard_normal((n, 6)).astype(np.float32)
            ids = rng.integers(-(1 << 62), 1 << 62, n)
            buf = faiss.serialize_idmap(6, metric, xb, ids)
            assert buf[:4] == b"IxMp"
            flat = faiss.serialize_flat(6, metric, xb)
            assert buf[faiss._HDR.size:faiss._HDR.size + len(flat)] == flat          # the sub-index as written today
            assert buf[faiss._HDR.size + len(flat):] == struct.pack("<Q", n) + ids.astype("<i8").tobytes()
            d, m, xb2, ids2 = faiss.parse_idmap(buf)
            assert (d, m) == (6, metric) and np.array_equal(xb2, xb) and np.array_equal(ids2, ids)
            assert ids2.dtype == np.int64
            if n:
                for cut in (1, 8 * n, 8 * n + 1, 8 * n + 8):
                    with pytest.raises(RuntimeError):
                        faiss.parse_idmap(buf[:-cut])
            with pytest.raises(RuntimeError):
                faiss.parse_idmap(b"IxQZ" + buf[4:])
            with pytest.raises(RuntimeError):
                faiss.parse_idmap(flat)          # a plain flat file is not an IndexIDMap
            with pytest.raises(RuntimeError):
                faiss.parse_flat(buf)            # ... and the reverse


# ------------------------------------------------------------------------------------------------ engine
class _FakeIndex:
    """Ten-line stand-in for IndexFlat: rows on the host, remove_ids calls recorded."""

    def __init__(self, xb):
        self.xb, self.d, self.metric_type, self.calls = xb.copy(), xb.shape[1], 1, []

    ntotal = property(lambda self: self.xb.shape[0])

    def remove_ids(self, ids):
        self.calls.append(np.asarray(ids).tolist())
        before = self.ntotal
        self.xb = np.delete(self.xb, np.asarray(ids, dtype=np.int64), axis=0)
        return before - self.ntotal

    def reconstruct_n(self, i0, n):
        return self.xb[i0:i0 + n]


@pytest.fixture
def bound_engine(tmp_path):
    from image_search_engine_amd import engine

    saved = (engine.index, engine.images_paths, engine.index_file)
    xb = np.arange(24, dtype=np.float32).reshape(8, 3)
    engine.index = _FakeIndex(xb)
    engine.images_paths = [tmp_path / f"img_{i}.png" for i in range(8)]
    engine.index_file = None
    yield engine, xb, tmp_path
    engine.index, engine.images_paths, engine.index_file = saved


def test_engine_remove_images_keeps_paths_in_step(bound_engine):
    engine, xb, tmp = bound_engine
    paths = list(engine.images_paths)
    assert engine.remove_images([tmp / "nope.png"]) == 0 and engine.index.calls == []
    n = engine.remove_images([paths[5], str(paths[1]), tmp / "nope.png", paths[5]])
    assert n == 2 and engine.index.calls == [[1, 5]]
    assert engine.images_paths == [p for i, p in enumerate(paths) if i not in (1, 5)]
    assert np.array_equal(engine.index.xb, np.delete(xb, [1, 5], axis=0))
    assert not engine.paths_file_for(tmp / "i.faiss").exists()  # not loaded from a file: nothing written


def test_engine_remove_images_rewrites_the_files(bound_engine):
    import image_search_engine_amd.faiss_compat as faiss

    engine, xb, tmp = bound_engine
    paths = list(engine.images_paths)
    engine.index_file = tmp / "i.faiss"
    faiss.write_index(engine.index, engine.index_file)
    with open(engine.paths_file_for(engine.index_file), "w") as f:
        json.dump({"ntotal": 8, "index_crc32": engine.file_crc32(engine.index_file), "paths": [str(p) for p in paths]}, f)
    assert engine.remove_images([paths[0], paths[7]]) == 2
    with open(engine.paths_file_for(engine.index_file)) as f:
        rec = json.load(f)
    assert rec["ntotal"] == 6 and rec["paths"] == [str(p) for p in paths[1:7]]
    assert rec["index_crc32"] == engine.file_crc32(engine.index_file)
    with open(engine.index_file, "rb") as f:
        d, metric, rows = faiss.parse_flat(f.read())
    assert np.array_equal(rows, xb[1:7])
    assert engine.read_paths_file(engine.index_file, 6) == paths[1:7]  # what engine.load accepts
