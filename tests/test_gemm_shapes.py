"""CPU tests of tests/gemm_ref.py and of the case tables of tests/test_gemm_shapes_gpu.py: every case the GPU file
calls "on" the large-batch path is on it by the restated gate, every "off" case off, and the tail lengths hit the
residue classes they are there for."""
import re

import pytest

from tests import gemm_ref as gr
from tests import test_gemm_shapes_gpu as cases

L2, IP = gr.L2, gr.IP
N1 = gr.GEMM_MIN_ROWS + 1


def test_pad_dim_and_the_ranges_of_d_the_gate_admits():
    f32 = [d for d in range(1, 600) if gr.pad_dim(d, "f32") % 128 == 0 and gr.pad_dim(d, "f32") <= 512]
    assert f32 == [*range(65, 129), *range(193, 257), *range(321, 385), *range(449, 513)]
    bf16 = [d for d in range(1, 600) if gr.pad_dim(d, "bf16") % 128 == 0 and gr.pad_dim(d, "bf16") <= 512]
    assert bf16 == list(range(97, 513))
    assert [gr.pad_dim(d, "f32") for d in (64, 65, 129, 257, 449)] == [64, 128, 192, 320, 512]
    assert [gr.pad_dim(d, "bf16") for d in (96, 97, 128, 129, 512, 513)] == [96, 128, 128, 256, 512, 640]


def test_constants_match_the_sources():
    """The gate's constants, read from the sources they restate."""
    import os

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-search-engine_amd", "csrc")
    knn = open(os.path.join(csrc, "ise_knn.hip")).read()
    scan = open(os.path.join(csrc, "ise_gemm_scan.hpp")).read()
    bf16 = open(os.path.join(csrc, "ise_gemm_bf16.hpp")).read()
    flat = open(os.path.join(csrc, "ise_flat.hpp")).read()

    def define(src, name):
        return int(re.search(rf"#define {name} (\d+)", src).group(1))

    assert define(knn, "GEMM_MIN_NQ") == gr.GEMM_MIN_NQ
    assert define(knn, "GEMM_CAPQ") == gr.GEMM_CAPQ
    assert define(scan, "GEMM_NQ_MAX") == gr.GEMM_NQ_MAX
    assert define(flat, "XPASS_MAX") == gr.XPASS_MAX
    assert (define(scan, "GQ"), define(bf16, "GB_GQ")) == (gr.STAGE["f32"], gr.STAGE["bf16"])
    assert 8 * define(bf16, "GB_XT") * 16 == gr.SLAB["bf16"]
    assert "h->n < 128ll * 1024" in knn and gr.GEMM_MIN_ROWS == 128 * 1024
    assert "std::min<long long>(min_nq, 128)" in knn and gr.GEMM_MIN_NQ_BF16 == 128
    assert "h->dp > 512 || h->dp % 128 != 0" in knn and (gr.GEMM_DP_MAX, gr.GEMM_DP_STEP) == (512, 128)


@pytest.mark.parametrize("metric,storage", cases.FLAVOURS)
def test_gate_edges(metric, storage):
    nq_min = 128 if storage == "bf16" else 256
    k_max = 28 if (metric == L2 and storage == "f32") else 32
    on = dict(n=gr.GEMM_MIN_ROWS, d=100, storage=storage, metric=metric, nq=nq_min, k=k_max)
    assert gr.expects_gemm(**on)
    for change in (dict(n=gr.GEMM_MIN_ROWS - 1), dict(nq=nq_min - 1), dict(k=k_max + 1), dict(d=64), dict(d=513)):
        assert not gr.expects_gemm(**{**on, **change}), change
    assert [gr.chunks(nq) for nq in (1, 1024, 1025, 2048, 2049)] == [1, 1, 2, 2, 3]


def test_every_on_case_is_on_and_every_off_case_off():
    assert (cases.BASE, cases.D0, cases.NQ0, cases.K0) == (gr.GEMM_MIN_ROWS, 100, 256, 10)
    for metric, storage in cases.FLAVOURS:
        for r in (0,) + cases.WALK[storage]:
            assert gr.expects_gemm(cases.BASE + r, cases.D0, storage, metric, cases.NQ0, cases.K0)
        for d in cases.DIMS_ON[storage]:
            assert gr.expects_gemm(N1, d, storage, metric, cases.NQ0, cases.K0), d
            assert d < gr.pad_dim(d, storage), "the case is about d below dp"
        for d in cases.DIMS_OFF[storage]:
            assert not gr.expects_gemm(N1, d, storage, metric, cases.NQ0, cases.K0), d
        # (f): on after the first removal, off after the second
        assert gr.expects_gemm(cases.BASE + 5, cases.D0, storage, metric, cases.NQ0, cases.K0)
        assert not gr.expects_gemm(cases.BASE - 1, cases.D0, storage, metric, cases.NQ0, cases.K0)
    assert sorted(set(cases.DIM_CASES)) == cases.DIM_CASES
    assert len(cases.DIM_CASES) == 2 * sum(len(t[s]) for t in (cases.DIMS_ON, cases.DIMS_OFF) for s in ("f32", "bf16"))
    for d, metric, storage, on in cases.DIM_CASES:
        assert gr.expects_gemm(N1, d, storage, metric, cases.NQ0, cases.K0) == on
    # every padded dimension of the ladders is met with d < dp: 128, 256, 384, 512
    for storage in ("f32", "bf16"):
        assert {gr.pad_dim(d, storage) for d in cases.DIMS_ON[storage]} == {128, 256, 384, 512}
    assert any(d % 2 for d in cases.DIMS_ON["bf16"]), "an odd d: the half pair of the bf16 query prep"
    for metric, storage, nq in cases.NQ_EDGE_CASES:
        assert gr.expects_gemm(N1, cases.D0, storage, metric, nq, cases.K0), nq
    for storage in ("f32", "bf16"):  # every batch size runs for L2, all but 1025 for the inner product too
        for metric in (L2, IP):
            got = {nq for m, s, nq in cases.NQ_EDGE_CASES if (m, s) == (metric, storage)}
            assert got == set(cases.NQ_EDGES[storage]) - (set() if metric == L2 else {1025})
    assert sorted((m, s) for m, s, _, _ in cases.K_GATE) == sorted(cases.FLAVOURS)
    for metric, storage, k_on, k_off in cases.K_GATE:
        assert k_off == k_on + 1 <= cases.KREF
        assert gr.expects_gemm(N1, cases.D0, storage, metric, cases.NQ0, k_on)
        assert not gr.expects_gemm(N1, cases.D0, storage, metric, cases.NQ0, k_off)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_the_tail_lengths_hit_their_residue_classes(storage):
    """A lane's four rows: one row, all but one, all four.  A 16-row tile and a slab: one row, all but one, all,
    one more (bf16: also a wave's pair of tiles, 32 rows)."""
    walk, slab = cases.WALK[storage], gr.SLAB[storage]
    assert gr.GEMM_MIN_ROWS % slab == 0 and list(walk) == sorted(set(walk))
    assert {r % gr.QUAD for r in walk} >= {0, 1, gr.QUAD - 1}
    units = (gr.TILE, slab) + ((2 * gr.TILE,) if storage == "bf16" else ())
    for unit in units:
        assert {1, unit - 1, unit, unit + 1} <= set(walk), unit
        assert {r % unit for r in walk} >= {0, 1, unit - 1}
    assert walk[0] == 1, "a slab of a single row"
    assert max(walk) > cases.NQ0 or storage == "f32"  # bf16: a second copy of query 0 behind the first


def test_batch_sizes_split_their_stages_unevenly():
    """The threshold sample splits a chunk's stages over qparts blocks per slab (256 CUs: 128 float32 slabs -> up to
    4 parts, 64 bf16 slabs -> up to 8): 257 float32 queries are 9 stages over 4 parts, 129 bf16 queries 3 stages
    over 3 parts; the chunk behind 1024 queries is one stage in one part."""
    assert gr.stage_split(257, "f32") == [2, 2, 2, 3]
    assert gr.stage_split(287, "f32") == [2, 2, 2, 3]
    assert gr.stage_split(129, "bf16") == [1, 1, 1]
    assert gr.stage_split(128, "bf16") == [1, 1]
    assert gr.stage_split(191, "bf16") == [1, 1, 1]
    assert gr.stage_split(1, "f32") == [1] and gr.stage_split(1, "bf16") == [1]
    assert gr.stage_split(1024, "f32") == [8, 8, 8, 8] and gr.stage_split(1024, "bf16") == [2] * 8
    assert {257, 287, 1025} <= set(cases.NQ_EDGES["f32"]) and {128, 129, 191, 1025} <= set(cases.NQ_EDGES["bf16"])
