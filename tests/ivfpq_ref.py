"""numpy reference of the inverted-list index over product-quantiser codes (tests only): the expected results --
the complete float64 ranking over ``pq_ref.decode(codes)`` (or the table-lookup scores ``pq_ref.adc_scores``) cut to
``ivf_ref.probed_members`` -- which 64-row tiles a pass visits, and the statistics a search adds."""
import numpy as np

from tests import ivf_ref, ivfsq_ref, pq_ref
from tests.knn_checks import brute_knn

TILE_ROWS = ivfsq_ref.TILE_ROWS  # 64: a wave's unit in the scan
TAB_CHUNK = 64                   # queries per table build
KPASS = 32                       # results per pass


def full_ranking(xq, C, codes, metric):
    """(D, I) of every query against every decoded row: the complete ranking, float64 brute force."""
    dec = pq_ref.decode(codes, C)
    return brute_knn(dec, np.asarray(xq, np.float32), len(dec), metric)


def expected(xq, C, codes, probes, assign, nlist: int, k: int, metric: int, full=None):
    """-> (D, I): the k best of each query's probed members by the score against the decoded rows.  ``full``: the
    complete ranking ``full_ranking(xq, C, codes, metric)``, if the caller keeps one."""
    if full is None:
        full = full_ranking(xq, C, codes, metric)
    members = ivf_ref.probed_members(probes, assign, nlist)
    return ivf_ref.expected_from_ranking(full[0], full[1], members, k, metric)


def expected_adc(xq, C, codes, probes, assign, nlist: int, k: int, metric: int):
    """The same from the table-lookup definition: ``pq_ref.adc_scores`` restricted per query to its probed members."""
    scores = pq_ref.adc_scores(xq, C, codes, metric)
    members = ivf_ref.probed_members(probes, assign, nlist)
    D = np.empty((len(members), k), np.float32)
    I = np.empty((len(members), k), np.int64)
    for q, mem in enumerate(members):
        Dq, Iq = pq_ref.adc_topk(scores[q:q + 1, mem], k, metric)
        D[q] = Dq[0]
        I[q] = np.where(Iq[0] >= 0, mem[np.maximum(Iq[0], 0)], -1) if len(mem) else -1
    return D, I


def pass_tile_counts(probes, sizes, M: int) -> list:
    """Per group of QT(M) queries, the tiles a pass visits: every tile of every list that at least one query of the
    group names (``ivfsq_ref.masks_of``: entries outside [0, nlist) name nothing, a list named twice counts once)."""
    masks = ivfsq_ref.masks_of(probes, len(sizes), pq_ref.qt_of(M))
    sizes = np.asarray(sizes)
    return [ivfsq_ref.tiles_of(sizes[gm != 0]) for gm in masks]


def stats_of(probes, sizes, M: int, k: int, nq: int) -> dict:
    """What one search call of ``nq`` queries adds to ``ivfpq_stats`` on an index that holds rows."""
    probes = np.asarray(probes, dtype=np.int64).reshape(nq, -1)
    qt, per = pq_ref.qt_of(M), -(-int(k) // KPASS)
    passes = sum(-(-min(TAB_CHUNK, nq - c0) // qt) * per for c0 in range(0, nq, TAB_CHUNK))
    counts = pass_tile_counts(probes, sizes, M)
    assert len(counts) * per == passes  # a chunk is whole groups
    return {"batches": 1, "passes": passes, "tiles_loaded": sum(counts) * per, "table_builds": -(-nq // TAB_CHUNK)}
