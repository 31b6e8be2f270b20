"""Restatement of the large-batch path's gate (tests only; no numpy): which (index, batch) shapes
``search_large_chunk`` answers.  Every constant names its source in csrc/."""
from tests.rerank_ref import pad_dim as _pad_dim_f32

GEMM_MIN_ROWS = 128 * 1024      # gemm_applies (csrc/ise_knn.hip): h->n < 128ll * 1024 stays on the streaming passes
GEMM_MIN_NQ = 256               # GEMM_MIN_NQ (csrc/ise_knn.hip)
GEMM_MIN_NQ_BF16 = 128          # gemm_applies: std::min(min_nq, 128) for bf16 rows
GEMM_NQ_MAX = 1024              # GEMM_NQ_MAX (csrc/ise_gemm_scan.hpp): queries per chunk
GEMM_DP_STEP, GEMM_DP_MAX = 128, 512  # gemm_applies: dp % 128 == 0 and dp <= 512
XPASS_MAX = 32                  # XPASS_MAX (csrc/ise_flat.hpp)
EXACT_EXTRA = 4                 # exact_extra (csrc/ise_knn.hip): spare candidates of the float32 L2 re-rank
GEMM_CAPQ = 4096                # GEMM_CAPQ (csrc/ise_knn.hip): candidate slots per query
L2, IP = 1, 0                   # ISE_METRIC_L2, ISE_METRIC_INNER_PRODUCT (include/ise_knn.h)

# rows per slab, per tile and per lane of a tile (csrc/ise_gemm_scan.hpp: 8 waves x 16 rows; csrc/ise_gemm_bf16.hpp:
# 8 waves x GB_XT = 2 tiles of 16 rows), and queries per LDS stage (GQ, GB_GQ)
SLAB = {"f32": 128, "bf16": 256}
TILE, QUAD = 16, 4
STAGE = {"f32": 32, "bf16": 64}


def pad_dim(d: int, storage: str = "f32") -> int:
    """dp (csrc/ise_geometry.hpp, pad_dim): whole 64-byte k-steps, whole groups of four of them beyond four."""
    if storage == "f32":
        return _pad_dim_f32(d)
    steps = -(-d // 32)
    return (-(-steps // 4) * 4 if steps > 4 else steps) * 32


def expects_gemm(n: int, d: int, storage: str, metric: int, nq: int, k: int) -> bool:
    """gemm_applies (csrc/ise_knn.hip) with the default environment."""
    bf16 = storage == "bf16"
    if nq < (GEMM_MIN_NQ_BF16 if bf16 else GEMM_MIN_NQ) or n < GEMM_MIN_ROWS:
        return False
    dp = pad_dim(d, storage)
    if dp > GEMM_DP_MAX or dp % GEMM_DP_STEP != 0:
        return False
    if not bf16 and metric == L2:  # uses_shift: the select stage hands at most XPASS_MAX candidates to the re-rank
        return k + EXACT_EXTRA <= XPASS_MAX
    return k <= XPASS_MAX


def chunks(nq: int) -> int:
    """search_enqueue: chunks of GEMM_NQ_MAX queries."""
    return -(-nq // GEMM_NQ_MAX)


def stage_split(nq: int, storage: str, num_cu: int = 256, slabs: int = None) -> list:
    """Stages per part of the threshold sample of a chunk of nq queries (search_large_chunk: qparts = min(stages,
    2 num_cu / sampled slabs), part p takes the stages [p * stages / qparts, (p + 1) * stages / qparts))."""
    stages = -(-nq // STAGE[storage])
    if slabs is None:
        slabs = 128 * 128 // SLAB[storage]  # GEMM_SAMPLE_SLABS * 128 / rows per slab
    qparts = max(1, min(stages, 2 * num_cu // slabs))
    return [(p + 1) * stages // qparts - p * stages // qparts for p in range(qparts)]
