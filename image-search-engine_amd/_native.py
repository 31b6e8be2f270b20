"""ctypes binding of the gfx950 kNN library (include/ise_knn.h).

The product path has no CPU fallback: if ``csrc/libise_knn.so`` is missing the
import of this module raises, and if no MI355X is visible every entry point
that computes raises ``RuntimeError`` with the library's message.
"""
from __future__ import annotations

import ctypes
import os

# PyTorch-ROCm bundles its own libamdhip64.so.7; importing torch first makes
# this library bind to the same HIP runtime, so torch device pointers and
# streams can be handed straight through the C ABI.
import torch  # noqa: F401  (must precede the CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
# $ISE_KNN_LIB selects a dev build of the same library (e.g. csrc/libise_knn_ablate.so)
LIB_PATH = os.environ.get("ISE_KNN_LIB") or os.path.join(_HERE, "csrc", "libise_knn.so")

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1
MAX_K = 2048
PQ_MAX_M = 64
SQ_MAX_D = 2048
LINEAR_MAX_D = 4096
LINEAR_FEW_ROWS = 64  # n <= this: the few-row launch shape of ise_linear_apply_*
LINEAR_KSEG = 256  # k entries of one fmaf chain of ise_linear_apply_*
SQ_8BIT, SQ_8BIT_UNIFORM = 0, 2
STORE_F32, STORE_BF16 = 0, 1

E_INVALID, E_HIP, E_NOMEM, E_NODEVICE = -1, -2, -3, -4

# every symbol include/ise_knn.h declares: (name, restype, argtypes)
_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
PROTOTYPES = [
    ("ise_version", _int, []),
    ("ise_last_error", ctypes.c_char_p, []),
    ("ise_device_count", _int, [ctypes.POINTER(_int)]),
    ("ise_device_arch", _int, [_int, ctypes.c_char_p, _int]),
    ("ise_index_create", _int, [ctypes.POINTER(_vp), _int, _int, _int]),
    ("ise_index_create_ex", _int, [ctypes.POINTER(_vp), _int, _int, _int, _int]),
    ("ise_index_destroy", _int, [_vp]),
    ("ise_index_reset", _int, [_vp]),
    ("ise_index_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), _i64p, ctypes.POINTER(_int)]),
    ("ise_index_set_shift", _int, [_vp, _vp]),
    ("ise_index_get_shift", _int, [_vp, _vp]),
    ("ise_index_stats", _int, [_vp, _u64p]),
    ("ise_index_gemm_stats", _int, [_vp, _u64p]),
    ("ise_index_host_stats", _int, [_vp, _u64p]),
    ("ise_index_reserve_workspaces", _int, [_vp, _i64, _int]),
    ("ise_index_add_host", _int, [_vp, _vp, _i64]),
    ("ise_index_add_device", _int, [_vp, _vp, _i64, _vp]),
    ("ise_index_reconstruct_host", _int, [_vp, _i64, _i64, _vp]),
    ("ise_index_search_host", _int, [_vp, _vp, _i64, _int, _vp, _vp]),
    ("ise_index_search_device", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    ("ise_index_search_keys_device", _int, [_vp, _vp, _i64, _int, ctypes.c_uint32, _vp, _vp]),
    ("ise_index_assign_device", _int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    ("ise_merge_keys_device", _int, [_vp, _int, _i64, _int, _int, _vp, _vp, _int, _vp]),
    ("ise_normalize_rows_device", _int, [_vp, _i64, _int, _int, _vp]),
    ("ise_normalize_rows_host", _int, [_vp, _i64, _int, _int]),
    ("ise_bovw_histogram_device", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp]),
    ("ise_index_short_stats", _int, [_vp, _vp]),
    ("ise_index_half_stats", _int, [_vp, _u64p]),
    ("ise_index_shadow_row", _int, [_vp, _i64, _f32p]),
    ("ise_index_byte_stats", _int, [_vp, _u64p]),
    ("ise_index_depth_stats", _int, [_vp, _u64p]),
    ("ise_index_byte_row", _int, [_vp, _i64, _f32p]),
    ("ise_index_byte_row_codes", _int, [_vp, _i64, _vp]),
    ("ise_index_stage_query_debug", _int, [_vp, _vp, _int, _vp, _i64, _f32p, ctypes.POINTER(ctypes.c_int32)]),
    ("ise_index_range_search_host", _int, [_vp, _vp, _i64, ctypes.c_float, ctypes.POINTER(_vp)]),
    ("ise_range_result_get", _int, [_vp, _i64p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    ("ise_range_result_destroy", _int, [_vp]),
    ("ise_index_range_stats", _int, [_vp, _u64p]),
    ("ise_index_remove_ids_host", _int, [_vp, _vp, _i64, _i64p]),
    ("ise_index_remove_range", _int, [_vp, _i64, _i64, _i64p]),
    ("ise_index_remove_stats", _int, [_vp, _u64p]),
    ("ise_index_remove_last_timing", _int, [_vp, _f32p, _u64p]),
    ("ise_selector_create_range", _int, [_vp, _i64, _i64, ctypes.POINTER(_vp)]),
    ("ise_selector_create_ids", _int, [_vp, _vp, _i64, _int, ctypes.POINTER(_vp)]),
    ("ise_selector_create_bitmap", _int, [_vp, _vp, _i64, ctypes.POINTER(_vp)]),
    ("ise_selector_info", _int, [_vp, _i64p]),
    ("ise_selector_destroy", _int, [_vp]),
    ("ise_index_search_sel_device", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    ("ise_index_search_sel_host", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    ("ise_index_range_search_sel_host", _int, [_vp, _vp, _i64, ctypes.c_float, _vp, ctypes.POINTER(_vp)]),
    ("ise_index_sel_stats", _int, [_vp, _u64p]),
    ("ise_index_search_subset_device", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp]),
    ("ise_index_search_subset_host", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp]),
    ("ise_index_distance_subset_device", _int, [_vp, _vp, _i64, _vp, _int, _vp, _vp]),
    ("ise_index_distance_subset_host", _int, [_vp, _vp, _i64, _vp, _int, _vp]),
    ("ise_index_subset_stats", _int, [_vp, _u64p]),
    ("ise_binary_index_create", _int, [ctypes.POINTER(_vp), _int, _int]),
    ("ise_binary_index_destroy", _int, [_vp]),
    ("ise_binary_index_reset", _int, [_vp]),
    ("ise_binary_index_info", _int, [_vp, ctypes.POINTER(_int), _i64p, ctypes.POINTER(_int)]),
    ("ise_binary_index_add_host", _int, [_vp, _vp, _i64]),
    ("ise_binary_index_add_device", _int, [_vp, _vp, _i64, _vp]),
    ("ise_binary_index_reconstruct_host", _int, [_vp, _i64, _i64, _vp]),
    ("ise_binary_index_search_host", _int, [_vp, _vp, _i64, _int, _vp, _vp]),
    ("ise_binary_index_search_device", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    ("ise_binary_index_range_search_host", _int, [_vp, _vp, _i64, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("ise_binary_range_result_get", _int, [_vp, _i64p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    ("ise_binary_range_result_destroy", _int, [_vp]),
    ("ise_binary_index_stats", _int, [_vp, _u64p]),
    ("ise_binary_index_remove_ids_host", _int, [_vp, _vp, _i64, _i64p]),
    ("ise_binary_index_remove_range", _int, [_vp, _i64, _i64, _i64p]),
    ("ise_binary_index_remove_stats", _int, [_vp, _u64p]),
    ("ise_binary_selector_create_range", _int, [_vp, _i64, _i64, ctypes.POINTER(_vp)]),
    ("ise_binary_selector_create_ids", _int, [_vp, _vp, _i64, _int, ctypes.POINTER(_vp)]),
    ("ise_binary_selector_create_bitmap", _int, [_vp, _vp, _i64, ctypes.POINTER(_vp)]),
    ("ise_binary_selector_info", _int, [_vp, _i64p]),
    ("ise_binary_selector_destroy", _int, [_vp]),
    ("ise_binary_index_search_sel_host", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    ("ise_binary_index_search_sel_device", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    ("ise_binary_index_range_search_sel_host", _int, [_vp, _vp, _i64, ctypes.c_int32, _vp, ctypes.POINTER(_vp)]),
    ("ise_binary_index_sel_stats", _int, [_vp, _u64p]),
    ("ise_ivf_create", _int, [ctypes.POINTER(_vp), _int, _int, _int, _int]),
    ("ise_ivf_destroy", _int, [_vp]),
    ("ise_ivf_reset", _int, [_vp]),
    ("ise_ivf_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), _i64p, ctypes.POINTER(_int)]),
    ("ise_ivf_add_host", _int, [_vp, _vp, _vp, _i64]),
    ("ise_ivf_add_device", _int, [_vp, _vp, _vp, _i64, _vp]),
    ("ise_ivf_list_sizes_host", _int, [_vp, _vp]),
    ("ise_ivf_list_host", _int, [_vp, _int, _vp, _vp]),
    ("ise_ivf_search_device", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp]),
    ("ise_ivf_search_host", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp]),
    ("ise_ivf_stats", _int, [_vp, _u64p]),
    ("ise_pq_create", _int, [ctypes.POINTER(_vp), _int, _int, _int, _int, _int]),
    ("ise_pq_destroy", _int, [_vp]),
    ("ise_pq_reset", _int, [_vp]),
    ("ise_pq_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), _i64p,
                           ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    ("ise_pq_set_centroids_host", _int, [_vp, _vp]),
    ("ise_pq_get_centroids_host", _int, [_vp, _vp]),
    ("ise_pq_encode_host", _int, [_vp, _vp, _i64, _vp]),
    ("ise_pq_encode_device", _int, [_vp, _vp, _i64, _vp, _vp]),
    ("ise_pq_decode_host", _int, [_vp, _vp, _i64, _vp]),
    ("ise_pq_add_host", _int, [_vp, _vp, _i64]),
    ("ise_pq_add_device", _int, [_vp, _vp, _i64, _vp]),
    ("ise_pq_add_codes_host", _int, [_vp, _vp, _i64]),
    ("ise_pq_codes_host", _int, [_vp, _i64, _i64, _vp]),
    ("ise_pq_reconstruct_host", _int, [_vp, _i64, _i64, _vp]),
    ("ise_pq_search_host", _int, [_vp, _vp, _i64, _int, _vp, _vp]),
    ("ise_pq_search_device", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    ("ise_pq_stats", _int, [_vp, _u64p]),
    ("ise_sq_create", _int, [ctypes.POINTER(_vp), _int, _int, _int, _int]),
    ("ise_sq_destroy", _int, [_vp]),
    ("ise_sq_reset", _int, [_vp]),
    ("ise_sq_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), _i64p, ctypes.POINTER(_int),
                           ctypes.POINTER(_int)]),
    ("ise_sq_set_trained_host", _int, [_vp, _vp]),
    ("ise_sq_get_trained_host", _int, [_vp, _vp]),
    ("ise_sq_encode_host", _int, [_vp, _vp, _i64, _vp]),
    ("ise_sq_encode_device", _int, [_vp, _vp, _i64, _vp, _vp]),
    ("ise_sq_decode_host", _int, [_vp, _vp, _i64, _vp]),
    ("ise_sq_add_host", _int, [_vp, _vp, _i64]),
    ("ise_sq_add_device", _int, [_vp, _vp, _i64, _vp]),
    ("ise_sq_add_codes_host", _int, [_vp, _vp, _i64]),
    ("ise_sq_codes_host", _int, [_vp, _i64, _i64, _vp]),
    ("ise_sq_reconstruct_host", _int, [_vp, _i64, _i64, _vp]),
    ("ise_sq_search_host", _int, [_vp, _vp, _i64, _int, _vp, _vp]),
    ("ise_sq_search_device", _int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    ("ise_sq_stats", _int, [_vp, _u64p]),
    ("ise_ivfsq_create", _int, [ctypes.POINTER(_vp), _int, _int, _int, _int, _int]),
    ("ise_ivfsq_destroy", _int, [_vp]),
    ("ise_ivfsq_reset", _int, [_vp]),
    ("ise_ivfsq_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), _i64p,
                              ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    ("ise_ivfsq_set_trained_host", _int, [_vp, _vp]),
    ("ise_ivfsq_get_trained_host", _int, [_vp, _vp]),
    ("ise_ivfsq_add_host", _int, [_vp, _vp, _vp, _i64]),
    ("ise_ivfsq_add_device", _int, [_vp, _vp, _vp, _i64, _vp]),
    ("ise_ivfsq_add_codes_host", _int, [_vp, _vp, _vp, _i64]),
    ("ise_ivfsq_list_sizes_host", _int, [_vp, _vp]),
    ("ise_ivfsq_list_host", _int, [_vp, _int, _vp, _vp]),
    ("ise_ivfsq_search_host", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp]),
    ("ise_ivfsq_search_device", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp]),
    ("ise_ivfsq_stats", _int, [_vp, _u64p]),
    ("ise_ivfpq_create", _int, [ctypes.POINTER(_vp), _int, _int, _int, _int, _int, _int]),
    ("ise_ivfpq_destroy", _int, [_vp]),
    ("ise_ivfpq_reset", _int, [_vp]),
    ("ise_ivfpq_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int),
                              ctypes.POINTER(_int), _i64p, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    ("ise_ivfpq_set_centroids_host", _int, [_vp, _vp]),
    ("ise_ivfpq_get_centroids_host", _int, [_vp, _vp]),
    ("ise_ivfpq_add_host", _int, [_vp, _vp, _vp, _i64]),
    ("ise_ivfpq_add_device", _int, [_vp, _vp, _vp, _i64, _vp]),
    ("ise_ivfpq_add_codes_host", _int, [_vp, _vp, _vp, _i64]),
    ("ise_ivfpq_list_sizes_host", _int, [_vp, _vp]),
    ("ise_ivfpq_list_host", _int, [_vp, _int, _vp, _vp]),
    ("ise_ivfpq_search_host", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp]),
    ("ise_ivfpq_search_device", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp]),
    ("ise_ivfpq_stats", _int, [_vp, _u64p]),
    ("ise_binary_ivf_create", _int, [ctypes.POINTER(_vp), _int, _int, _int]),
    ("ise_binary_ivf_destroy", _int, [_vp]),
    ("ise_binary_ivf_reset", _int, [_vp]),
    ("ise_binary_ivf_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), _i64p, ctypes.POINTER(_int)]),
    ("ise_binary_ivf_add_host", _int, [_vp, _vp, _vp, _i64]),
    ("ise_binary_ivf_add_device", _int, [_vp, _vp, _vp, _i64, _vp]),
    ("ise_binary_ivf_list_sizes_host", _int, [_vp, _vp]),
    ("ise_binary_ivf_list_host", _int, [_vp, _int, _vp, _vp]),
    ("ise_binary_ivf_search_host", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp]),
    ("ise_binary_ivf_search_device", _int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp]),
    ("ise_binary_ivf_stats", _int, [_vp, _u64p]),
    ("ise_linear_create", _int, [ctypes.POINTER(_vp), _int, _int, _vp, _vp, _int]),
    ("ise_linear_destroy", _int, [_vp]),
    ("ise_linear_info", _int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    ("ise_linear_apply_device", _int, [_vp, _vp, _i64, _vp, _vp]),
    ("ise_linear_apply_host", _int, [_vp, _vp, _i64, _vp]),
    ("ise_linear_stats", _int, [_vp, _u64p]),
    ("ise_refresh_env_knobs", _int, []),
    ("ise_comm_precheck", _int, [_int]),
    ("ise_comm_unique_id", _int, [_vp]),
    ("ise_comm_create", _int, [ctypes.POINTER(_vp), _vp, _int, _int, _int]),
    ("ise_comm_allgather_keys", _int, [_vp, _vp, _vp, _i64, _vp]),
    ("ise_comm_destroy", _int, [_vp]),
    ("ise_index_search_timed_device", _int,
     [_vp, _vp, _i64, _int, _vp, _vp, _vp, _int, _f32p, _f32p]),
]

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (or "
        f"`make -C {os.path.join(_HERE, 'csrc')}`). There is no CPU fallback for the kNN path."
    )

lib = ctypes.CDLL(LIB_PATH)
for _name, _res, _args in PROTOTYPES:
    _fn = getattr(lib, _name)  # AttributeError here = the .so is stale
    _fn.restype = _res
    _fn.argtypes = _args


class IseError(RuntimeError):
    """Error reported through the C ABI (Faiss surfaces C++ errors as RuntimeError too)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"ise_knn error {code}: {msg}")
        self.code = code


def check(rc: int) -> None:
    if rc != 0:
        raise IseError(rc, lib.ise_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    n = _int(0)
    rc = lib.ise_device_count(ctypes.byref(n))
    return int(n.value) if rc == 0 else 0
