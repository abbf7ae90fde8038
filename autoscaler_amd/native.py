"""Loader and thin object wrapper of ``libcasim.so`` (the MI355X product path).

There is no fallback: if the in-tree library is missing, or no HIP device is
visible, every constructor raises.  The wrapper only marshals numpy arrays into
the C ABI of ``include/casim.h``; all simulation work happens in the library.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import ptr

_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libcasim.so")


# ca_estimate_plan_option_sums (csrc/expander.hip): list positions per block, and the most
# score classes a block counts in LDS (above: a gather per id)
OPTION_SUMS_TILE = 2048
OPTION_SUMS_LDS_CLASSES = 2048
# ca_estimate_plan_option_price_sums (csrc/expander.hip): list positions a wave hands to its add
# chain per step, and options (waves) per block
PRICE_SUMS_CHUNK = 256
PRICE_SUMS_WAVES = 4
# ca_estimate_plan_groups_missing_pods (csrc/nodegroupset.hip): list positions per block, the
# most candidate rows one block of the test kernel walks, and the default bound on the bitmap
# rows resident at once (bytes; CASIM_MISSING_SCRATCH under CASIM_KNOBS overrides it per call)
MISSING_PODS_TILE = 2048
MISSING_PODS_ROWS = 64
MISSING_PODS_SCRATCH = 64 << 20


class CasimError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: status {status} ({_status_string(status)})")


def _status_string(status: int) -> str:
    try:
        return load().ca_status_string(status).decode()
    except Exception:  # pragma: no cover - only while the library is unusable
        return "?"


def load() -> C.CDLL:
    """Load the in-tree libcasim.so (raises if it was not built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("CASIM_LIB_PATH", LIB_PATH)    # diagnostics builds only (Makefile: prof)
    if not os.path.exists(path):
        raise RuntimeError(f"libcasim.so not built: {path} missing (run __graft_entry__.build())")
    lib = C.CDLL(path)
    vp, i32, p = C.c_void_p, C.c_int32, C.POINTER
    sigs = {
        "ca_abi_version": ([], C.c_int),
        "ca_abi_struct_sizes": ([p(i32), i32], C.c_int),
        "ca_device_count": ([p(i32)], C.c_int),
        "ca_status_string": ([C.c_int], C.c_char_p),
        "ca_host_alloc": ([C.c_size_t, p(vp)], C.c_int),
        "ca_host_free": ([vp], C.c_int),
        "ca_mirror_create": ([i32, p(vp)], C.c_int),
        "ca_mirror_destroy": ([vp], C.c_int),
        "ca_mirror_clear": ([vp], C.c_int),
        "ca_mirror_add_nodes": ([vp, vp, i32, p(i32)], C.c_int),
        "ca_mirror_add_pods": ([vp, vp, vp, vp, i32, vp], C.c_int),
        "ca_mirror_remove_pod": ([vp, i32], C.c_int),
        "ca_mirror_remove_node": ([vp, i32], C.c_int),
        "ca_mirror_scope_blockers": ([vp, p(i32)], C.c_int),
        "ca_mirror_fork": ([vp], C.c_int),
        "ca_mirror_revert": ([vp], C.c_int),
        "ca_mirror_commit": ([vp], C.c_int),
        "ca_mirror_node_count": ([vp, p(i32)], C.c_int),
        "ca_mirror_pod_node": ([vp, i32, p(i32)], C.c_int),
        "ca_mirror_node_pods": ([vp, i32, vp, i32, p(i32)], C.c_int),
        "ca_podset_create": ([vp, vp, p(vp)], C.c_int),
        "ca_podset_destroy": ([vp], C.c_int),
        "ca_fits_any_node": ([vp, vp, i32, vp, p(i32), p(i32), p(i32), p(C.c_uint64)], C.c_int),
        "ca_check_predicates": ([vp, vp, i32, i32, vp], C.c_int),
        "ca_fits_matrix": ([vp, vp, vp], C.c_int),
        "ca_check_templates": ([vp, vp, vp, i32, vp, i32, vp, vp], C.c_int),
        "ca_expansion_plan_create": ([vp, vp, i32, p(vp)], C.c_int),
        "ca_expansion_plan_run": ([vp, vp, vp, i32, vp, vp], C.c_int),
        "ca_expansion_plan_destroy": ([vp], C.c_int),
        "ca_expansion_plan_kernel_ms": ([vp, p(C.c_float)], C.c_int),
        "ca_estimate_batch": ([vp, vp, vp, vp, vp, i32, vp, p(i32), vp, vp, vp], C.c_int),
        "ca_estimate_plan_create": ([vp, vp, vp, vp, vp, i32, p(vp)], C.c_int),
        "ca_estimate_plan_create_options": ([vp, vp, vp, vp, i32, vp, vp, i32, vp, p(vp)], C.c_int),
        "ca_estimate_plan_fetch_lists": ([vp, vp, vp], C.c_int),
        "ca_estimate_plan_fetch_class_counts": ([vp, vp, p(i32)], C.c_int),
        "ca_pod_groups_create": ([vp, vp, vp, i32, vp, vp, i32, p(vp)], C.c_int),
        "ca_pod_groups_info": ([vp, p(i32), p(i32)], C.c_int),
        "ca_pod_groups_fetch": ([vp, vp, vp], C.c_int),
        "ca_pod_groups_timings": ([vp, p(C.c_float), i32], C.c_int),
        "ca_pod_groups_destroy": ([vp], C.c_int),
        "ca_expansion_plan_run_groups": ([vp, vp, vp, vp, vp], C.c_int),
        "ca_estimate_plan_create_groups": ([vp, vp, vp, vp, vp, i32, vp, p(vp)], C.c_int),
        "ca_estimate_plan_run": ([vp, vp, p(i32), vp, vp, vp], C.c_int),
        "ca_estimate_plan_run_u16": ([vp, vp, p(i32), vp, vp], C.c_int),
        "ca_estimate_plan_destroy": ([vp], C.c_int),
        "ca_estimate_plan_fetch": ([vp, vp], C.c_int),
        "ca_estimate_plan_device_results": ([vp, p(vp)], C.c_int),
        "ca_estimate_plan_stats": ([vp, p(i32), p(C.c_float), p(C.c_float), p(C.c_float)], C.c_int),
        "ca_estimate_plan_chain_info": ([vp, p(i32), p(i32)], C.c_int),
        "ca_estimate_plan_rebase": ([vp, vp, i32, p(i32)], C.c_int),
        "ca_go_sort_ranks": ([i32, vp, i32, i32, i32, vp], C.c_int),
        "ca_go_sort_ranks_fan": ([i32, vp, i32, i32, i32, i32, vp, p(i32)], C.c_int),
        "ca_estimate_plan_timings": ([vp, p(C.c_float), i32], C.c_int),
        "ca_estimate_plan_set_phase_timing": ([vp, i32], C.c_int),
        "ca_estimate_plan_group_ticks": ([vp, p(C.c_uint64), i32], C.c_int),
        "ca_estimate_plan_option_sums": ([vp, vp, vp], C.c_int),
        "ca_estimate_plan_option_sums_ms": ([vp, p(C.c_float)], C.c_int),
        "ca_estimate_plan_option_price_sums": ([vp, vp, i32, vp], C.c_int),
        "ca_estimate_plan_option_price_sums_ms": ([vp, p(C.c_float)], C.c_int),
        "ca_estimate_plan_fetch_group": ([vp, i32, vp, i32, p(i32)], C.c_int),
        "ca_expander_best_options": ([i32, vp, vp, vp, vp, vp, vp, i32, vp, p(i32), vp], C.c_int),
        "ca_estimate_plan_groups_missing_pods": ([vp, i32, vp, i32, vp, vp], C.c_int),
        "ca_estimate_plan_groups_missing_pods_ms": ([vp, p(C.c_float)], C.c_int),
        "ca_find_nodes_to_remove": ([vp, vp, i32, vp, vp, vp, vp, vp, p(i32), vp, vp], C.c_int),
        "ca_removal_stats": ([vp, p(i32), p(C.c_float), p(C.c_float)], C.c_int),
        "ca_removal_plan_create": ([vp, vp, i32, vp, vp, vp, vp, p(vp)], C.c_int),
        "ca_removal_plan_run": ([vp, vp, p(i32), vp, vp], C.c_int),
        "ca_removal_plan_destroy": ([vp], C.c_int),
        "ca_removal_plan_sensitive_pods": ([vp, p(C.c_int64)], C.c_int),
        "ca_removal_plan_phased": ([vp, p(i32)], C.c_int),
        "ca_removal_plan_run_phase": ([vp, vp, vp, p(i32), vp, vp], C.c_int),
        "ca_sweep_compose": ([vp, i32, i32, i32, vp, p(i32)], C.c_int),
        "ca_mirror_set_hints": ([vp, vp, i32], C.c_int),
        "ca_mirror_get_hints": ([vp, vp, i32], C.c_int),
        "ca_mirror_sync_stats": ([vp, p(C.c_int64), i32], C.c_int),
        "ca_mirror_reorder_nodes": ([vp, vp, i32], C.c_int),
        "ca_mirror_reorder_stats": ([vp, p(C.c_int64), i32], C.c_int),
        "ca_multi_reorder_nodes": ([vp, vp, i32], C.c_int),
        "ca_removal_candidate_ticks": ([vp, p(C.c_uint64), i32], C.c_int),
        "ca_removal_timings": ([vp, p(C.c_float), i32], C.c_int),
        "ca_filter_out_schedulable": ([vp, vp, vp, vp, i32, vp, i32, vp, p(i32), vp, vp, p(i32), p(C.c_uint64), p(i32)],
                                      C.c_int),
        "ca_try_schedule_pods": ([vp, vp, vp, vp, i32, vp, i32, vp, i32, vp, p(i32), vp, vp, vp, p(i32),
                                  p(C.c_uint64), p(i32), p(i32)], C.c_int),
        "ca_filter_stats": ([vp, p(C.c_float), i32], C.c_int),
        "ca_util_table_create": ([i32, vp, i32, vp, vp, p(vp)], C.c_int),
        "ca_util_table_destroy": ([vp], C.c_int),
        "ca_util_table_update": ([vp, vp, i32, vp, vp], C.c_int),
        "ca_util_table_set_added": ([vp, vp, vp, i32], C.c_int),
        "ca_util_calculate": ([vp, i32, i32, C.c_int64, vp, p(C.c_float)], C.c_int),
        "ca_util_device_results": ([vp, p(vp)], C.c_int),
        "ca_mirror_utilization": ([vp, vp, vp, vp, p(C.c_float)], C.c_int),
        "ca_scale_down_candidates_create": ([vp, vp, C.c_double, C.c_double, vp, p(vp)], C.c_int),
        "ca_scale_down_candidates_info": ([vp, p(i32), p(i32), p(i32), p(i32)], C.c_int),
        "ca_scale_down_candidates_fetch": ([vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ca_scale_down_candidates_timings": ([vp, p(C.c_float), i32], C.c_int),
        "ca_scale_down_candidates_destroy": ([vp], C.c_int),
        "ca_mirror_set_pod_util_rows": ([vp, vp, vp, i32], C.c_int),
        "ca_mirror_get_pod_util_rows": ([vp, vp, vp, vp, i32], C.c_int),
        "ca_mirror_utilization_resident": ([vp, vp, vp, vp, p(C.c_float)], C.c_int),
        "ca_scale_down_candidates_create_resident": ([vp, vp, C.c_double, C.c_double, vp, p(vp)], C.c_int),
        "ca_mirror_fetch_pod_columns": ([vp, vp, vp, i32], C.c_int),
        "ca_mirror_pod_column_stats": ([vp, p(C.c_int64), i32], C.c_int),
        "ca_mirror_pod_count": ([vp, p(i32)], C.c_int),
        "ca_removal_plan_create_candidates": ([vp, vp, i32, vp, p(vp)], C.c_int),
        "ca_multi_create": ([p(vp), i32, p(vp)], C.c_int),
        "ca_multi_destroy": ([vp], C.c_int),
        "ca_multi_estimate_plan_create": ([vp, vp, vp, vp, vp, i32, p(vp)], C.c_int),
        "ca_multi_estimate_plan_create_options": ([vp, vp, vp, vp, i32, vp, vp, i32, vp, p(vp)], C.c_int),
        "ca_multi_estimate_plan_create_groups": ([vp, vp, vp, vp, vp, i32, vp, p(vp)], C.c_int),
        "ca_multi_estimate_plan_fetch_lists": ([vp, vp, vp], C.c_int),
        "ca_multi_estimate_plan_lists_ms": ([vp, vp, i32], C.c_int),
        "ca_multi_estimate_plan_run": ([vp, vp, p(i32), vp, vp, vp], C.c_int),
        "ca_multi_estimate_plan_stats": ([vp, p(i32), p(i32), vp, i32], C.c_int),
        "ca_multi_estimate_plan_rerun_units": ([vp, p(i32)], C.c_int),
        "ca_multi_estimate_plan_option_sums": ([vp, vp, vp], C.c_int),
        "ca_multi_estimate_plan_option_price_sums": ([vp, vp, i32, vp], C.c_int),
        "ca_multi_estimate_plan_fetch_group": ([vp, i32, vp, i32, p(i32)], C.c_int),
        "ca_multi_estimate_plan_fetch": ([vp, vp], C.c_int),
        "ca_multi_estimate_plan_groups_missing_pods": ([vp, i32, vp, i32, vp, vp], C.c_int),
        "ca_multi_estimate_plan_reader_ms": ([vp, i32, vp, i32], C.c_int),
        "ca_multi_estimate_plan_export_stats": ([vp, p(C.c_int64), p(i32)], C.c_int),
        "ca_multi_estimate_plan_destroy": ([vp], C.c_int),
        "ca_multi_estimate_batch": ([vp, vp, vp, vp, vp, i32, vp, p(i32), vp, vp, vp], C.c_int),
        "ca_multi_removal_plan_create": ([vp, vp, i32, vp, vp, vp, vp, p(vp)], C.c_int),
        "ca_multi_removal_plan_run": ([vp, vp, i32, p(i32), vp, vp], C.c_int),
        "ca_multi_removal_plan_stats": ([vp, p(i32), p(i32), vp, i32], C.c_int),
        "ca_multi_removal_plan_rerun_units": ([vp, p(i32)], C.c_int),
        "ca_multi_removal_plan_timings": ([vp, vp, i32], C.c_int),
        "ca_multi_removal_plan_destroy": ([vp], C.c_int),
        "ca_multi_find_nodes_to_remove": ([vp, vp, i32, vp, vp, vp, vp, vp, i32, p(i32), vp, vp], C.c_int),
        "ca_plan_removals": ([vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, p(i32), vp, vp, i32, p(i32)], C.c_int),
        "ca_plan_last_moves": ([vp, vp, i32], C.c_int),
        "ca_plan_stats": ([vp, p(i32), p(i32), p(i32), p(C.c_float)], C.c_int),
        "ca_plan_last_path": ([vp], C.c_int),
        "ca_plan_chain_profile": ([vp, vp, i32, vp], C.c_int),
        "ca_interner_create": ([p(vp)], C.c_int),
        "ca_interner_destroy": ([vp], C.c_int),
        "ca_interner_size": ([vp, i32, p(i32), p(i32)], C.c_int),
        "ca_is_scalar_resource": ([C.c_char_p], C.c_int),
        "ca_intern_taint": ([vp, C.c_char_p, C.c_char_p, C.c_char_p, p(i32)], C.c_int),
        "ca_intern_label_pair": ([vp, C.c_char_p, C.c_char_p, p(i32)], C.c_int),
        "ca_intern_label_key": ([vp, C.c_char_p, p(i32)], C.c_int),
        "ca_intern_int_key": ([vp, C.c_char_p, p(i32)], C.c_int),
        "ca_intern_port": ([vp, C.c_char_p, C.c_char_p, i32, p(i32)], C.c_int),
        "ca_intern_resource": ([vp, C.c_char_p, p(i32)], C.c_int),
        "ca_intern_name": ([vp, C.c_char_p, p(i32)], C.c_int),
        "ca_intern_encode_node": ([vp, vp, i32, vp, i32, vp], C.c_int),
        "ca_intern_encode_tolerations": ([vp, vp, i32, vp, p(i32)], C.c_int),
        "ca_intern_encode_ports": ([vp, vp, i32, vp, p(i32)], C.c_int),
        "ca_intern_encode_node_selector": ([vp, vp, i32, vp, p(i32)], C.c_int),
        "ca_intern_compile_term": ([vp, vp, i32, vp, i32, p(i32), p(i32)], C.c_int),
    }
    for name, (args, res) in sigs.items():
        if path != LIB_PATH and not hasattr(lib, name):
            continue                      # an older diagnostics build (A/B runs)
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    _LIB = lib
    return lib


def _fast_copy(a: np.ndarray) -> np.ndarray:
    """Copy of a C-contiguous array through a byte view: numpy copies structured (record)
    arrays field by field (~100 us for 5 000 sweep results), bytes in one memcpy."""
    if a is None:
        return None
    return a.view(np.uint8).copy().view(a.dtype) if a.dtype.fields else a.copy()


def _check(status: int, what: str) -> None:
    if status != abi.CA_OK:
        raise CasimError(status, what)


def exported_symbols() -> list[str]:
    return [
        "ca_abi_version", "ca_abi_struct_sizes", "ca_device_count", "ca_status_string", "ca_host_alloc",
        "ca_host_free", "ca_mirror_create",
        "ca_mirror_destroy", "ca_mirror_clear", "ca_mirror_add_nodes", "ca_mirror_add_pods", "ca_mirror_remove_pod",
        "ca_mirror_remove_node", "ca_mirror_scope_blockers",
        "ca_mirror_fork", "ca_mirror_revert", "ca_mirror_commit", "ca_mirror_node_count", "ca_mirror_pod_node",
        "ca_mirror_node_pods", "ca_podset_create", "ca_podset_destroy", "ca_fits_any_node", "ca_check_predicates",
        "ca_fits_matrix", "ca_check_templates", "ca_expansion_plan_create", "ca_expansion_plan_run",
        "ca_expansion_plan_destroy", "ca_expansion_plan_kernel_ms", "ca_estimate_batch", "ca_estimate_plan_create", "ca_estimate_plan_run",
        "ca_estimate_plan_create_options", "ca_estimate_plan_fetch_lists", "ca_estimate_plan_fetch_class_counts",
        "ca_pod_groups_create", "ca_pod_groups_info", "ca_pod_groups_fetch", "ca_pod_groups_timings",
        "ca_pod_groups_destroy", "ca_expansion_plan_run_groups", "ca_estimate_plan_create_groups",
        "ca_estimate_plan_run_u16",
        "ca_estimate_plan_destroy", "ca_estimate_plan_stats", "ca_estimate_plan_chain_info", "ca_estimate_plan_rebase",
        "ca_estimate_plan_timings",
        "ca_estimate_plan_set_phase_timing",
        "ca_estimate_plan_group_ticks", "ca_estimate_plan_fetch", "ca_estimate_plan_device_results",
        "ca_estimate_plan_option_sums", "ca_estimate_plan_option_sums_ms", "ca_estimate_plan_fetch_group",
        "ca_expander_best_options", "ca_estimate_plan_option_price_sums", "ca_estimate_plan_option_price_sums_ms",
        "ca_estimate_plan_groups_missing_pods", "ca_estimate_plan_groups_missing_pods_ms",
        "ca_go_sort_ranks", "ca_go_sort_ranks_fan",
        "ca_find_nodes_to_remove",
        "ca_removal_stats", "ca_removal_timings", "ca_removal_plan_create", "ca_removal_plan_run",
        "ca_removal_plan_destroy", "ca_removal_plan_sensitive_pods", "ca_removal_plan_phased",
        "ca_removal_plan_run_phase", "ca_sweep_compose", "ca_mirror_set_hints", "ca_mirror_get_hints",
        "ca_mirror_sync_stats", "ca_mirror_reorder_nodes", "ca_mirror_reorder_stats", "ca_multi_reorder_nodes",
        "ca_removal_candidate_ticks", "ca_filter_out_schedulable", "ca_try_schedule_pods", "ca_filter_stats",
        "ca_util_table_create", "ca_util_table_destroy", "ca_util_calculate", "ca_util_device_results",
        "ca_util_table_update", "ca_util_table_set_added",
        "ca_mirror_utilization", "ca_scale_down_candidates_create", "ca_scale_down_candidates_info",
        "ca_scale_down_candidates_fetch", "ca_scale_down_candidates_timings", "ca_scale_down_candidates_destroy",
        "ca_removal_plan_create_candidates", "ca_multi_create", "ca_multi_destroy",
        "ca_mirror_set_pod_util_rows", "ca_mirror_get_pod_util_rows", "ca_mirror_utilization_resident",
        "ca_scale_down_candidates_create_resident", "ca_mirror_fetch_pod_columns", "ca_mirror_pod_column_stats",
        "ca_mirror_pod_count",
        "ca_multi_estimate_plan_create", "ca_multi_estimate_plan_run",
        "ca_multi_estimate_plan_stats", "ca_multi_estimate_plan_rerun_units", "ca_multi_estimate_plan_destroy", "ca_multi_estimate_batch",
        "ca_multi_estimate_plan_option_sums", "ca_multi_estimate_plan_option_price_sums",
        "ca_multi_estimate_plan_fetch_group", "ca_multi_estimate_plan_fetch",
        "ca_multi_estimate_plan_groups_missing_pods", "ca_multi_estimate_plan_reader_ms",
        "ca_multi_estimate_plan_export_stats",
        "ca_multi_estimate_plan_create_options", "ca_multi_estimate_plan_create_groups",
        "ca_multi_estimate_plan_fetch_lists", "ca_multi_estimate_plan_lists_ms",
        "ca_multi_removal_plan_create", "ca_multi_removal_plan_run", "ca_multi_removal_plan_stats",
        "ca_multi_removal_plan_rerun_units", "ca_multi_removal_plan_timings",
        "ca_multi_removal_plan_destroy", "ca_multi_find_nodes_to_remove",
        "ca_plan_removals", "ca_plan_last_moves", "ca_plan_stats", "ca_plan_last_path", "ca_plan_chain_profile",
        "ca_interner_create", "ca_interner_destroy", "ca_interner_size", "ca_is_scalar_resource", "ca_intern_taint",
        "ca_intern_label_pair", "ca_intern_label_key", "ca_intern_int_key", "ca_intern_port", "ca_intern_resource",
        "ca_intern_name", "ca_intern_encode_node", "ca_intern_encode_tolerations", "ca_intern_encode_ports",
        "ca_intern_encode_node_selector", "ca_intern_compile_term",
    ]


def go_sort_ranks(ranks, store: int = 0, limit: int = 0, device: int = 0) -> np.ndarray:
    """Go 1.19 sort.Slice of a slice by dense rank on the device (ca_go_sort_ranks): the
    permutation (perm[k] = input index of the element at position k)."""
    r = np.ascontiguousarray(ranks, dtype=np.uint32)
    perm = np.zeros(max(len(r), 1), np.int32)
    st = load().ca_go_sort_ranks(device, r.ctypes.data, len(r), store, limit, perm.ctypes.data)
    if st != abi.CA_OK:
        raise CasimError(st, "go_sort_ranks")
    return perm[: len(r)]


def go_sort_ranks_fan(ranks, parts: int = 8, top_steps: int = 4, limit: int = 0, device: int = 0) -> tuple:
    """The same permutation through the two-launch LDS-store sort (ca_go_sort_ranks_fan):
    (perm, number of parts the split produced)."""
    r = np.ascontiguousarray(ranks, dtype=np.uint32)
    perm = np.zeros(max(len(r), 1), np.int32)
    n_parts = C.c_int32(0)
    st = load().ca_go_sort_ranks_fan(device, r.ctypes.data, len(r), parts, top_steps, limit, perm.ctypes.data,
                                     C.byref(n_parts))
    if st != abi.CA_OK:
        raise CasimError(st, "go_sort_ranks_fan")
    return perm[: len(r)], n_parts.value


def sweep_compose(recs: np.ndarray, n_nodes: int, last_index: int) -> np.ndarray:
    """ca_sweep_compose: every block's exact input lastIndex from the blocks' MAP records
    (abi.CA_SWEEP_NOT_REACHED where the maps cannot carry the chain)."""
    r = np.ascontiguousarray(recs, dtype=abi.SWEEP_PHASE_DTYPE)
    lin = np.zeros(max(len(r), 1), np.int32)
    _check(load().ca_sweep_compose(r.ctypes.data, len(r), n_nodes, last_index, lin.ctypes.data, None),
           "ca_sweep_compose")
    return lin[: len(r)]


def expander_best_options(filter_id: int, results: np.ndarray, req_milli_cpu, req_memory, cap_milli_cpu, cap_memory,
                          options) -> tuple:
    """ca_expander_best_options (host code, no device): Filter.BestOptions of least-waste /
    most-pods over `options` (indices into the per-group arrays).  Returns (surviving
    indices in input order, float64 score per input option)."""
    res = np.ascontiguousarray(results, dtype=abi.ESTIMATE_RESULT_DTYPE)
    opts = np.ascontiguousarray(options, dtype=np.int32)
    i64 = [None if a is None else np.ascontiguousarray(a, dtype=np.int64)
           for a in (req_milli_cpu, req_memory, cap_milli_cpu, cap_memory)]
    best = np.zeros(max(len(opts), 1), np.int32)
    scores = np.zeros(max(len(opts), 1), np.float64)
    n = C.c_int32(0)
    _check(load().ca_expander_best_options(filter_id, ptr(res), *[ptr(a) for a in i64], ptr(opts), len(opts),
                                           ptr(best), C.byref(n), ptr(scores)), "ca_expander_best_options")
    return best[: n.value], scores[: len(opts)]


def device_count() -> int:
    n = C.c_int32(0)
    st = load().ca_device_count(C.byref(n))
    return n.value if st == abi.CA_OK else 0


@dataclass
class EstimateOutput:
    results: np.ndarray          # ESTIMATE_RESULT_DTYPE [G]
    sched_pod: np.ndarray        # int32 [total], CSR by group_off
    sched_node: np.ndarray       # int32 [total]
    last_index: int


@dataclass
class RemovalOutput:
    results: np.ndarray          # REMOVAL_RESULT_DTYPE [C]
    dest: np.ndarray             # int32 [M]
    hints: np.ndarray            # int32 [pods]
    last_index: int


@dataclass
class PlanOutput:
    results: np.ndarray          # PLAN_RESULT_DTYPE [C]
    moves: np.ndarray            # PLAN_MOVE_DTYPE [n_moves]
    hints: np.ndarray            # int32 [pods]
    last_index: int
    allowed: np.ndarray          # int32 [n_pdbs]: the PDB budgets after the call


@dataclass
class _PlanArgs:
    cand: np.ndarray
    mask: np.ndarray
    status: np.ndarray
    off: np.ndarray
    moves: np.ndarray
    hints: np.ndarray
    allowed: np.ndarray
    pdb_c: object
    keep: tuple
    res: np.ndarray
    out_moves: np.ndarray

    @property
    def pdb_ptr(self):
        return None if self.pdb_c is None else C.byref(self.pdb_c)

    def output(self, last_index: int, n_moves: int) -> PlanOutput:
        return PlanOutput(self.res, self.out_moves[:n_moves], self.hints, last_index, self.allowed)


def plan_args(candidates, dest_mask, cand_status, move_off, move_pods, hints, pdb_allowed=None, pdb_pod_off=None,
              pdb_pod=None) -> _PlanArgs:
    """Marshal the arguments of ca_plan_removals / or_plan_removals.  PDBs (optional):
    pdb_allowed[n_pdbs] DisruptionsAllowed, pdb_pod_off/pdb_pod the memberships (CSR by pod id)."""
    cand = np.ascontiguousarray(candidates, dtype=np.int32)
    status = np.ascontiguousarray(cand_status if cand_status is not None else np.zeros(len(cand)), dtype=np.int32)
    moves = np.ascontiguousarray(move_pods, dtype=np.int32)
    allowed = np.array(pdb_allowed if pdb_allowed is not None else [], dtype=np.int32)
    pdb_c, keep = None, ()
    if len(allowed):
        po = np.ascontiguousarray(pdb_pod_off, dtype=np.int32)
        pp = np.ascontiguousarray(pdb_pod if len(pdb_pod) else [0], dtype=np.int32)
        pdb_c = abi.PdbTableC(len(allowed), ptr(allowed), ptr(po), ptr(pp))
        keep = (po, pp)
    cap = 4 * len(moves) + 256
    return _PlanArgs(cand, np.ascontiguousarray(dest_mask, dtype=np.uint8), status,
                     np.ascontiguousarray(move_off, dtype=np.int32), moves,
                     np.array(hints, dtype=np.int32, copy=True), allowed, pdb_c, keep,
                     np.zeros(max(len(cand), 1), abi.PLAN_RESULT_DTYPE), np.zeros(cap, abi.PLAN_MOVE_DTYPE))


@dataclass
class FilterOutput:
    node: np.ndarray             # int32 [n]: node position per processed pod, -1 still pending
    pod_id: np.ndarray           # int32 [n]: mirror pod id of the added pod, -1
    hints: np.ndarray            # int32 [n]: hints after the call (Hints.Set)
    placed: int
    last_index: int
    evals: int
    n_overflowing: int


@dataclass
class TryScheduleOutput(FilterOutput):
    """ca_try_schedule_pods: FilterOutput plus the break position and the hint checks."""
    tried: int = 0               # pods processed (the one the break stopped at included)
    hint_ok: np.ndarray = None   # uint8 [n]: the pod's hint passed CheckPredicates (Hints.Set, :95)


@dataclass
class _FilterArgs:
    order: np.ndarray
    n: int
    owner: object
    n_classes: int
    hints: np.ndarray
    node: np.ndarray
    pod_id: np.ndarray

    @property
    def owner_ptr(self):
        return None if self.owner is None else ptr(self.owner)

    def output(self, placed: int, last_index: int, evals: int, n_overflowing: int) -> FilterOutput:
        return FilterOutput(self.node[: self.n], self.pod_id[: self.n], self.hints[: self.n], placed, last_index,
                            evals, n_overflowing)


def filter_args(table: abi.PodTable, order=None, class_owner=None, hints=None) -> _FilterArgs:
    """Marshal the arguments of ca_filter_out_schedulable / or_filter_out_schedulable."""
    n_pods = len(table.pods)
    order = np.arange(n_pods, dtype=np.int32) if order is None else np.ascontiguousarray(order, dtype=np.int32)
    n = len(order)
    cls = table.pods["similar_class"]
    n_classes = int(cls.max()) + 1 if n_pods else 0
    owner = None
    if class_owner is not None:
        owner = np.full(max(n_classes, 1), -1, np.int32)
        co = np.ascontiguousarray(class_owner, dtype=np.int32)
        owner[: min(len(co), n_classes)] = co[:n_classes]
        n_classes = max(n_classes, 0)
    h = np.full(max(n, 1), -1, np.int32)
    if hints is not None:
        h[:n] = np.asarray(hints, dtype=np.int32)
    return _FilterArgs(order if n else np.zeros(1, np.int32), n, owner, max(n_classes, 0), h,
                       np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32))


class Mirror:
    """A ``ca_mirror``: the HBM-resident ClusterSnapshot data plane."""

    backend_name = "native"
    batched_try_schedule = True      # try_schedule_pods(table, ...): HintingSimulator's one-call path

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.ca_mirror_create(device, C.byref(h)), "ca_mirror_create")
        self.h = h
        self._keep: list = []

    def close(self) -> None:
        if self.h:
            self.lib.ca_mirror_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- snapshot data plane --------------------------------------------------
    def clear(self) -> None:
        _check(self.lib.ca_mirror_clear(self.h), "ca_mirror_clear")

    def add_nodes(self, nodes: np.ndarray) -> int:
        nodes = np.ascontiguousarray(nodes, dtype=abi.NODE_DTYPE)
        first = C.c_int32(0)
        _check(self.lib.ca_mirror_add_nodes(self.h, ptr(nodes), len(nodes), C.byref(first)), "ca_mirror_add_nodes")
        return first.value

    def add_pods(self, table: abi.PodTable, idx, node_pos) -> np.ndarray:
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        node_pos = np.ascontiguousarray(node_pos, dtype=np.int32)
        out = np.zeros(len(idx), np.int32)
        _check(self.lib.ca_mirror_add_pods(self.h, table.ref, ptr(idx), ptr(node_pos), len(idx), ptr(out)),
               "ca_mirror_add_pods")
        return out

    def remove_pod(self, pod_id: int) -> None:
        _check(self.lib.ca_mirror_remove_pod(self.h, pod_id), "ca_mirror_remove_pod")

    def remove_node(self, pos: int) -> None:
        _check(self.lib.ca_mirror_remove_node(self.h, pos), "ca_mirror_remove_node")

    def scope_blockers(self) -> int:
        n = C.c_int32(0)
        _check(self.lib.ca_mirror_scope_blockers(self.h, C.byref(n)), "ca_mirror_scope_blockers")
        return n.value

    def fork(self) -> None:
        _check(self.lib.ca_mirror_fork(self.h), "ca_mirror_fork")

    def revert(self) -> None:
        _check(self.lib.ca_mirror_revert(self.h), "ca_mirror_revert")

    def commit(self) -> None:
        _check(self.lib.ca_mirror_commit(self.h), "ca_mirror_commit")

    def node_count(self) -> int:
        n = C.c_int32(0)
        _check(self.lib.ca_mirror_node_count(self.h, C.byref(n)), "ca_mirror_node_count")
        return n.value

    def pod_node(self, pod_id: int) -> int:
        n = C.c_int32(0)
        _check(self.lib.ca_mirror_pod_node(self.h, pod_id, C.byref(n)), "ca_mirror_pod_node")
        return n.value

    def node_pods(self, node: int) -> list[int]:
        cap = 256
        while True:
            out = np.zeros(cap, np.int32)
            n = C.c_int32(0)
            st = self.lib.ca_mirror_node_pods(self.h, node, ptr(out), cap, C.byref(n))
            if st == abi.CA_ECAPACITY:
                cap = n.value
                continue
            _check(st, "ca_mirror_node_pods")
            return out[: n.value].tolist()

    # -- scale-down eligibility from the mirror's own state -----------------------
    def utilization(self, skip_ds: bool, skip_mirror: bool, now_ns: int, node_over=None, pod_over=None,
                    out: np.ndarray = None, want_drain: bool = False, resident: bool = False):
        """utilization.Calculate of every node from the mirror's pods (ca_mirror_utilization):
        UTIL_INFO rows in position order, and with want_drain also each node's drain bits.
        node_over = (positions, UTIL_NODE rows), pod_over = (mirror pod ids, UTIL_POD rows):
        rows that replace the defaults, ids strictly ascending.  out: a caller's (page-locked)
        result array, else a new one.  resident: from the resident pod columns
        (ca_mirror_utilization_resident): a pod's row is its pod_over row, else the row
        set_pod_util_rows gave it, else the default."""
        n = self.node_count()
        args, keep = abi.mirror_util_args(skip_ds, skip_mirror, now_ns, node_over, pod_over)
        if out is None:
            out = np.zeros(n, abi.UTIL_INFO_DTYPE)
        drain = np.zeros(n, np.int32) if want_drain else None
        ms = C.c_float(0)
        fn = self.lib.ca_mirror_utilization_resident if resident else self.lib.ca_mirror_utilization
        _check(fn(self.h, C.byref(args), ptr(out), ptr(drain), C.byref(ms)),
               "ca_mirror_utilization_resident" if resident else "ca_mirror_utilization")
        del keep
        self.util_kernel_ms = ms.value
        return (out, drain) if want_drain else out

    def scale_down_candidates(self, skip_ds: bool, skip_mirror: bool, now_ns: int, threshold: float,
                              gpu_threshold: float, eligible=None, node_over=None,
                              pod_over=None, resident: bool = False) -> "ScaleDownCandidates":
        return ScaleDownCandidates(self, skip_ds, skip_mirror, now_ns, threshold, gpu_threshold, eligible,
                                   node_over, pod_over, resident)

    # -- resident per-pod columns: node, slot and util row per mirror pod id ----
    def set_pod_util_rows(self, ids, rows) -> None:
        """ca_mirror_set_pod_util_rows: UTIL_POD rows that stay with mirror pods `ids` (strictly
        ascending) until changed; rows=None clears them back to the default rule."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        r = None if rows is None else np.ascontiguousarray(rows, dtype=abi.UTIL_POD_DTYPE)
        if r is not None and len(r) != len(ids):
            raise ValueError("ids and rows differ in length")
        if r is not None and r.size == 0:
            return
        _check(self.lib.ca_mirror_set_pod_util_rows(self.h, ptr(ids), ptr(r), len(ids)), "ca_mirror_set_pod_util_rows")

    def pod_util_rows(self, ids) -> tuple:
        """(UTIL_POD rows, has-row flags) of mirror pods `ids`, from the host copy."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        rows = np.zeros(len(ids), abi.UTIL_POD_DTYPE)
        has = np.zeros(len(ids), np.uint8)
        _check(self.lib.ca_mirror_get_pod_util_rows(self.h, ptr(ids), ptr(rows), ptr(has), len(ids)),
               "ca_mirror_get_pod_util_rows")
        return rows, has

    def pod_count(self) -> int:
        """Mirror pod ids handed out so far (detached pods keep theirs)."""
        n = C.c_int32(0)
        _check(self.lib.ca_mirror_pod_count(self.h, C.byref(n)), "ca_mirror_pod_count")
        return n.value

    def pod_columns(self) -> tuple:
        """(node, slot) per mirror pod id as the device holds them after a sync
        (ca_mirror_fetch_pod_columns); slot is meaningful where node >= 0."""
        n = self.pod_count()
        node, slot = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(self.lib.ca_mirror_fetch_pod_columns(self.h, ptr(node), ptr(slot), n), "ca_mirror_fetch_pod_columns")
        return node, slot

    def pod_column_stats(self) -> dict:
        """Counters of the resident pod columns since they came into being (ca_mirror_pod_column_stats)."""
        out = (C.c_int64 * 8)()
        self.lib.ca_mirror_pod_column_stats(self.h, out, 8)
        names = ["full_uploads", "staged_syncs", "entries_staged", "tail_appended", "device_reorders",
                 "device_shifts", "rows_uploaded", "bytes_uploaded"]
        return dict(zip(names, (int(v) for v in out)))

    # -- predicate checker ----------------------------------------------------
    def fits_any_node(self, table: abi.PodTable, pod: int, match=None, last_index: int = 0):
        ms, mask = abi.match_spec(*(match or ()))
        li = C.c_int32(last_index)
        out = C.c_int32(-1)
        pf = C.c_int32(0)
        ev = C.c_uint64(0)
        _check(self.lib.ca_fits_any_node(self.h, table.ref, pod, C.byref(ms), C.byref(li), C.byref(out),
                                         C.byref(pf), C.byref(ev)), "ca_fits_any_node")
        del mask
        return out.value, li.value, pf.value, ev.value

    def check_predicates(self, table: abi.PodTable, pod: int, node: int):
        r = abi.PredResultC()
        _check(self.lib.ca_check_predicates(self.h, table.ref, pod, node, C.byref(r)), "ca_check_predicates")
        return r.type, r.plugin, r.reasons, r.taint

    def podset(self, table: abi.PodTable) -> "PodSet":
        """`table` resident in device memory, for several calls (close() it after)."""
        return PodSet(self, table)

    def fits_matrix(self, table: abi.PodTable) -> np.ndarray:
        s = C.c_void_p()
        _check(self.lib.ca_podset_create(self.h, table.ref, C.byref(s)), "ca_podset_create")
        try:
            out = np.zeros((len(table), self.node_count()), np.uint8)
            _check(self.lib.ca_fits_matrix(self.h, s, ptr(out)), "ca_fits_matrix")
        finally:
            self.lib.ca_podset_destroy(s)
        return out

    # -- estimator ------------------------------------------------------------
    def estimate(self, table: abi.PodTable, group_off, pod_idx, templates: np.ndarray, max_nodes: int,
                 last_index: int = 0, want_nodes: bool = True, podset=None) -> EstimateOutput:
        with EstimatePlan(self, table, group_off, pod_idx, templates, podset=podset) as plan:
            return plan.run(max_nodes, last_index, want_nodes=want_nodes)

    def estimate_options(self, table_or_podset, eg_off, eg_pod, ok, templates: np.ndarray, max_nodes: int,
                         last_index: int = 0, want_nodes: bool = True, groups=None) -> tuple:
        """Mirror.estimate on the options' lists built in device memory from the pod
        equivalence groups and the verdict matrix (EstimatePlan.from_options): plan, one run,
        teardown.  Returns (EstimateOutput, group_off): group g's results lie at
        sched_pod[group_off[g]:group_off[g + 1]].  `groups` (a PodGroups built on the same
        resident PodSet): the equivalence groups are read from the handle's device memory
        (EstimatePlan.from_groups) and eg_off / eg_pod are not read."""
        if groups is not None:
            plan = EstimatePlan.from_groups(self, table_or_podset, groups, ok, templates)
        else:
            plan = EstimatePlan.from_options(self, table_or_podset, eg_off, eg_pod, ok, templates)
        with plan:
            return plan.run(max_nodes, last_index, want_nodes=want_nodes), plan.group_off

    def build_pod_groups(self, podset: "PodSet", order=None, node=None, class_owner=None) -> "PodGroups":
        """equivalence.BuildPodGroups on the device (ca_pod_groups_create): the pods
        order[k] of `podset` (None: table order) with node[k] < 0 (None: all of them), grouped
        by similar class with at most 10 groups per controller (class_owner[c]: the controller
        of class c, Interner.class_owners; None: no cap)."""
        return PodGroups(self, podset, order, node, class_owner)

    def check_templates(self, table: abi.PodTable, samples, templates: np.ndarray, podset=None,
                        verdict_only: bool = False, out=None) -> np.ndarray:
        """ComputeExpansionOption's feasibility (orchestrator.go:455-481) for every (node
        group, pod equivalence group): [G][E] ca_pred_result of CheckPredicates(sample pod,
        a fresh copy of the template), or with verdict_only a [G][E] uint8 (1 = fits).
        `podset`: a resident PodSet of `table` (else the table is uploaded for the call);
        `out`: a caller buffer of the result shape (e.g. page-locked)."""
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        tm = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        if out is None:
            out = np.zeros((len(tm), len(sm)), np.uint8 if verdict_only else abi.PRED_RESULT_DTYPE)
        own = podset is None
        ps = PodSet(self, table) if own else podset
        try:
            full, ok = (None, out) if verdict_only else (out, None)
            _check(self.lib.ca_check_templates(self.h, ps.h, ptr(sm), len(sm), ptr(tm), len(tm),
                                               ptr(full) if full is not None else None,
                                               ptr(ok) if ok is not None else None),
                   "ca_check_templates")
        finally:
            if own:
                ps.close()
        return out

    # -- removal simulator ----------------------------------------------------
    def filter_out_schedulable(self, table: abi.PodTable, order=None, class_owner=None, hints=None,
                               last_index: int = 0, podset=None) -> FilterOutput:
        """ca_filter_out_schedulable: TrySchedulePods(pending, ScheduleAnywhere, breakOnFailure=false)
        committed into the mirror (filter_out_schedulable.go:95-124)."""
        a = filter_args(table, order, class_owner, hints)
        li = C.c_int32(last_index)
        ev = C.c_uint64(0)
        ov = C.c_int32(0)
        placed = C.c_int32(0)
        _check(self.lib.ca_filter_out_schedulable(self.h, table.ref, podset.h if podset is not None else None,
                                                  ptr(a.order), a.n, a.owner_ptr, a.n_classes, ptr(a.hints),
                                                  C.byref(li), ptr(a.node), ptr(a.pod_id), C.byref(ov),
                                                  C.byref(ev), C.byref(placed)), "ca_filter_out_schedulable")
        return a.output(placed.value, li.value, ev.value, ov.value)

    def try_schedule_pods(self, table: abi.PodTable, order=None, match=None, break_on_failure: bool = False,
                          class_owner=None, hints=None, last_index: int = 0, podset=None) -> TryScheduleOutput:
        """ca_try_schedule_pods: HintingSimulator.TrySchedulePods(pods, isNodeAcceptable,
        breakOnFailure) in one device call (hinting_simulator.go:58-125).  `match`: the
        (kind, lo, hi, exclude, mask) tuple of fits_any_node, None for every node."""
        a = filter_args(table, order, class_owner, hints)
        ms, mask = abi.match_spec(*(match or ()))
        li = C.c_int32(last_index)
        ev = C.c_uint64(0)
        ov = C.c_int32(0)
        placed = C.c_int32(0)
        tried = C.c_int32(0)
        hok = np.zeros(max(a.n, 1), np.uint8)
        _check(self.lib.ca_try_schedule_pods(self.h, table.ref, podset.h if podset is not None else None,
                                             ptr(a.order), a.n, C.byref(ms) if match is not None else None,
                                             int(bool(break_on_failure)), a.owner_ptr, a.n_classes, ptr(a.hints),
                                             C.byref(li), ptr(a.node), ptr(a.pod_id), ptr(hok), C.byref(ov),
                                             C.byref(ev), C.byref(placed), C.byref(tried)), "ca_try_schedule_pods")
        del mask
        o = a.output(placed.value, li.value, ev.value, ov.value)
        return TryScheduleOutput(o.node, o.pod_id, o.hints, o.placed, o.last_index, o.evals, o.n_overflowing,
                                 tried.value, hok[: a.n])

    def filter_stats(self) -> dict:
        """What the last filter_out_schedulable / try_schedule_pods call did (a call with an
        empty order leaves the earlier values).  `path`: "bitmap" (k_fb_walk) or "window"
        (k_filter_out).  `shapes` (live request shapes plus one row for all dead ones),
        `static_classes` and `static_in_lds` describe the bitmap walk: the first two are 0 on
        the window kernel, which leaves `static_in_lds` as it was.  `phases` is the number of 64-pod batches begun.  Three keys count
        different things on the two paths:

        =============  ====================================  =====================================
        key            bitmap walk                           window sequencer
        =============  ====================================  =====================================
        block_steps    mixed-run attempts (every time two    block-wide steps of any kind (mark,
                       or more eligible pods are tried       next phase, ring scan, window load)
                       together, placed or not)
        ring_scans     pods those mixed runs placed          block-wide ring scans behind the
                                                             512-row window
        windows        steps of the one-by-one path (a       window loads after the first one (a
                       hint check, a single-shape run, a     ring-scan placement or the cursor
                       marked or PreFilter-failed pod)       running off the window)
        =============  ====================================  =====================================

        So one mixed run that places 30 pods reports (1, 30, 0) on the bitmap walk, a pure
        single-shape run reports ring_scans == 0, and on the window kernel a ring of at most
        512 nodes reports ring_scans == windows == 0."""
        out = (C.c_float * 16)()
        self.lib.ca_filter_stats(self.h, out, 16)
        return {"kernel_ms": out[0], "total_ms": out[1], "phases": int(out[2]), "block_steps": int(out[3]),
                "ring_scans": int(out[4]), "windows": int(out[5]), "seq_share": out[6],
                "walk_cycles_per_pod": out[7], "path": "bitmap" if out[8] else "window", "shapes": int(out[9]),
                "static_classes": int(out[10]), "fb_cycles_per_pod": [out[11], out[12], out[13]],
                "static_in_lds": bool(out[15])}

    def find_nodes_to_remove(self, candidates, dest_mask, cand_status, move_off, move_pods, hints,
                             last_index: int = 0) -> RemovalOutput:
        cand = np.ascontiguousarray(candidates, dtype=np.int32)
        mask = np.ascontiguousarray(dest_mask, dtype=np.uint8)
        status = np.ascontiguousarray(cand_status if cand_status is not None else np.zeros(len(cand)), dtype=np.int32)
        off = np.ascontiguousarray(move_off, dtype=np.int32)
        moves = np.ascontiguousarray(move_pods, dtype=np.int32)
        hints = np.array(hints, dtype=np.int32, copy=True)
        res = np.zeros(len(cand), abi.REMOVAL_RESULT_DTYPE)
        dest = np.full(max(len(moves), 1), -1, np.int32)
        li = C.c_int32(last_index)
        _check(self.lib.ca_find_nodes_to_remove(self.h, ptr(cand), len(cand), ptr(mask), ptr(status), ptr(off),
                                                ptr(moves), ptr(hints), C.byref(li), ptr(res), ptr(dest)),
               "ca_find_nodes_to_remove")
        return RemovalOutput(res, dest[: len(moves)], hints, li.value)

    def plan_removals(self, candidates, dest_mask, cand_status, move_off, move_pods, hints, last_index: int = 0,
                      max_removable: int = 0, pdb_allowed=None, pdb_pod_off=None, pdb_pod=None) -> PlanOutput:
        """ca_plan_removals: Planner.categorizeNodes' loop with canPersist=true; commits into
        the mirror.  hints: per mirror pod (len = the mirror's pod count)."""
        a = plan_args(candidates, dest_mask, cand_status, move_off, move_pods, hints, pdb_allowed, pdb_pod_off, pdb_pod)
        li = C.c_int32(last_index)
        nm = C.c_int32(0)
        _check(self.lib.ca_plan_removals(self.h, ptr(a.cand), len(a.cand), ptr(a.mask), ptr(a.status), ptr(a.off),
                                         ptr(a.moves), int(max_removable), a.pdb_ptr, ptr(a.hints), len(a.hints),
                                         C.byref(li), ptr(a.res), ptr(a.out_moves), len(a.out_moves), C.byref(nm)),
               "ca_plan_removals")
        if nm.value > len(a.out_moves):
            a.out_moves = np.zeros(nm.value, abi.PLAN_MOVE_DTYPE)
            self.lib.ca_plan_last_moves(self.h, ptr(a.out_moves), nm.value)
        a.res = a.res[: len(a.cand)]
        return a.output(li.value, nm.value)

    def plan_stats(self) -> dict:
        r, c, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        t = C.c_float(0)
        _check(self.lib.ca_plan_stats(self.h, C.byref(r), C.byref(c), C.byref(s), C.byref(t)), "ca_plan_stats")
        return {"rounds": r.value, "conflicts": c.value, "simulated": s.value, "total_ms": t.value,
                "path": "chain" if self.lib.ca_plan_last_path(self.h) == 1 else "speculative"}

    def plan_chain_profile(self) -> dict:
        """Phase cycle counters and host timings of the last device-chain planner call."""
        cyc = np.zeros(32, np.uint64)
        hm = np.zeros(5, np.float32)
        k = self.lib.ca_plan_chain_profile(self.h, cyc.ctypes.data, 32, hm.ctypes.data)
        names = ["init", "lists", "pdb", "fork", "hint", "scan", "add", "commit", "revert", "total", "blocks",
                 "windows", "handoffs", "bulk", "prep", "win", "loadchk", "skyb", "r_pod", "r_win", "r_blk", "r_sky",
                 "r_add", "r_npods", "r_nblk", "r_nwin", "r_nsky", "r_nruns"]
        out = {nm: int(v) for nm, v in zip(names, cyc[:max(k, 0)])}
        out.update({h: float(v) for h, v in zip(["sync_ms", "launch_kernel_ms", "kernel_ms", "readback_ms",
                                                   "replay_ms"], hm)})
        return out

    def set_hints(self, hints) -> None:
        """The mirror's resident HintingSimulator hints (node per mirror pod, -1 = none)."""
        h = np.ascontiguousarray(hints, dtype=np.int32)
        _check(self.lib.ca_mirror_set_hints(self.h, ptr(h), len(h)), "ca_mirror_set_hints")

    def get_hints(self, n_pods: int) -> np.ndarray:
        h = np.zeros(n_pods, np.int32)
        _check(self.lib.ca_mirror_get_hints(self.h, ptr(h), n_pods), "ca_mirror_get_hints")
        return h

    def sync_stats(self) -> dict:
        """How the device rows were brought up to date since create / clear (ca_mirror_sync_stats)."""
        out = (C.c_int64 * 8)()
        self.lib.ca_mirror_sync_stats(self.h, out, 8)
        names = ["full_syncs", "staged_syncs", "rows_staged", "static_uploads", "growths", "device_rows",
                 "fill_threads", "placed_threads"]
        return {nm: int(v) for nm, v in zip(names, out)}

    def reorder_nodes(self, order) -> None:
        """ca_mirror_reorder_nodes: the node now at position order[k] moves to position k (the
        list the Go snapshot's next NodeInfos().List() returned); depth 0 only."""
        o = np.ascontiguousarray(order, dtype=np.int32)
        _check(self.lib.ca_mirror_reorder_nodes(self.h, ptr(o) if len(o) else None, len(o)),
               "ca_mirror_reorder_nodes")

    def reorder_stats(self) -> tuple:
        """(reorders since create / clear, those permuted on the device, device time of the
        last one in microseconds) (ca_mirror_reorder_stats)."""
        out = (C.c_int64 * 3)()
        self.lib.ca_mirror_reorder_stats(self.h, out, 3)
        return tuple(int(v) for v in out)

    def candidate_ticks(self, n_candidates: int) -> np.ndarray:
        """Per candidate of the last sweep: device time of its simulation, us."""
        a = np.zeros(n_candidates, np.uint64)
        _check(self.lib.ca_removal_candidate_ticks(self.h, a.ctypes.data_as(C.POINTER(C.c_uint64)), n_candidates),
               "ca_removal_candidate_ticks")
        return a.astype(np.float64) / 100.0

    def removal_stats(self) -> dict:
        r, k, t = C.c_int32(0), C.c_float(0), C.c_float(0)
        self.lib.ca_removal_stats(self.h, C.byref(r), C.byref(k), C.byref(t))
        tm = (C.c_float * 4)()
        self.lib.ca_removal_timings(self.h, tm, 4)
        return {"rounds": r.value, "kernel_ms": k.value, "total_ms": t.value, "exact_ms": float(tm[1]),
                "walk_ms": float(tm[2])}


class RemovalPlan:
    """``ca_removal_plan``: FindNodesToRemove inputs resident in HBM for repeated sweeps."""

    def __init__(self, mirror: Mirror, candidates, dest_mask, cand_status, move_off, move_pods):
        self.m = mirror
        self.lib = mirror.lib
        self.cand = np.ascontiguousarray(candidates, dtype=np.int32)
        mask = np.ascontiguousarray(dest_mask, dtype=np.uint8)
        status = np.ascontiguousarray(cand_status if cand_status is not None else np.zeros(len(self.cand)),
                                      dtype=np.int32)
        off = np.ascontiguousarray(move_off, dtype=np.int32)
        self.moves = np.ascontiguousarray(move_pods, dtype=np.int32)
        p = C.c_void_p()
        _check(self.lib.ca_removal_plan_create(mirror.h, ptr(self.cand), len(self.cand), ptr(mask), ptr(status),
                                               ptr(off), ptr(self.moves), C.byref(p)), "ca_removal_plan_create")
        self._adopt(p)

    def _adopt(self, handle) -> None:
        self.h = handle
        self.results = np.zeros(len(self.cand), abi.REMOVAL_RESULT_DTYPE)
        self._dest = PinnedArray(self.lib, max(len(self.moves), 1), np.int32)

    @classmethod
    def from_handle(cls, mirror: Mirror, handle, candidates, move_pods) -> "RemovalPlan":
        """Wrap a ca_removal_plan the library built itself (ScaleDownCandidates.removal_plan);
        `candidates` and `move_pods` are its lists, for the result and destination arrays."""
        self = cls.__new__(cls)
        self.m = mirror
        self.lib = mirror.lib
        self.cand = np.ascontiguousarray(candidates, dtype=np.int32)
        self.moves = np.ascontiguousarray(move_pods, dtype=np.int32)
        self._adopt(handle)
        return self

    def run(self, last_index: int = 0, hints=None, want_dest: bool = False) -> RemovalOutput:
        """One sweep.  hints=None: the mirror's resident hints are used and updated
        (Mirror.set_hints / get_hints); else a per-pod array, updated in place."""
        h = None if hints is None else np.ascontiguousarray(hints, dtype=np.int32)
        li = C.c_int32(last_index)
        dest = self._dest.array if want_dest else None
        _check(self.lib.ca_removal_plan_run(self.h, ptr(h) if h is not None else None, C.byref(li), ptr(self.results),
                                            ptr(dest) if dest is not None else None), "ca_removal_plan_run")
        return RemovalOutput(_fast_copy(self.results), dest[: len(self.moves)].copy() if dest is not None else None, h,
                             li.value)

    # -- the phased sweep of one block (casim.h "one process per GPU"; shard.sweep_sharded) --
    def sensitive_pods(self) -> int:
        v = C.c_int64(0)
        _check(self.lib.ca_removal_plan_sensitive_pods(self.h, C.byref(v)), "ca_removal_plan_sensitive_pods")
        return v.value

    def phased(self) -> bool:
        v = C.c_int32(0)
        _check(self.lib.ca_removal_plan_phased(self.h, C.byref(v)), "ca_removal_plan_phased")
        return bool(v.value)

    def run_phase(self, rec: np.ndarray, hints: np.ndarray, last_index: int, want_dest: bool = True):
        """One phase (rec["kind"]) of this block; rec is a 1-element SWEEP_PHASE_DTYPE array,
        updated in place; hints (int32, per mirror pod) read, and for RESOLVE updated for the
        block's pods.  RESOLVE returns the block's RemovalOutput (dest: the block's moves)."""
        assert rec.dtype == abi.SWEEP_PHASE_DTYPE and rec.flags["C_CONTIGUOUS"]
        assert hints.dtype == np.int32 and hints.flags["C_CONTIGUOUS"]
        li = C.c_int32(last_index)
        dest = self._dest.array if want_dest else None
        _check(self.lib.ca_removal_plan_run_phase(self.h, rec.ctypes.data, ptr(hints), C.byref(li), ptr(self.results),
                                                  ptr(dest) if dest is not None else None), "ca_removal_plan_run_phase")
        if int(rec["kind"][0]) != abi.CA_SWEEP_PHASE_RESOLVE:
            return None
        return RemovalOutput(_fast_copy(self.results), dest[: len(self.moves)].copy() if dest is not None else None,
                             hints, li.value)

    def close(self) -> None:
        if self.h:
            self.lib.ca_removal_plan_destroy(self.h)
            self.h = None
            self._dest.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class PinnedArray:
    """A numpy array over ca_host_alloc (page-locked) memory."""

    def __init__(self, lib, n: int, dtype):
        self.lib = lib
        dt = np.dtype(dtype)
        p = C.c_void_p()
        _check(lib.ca_host_alloc(max(n, 1) * dt.itemsize, C.byref(p)), "ca_host_alloc")
        self.p = p
        buf = (C.c_char * (max(n, 1) * dt.itemsize)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=n)

    def close(self) -> None:
        if self.p:
            self.array = None
            self.lib.ca_host_free(self.p)
            self.p = None


class PinnedRows:
    """Reusable page-locked (ca_host_alloc) arrays for rows a caller builds and uploads
    every loop: the H2D copy then runs at the link's DMA rate instead of through a
    pageable staging copy."""

    def __init__(self, lib=None):
        self.lib = lib or load()
        self._bufs = {}

    def zeros(self, key: str, n: int, dtype, zero: bool = True) -> np.ndarray:
        dt = np.dtype(dtype)
        b = self._bufs.get(key)
        if b is None or b.array.size < n or b.array.dtype != dt:
            if b is not None:
                b.close()
            b = PinnedArray(self.lib, max(n, 1), dt)
            self._bufs[key] = b
        a = b.array[:n]
        if zero:
            a.view(np.uint8)[...] = 0
        return a

    def close(self) -> None:
        for b in self._bufs.values():
            b.close()
        self._bufs = {}


class PodSet:
    """A pod table resident in device memory (ca_podset): uploaded once, reused by calls."""

    def __init__(self, mirror: "Mirror", table: abi.PodTable):
        self.lib = mirror.lib
        self.table = table                      # keeps the host arrays alive
        h = C.c_void_p()
        _check(self.lib.ca_podset_create(mirror.h, table.ref, C.byref(h)), "ca_podset_create")
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.ca_podset_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PodGroups:
    """``ca_pod_groups``: the pod equivalence groups of a resident PodSet's unschedulable pods,
    built and kept in device memory (include/casim.h; equivalence/groups.go:38-102).  A CSR:
    group e's pods are eg_pod[eg_off[e]:eg_off[e + 1]] (pod-set indices), its sample the first
    of them.  Feeds ExpansionPlan.run(groups=) and EstimatePlan.from_groups."""

    def __init__(self, mirror: "Mirror", podset: "PodSet", order=None, node=None, class_owner=None):
        self.lib = mirror.lib
        self.mirror = mirror
        self.podset = podset
        self.h = None
        od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        nd = None if node is None else np.ascontiguousarray(node, dtype=np.int32)
        n = len(od) if od is not None else (len(nd) if nd is not None else len(podset.table))
        if nd is not None and len(nd) != n:
            raise ValueError("node: one entry per listed pod")
        co = None if class_owner is None else np.ascontiguousarray(class_owner, dtype=np.int32)
        h = C.c_void_p()
        _check(self.lib.ca_pod_groups_create(mirror.h, podset.h, ptr(od) if od is not None else None, n,
                                             ptr(nd) if nd is not None else None,
                                             ptr(co) if co is not None else None, len(co) if co is not None else 0,
                                             C.byref(h)), "ca_pod_groups_create")
        self.h = h
        a, b = C.c_int32(0), C.c_int32(0)
        _check(self.lib.ca_pod_groups_info(self.h, C.byref(a), C.byref(b)), "ca_pod_groups_info")
        self.n_groups, self.n_pods = a.value, b.value

    def fetch(self) -> tuple:
        """(eg_off [n_groups + 1], eg_pod [n_pods]) int32."""
        eg_off = np.zeros(self.n_groups + 1, np.int32)
        eg_pod = np.zeros(self.n_pods, np.int32)
        _check(self.lib.ca_pod_groups_fetch(self.h, ptr(eg_off), ptr(eg_pod) if self.n_pods else None),
               "ca_pod_groups_fetch")
        return eg_off, eg_pod

    def samples(self) -> np.ndarray:
        """The first pod of every group."""
        eg_off, eg_pod = self.fetch()
        return eg_pod[eg_off[:-1]] if self.n_groups else np.zeros(0, np.int32)

    def timings(self) -> dict:
        t = (C.c_float * 2)()
        self.lib.ca_pod_groups_timings(self.h, t, 2)
        return {"build_ms": float(t[0]), "launches": int(t[1])}

    def close(self) -> None:
        if self.h:
            self.lib.ca_pod_groups_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EstimatePlan:
    """``ca_estimate_plan``: device-resident groups for repeated Estimate batches."""

    def __init__(self, mirror: Mirror, table: abi.PodTable, group_off, pod_idx, templates: np.ndarray,
                 podset: "PodSet" = None):
        """`podset`: a resident PodSet of `table` to use (else the table is uploaded here)."""
        self.m = mirror
        self.lib = mirror.lib
        self.group_off = np.ascontiguousarray(group_off, dtype=np.int32)
        self.pod_idx = np.ascontiguousarray(pod_idx, dtype=np.int32)
        self.templates = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        self.G = len(self.templates)
        s = self._podset_handle(mirror, table, podset)
        p = C.c_void_p()
        st = self.lib.ca_estimate_plan_create(mirror.h, s, ptr(self.group_off), ptr(self.pod_idx),
                                              ptr(self.templates), self.G, C.byref(p))
        self._created(st, p, "ca_estimate_plan_create")

    @classmethod
    def from_options(cls, mirror: Mirror, table_or_podset, eg_off, eg_pod, ok, templates: np.ndarray) -> "EstimatePlan":
        """The plan of ComputeExpansionOption's lists (orchestrator.go:468-482) without the lists
        (ca_estimate_plan_create_options): the pods of pod equivalence group e are
        eg_pod[eg_off[e]:eg_off[e + 1]] (indices into the pod table), `ok` is the [G][E] verdict
        matrix (nonzero = the group's sample passed, Mirror.check_templates(verdict_only=True) or
        ``feas["type"] == CA_PRED_OK``), and group g's list is the concatenation of the passing
        groups' pods in group order.  The lists are built in device memory; `.group_off` comes
        from the library and `.pod_idx` is None (fetch_lists() copies the lists out).
        `table_or_podset`: an abi.PodTable (uploaded here) or a resident PodSet."""
        self = cls.__new__(cls)
        self.m = mirror
        self.lib = mirror.lib
        self.templates = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        self.G = len(self.templates)
        self.pod_idx = None
        ego = np.ascontiguousarray(eg_off, dtype=np.int32)
        egp = np.ascontiguousarray(eg_pod, dtype=np.int32)
        if ego.ndim != 1 or len(ego) < 1:
            raise ValueError("eg_off: n_eg + 1 offsets")
        n_eg = len(ego) - 1
        if len(egp) < int(ego[-1]):
            raise ValueError("eg_pod is shorter than eg_off[-1]")
        okm = np.ascontiguousarray(ok)
        if okm.dtype != np.uint8:
            okm = np.ascontiguousarray(okm != 0, dtype=np.uint8)
        if okm.size != self.G * n_eg:
            raise ValueError("ok: one verdict per (node group, pod equivalence group)")
        self.group_off = np.zeros(self.G + 1, np.int32)
        is_set = isinstance(table_or_podset, PodSet)
        s = self._podset_handle(mirror, None if is_set else table_or_podset, table_or_podset if is_set else None)
        p = C.c_void_p()
        st = self.lib.ca_estimate_plan_create_options(mirror.h, s, ptr(ego), ptr(egp), n_eg, ptr(okm),
                                                      ptr(self.templates), self.G, ptr(self.group_off), C.byref(p))
        self._created(st, p, "ca_estimate_plan_create_options")
        return self

    @classmethod
    def from_groups(cls, mirror: Mirror, podset: "PodSet", groups: "PodGroups", ok, templates: np.ndarray) -> "EstimatePlan":
        """from_options with the pod equivalence groups taken from a PodGroups handle built on
        `podset` (ca_estimate_plan_create_groups): the CSR is read where it lies in device
        memory; only `ok` ([G][groups.n_groups]) is uploaded.  The same plan as from_options on
        groups.fetch()."""
        self = cls.__new__(cls)
        self.m = mirror
        self.lib = mirror.lib
        self.templates = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        self.G = len(self.templates)
        self.pod_idx = None
        if not isinstance(podset, PodSet) or groups.podset is not podset:
            raise ValueError("from_groups: the PodSet the groups were built on")
        okm = np.ascontiguousarray(ok)
        if okm.dtype != np.uint8:
            okm = np.ascontiguousarray(okm != 0, dtype=np.uint8)
        if okm.size != self.G * groups.n_groups:
            raise ValueError("ok: one verdict per (node group, pod equivalence group)")
        self.group_off = np.zeros(self.G + 1, np.int32)
        s = self._podset_handle(mirror, None, podset)
        p = C.c_void_p()
        st = self.lib.ca_estimate_plan_create_groups(mirror.h, s, groups.h, ptr(okm), ptr(self.templates), self.G,
                                                     ptr(self.group_off), C.byref(p))
        self._created(st, p, "ca_estimate_plan_create_groups")
        return self

    def _podset_handle(self, mirror: Mirror, table, podset):
        if podset is None:
            s = C.c_void_p()
            _check(self.lib.ca_podset_create(mirror.h, table.ref, C.byref(s)), "ca_podset_create")
            self.podset = s
            return s
        self.podset = None
        return podset.h

    def _created(self, st: int, p, what: str) -> None:
        if st != abi.CA_OK:
            if self.podset:
                self.lib.ca_podset_destroy(self.podset)
            raise CasimError(st, what)
        self.h = p
        self.total = int(self.group_off[-1]) if len(self.group_off) else 0
        n = max(self.total, 1)
        self._pinned = PinnedArray(self.lib, 2 * n, np.int32)     # sched_pod | sched_node
        self.sched_pod = self._pinned.array[:n]
        self.sched_node = self._pinned.array[n:]
        self.results = np.zeros(self.G, abi.ESTIMATE_RESULT_DTYPE)
        self._pinned16 = None

    def run_u16(self, max_nodes: int, last_index: int = 0, copy: bool = True) -> EstimateOutput:
        """One Estimate batch with the scheduled pods as 16-bit podset indices
        (ca_estimate_plan_run_u16: podsets of at most 65535 pods; 0xFFFF = not scheduled).
        sched_node of the returned output is None."""
        if self._pinned16 is None:
            self._pinned16 = PinnedArray(self.lib, max(self.total, 1), np.uint16)
            # the call's arguments, built once (a step of the bench's headline loop is ~0.5 ms:
            # the per-call ctypes conversions were a few percent of it)
            self._u16_lim = abi.LimiterC(0, 0)
            self._u16_li = C.c_int32(0)
            self._u16_args = (self.h, C.byref(self._u16_lim), C.byref(self._u16_li), ptr(self.results),
                              ptr(self._pinned16.array))
            self._u16_view = self._pinned16.array[: self.total]
        self._u16_lim.max_nodes = max_nodes
        self._u16_li.value = last_index
        _check(self.lib.ca_estimate_plan_run_u16(*self._u16_args), "ca_estimate_plan_run_u16")
        if copy:
            return EstimateOutput(_fast_copy(self.results), self._u16_view.copy(), None, self._u16_li.value)
        return EstimateOutput(self.results, self._u16_view, None, self._u16_li.value)

    def run(self, max_nodes: int, last_index: int = 0, want_nodes: bool = True, copy: bool = True,
            device_results: bool = False) -> EstimateOutput:
        """One Estimate batch.  With copy=False the returned arrays are views of the plan's
        page-locked result buffers, overwritten by the next run.  With device_results=True
        the scheduled pods stay in device memory (sched_pod/sched_node of the returned
        output are None; fetch() copies them)."""
        lim = abi.LimiterC(max_nodes, 0)
        li = C.c_int32(last_index)
        if device_results:
            _check(self.lib.ca_estimate_plan_run(self.h, C.byref(lim), C.byref(li), ptr(self.results), None, None),
                   "ca_estimate_plan_run")
            return EstimateOutput(_fast_copy(self.results) if copy else self.results, None, None, li.value)
        _check(self.lib.ca_estimate_plan_run(self.h, C.byref(lim), C.byref(li), ptr(self.results),
                                             ptr(self.sched_pod), ptr(self.sched_node) if want_nodes else None),
               "ca_estimate_plan_run")
        f = _fast_copy if copy else (lambda a: a)
        return EstimateOutput(f(self.results), f(self.sched_pod[: self.total]), f(self.sched_node[: self.total]),
                              li.value)

    def fetch(self) -> np.ndarray:
        """The scheduled pods of the last run, copied from device memory."""
        out = np.full(max(self.total, 1), -1, np.int32)
        _check(self.lib.ca_estimate_plan_fetch(self.h, ptr(out)), "ca_estimate_plan_fetch")
        return out[: self.total]

    def fetch_lists(self) -> tuple:
        """The plan's device lists (ca_estimate_plan_fetch_lists): (pod_idx [total], the score
        class of every item [total], or None off the bucket path)."""
        pod_idx = np.full(max(self.total, 1), -1, np.int32)
        item_cls = np.full(max(self.total, 1), -1, np.int32)
        _check(self.lib.ca_estimate_plan_fetch_lists(self.h, ptr(pod_idx), ptr(item_cls)), "ca_estimate_plan_fetch_lists")
        has_cls = self.total == 0 or bool((item_cls[: self.total] >= 0).all())
        return pod_idx[: self.total], (item_cls[: self.total] if has_cls else None)

    def fetch_class_counts(self) -> np.ndarray:
        """[G, U] items of each score class in each group's list, as the device counted them
        when the plan was created (ca_estimate_plan_fetch_class_counts)."""
        u = C.c_int32(0)
        _check(self.lib.ca_estimate_plan_fetch_class_counts(self.h, None, C.byref(u)), "ca_estimate_plan_fetch_class_counts")
        out = np.zeros(max(self.G * u.value, 1), np.int32)
        _check(self.lib.ca_estimate_plan_fetch_class_counts(self.h, ptr(out), None), "ca_estimate_plan_fetch_class_counts")
        return out[: self.G * u.value].reshape(self.G, u.value)

    def option_sums(self) -> tuple:
        """resourcesForPods (waste.go:74-87) of every group of the last run, summed on the
        device over the resident lists: (milli cpu [G], memory [G]) int64.  Raises CasimError
        (CA_ESTATE) unless the last run left its final lists in device memory
        (device_results=True always does)."""
        cpu, mem = np.zeros(max(self.G, 1), np.int64), np.zeros(max(self.G, 1), np.int64)
        _check(self.lib.ca_estimate_plan_option_sums(self.h, ptr(cpu), ptr(mem)), "ca_estimate_plan_option_sums")
        return cpu[: self.G], mem[: self.G]

    def option_sums_ms(self) -> float:
        """Device time of the last option_sums kernel (ms)."""
        ms = C.c_float(0)
        _check(self.lib.ca_estimate_plan_option_sums_ms(self.h, C.byref(ms)), "ca_estimate_plan_option_sums_ms")
        return ms.value

    def option_price_sums(self, pod_price) -> np.ndarray:
        """totalPodPrice of the price expander (price.go:126-134) of every group of the last run:
        the left-to-right float64 sum of `pod_price` (one value per pod of the plan's pod set, in
        pod-set index order; NaN for a pod whose PodPrice failed) over each resident list, [G]
        float64, bit for bit the reference's loop.  CA_ESTATE as option_sums; CA_EINVAL unless
        len(pod_price) is the pod set's size."""
        price = np.ascontiguousarray(pod_price, dtype=np.float64)
        if price.ndim != 1:
            raise ValueError("pod_price: one value per pod of the pod set")
        out = np.zeros(max(self.G, 1), np.float64)
        _check(self.lib.ca_estimate_plan_option_price_sums(self.h, ptr(price), len(price), ptr(out)),
               "ca_estimate_plan_option_price_sums")
        return out[: self.G]

    def option_price_sums_ms(self) -> float:
        """Device time of the last option_price_sums kernel (ms)."""
        ms = C.c_float(0)
        _check(self.lib.ca_estimate_plan_option_price_sums_ms(self.h, C.byref(ms)),
               "ca_estimate_plan_option_price_sums_ms")
        return ms.value

    def fetch_group(self, g: int) -> np.ndarray:
        """The scheduled pods of group `g` of the last run (n_scheduled ids), copied from
        device memory; CA_ESTATE as option_sums."""
        cap = int(self.group_off[g + 1] - self.group_off[g]) if 0 <= g < self.G else 0
        out = np.full(max(cap, 1), -1, np.int32)
        n = C.c_int32(0)
        _check(self.lib.ca_estimate_plan_fetch_group(self.h, g, ptr(out), cap, C.byref(n)),
               "ca_estimate_plan_fetch_group")
        return out[: n.value]

    def groups_missing_pods(self, required: int, groups) -> tuple:
        """filterNodeGroupsByPods (orchestrator.go:596-628) on the last run's resident lists:
        per entry of `groups`, (how many positions of group `required`'s list name a pod that
        the entry's list lacks, the first such position or -1) as int32 arrays.  A group is kept
        by the reference iff its count is 0.  Pods are compared by pod-set index, so the groups'
        pod_idx slices must index one shared pod table.  CA_ESTATE as option_sums."""
        gs = np.ascontiguousarray(groups, dtype=np.int32)
        n_missing, first = np.zeros(max(len(gs), 1), np.int32), np.full(max(len(gs), 1), -1, np.int32)
        _check(self.lib.ca_estimate_plan_groups_missing_pods(self.h, int(required), ptr(gs), len(gs), ptr(n_missing),
                                                             ptr(first)), "ca_estimate_plan_groups_missing_pods")
        return n_missing[: len(gs)], first[: len(gs)]

    def groups_missing_pods_ms(self) -> float:
        """Device time of the last groups_missing_pods call's kernels (ms); 0 if it launched none."""
        ms = C.c_float(0)
        _check(self.lib.ca_estimate_plan_groups_missing_pods_ms(self.h, C.byref(ms)),
               "ca_estimate_plan_groups_missing_pods_ms")
        return ms.value

    def stats(self) -> dict:
        r, a, b, c = C.c_int32(0), C.c_float(0), C.c_float(0), C.c_float(0)
        self.lib.ca_estimate_plan_stats(self.h, C.byref(r), C.byref(a), C.byref(b), C.byref(c))
        sens, succ = C.c_int32(0), C.c_int32(0)
        self.lib.ca_estimate_plan_chain_info(self.h, C.byref(sens), C.byref(succ))
        t = (C.c_float * 15)()
        self.lib.ca_estimate_plan_timings(self.h, t, 15)
        names = ("score_ms", "merge_ms", "emit_ms", "chain_ms", "compact_ms", "d2h_ms", "host_ms")
        return {"rounds": r.value, "chain_ms": a.value, "sort_ms": b.value, "total_ms": c.value,
                "lin_sensitive": sens.value, "had_success": succ.value,
                "phases": {k: float(v) for k, v in zip(names, t)},
                "results_path": ("copied", "published", "publisher_gave_up")[int(t[7])],
                "decoupled": bool(t[8]), "table_chain": bool(t[9]), "lean_chain": bool(t[13]), "sorts": int(t[10]),
                "sort_parts": int(t[11]), "sort_reused": bool(t[14]), "option_lists_ms": float(t[12])}

    def set_phase_timing(self, on: bool) -> None:
        """Per-phase timing events on later runs (on by default; off keeps them off the
        launch path — stats() phases then read 0)."""
        _check(self.lib.ca_estimate_plan_set_phase_timing(self.h, 1 if on else 0), "ca_estimate_plan_set_phase_timing")

    def chain_info(self) -> tuple:
        """(lastIndex-sensitive, had a FitsAnyNode success) of the last run: one call."""
        sens, succ = C.c_int32(0), C.c_int32(0)
        self.lib.ca_estimate_plan_chain_info(self.h, C.byref(sens), C.byref(succ))
        return sens.value, succ.value

    def rebase(self, results: np.ndarray, last_index_in: int) -> int:
        """ca_estimate_plan_rebase: `results` (this plan's last run, a writable copy) re-based
        in place to the exact input lastIndex; returns the batch's exact output."""
        lo = C.c_int32(0)
        _check(self.lib.ca_estimate_plan_rebase(self.h, ptr(results), last_index_in, C.byref(lo)),
               "ca_estimate_plan_rebase")
        return lo.value

    def group_ticks(self) -> np.ndarray:
        """Per group of the last run: (chain device time in us, single-pod steps)."""
        n = self.lib.ca_estimate_plan_group_ticks(self.h, None, 0)
        a = np.zeros(max(n, 0), np.uint64)
        if n > 0:
            self.lib.ca_estimate_plan_group_ticks(self.h, a.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        return np.stack([(a & 0xFFFFFFFF).astype(np.float64) / 100.0, (a >> 32).astype(np.float64)], axis=1)

    def close(self) -> None:
        if self.h:
            self.lib.ca_estimate_plan_destroy(self.h)
            if self.podset:
                self.lib.ca_podset_destroy(self.podset)
            self.h = None
            self.sched_pod = self.sched_node = None
            self._pinned.close()
            if self._pinned16 is not None:
                self._pinned16.close()
                self._pinned16 = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ExpansionPlan:
    """ComputeExpansionOption's check with the node groups resident (ca_expansion_plan_*,
    include/casim.h; CA/core/scaleup/orchestrator/orchestrator.go:455-481): the templates'
    test-node rows are uploaded once; run() checks a pod set's samples against all of them."""

    def __init__(self, mirror: "Mirror", templates: np.ndarray):
        self.lib = load()
        self.mirror = mirror
        self.templates = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        h = C.c_void_p()
        _check(self.lib.ca_expansion_plan_create(mirror.h, ptr(self.templates), len(self.templates), C.byref(h)),
               "ca_expansion_plan_create")
        self.h = h

    def run(self, podset: "PodSet", samples=None, verdict_only: bool = False, out=None, groups=None) -> np.ndarray:
        """[G][E] ca_pred_result (or with verdict_only a [G][E] uint8, 1 = fits), as
        Mirror.check_templates returns it.  `groups` (a PodGroups built on `podset`): the samples
        are the groups' first pods, read from the handle's device memory
        (ca_expansion_plan_run_groups); `samples` is not read."""
        G = len(self.templates)
        if groups is not None:
            if out is None:
                out = np.zeros((G, groups.n_groups), np.uint8 if verdict_only else abi.PRED_RESULT_DTYPE)
            full, ok = (None, out) if verdict_only else (out, None)
            _check(self.lib.ca_expansion_plan_run_groups(self.h, podset.h, groups.h,
                                                         ptr(full) if full is not None else None,
                                                         ptr(ok) if ok is not None else None),
                   "ca_expansion_plan_run_groups")
            return out
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        if out is None:
            out = np.zeros((G, len(sm)), np.uint8 if verdict_only else abi.PRED_RESULT_DTYPE)
        full, ok = (None, out) if verdict_only else (out, None)
        _check(self.lib.ca_expansion_plan_run(self.h, podset.h, ptr(sm), len(sm),
                                              ptr(full) if full is not None else None,
                                              ptr(ok) if ok is not None else None), "ca_expansion_plan_run")
        return out

    @property
    def kernel_ms(self) -> float:
        """The last run's kernel time (HIP events)."""
        v = C.c_float(0)
        _check(self.lib.ca_expansion_plan_kernel_ms(self.h, C.byref(v)), "ca_expansion_plan_kernel_ms")
        return v.value

    def close(self) -> None:
        if self.h:
            self.lib.ca_expansion_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UtilTable:
    """Device-resident node/pod table for utilization.Calculate over every node
    (include/casim.h ca_util_*; CA/simulator/utilization/info.go:48-127)."""

    def __init__(self, device: int, nodes: np.ndarray, pod_off: np.ndarray, pods: np.ndarray):
        self.lib = load()
        self.nodes = np.ascontiguousarray(nodes, abi.UTIL_NODE_DTYPE)
        self.pod_off = np.ascontiguousarray(pod_off, np.int32)
        self.pods = np.ascontiguousarray(pods, abi.UTIL_POD_DTYPE)
        if len(self.pod_off) != len(self.nodes) + 1 or int(self.pod_off[-1]) != len(self.pods):
            raise ValueError("pod_off must have n_nodes + 1 entries ending at len(pods)")
        h = C.c_void_p()
        _check(self.lib.ca_util_table_create(device, ptr(self.nodes), len(self.nodes), ptr(self.pod_off),
                                             ptr(self.pods), C.byref(h)), "ca_util_table_create")
        self.h = h
        self.kernel_ms = 0.0

    def update(self, nodes: np.ndarray, pod_off: np.ndarray, pods: np.ndarray) -> None:
        """New rows (the snapshot changed), in the table's device buffers."""
        self.nodes = np.ascontiguousarray(nodes, abi.UTIL_NODE_DTYPE)
        self.pod_off = np.ascontiguousarray(pod_off, np.int32)
        self.pods = np.ascontiguousarray(pods, abi.UTIL_POD_DTYPE)
        _check(self.lib.ca_util_table_update(self.h, ptr(self.nodes), len(self.nodes), ptr(self.pod_off),
                                             ptr(self.pods)), "ca_util_table_update")

    def set_added(self, node, pods) -> None:
        """Pods added to the snapshot since the rows were set: pods[k] on node[k]."""
        self.added_node = np.ascontiguousarray(node, np.int32)
        self.added_pods = np.ascontiguousarray(pods, abi.UTIL_POD_DTYPE)
        _check(self.lib.ca_util_table_set_added(self.h, ptr(self.added_node), ptr(self.added_pods),
                                                len(self.added_node)), "ca_util_table_set_added")

    def calculate(self, skip_daemonset_pods: bool, skip_mirror_pods: bool, now_ns: int,
                  to_host: bool = True, out: np.ndarray = None):
        """out: a caller's (page-locked) result array, else a new one."""
        if to_host and out is None:
            out = np.zeros(len(self.nodes), abi.UTIL_INFO_DTYPE)
        ms = C.c_float(0)
        _check(self.lib.ca_util_calculate(self.h, int(skip_daemonset_pods), int(skip_mirror_pods), int(now_ns),
                                          ptr(out) if to_host else None, C.byref(ms)), "ca_util_calculate")
        self.kernel_ms = ms.value
        return out

    def close(self) -> None:
        if self.h:
            self.lib.ca_util_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class ScaleDownLists:
    """ScaleDownCandidates.fetch(): the handle's host lists."""
    info: np.ndarray            # UTIL_INFO rows per node position
    node_class: np.ndarray      # abi.CA_SD_* per node position
    empty: np.ndarray           # class-1 positions, ascending
    cand: np.ndarray            # class-2 positions, ascending
    cand_status: np.ndarray     # CA_UNREMOVABLE_BLOCKED_BY_POD or 0 per candidate
    move_off: np.ndarray        # [n_cand + 1]
    move_pods: np.ndarray       # mirror pod ids, NodeInfo.Pods order within a candidate


class ScaleDownCandidates:
    """``ca_scale_down_candidates``: utilization from the mirror's own state, the nodes classified
    against the thresholds and the removal sweep's inputs, built inside the library."""

    def __init__(self, mirror: Mirror, skip_ds: bool, skip_mirror: bool, now_ns: int, threshold: float,
                 gpu_threshold: float, eligible=None, node_over=None, pod_over=None, resident: bool = False):
        self.m = mirror
        self.lib = mirror.lib
        self.h = None
        args, keep = abi.mirror_util_args(skip_ds, skip_mirror, now_ns, node_over, pod_over)
        el = None if eligible is None else np.ascontiguousarray(eligible, dtype=np.uint8)
        if el is not None and len(el) != mirror.node_count():
            raise ValueError("eligible needs one byte per node")
        h = C.c_void_p()
        create = (self.lib.ca_scale_down_candidates_create_resident if resident
                  else self.lib.ca_scale_down_candidates_create)
        _check(create(mirror.h, C.byref(args), float(threshold), float(gpu_threshold), ptr(el), C.byref(h)),
               "ca_scale_down_candidates_create_resident" if resident else "ca_scale_down_candidates_create")
        del keep
        self.h = h
        self._lists = None

    @property
    def info(self) -> dict:
        v = [C.c_int32(0) for _ in range(4)]
        _check(self.lib.ca_scale_down_candidates_info(self.h, *[C.byref(x) for x in v]), "ca_scale_down_candidates_info")
        return dict(zip(("n_nodes", "n_empty", "n_cand", "n_moves"), (x.value for x in v)))

    def fetch(self) -> ScaleDownLists:
        if self._lists is None:
            s = self.info
            n, nc = s["n_nodes"], s["n_cand"]
            out = ScaleDownLists(np.zeros(n, abi.UTIL_INFO_DTYPE), np.zeros(n, np.uint8), np.zeros(s["n_empty"], np.int32),
                                 np.zeros(nc, np.int32), np.zeros(nc, np.int32), np.zeros(nc + 1, np.int32),
                                 np.zeros(s["n_moves"], np.int32))
            _check(self.lib.ca_scale_down_candidates_fetch(self.h, ptr(out.info), ptr(out.node_class), ptr(out.empty),
                                                           ptr(out.cand), ptr(out.cand_status), ptr(out.move_off),
                                                           ptr(out.move_pods)), "ca_scale_down_candidates_fetch")
            self._lists = out
        return self._lists

    def timings(self) -> dict:
        t = (C.c_float * 7)()
        self.lib.ca_scale_down_candidates_timings(self.h, t, 7)
        return {"util_kernel_ms": float(t[0]), "classify_kernel_ms": float(t[1]), "stage_ms": float(t[2]),
                "move_lists_ms": float(t[3]), "create_ms": float(t[4]), "h2d_bytes": int(t[5]), "d2h_bytes": int(t[6])}

    def removal_plan(self, nodes=None, dest_mask=None) -> "RemovalPlan":
        """The sweep over every candidate (nodes=None) or over the given class-2 positions in
        the given order; `dest_mask`: one byte per node (None: every node is a destination)."""
        n_nodes = self.info["n_nodes"]
        mask = np.ascontiguousarray(dest_mask if dest_mask is not None else np.ones(n_nodes, np.uint8), dtype=np.uint8)
        if len(mask) != n_nodes:
            raise ValueError("dest_mask needs one byte per node")
        sel = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        if sel is not None and sel.size == 0:
            sel = np.zeros(1, np.int32)[:0]
        p = C.c_void_p()
        st = self.lib.ca_removal_plan_create_candidates(self.h, sel.ctypes.data if sel is not None else None,
                                                        0 if sel is None else len(sel), ptr(mask), C.byref(p))
        _check(st, "ca_removal_plan_create_candidates")
        ls = self.fetch()
        if sel is None:
            cand, moves = ls.cand, ls.move_pods
        else:
            at = np.searchsorted(ls.cand, sel)
            cand = sel
            moves = (np.concatenate([ls.move_pods[ls.move_off[c]:ls.move_off[c + 1]] for c in at])
                     if len(at) else np.zeros(0, np.int32))
        return RemovalPlan.from_handle(self.m, p, cand, moves)

    def close(self) -> None:
        if self.h:
            self.lib.ca_scale_down_candidates_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """``ca_multi``: replicated mirrors, one per device.  The caller keeps
    them identical; `mirrors` may repeat a device (tests shard over two mirrors on one GPU)."""

    def __init__(self, mirrors):
        self.mirrors = list(mirrors)
        self.lib = self.mirrors[0].lib
        arr = (C.c_void_p * len(self.mirrors))(*[m.h for m in self.mirrors])
        h = C.c_void_p()
        _check(self.lib.ca_multi_create(arr, len(self.mirrors), C.byref(h)), "ca_multi_create")
        self.h = h

    def for_each(self, fn):
        """Apply a snapshot change to every replica, in order."""
        return [fn(m) for m in self.mirrors]

    def reorder_nodes(self, order) -> None:
        """ca_multi_reorder_nodes: the same new node order on every replica, all or none."""
        o = np.ascontiguousarray(order, dtype=np.int32)
        _check(self.lib.ca_multi_reorder_nodes(self.h, ptr(o) if len(o) else None, len(o)),
               "ca_multi_reorder_nodes")

    def close(self) -> None:
        if self.h:
            self.lib.ca_multi_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class MultiEstimatePlan:
    """``ca_multi_estimate_plan``: node groups in contiguous blocks over the replicas."""

    def __init__(self, multi: Multi, table: abi.PodTable, group_off, pod_idx, templates: np.ndarray):
        self.lib = multi.lib
        self.group_off = np.ascontiguousarray(group_off, dtype=np.int32)
        self.pod_idx = np.ascontiguousarray(pod_idx, dtype=np.int32)
        self.templates = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        self.G = len(self.templates)
        h = C.c_void_p()
        _check(self.lib.ca_multi_estimate_plan_create(multi.h, table.ref, ptr(self.group_off), ptr(self.pod_idx),
                                                      ptr(self.templates), self.G, C.byref(h)),
               "ca_multi_estimate_plan_create")
        self._created(h)

    def _created(self, h) -> None:
        self.h = h
        self.total = int(self.group_off[-1]) if len(self.group_off) else 0
        n = max(self.total, 1)
        self._pinned = PinnedArray(self.lib, 2 * n, np.int32)
        self.sched_pod = self._pinned.array[:n]
        self.sched_node = self._pinned.array[n:]
        self.results = np.zeros(self.G, abi.ESTIMATE_RESULT_DTYPE)

    @classmethod
    def _options_plan(cls, multi: Multi, n_eg: int, ok, templates: np.ndarray) -> tuple:
        """The fields every option-matrix plan starts from, and `ok` as [G * n_eg] uint8."""
        self = cls.__new__(cls)
        self.lib = multi.lib
        self.h = None
        self.templates = np.ascontiguousarray(templates, dtype=abi.TEMPLATE_DTYPE)
        self.G = len(self.templates)
        self.pod_idx = None
        okm = np.ascontiguousarray(ok)
        if okm.dtype != np.uint8:
            okm = np.ascontiguousarray(okm != 0, dtype=np.uint8)
        if okm.size != self.G * n_eg:
            raise ValueError("ok: one verdict per (node group, pod equivalence group)")
        self.group_off = np.zeros(self.G + 1, np.int32)
        return self, okm

    @classmethod
    def from_options(cls, multi: Multi, table: abi.PodTable, eg_off, eg_pod, ok, templates: np.ndarray) -> "MultiEstimatePlan":
        """EstimatePlan.from_options over the replicas (ca_multi_estimate_plan_create_options):
        the blocks are split by the rows' totals, the split the list form takes from its
        group_off, and every block builds its lists in its own device's memory from the CSR and
        its own rows of `ok`.  `.group_off` comes from the library and `.pod_idx` is None
        (fetch_lists() copies the lists out)."""
        ego = np.ascontiguousarray(eg_off, dtype=np.int32)
        egp = np.ascontiguousarray(eg_pod, dtype=np.int32)
        if ego.ndim != 1 or len(ego) < 1:
            raise ValueError("eg_off: n_eg + 1 offsets")
        n_eg = len(ego) - 1
        if len(egp) < int(ego[-1]):
            raise ValueError("eg_pod is shorter than eg_off[-1]")
        self, okm = cls._options_plan(multi, n_eg, ok, templates)
        h = C.c_void_p()
        _check(self.lib.ca_multi_estimate_plan_create_options(multi.h, table.ref, ptr(ego), ptr(egp), n_eg, ptr(okm),
                                                              ptr(self.templates), self.G, ptr(self.group_off),
                                                              C.byref(h)), "ca_multi_estimate_plan_create_options")
        self._created(h)
        return self

    @classmethod
    def from_groups(cls, multi: Multi, table: abi.PodTable, groups: "PodGroups", ok, templates: np.ndarray) -> "MultiEstimatePlan":
        """from_options with the pod equivalence groups taken from a PodGroups handle
        (ca_multi_estimate_plan_create_groups): the handle's host copy of its CSR is read, so it
        may have been built on any mirror, over a pod set of `table`'s size.  The same plan as
        from_options on groups.fetch()."""
        if not isinstance(groups, PodGroups):
            raise ValueError("from_groups: a PodGroups handle")
        self, okm = cls._options_plan(multi, groups.n_groups, ok, templates)
        h = C.c_void_p()
        _check(self.lib.ca_multi_estimate_plan_create_groups(multi.h, table.ref, groups.h, ptr(okm), ptr(self.templates),
                                                             self.G, ptr(self.group_off), C.byref(h)),
               "ca_multi_estimate_plan_create_groups")
        self._created(h)
        return self

    READERS = {"sums": 0, "price": 1, "missing": 2}          # CA_MULTI_READER_*

    def run(self, max_nodes: int, last_index: int = 0, want_nodes: bool = True, copy: bool = True,
            device_results: bool = False) -> EstimateOutput:
        """One Estimate batch over the blocks.  With device_results=True every block's lists stay
        in its own device's memory (sched_pod / sched_node of the returned output are None) and
        the readers below work until the next run; after any other run they raise CasimError
        (CA_ESTATE)."""
        lim = abi.LimiterC(max_nodes, 0)
        li = C.c_int32(last_index)
        if device_results:
            _check(self.lib.ca_multi_estimate_plan_run(self.h, C.byref(lim), C.byref(li), ptr(self.results), None,
                                                       None), "ca_multi_estimate_plan_run")
            return EstimateOutput(_fast_copy(self.results) if copy else self.results, None, None, li.value)
        _check(self.lib.ca_multi_estimate_plan_run(self.h, C.byref(lim), C.byref(li), ptr(self.results),
                                                   ptr(self.sched_pod), ptr(self.sched_node) if want_nodes else None),
               "ca_multi_estimate_plan_run")
        f = _fast_copy if copy else (lambda a: a)
        return EstimateOutput(f(self.results), f(self.sched_pod[: self.total]), f(self.sched_node[: self.total]),
                              li.value)

    def stats(self) -> dict:
        nb, rr = C.c_int32(0), C.c_int32(0)
        first = np.zeros(65, np.int32)
        self.lib.ca_multi_estimate_plan_stats(self.h, C.byref(nb), C.byref(rr), ptr(first), len(first))
        ru = C.c_int32(0)
        self.lib.ca_multi_estimate_plan_rerun_units(self.h, C.byref(ru))
        return {"blocks": nb.value, "reruns": rr.value, "block_first_group": first[: nb.value + 1].tolist(),
                "rerun_groups": ru.value}

    def fetch_lists(self) -> tuple:
        """The blocks' device lists in global group order (ca_multi_estimate_plan_fetch_lists;
        plans of any constructor): (group_off, pod_idx [total], the score class of every item
        [total], or None off the bucket path)."""
        pod_idx = np.full(max(self.total, 1), -1, np.int32)
        item_cls = np.full(max(self.total, 1), -1, np.int32)
        _check(self.lib.ca_multi_estimate_plan_fetch_lists(self.h, ptr(pod_idx), ptr(item_cls)),
               "ca_multi_estimate_plan_fetch_lists")
        has_cls = self.total == 0 or bool((item_cls[: self.total] >= 0).all())
        return self.group_off.copy(), pod_idx[: self.total], (item_cls[: self.total] if has_cls else None)

    def lists_ms(self) -> np.ndarray:
        """Per block, the device time (ms) of the kernels that built its lists from the option
        matrix when the plan was created; 0 for a plan created from host lists."""
        nb = C.c_int32(0)
        _check(self.lib.ca_multi_estimate_plan_stats(self.h, C.byref(nb), None, None, 0),
               "ca_multi_estimate_plan_stats")
        ms = np.zeros(max(nb.value, 1), np.float32)
        self.lib.ca_multi_estimate_plan_lists_ms(self.h, ptr(ms), nb.value)          # (returns the block count)
        return ms[: nb.value]

    # The readers of EstimatePlan, same names and return shapes, over the blocks of the last
    # resident run (expander.DeviceOptions and nodegroupset.filter_plan_groups_by_pods take
    # either plan).  A group that is not CA_OK in that run's results reads as an empty list.
    def fetch(self) -> np.ndarray:
        """All lists in the group_off layout; -1 behind n_scheduled and in groups that are not
        CA_OK."""
        out = np.full(max(self.total, 1), -1, np.int32)
        _check(self.lib.ca_multi_estimate_plan_fetch(self.h, ptr(out)), "ca_multi_estimate_plan_fetch")
        return out[: self.total]

    def option_sums(self) -> tuple:
        """EstimatePlan.option_sums over the blocks: (milli cpu [G], memory [G]) int64."""
        cpu, mem = np.zeros(max(self.G, 1), np.int64), np.zeros(max(self.G, 1), np.int64)
        _check(self.lib.ca_multi_estimate_plan_option_sums(self.h, ptr(cpu), ptr(mem)),
               "ca_multi_estimate_plan_option_sums")
        return cpu[: self.G], mem[: self.G]

    def option_price_sums(self, pod_price) -> np.ndarray:
        """EstimatePlan.option_price_sums over the blocks: one price per pod of the plan's pod
        table, [G] float64, the reference's in-order sums bit for bit."""
        price = np.ascontiguousarray(pod_price, dtype=np.float64)
        if price.ndim != 1:
            raise ValueError("pod_price: one value per pod of the pod set")
        out = np.zeros(max(self.G, 1), np.float64)
        _check(self.lib.ca_multi_estimate_plan_option_price_sums(self.h, ptr(price), len(price), ptr(out)),
               "ca_multi_estimate_plan_option_price_sums")
        return out[: self.G]

    def fetch_group(self, g: int) -> np.ndarray:
        """The scheduled pods of (global) group `g` of the last run, from its block's device."""
        cap = int(self.group_off[g + 1] - self.group_off[g]) if 0 <= g < self.G else 0
        out = np.full(max(cap, 1), -1, np.int32)
        n = C.c_int32(0)
        _check(self.lib.ca_multi_estimate_plan_fetch_group(self.h, g, ptr(out), cap, C.byref(n)),
               "ca_multi_estimate_plan_fetch_group")
        return out[: n.value]

    def groups_missing_pods(self, required: int, groups) -> tuple:
        """EstimatePlan.groups_missing_pods with global group indices.  The required list is
        copied to the other blocks' devices (through host memory) only when a candidate outside
        the required group's block needs it: export_stats() says what moved."""
        gs = np.ascontiguousarray(groups, dtype=np.int32)
        n_missing, first = np.zeros(max(len(gs), 1), np.int32), np.full(max(len(gs), 1), -1, np.int32)
        _check(self.lib.ca_multi_estimate_plan_groups_missing_pods(self.h, int(required), ptr(gs), len(gs),
                                                                   ptr(n_missing), ptr(first)),
               "ca_multi_estimate_plan_groups_missing_pods")
        return n_missing[: len(gs)], first[: len(gs)]

    def reader_ms(self, which) -> np.ndarray:
        """Per block, the device time (ms) of the kernels of the last call of reader `which`
        ("sums", "price", "missing" or its CA_MULTI_READER_* number); 0 where a block launched
        nothing."""
        w = self.READERS[which] if isinstance(which, str) else int(which)
        if w not in self.READERS.values():
            raise ValueError(f"reader_ms: unknown reader {which!r}")
        nb = C.c_int32(0)
        _check(self.lib.ca_multi_estimate_plan_stats(self.h, C.byref(nb), None, None, 0),
               "ca_multi_estimate_plan_stats")
        ms = np.zeros(max(nb.value, 1), np.float32)
        self.lib.ca_multi_estimate_plan_reader_ms(self.h, w, ptr(ms), nb.value)     # (returns the block count)
        return ms[: nb.value]

    def export_stats(self) -> dict:
        """The last groups_missing_pods call's exchange: bytes of the required list that left its
        device, and the blocks that uploaded it."""
        b, n = C.c_int64(0), C.c_int32(0)
        _check(self.lib.ca_multi_estimate_plan_export_stats(self.h, C.byref(b), C.byref(n)),
               "ca_multi_estimate_plan_export_stats")
        return {"exported_bytes": b.value, "importing_blocks": n.value}

    def close(self) -> None:
        if self.h:
            self.lib.ca_multi_estimate_plan_destroy(self.h)
            self.h = None
            self._pinned.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class MultiRemovalPlan:
    """``ca_multi_removal_plan``: FindNodesToRemove candidates in contiguous blocks."""

    def __init__(self, multi: Multi, candidates, dest_mask, cand_status, move_off, move_pods):
        self.lib = multi.lib
        self.cand = np.ascontiguousarray(candidates, dtype=np.int32)
        mask = np.ascontiguousarray(dest_mask, dtype=np.uint8)
        status = np.ascontiguousarray(cand_status if cand_status is not None else np.zeros(len(self.cand)),
                                      dtype=np.int32)
        off = np.ascontiguousarray(move_off, dtype=np.int32)
        self.moves = np.ascontiguousarray(move_pods, dtype=np.int32)
        h = C.c_void_p()
        _check(self.lib.ca_multi_removal_plan_create(multi.h, ptr(self.cand), len(self.cand), ptr(mask), ptr(status),
                                                     ptr(off), ptr(self.moves), C.byref(h)),
               "ca_multi_removal_plan_create")
        self.h = h
        self.results = np.zeros(len(self.cand), abi.REMOVAL_RESULT_DTYPE)

    def run(self, hints, last_index: int = 0) -> RemovalOutput:
        hints = np.array(hints, dtype=np.int32, copy=True)
        dest = np.full(max(len(self.moves), 1), -1, np.int32)
        li = C.c_int32(last_index)
        _check(self.lib.ca_multi_removal_plan_run(self.h, ptr(hints), len(hints), C.byref(li), ptr(self.results),
                                                  ptr(dest)), "ca_multi_removal_plan_run")
        return RemovalOutput(_fast_copy(self.results), dest[: len(self.moves)], hints, li.value)

    def stats(self) -> dict:
        nb, rr = C.c_int32(0), C.c_int32(0)
        first = np.zeros(65, np.int32)
        self.lib.ca_multi_removal_plan_stats(self.h, C.byref(nb), C.byref(rr), ptr(first), len(first))
        ru = C.c_int32(0)
        self.lib.ca_multi_removal_plan_rerun_units(self.h, C.byref(ru))
        tm = np.zeros(5, np.float32)
        self.lib.ca_multi_removal_plan_timings(self.h, tm.ctypes.data, 5)
        return {"blocks": nb.value, "reruns": rr.value, "block_first_candidate": first[: nb.value + 1].tolist(),
                "rerun_candidates": ru.value,
                "phase_ms": dict(zip(("probe", "map", "compose", "resolve", "fixup"), tm.tolist()))}

    def close(self) -> None:
        if self.h:
            self.lib.ca_multi_removal_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- interning through the C ABI (casim.h "interning"; host-only, no device needed) ------

class _StrPair(C.Structure):
    _fields_ = [("key", C.c_char_p), ("value", C.c_char_p)]


class _TaintStr(C.Structure):
    _fields_ = [("key", C.c_char_p), ("value", C.c_char_p), ("effect", C.c_char_p)]


class _TolerationStr(C.Structure):
    _fields_ = [("key", C.c_char_p), ("op", C.c_char_p), ("value", C.c_char_p), ("effect", C.c_char_p)]


class _PortStr(C.Structure):
    _fields_ = [("host_ip", C.c_char_p), ("protocol", C.c_char_p), ("host_port", C.c_int32), ("reserved", C.c_int32)]


class _RequirementStr(C.Structure):
    _fields_ = [("key", C.c_char_p), ("op", C.c_char_p), ("values", C.POINTER(C.c_char_p)), ("n_values", C.c_int32),
                ("is_field", C.c_int32)]


def _b(x) -> bytes:
    return (x or "").encode()


class CInterner:
    """``ca_interner``: the library's interning (what a cgo shim binds), driven with Python
    strings.  Ids and encodings equal autoscaler_amd/intern.py's (tests/test_intern_c.py)."""

    def __init__(self):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.ca_interner_create(C.byref(h)), "ca_interner_create")
        self.h = h

    def close(self):
        if self.h:
            self.lib.ca_interner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _id(self, fn, *a) -> int:
        i = C.c_int32(0)
        _check(getattr(self.lib, fn)(self.h, *a, C.byref(i)), fn)
        return i.value

    def taint(self, k, v, e):
        return self._id("ca_intern_taint", _b(k), _b(v), _b(e))

    def label_pair(self, k, v):
        return self._id("ca_intern_label_pair", _b(k), _b(v))

    def label_key(self, k):
        return self._id("ca_intern_label_key", _b(k))

    def int_key(self, k):
        return self._id("ca_intern_int_key", _b(k))

    def port(self, ip, proto, port):
        return self._id("ca_intern_port", _b(ip), _b(proto), int(port))

    def resource(self, name):
        return self._id("ca_intern_resource", _b(name))

    def name(self, n):
        return self._id("ca_intern_name", _b(n))

    def size(self, universe: int) -> tuple:
        n, o = C.c_int32(0), C.c_int32(0)
        _check(self.lib.ca_interner_size(self.h, universe, C.byref(n), C.byref(o)), "ca_interner_size")
        return n.value, o.value

    def encode_node(self, labels: dict, taints, rec) -> None:
        """labels {k: v}; taints [(key, value, effect)]; rec: an abi.NODE_DTYPE record (array of 1)."""
        lb = (_StrPair * max(len(labels), 1))(*[_StrPair(_b(k), _b(v)) for k, v in labels.items()])
        tt = (_TaintStr * max(len(taints), 1))(*[_TaintStr(_b(k), _b(v), _b(e)) for k, v, e in taints])
        _check(self.lib.ca_intern_encode_node(self.h, lb, len(labels), tt, len(taints), rec.ctypes.data),
               "ca_intern_encode_node")

    def encode_tolerations(self, tols, rec) -> int:
        """tols [(key, op, value, effect)]; rec: abi.POD_DTYPE array of 1.  Returns out_of_scope."""
        tt = (_TolerationStr * max(len(tols), 1))(*[_TolerationStr(_b(k), _b(o), _b(v), _b(e)) for k, o, v, e in tols])
        o = C.c_int32(0)
        _check(self.lib.ca_intern_encode_tolerations(self.h, tt, len(tols), rec.ctypes.data, C.byref(o)),
               "ca_intern_encode_tolerations")
        return o.value

    def encode_ports(self, ports, rec) -> int:
        """ports [(host_ip, protocol, host_port)] of the pod's containers."""
        pp = (_PortStr * max(len(ports), 1))(*[_PortStr(_b(i), _b(pr), int(pt), 0) for i, pr, pt in ports])
        o = C.c_int32(0)
        _check(self.lib.ca_intern_encode_ports(self.h, pp, len(ports), rec.ctypes.data, C.byref(o)),
               "ca_intern_encode_ports")
        return o.value

    def encode_node_selector(self, sel: dict, rec) -> int:
        ss = (_StrPair * max(len(sel), 1))(*[_StrPair(_b(k), _b(v)) for k, v in sel.items()])
        o = C.c_int32(0)
        _check(self.lib.ca_intern_encode_node_selector(self.h, ss, len(sel), rec.ctypes.data, C.byref(o)),
               "ca_intern_encode_node_selector")
        return o.value

    def compile_term(self, reqs) -> tuple:
        """reqs [(key, op, [values], is_field)] -> (abi.REQ_DTYPE rows, out_of_scope)."""
        keep = []
        rr = (_RequirementStr * max(len(reqs), 1))()
        for i, (k, op, vals, f) in enumerate(reqs):
            va = (C.c_char_p * max(len(vals), 1))(*[_b(v) for v in vals])
            keep.append(va)
            rr[i] = _RequirementStr(_b(k), _b(op), C.cast(va, C.POINTER(C.c_char_p)), len(vals), int(bool(f)))
        out = np.zeros(max(len(reqs), 1), abi.REQ_DTYPE)
        nr, o = C.c_int32(0), C.c_int32(0)
        _check(self.lib.ca_intern_compile_term(self.h, rr, len(reqs), out.ctypes.data, len(out), C.byref(nr),
                                               C.byref(o)), "ca_intern_compile_term")
        del keep
        return out[: nr.value], o.value
