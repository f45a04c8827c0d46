"""hclib_amd — MI355X-native HClib task-scheduling hot path.

Python mirror of the module's C ABI (include/hclib_hip.h). The compute
entry points run only through the in-tree HIP library
hclib_amd/lib/libhclib_amd.so; there is no CPU fallback — if the library or
a gfx950 device is missing they raise HclibError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

PKG = os.path.dirname(os.path.abspath(__file__))
# HCLIB_AMD_LIB selects a diagnostic variant (python -m hclib_amd.build --variant X)
LIB_PATH = os.environ.get("HCLIB_AMD_LIB") or os.path.join(PKG, "lib", "libhclib_amd.so")

HCLIB_HIP_OK = 0
FORASYNC_MODE_FLAT = 0       # inc/hclib.h:161
FORASYNC_MODE_RECURSIVE = 1  # inc/hclib.h:159
BODY_TRIAD_F32 = 1
BODY_IOTA_CHECK = 2
BODY_VISIT_COUNT = 3


class HclibError(RuntimeError):
    pass


class LoopDomain(C.Structure):
    """hclib_loop_domain_t, inc/hclib-task.h:53-58."""

    _fields_ = [("low", C.c_int), ("high", C.c_int), ("stride", C.c_int), ("tile", C.c_int)]


class TriadArgs(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p), ("s", C.c_float)]


class IotaArgs(C.Structure):
    _fields_ = [("ran", C.c_void_p), ("errors", C.c_void_p)]


class VisitArgs(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("base", C.c_int * 3), ("extent", C.c_int * 3)]


class UtsParams(C.Structure):
    """hclib_hip_uts_params_t — the UTS CLI flags of test/uts/uts.c:380-420."""

    _fields_ = [
        ("type", C.c_int), ("shape_fn", C.c_int), ("gen_mx", C.c_int), ("root_id", C.c_int),
        ("non_leaf_bf", C.c_int), ("compute_gran", C.c_int), ("b_0", C.c_double),
        ("non_leaf_prob", C.c_double), ("shift_depth", C.c_double),
    ]


class UtsResult(C.Structure):
    _fields_ = [
        ("nodes", C.c_uint64), ("leaves", C.c_uint64), ("max_depth", C.c_uint64),
        ("chunks_pushed", C.c_uint64), ("chunks_stolen", C.c_uint64), ("batches", C.c_uint64),
        ("kernel_ms", C.c_double), ("busy_frac", C.c_double), ("us_per_batch", C.c_double),
    ]


class UtsLaunch(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("mode", "feat", "workers_per_group", "grid", "ring", "seeded",
                                       "seed_target", "spill_lo", "waves_per_cu")]


UTS_MODES = {0: "rules_global", 1: "rules_lds", 2: "bin", 3: "geo_fixed"}


class FibResult(C.Structure):
    _fields_ = [("tasks", C.c_uint64), ("joins", C.c_uint64), ("chunks_pushed", C.c_uint64),
                ("chunks_stolen", C.c_uint64), ("kernel_ms", C.c_double),
                ("busy_frac", C.c_double)]


class SwResult(C.Structure):
    _fields_ = [("tiles", C.c_uint64), ("releases", C.c_uint64), ("kernel_ms", C.c_double),
                ("cells_per_s", C.c_double), ("tile_us", C.c_double), ("release_us", C.c_double)]


class SwEdges(C.Structure):
    """hclib_hip_sw_edges_t."""

    _fields_ = [("bottoms", C.c_void_p), ("rights", C.c_void_p), ("corners", C.c_void_p),
                ("path", C.c_int), ("form", C.c_int)]


SW_EDGE_BOTTOMS, SW_EDGE_RIGHTS, SW_EDGE_CORNERS = 1, 2, 4
# HCLIB_HIP_SW_PATH_*
SW_PATHS = {1: "queue", 2: "rows1", 3: "band-rows", 4: "dag-wave", 5: "dag-wg", 6: "dag-pk"}


class CholeskyResult(C.Structure):
    """hclib_hip_cholesky_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("puts", C.c_uint64), ("releases", C.c_uint64),
                ("potrf", C.c_uint64), ("trsm", C.c_uint64), ("syrk", C.c_uint64), ("gemm", C.c_uint64),
                ("kernel_ms", C.c_double), ("gflops", C.c_double), ("fail_col", C.c_int)]


class SortResult(C.Structure):
    """hclib_hip_sort_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("sort_leaf", C.c_uint64), ("sort_split", C.c_uint64),
                ("merge_leaf", C.c_uint64), ("merge_split", C.c_uint64), ("merge_empty", C.c_uint64),
                ("finishes", C.c_uint64), ("check_ins", C.c_uint64),
                ("kernel_ms", C.c_double), ("keys_per_s", C.c_double)]


class SparseLUResult(C.Structure):
    """hclib_hip_sparselu_result_t."""

    _fields_ = [("blocks_in", C.c_uint64), ("blocks_out", C.c_uint64),
                ("lu0", C.c_uint64), ("fwd", C.c_uint64), ("bdiv", C.c_uint64), ("bmod", C.c_uint64),
                ("tasks", C.c_uint64), ("puts", C.c_uint64), ("releases", C.c_uint64),
                ("kernel_ms", C.c_double), ("gflops", C.c_double), ("wgs_per_cu", C.c_int)]


class NQueensResult(C.Structure):
    """hclib_hip_nqueens_result_t."""

    _fields_ = [("solutions", C.c_uint64), ("tasks", C.c_uint64), ("items", C.c_uint64), ("scopes", C.c_uint64),
                ("joins", C.c_uint64), ("chunks_pushed", C.c_uint64), ("chunks_stolen", C.c_uint64),
                ("kernel_ms", C.c_double), ("busy_frac", C.c_double)]


class StrassenResult(C.Structure):
    """hclib_hip_strassen_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("splits", C.c_uint64), ("base", C.c_uint64), ("tiles", C.c_uint64),
                ("pre_bands", C.c_uint64), ("combine_bands", C.c_uint64), ("finishes", C.c_uint64),
                ("check_ins", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("kernel_ms", C.c_double), ("gflops", C.c_double)]


class FftResult(C.Structure):
    """hclib_hip_fft_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("leaves", C.c_uint64), ("calls", C.c_uint64), ("unsh_bands", C.c_uint64),
                ("twid_bands", C.c_uint64), ("finishes", C.c_uint64), ("check_ins", C.c_uint64),
                ("bytes_moved", C.c_uint64), ("nfactors", C.c_int32), ("factors", C.c_int32 * 40),
                ("cutoff", C.c_int32), ("band", C.c_int32), ("kernel_ms", C.c_double), ("gbytes_per_s", C.c_double)]


class JacobiResult(C.Structure):
    """hclib_hip_jacobi_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("puts", C.c_uint64), ("releases", C.c_uint64), ("supersteps", C.c_uint64),
                ("bytes_moved", C.c_uint64), ("block", C.c_int), ("fuse", C.c_int), ("wgs_per_cu", C.c_int),
                ("kernel_ms", C.c_double), ("gbytes_per_s", C.c_double), ("gcells_per_s", C.c_double)]


class BfsResult(C.Structure):
    """hclib_hip_bfs_result_t."""

    _fields_ = [("levels", C.c_uint64), ("reached", C.c_uint64), ("relaxed", C.c_uint64), ("items", C.c_uint64),
                ("chunks_pushed", C.c_uint64), ("chunks_stolen", C.c_uint64),
                ("kernel_ms", C.c_double), ("busy_frac", C.c_double)]


class CfdResult(C.Structure):
    """hclib_hip_cfd_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("puts", C.c_uint64), ("releases", C.c_uint64), ("stages", C.c_uint64),
                ("bytes_moved", C.c_uint64), ("block", C.c_int), ("form", C.c_int),
                ("kernel_ms", C.c_double), ("elements_per_s", C.c_double)]


class SradResult(C.Structure):
    """hclib_hip_srad_result_t."""

    _fields_ = [("tasks", C.c_uint64), ("puts", C.c_uint64), ("releases", C.c_uint64), ("awaits", C.c_uint64),
                ("iterations", C.c_uint64), ("bytes_moved", C.c_uint64), ("block", C.c_int), ("form", C.c_int),
                ("kernel_ms", C.c_double)]


class HealthParams(C.Structure):
    """hclib_hip_health_params_t: the ten settings of a BOTS health input file."""

    _fields_ = [(k, C.c_int) for k in ("level", "cities", "population_ratio", "sim_time", "assess_time",
                                       "convalescence_time")] + [("seed", C.c_int32)] + \
               [(k, C.c_float) for k in ("get_sick_p", "convalescence_p", "realloc_p")]


class HealthResult(C.Structure):
    """hclib_hip_health_result_t."""

    _fields_ = [(k, C.c_int64) for k in ("population", "hospitals", "personnel", "hosps_visited", "in_village",
                                         "waiting", "assess", "inside", "total_time")] + \
               [(k, C.c_uint64) for k in ("tasks", "finishes", "check_ins", "leaf_calls", "inner_calls", "posts")] + \
               [("kernel_ms", C.c_double), ("rounds_per_s", C.c_double)]


class HealthState(C.Structure):
    """hclib_hip_health_state_t."""

    _fields_ = [(k, C.c_void_p) for k in ("seed", "time", "time_left", "hosps_visited", "village", "lists")]


FLOORPLAN_MAX_CELLS, FLOORPLAN_MAX_SHAPES = 20, 8  # include/hclib_hip.h


class FloorplanInput(C.Structure):
    """hclib_hip_floorplan_input_t: arrays by cell id 1..n (entry 0 unused)."""

    _fields_ = [("n", C.c_int32), ("solution", C.c_int32), ("shapes", C.c_int32 * (FLOORPLAN_MAX_CELLS + 1)),
                ("shape", C.c_int32 * 2 * FLOORPLAN_MAX_SHAPES * (FLOORPLAN_MAX_CELLS + 1)),
                ("left", C.c_int32 * (FLOORPLAN_MAX_CELLS + 1)), ("above", C.c_int32 * (FLOORPLAN_MAX_CELLS + 1)),
                ("next", C.c_int32 * (FLOORPLAN_MAX_CELLS + 1))]


class FloorplanPlacement(C.Structure):
    """hclib_hip_floorplan_placement_t."""

    _fields_ = [("shape", C.c_int32), ("top", C.c_int32), ("lhs", C.c_int32)]


class FloorplanResult(C.Structure):
    """hclib_hip_floorplan_result_t."""

    _fields_ = [("min_area", C.c_int32), ("footprint", C.c_int32 * 2),
                ("placements", FloorplanPlacement * FLOORPLAN_MAX_CELLS)] + \
               [(k, C.c_uint64) for k in ("tasks", "items", "laid", "complete", "improvements", "chunks_pushed",
                                          "chunks_stolen")] + [("kernel_ms", C.c_double), ("busy_frac", C.c_double)]


class AlignmentInput(C.Structure):
    """hclib_hip_alignment_input_t."""

    _fields_ = [("nseqs", C.c_int32), ("total", C.c_int32), ("length", C.POINTER(C.c_int32)),
                ("offset", C.POINTER(C.c_int32)), ("codes", C.POINTER(C.c_uint8)), ("names", C.c_void_p)]


class AlignmentMatrix(C.Structure):
    """hclib_hip_alignment_matrix_t."""

    _fields_ = [("avscore", C.c_int32), ("score", C.c_int32 * 32 * 32)]


class AlignmentPair(C.Structure):
    """hclib_hip_alignment_pair_t."""

    _fields_ = [(k, C.c_int32) for k in ("si", "sj", "g", "gh", "maxscore", "se1", "se2", "sb1", "sb2", "matches",
                                         "diff_calls", "type2", "ties")]


class AlignmentResult(C.Structure):
    """hclib_hip_alignment_result_t."""

    _fields_ = [("scores", C.c_void_p)] + \
               [(k, C.c_uint64) for k in ("pairs", "tasks", "created", "promises", "pair_tasks", "spawn_tasks",
                                          "leaf_tasks", "matches", "diff_calls", "type2", "ties", "cells")] + \
               [("cutoff", C.c_int32), ("kernel_ms", C.c_double), ("cells_per_s", C.c_double)]


class AtomicViewStruct(C.Structure):
    """hclib_hip_atomic_view_t: what device code is handed for one atomic."""

    _fields_ = [("slots", C.c_void_p), ("nslots", C.c_uint32), ("stride", C.c_uint32),
                ("dtype", C.c_int), ("op", C.c_int)]


# every symbol include/hclib_hip.h and include/hclib.h declare (checked by tests)
EXPORTS_HIP = [
    "hclib_hip_init", "hclib_hip_finalize", "hclib_hip_device_memory_live", "hclib_hip_last_error",
    "hclib_hip_num_cus",
    "hclib_hip_version", "hclib_hip_forasync", "hclib_hip_forasync_triad_f32",
    "hclib_hip_num_workers", "hclib_hip_uts_search", "hclib_hip_uts_num_children_host",
    "hclib_hip_uts_bucket_check", "hclib_hip_sha1_calibrate",
    "hclib_hip_fib", "hclib_hip_sw", "hclib_hip_last_sched_counters", "hclib_hip_last_narrow_counters",
    "hclib_hip_last_phase_counters", "hclib_hip_last_shed_counters", "hclib_hip_last_comm_counters",
    "hclib_hip_sw_band_begin", "hclib_hip_sw_band_rows", "hclib_hip_sw_band_end",
    "hclib_hip_sw_edges", "hclib_hip_sw_band_bottoms",
    "hclib_hip_atomic_create", "hclib_hip_atomic_destroy", "hclib_hip_atomic_view",
    "hclib_hip_atomic_gather", "hclib_hip_atomic_gather_async", "hclib_hip_atomic_reset",
    "hclib_hip_forasync_reduce", "hclib_hip_cholesky", "hclib_hip_sort_i64", "hclib_hip_sort_bounds",
    "hclib_hip_sparselu_genmat", "hclib_hip_sparselu_plan", "hclib_hip_sparselu", "hclib_hip_sparselu_bmod_rate",
    "hclib_hip_nqueens", "hclib_hip_nqueens_bounds",
    "hclib_hip_strassen", "hclib_hip_strassen_bounds", "hclib_hip_strassen_last_ticks",
    "hclib_hip_health", "hclib_hip_health_bounds", "hclib_hip_health_last_ticks",
    "hclib_hip_floorplan", "hclib_hip_floorplan_read_input",
    "hclib_hip_alignment", "hclib_hip_alignment_read_input", "hclib_hip_alignment_free_input",
    "hclib_hip_alignment_read_matrix", "hclib_hip_alignment_bounds", "hclib_hip_alignment_last_ticks",
    "hclib_hip_fft", "hclib_hip_fft_factors", "hclib_hip_fft_twiddles", "hclib_hip_fft_bounds", "hclib_hip_fft_last_ticks",
    "hclib_hip_jacobi", "hclib_hip_jacobi_rhs", "hclib_hip_jacobi_bounds",
    "hclib_hip_bfs", "hclib_hip_bfs_bounds", "hclib_hip_bfs_read_input",
    "hclib_hip_cfd", "hclib_hip_cfd_bounds", "hclib_hip_cfd_read_input",
    "hclib_hip_srad", "hclib_hip_srad_image", "hclib_hip_srad_bounds",
    "hclib_atomic_create", "hclib_atomic_init", "hclib_atomic_update", "hclib_atomic_gather",
]

_lib = None


def lib():
    """Load the HIP module library (never a fallback: raises if absent)."""
    global _lib
    if _lib is None:
        try:  # share ONE HIP runtime with torch (same soname libamdhip64.so.7)
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise HclibError(f"{LIB_PATH} is missing: run `python -m hclib_amd.build`")
        L = C.CDLL(LIB_PATH)
        L.hclib_hip_version.restype = C.c_char_p
        L.hclib_hip_last_error.restype = C.c_char_p
        L.hclib_hip_finalize.restype = None
        L.hclib_hip_device_memory_live.argtypes = [C.POINTER(C.c_uint64)]
        L.hclib_hip_device_memory_live.restype = None
        L.hclib_hip_forasync_triad_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                                   C.c_int64, C.c_void_p]
        L.hclib_hip_forasync.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(LoopDomain),
                                         C.c_int, C.c_void_p]
        L.hclib_hip_uts_search.argtypes = [C.POINTER(UtsParams), C.c_int, C.c_int, C.c_int,
                                           C.POINTER(UtsResult), C.c_void_p, C.c_int]
        L.hclib_hip_uts_num_children_host.argtypes = [C.POINTER(UtsParams), C.c_int,
                                                      C.POINTER(C.c_uint32)]
        L.hclib_hip_fib.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(FibResult)]
        L.hclib_hip_sw.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int,
                                   C.c_int, C.POINTER(C.c_int), C.POINTER(SwResult)]
        L.hclib_hip_sw_band_begin.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                              C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(C.c_void_p)]
        L.hclib_hip_sw_band_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        L.hclib_hip_sw_band_end.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                            C.POINTER(C.c_uint64)]
        L.hclib_hip_sw_edges.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int,
                                         C.c_int, C.POINTER(C.c_int), C.POINTER(SwResult),
                                         C.POINTER(SwEdges), C.POINTER(C.c_uint32)]
        L.hclib_hip_sw_band_bottoms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.hclib_hip_atomic_calibrate.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double)]
        L.hclib_hip_sha1_calibrate.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double)]
        L.hclib_hip_uts_last_launch.argtypes = [C.POINTER(UtsLaunch)]
        L.hclib_hip_uts_bucket_check.argtypes = [C.POINTER(UtsParams), C.c_uint64, C.POINTER(C.c_uint64)]
        L.hclib_hip_global_bytes.restype = C.c_size_t
        L.hclib_hip_global_bytes.argtypes = [C.c_uint32]
        L.hclib_hip_global_init.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        L.hclib_hip_global_alloc.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.hclib_hip_global_free.argtypes = [C.c_void_p]
        L.hclib_hip_global_attach.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        L.hclib_hip_global_read.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.hclib_hip_ipc_export.argtypes = [C.c_void_p, C.c_void_p]
        L.hclib_hip_ipc_import.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.hclib_hip_ipc_close.argtypes = [C.c_void_p]
        L.hclib_hip_last_timeline.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
        L.hclib_hip_atomic_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.hclib_hip_atomic_destroy.argtypes = [C.c_void_p]
        L.hclib_hip_atomic_view.argtypes = [C.c_void_p, C.POINTER(AtomicViewStruct)]
        L.hclib_hip_atomic_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.hclib_hip_atomic_gather_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.hclib_hip_atomic_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.hclib_hip_forasync_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(LoopDomain),
                                                C.c_int, C.c_void_p]
        L.hclib_hip_cholesky.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.POINTER(CholeskyResult)]
        L.hclib_hip_sort_i64.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(SortResult)]
        L.hclib_hip_sort_bounds.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_sort_last_ticks.argtypes = [C.POINTER(C.c_uint64)]
        L.hclib_hip_sort_last_ticks.restype = None
        L.hclib_hip_sparselu_genmat.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.hclib_hip_sparselu_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.hclib_hip_sparselu.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.POINTER(SparseLUResult)]
        L.hclib_hip_sparselu_bmod_rate.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                                   C.POINTER(C.c_double)]
        L.hclib_hip_nqueens.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(NQueensResult), C.POINTER(C.c_uint64)]
        L.hclib_hip_nqueens_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_floorplan.argtypes = [C.POINTER(FloorplanInput), C.c_int, C.POINTER(FloorplanResult), C.c_void_p,
                                          C.POINTER(C.c_uint64)]
        L.hclib_hip_floorplan_read_input.argtypes = [C.c_char_p, C.POINTER(FloorplanInput)]
        L.hclib_hip_strassen.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(StrassenResult)]
        L.hclib_hip_strassen_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_strassen_last_ticks.argtypes = [C.POINTER(C.c_uint64)]
        L.hclib_hip_strassen_last_ticks.restype = None
        L.hclib_hip_health.argtypes = [C.POINTER(HealthParams), C.POINTER(HealthResult), C.POINTER(HealthState)]
        L.hclib_hip_health_bounds.argtypes = [C.POINTER(HealthParams), C.POINTER(C.c_uint64)]
        L.hclib_hip_health_last_ticks.argtypes = [C.POINTER(C.c_uint64)]
        L.hclib_hip_health_last_ticks.restype = None
        L.hclib_hip_alignment.argtypes = [C.POINTER(AlignmentInput), C.POINTER(AlignmentMatrix), C.c_int,
                                          C.POINTER(AlignmentResult), C.c_void_p]
        L.hclib_hip_alignment_read_input.argtypes = [C.c_char_p, C.POINTER(AlignmentInput)]
        L.hclib_hip_alignment_free_input.argtypes = [C.POINTER(AlignmentInput)]
        L.hclib_hip_alignment_free_input.restype = None
        L.hclib_hip_alignment_read_matrix.argtypes = [C.c_char_p, C.POINTER(AlignmentMatrix)]
        L.hclib_hip_alignment_bounds.argtypes = [C.POINTER(AlignmentInput), C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_alignment_last_ticks.argtypes = [C.POINTER(C.c_uint64)]
        L.hclib_hip_alignment_last_ticks.restype = None
        L.hclib_hip_fft.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(FftResult)]
        L.hclib_hip_fft_factors.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.hclib_hip_fft_twiddles.argtypes = [C.c_int, C.c_void_p]
        L.hclib_hip_fft_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_fft_last_ticks.argtypes = [C.POINTER(C.c_uint64)]
        L.hclib_hip_fft_last_ticks.restype = None
        L.hclib_hip_jacobi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.POINTER(JacobiResult)]
        L.hclib_hip_jacobi_rhs.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.hclib_hip_jacobi_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_bfs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.POINTER(BfsResult), C.c_void_p, C.c_void_p]
        L.hclib_hip_bfs_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_uint64)]
        L.hclib_hip_bfs_read_input.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.hclib_hip_cfd.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.POINTER(CfdResult)]
        L.hclib_hip_cfd_bounds.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hclib_hip_cfd_read_input.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.hclib_hip_srad.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SradResult)]
        L.hclib_hip_srad_image.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.hclib_hip_srad_bounds.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != HCLIB_HIP_OK:
        msg = lib().hclib_hip_last_error().decode(errors="replace")
        raise HclibError(f"{what} failed ({rc}): {msg}")


def version() -> str:
    return lib().hclib_hip_version().decode()


def init(device: int = 0) -> None:
    _check(lib().hclib_hip_init(device), "hclib_hip_init")


def finalize() -> None:
    """Free every device allocation the library holds on its own account; `init` starts again."""
    lib().hclib_hip_finalize()


def device_memory_live() -> Tuple[int, int]:
    """(live device allocations, their bytes) of the library's own account: arenas and per-call buffers."""
    out = (C.c_uint64 * 2)()
    lib().hclib_hip_device_memory_live(out)
    return int(out[0]), int(out[1])


def num_cus() -> int:
    return lib().hclib_hip_num_cus()


def num_workers() -> int:
    return lib().hclib_hip_num_workers()


# ------------------------------------------------------------------ forasync
def forasync(body: int, args: C.Structure, domains, mode: int, stream: Optional[int] = None):
    """hclib_forasync at the GPU locale (src/hclib.c:452-464); domains is a
    list of (low, high, stride, tile). Returns the domains after the tile==-1
    write-back, as the reference does."""
    dims = (LoopDomain * len(domains))(*[LoopDomain(*d) for d in domains])
    _check(lib().hclib_hip_forasync(body, C.byref(args), len(domains), dims, mode, stream),
           "hclib_hip_forasync")
    return [(d.low, d.high, d.stride, d.tile) for d in dims]


def triad_f32(a_ptr: int, b_ptr: int, c_ptr: int, s: float, n: int, stream: Optional[int] = None):
    _check(lib().hclib_hip_forasync_triad_f32(a_ptr, b_ptr, c_ptr, s, n, stream),
           "hclib_hip_forasync_triad_f32")


# ------------------------------------------------------- privatised atomics
ATOMIC_DTYPES = {"int32": (0, C.c_int32), "uint32": (1, C.c_uint32), "int64": (2, C.c_int64),
                 "uint64": (3, C.c_uint64), "float32": (4, C.c_float), "float64": (5, C.c_double)}
ATOMIC_OPS = {"sum": 0, "max": 1, "or": 2}


class Atomic:
    """A privatised atomic in device memory (hclib_hip_atomic_*, the device
    form of inc/hclib_atomic.h): one slot per wave, folded by gather().
    dtype is a key of ATOMIC_DTYPES (or anything whose str() ends in one, such
    as a numpy or torch dtype), op one of "sum", "max", "or" (logical or:
    0 or 1). Updates accumulate over launches until reset()."""

    def __init__(self, dtype, op: str, default=0):
        name = str(getattr(dtype, "__name__", dtype)).rsplit(".", 1)[-1]
        if name not in ATOMIC_DTYPES:
            raise ValueError(f"Atomic: dtype {dtype!r} is not one of {sorted(ATOMIC_DTYPES)}")
        if op not in ATOMIC_OPS:
            raise ValueError(f"Atomic: op {op!r} is not one of {sorted(ATOMIC_OPS)}")
        self.dtype, self.op = name, op
        code, self._ctype = ATOMIC_DTYPES[name]
        h = C.c_void_p()
        _check(lib().hclib_hip_atomic_create(code, ATOMIC_OPS[op], C.byref(self._ctype(default)), C.byref(h)),
               "hclib_hip_atomic_create")
        self._h = h

    def _handle(self):
        if self._h is None:
            raise HclibError("Atomic: used after close()")
        return self._h

    def view(self) -> AtomicViewStruct:
        v = AtomicViewStruct()
        _check(lib().hclib_hip_atomic_view(self._handle(), C.byref(v)), "hclib_hip_atomic_view")
        return v

    def gather(self, stream: Optional[int] = None):
        """Fold the slots on `stream` and wait; the value as a Python number."""
        out = self._ctype()
        _check(lib().hclib_hip_atomic_gather(self._handle(), stream, C.byref(out)), "hclib_hip_atomic_gather")
        return out.value

    def gather_async(self, device_out: int, stream: Optional[int] = None) -> None:
        _check(lib().hclib_hip_atomic_gather_async(self._handle(), stream, device_out),
               "hclib_hip_atomic_gather_async")

    def reset(self, stream: Optional[int] = None) -> None:
        _check(lib().hclib_hip_atomic_reset(self._handle(), stream), "hclib_hip_atomic_reset")

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None:
            _check(lib().hclib_hip_atomic_destroy(h), "hclib_hip_atomic_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def forasync_reduce(atomic: Atomic, ptr: int, domains, mode: int, stream: Optional[int] = None):
    """atomic.update(x[i]) over the forasync iteration set of the 1-D domain
    (hclib_hip_forasync_reduce); ptr is the device address of x, whose
    elements have the atomic's dtype. Asynchronous on `stream`; returns the
    domains after the tile == -1 write-back, like forasync()."""
    dims = (LoopDomain * len(domains))(*[LoopDomain(*d) for d in domains])
    _check(lib().hclib_hip_forasync_reduce(atomic._handle(), ptr, len(domains), dims, mode, stream),
           "hclib_hip_forasync_reduce")
    return [(d.low, d.high, d.stride, d.tile) for d in dims]


# ----------------------------------------------------------------------- UTS
def parse_uts_args(argv: str) -> UtsParams:
    """UTS argument string -> params (test/uts/uts.c:362-425; T1 defaults)."""
    p = UtsParams(type=1, shape_fn=3, gen_mx=10, root_id=19, non_leaf_bf=4, compute_gran=1,
                  b_0=4.0, non_leaf_prob=15.0 / 64.0, shift_depth=0.5)
    toks = argv.split()
    if len(toks) % 2:
        raise ValueError("UTS arguments come in flag/value pairs")
    for flag, val in zip(toks[::2], toks[1::2]):
        c = flag[1]
        if c == "q": p.non_leaf_prob = float(val)
        elif c == "m": p.non_leaf_bf = int(val)
        elif c == "r": p.root_id = int(val)
        elif c == "t": p.type = int(val)
        elif c == "a": p.shape_fn = int(val)
        elif c == "b": p.b_0 = float(val)
        elif c == "d": p.gen_mx = int(val)
        elif c == "f": p.shift_depth = float(val)
        elif c == "g": p.compute_gran = max(1, int(val))
        elif c in "cixv": pass
        else: raise ValueError(f"unknown UTS flag {flag}")
    return p


def uts(params, shard: int = 0, nshards: int = 1, split_depth: int = 0, max_levels: int = 0):
    """Search a UTS tree on the GPU; returns a dict of counts and stats."""
    if isinstance(params, str):
        params = parse_uts_args(params)
    r = UtsResult()
    hist = (C.c_uint64 * max_levels)() if max_levels else None
    _check(lib().hclib_hip_uts_search(C.byref(params), shard, nshards, split_depth, C.byref(r),
                                      hist, max_levels), "hclib_hip_uts_search")
    out = {k: getattr(r, k) for k, _ in UtsResult._fields_}
    if hist is not None:
        out["levels"] = list(hist)
    return out


def uts_last_launch() -> dict:
    """The launch shape of this thread's last uts() (hclib_hip_uts_last_launch)."""
    r = UtsLaunch()
    _check(lib().hclib_hip_uts_last_launch(C.byref(r)), "hclib_hip_uts_last_launch")
    out = {k: getattr(r, k) for k, _ in UtsLaunch._fields_}
    out["mode"] = UTS_MODES.get(out["mode"], out["mode"])
    return out


def uts_bucket_check(params, nrandom: int = 1 << 20):
    """Host check (no GPU) of the bucketed numChildren lookup the fixed-shape
    GEO kernels use: (mismatches, values compared)."""
    if isinstance(params, str):
        params = parse_uts_args(params)
    n = C.c_uint64()
    bad = lib().hclib_hip_uts_bucket_check(C.byref(params), nrandom, C.byref(n))
    if bad < 0:
        raise HclibError(f"hclib_hip_uts_bucket_check failed ({bad}): "
                         f"{lib().hclib_hip_last_error().decode(errors='replace')}")
    return bad, n.value


def uts_num_children_host(params, height: int, state_words) -> int:
    if isinstance(params, str):
        params = parse_uts_args(params)
    st = (C.c_uint32 * 5)(*state_words)
    return lib().hclib_hip_uts_num_children_host(C.byref(params), height, st)


# ----------------------------------------------------------------------- fib
def global_bytes(cap: int) -> int:
    """Bytes of a cross-GPU work-sharing region with `cap` chunk slots."""
    n = lib().hclib_hip_global_bytes(cap)
    if n == 0:
        raise HclibError("global_bytes: cap must be a power of two >= 2")
    return n


GLOBAL_MEM_KINDS = {"uncached": 0, "fine": 1, "device": 2}


def global_alloc(cap: int, kind: str = "uncached") -> int:
    """Allocate a work-sharing region (hclib_hip_global_alloc); kind is one of
    GLOBAL_MEM_KINDS."""
    p = C.c_void_p()
    _check(lib().hclib_hip_global_alloc(cap, GLOBAL_MEM_KINDS[kind], C.byref(p)), "hclib_hip_global_alloc")
    return p.value


def global_free(region: Optional[int]) -> None:
    _check(lib().hclib_hip_global_free(region), "hclib_hip_global_free")


def global_init(region: int, cap: int, nranks: int) -> None:
    _check(lib().hclib_hip_global_init(region, cap, nranks), "hclib_hip_global_init")


def global_attach(region: Optional[int], cap: int = 0, rank: int = 0) -> None:
    _check(lib().hclib_hip_global_attach(region, cap, rank), "hclib_hip_global_attach")


def global_read(region: int) -> dict:
    out = (C.c_uint64 * 35)()
    _check(lib().hclib_hip_global_read(region, out), "hclib_hip_global_read")
    return {"active": out[0], "idle": out[1], "queued": out[2],
            "exported": [out[3 + 2 * r] for r in range(16)], "imported": [out[4 + 2 * r] for r in range(16)]}


def ipc_export(dev_ptr: int) -> bytes:
    h = (C.c_char * 64)()
    _check(lib().hclib_hip_ipc_export(dev_ptr, h), "hclib_hip_ipc_export")
    return bytes(h)


def ipc_import(handle: bytes) -> int:
    p = C.c_void_p()
    _check(lib().hclib_hip_ipc_import(C.c_char_p(handle), C.byref(p)), "hclib_hip_ipc_import")
    return p.value


def ipc_close(dev_ptr: int) -> None:
    _check(lib().hclib_hip_ipc_close(dev_ptr), "hclib_hip_ipc_close")


def fib(n: int):
    v = C.c_int64()
    r = FibResult()
    _check(lib().hclib_hip_fib(n, C.byref(v), C.byref(r)), "hclib_hip_fib")
    return v.value, {k: getattr(r, k) for k, _ in FibResult._fields_}


# ------------------------------------------------------------------------ SW
def sw(s1: bytes, s2: bytes, tile_w: int, tile_h: int):
    """Tiled Smith-Waterman DAG on the GPU; sequences coded 1..4."""
    score = C.c_int()
    r = SwResult()
    _check(lib().hclib_hip_sw(s1, len(s1), s2, len(s2), tile_w, tile_h, C.byref(score),
                              C.byref(r)), "hclib_hip_sw")
    return score.value, {k: getattr(r, k) for k, _ in SwResult._fields_}


def sw_edges(s1: bytes, s2: bytes, tile_w: int, tile_h: int):
    """sw(), plus what every tile put (hclib_hip_sw_edges): returns
    (score, stats, edges). edges["bottoms"] is [nth][ntw*tw] (H of matrix
    rows th, 2 th, ...), edges["rights"] [ntw][nth*th] (H of matrix columns
    tw, 2 tw, ...), edges["corners"] [nth][ntw]: int32 arrays, or None where
    the schedule that ran keeps no such array on the device. edges["path"]
    names that schedule (SW_PATHS), edges["form"] its multi-wave band form."""
    import numpy as np

    ntw, nth = len(s1) // tile_w, len(s2) // tile_h
    nt = max(ntw * nth, 0)
    # poisoned: a value the read-back left alone cannot pass for a score
    bottoms = np.full((nth, ntw * tile_w), -(1 << 30), dtype=np.int32)
    rights = np.full((nt, tile_h), -(1 << 30), dtype=np.int32)
    corners = np.full((nth, ntw), -(1 << 30), dtype=np.int32)
    e = SwEdges(bottoms.ctypes.data, rights.ctypes.data, corners.ctypes.data, 0, 0)
    score, r, filled = C.c_int(), SwResult(), C.c_uint32()
    _check(lib().hclib_hip_sw_edges(s1, len(s1), s2, len(s2), tile_w, tile_h, C.byref(score), C.byref(r),
                                    C.byref(e), C.byref(filled)), "hclib_hip_sw_edges")
    m = filled.value
    edges = {
        "bottoms": bottoms if m & SW_EDGE_BOTTOMS else None,
        # [nth][ntw][th] -> [ntw][nth*th]: tile column j's right column, top to bottom
        "rights": (np.ascontiguousarray(rights.reshape(nth, ntw, tile_h).transpose(1, 0, 2))
                   .reshape(ntw, nth * tile_h) if m & SW_EDGE_RIGHTS else None),
        "corners": corners if m & SW_EDGE_CORNERS else None,
        "path": SW_PATHS.get(e.path), "form": e.form,
    }
    return score.value, {k: getattr(r, k) for k, _ in SwResult._fields_}, edges


class SwBand:
    """One rank's band of tile columns [j0, j1) of the SW tile grid
    (hclib_hip_sw_band_*, include/hclib_hip.h). rows() launches tile rows
    [i0, i1) on `stream` (a raw hipStream_t handle, e.g. torch's
    current_stream().cuda_stream); left_in / right_out are device pointers
    to nth*th int32 (H of matrix columns j0*tw and j1*tw, rows 1..)."""

    def __init__(self, s1: bytes, s2: bytes, tile_w: int, tile_h: int, j0: int, j1: int):
        self.ntw, self.nth = len(s1) // tile_w, len(s2) // tile_h
        self.tile_w, self.tile_h, self.j0, self.j1 = tile_w, tile_h, j0, j1
        h = C.c_void_p()
        _check(lib().hclib_hip_sw_band_begin(s1, len(s1), s2, len(s2), tile_w, tile_h, j0, j1,
                                             C.byref(h)), "hclib_hip_sw_band_begin")
        self._h = h

    def rows(self, i0: int, i1: int, left_in: int | None, right_out: int | None, stream: int):
        _check(lib().hclib_hip_sw_band_rows(self._h, i0, i1, left_in, right_out, stream),
               "hclib_hip_sw_band_rows")

    def bottoms(self, stream: int):
        """Before end(): synchronise and return the band's bottom rows, int32
        [nth][(j1-j0)*tile_w] (H of matrix rows th, 2 th, ..., the band's columns)."""
        import numpy as np

        out = np.full((self.nth, (self.j1 - self.j0) * self.tile_w), -(1 << 30), dtype=np.int32)
        _check(lib().hclib_hip_sw_band_bottoms(self._h, stream, out.ctypes.data), "hclib_hip_sw_band_bottoms")
        return out

    def end(self, stream: int):
        """Synchronise, free; returns (bottom-right cell of the band, tiles run)."""
        corner, tiles = C.c_int(), C.c_uint64()
        h, self._h = self._h, None
        _check(lib().hclib_hip_sw_band_end(h, stream, C.byref(corner), C.byref(tiles)),
               "hclib_hip_sw_band_end")
        return corner.value, tiles.value


def sw_map(text: bytes) -> bytes:
    """clear_whitespaces_do_mapping (smith_waterman.cpp:45-59): keep ACGT -> 1..4."""
    table = bytes.maketrans(b"ACGT", b"\x01\x02\x03\x04")
    return bytes(x for x in text if x in b"ACGT").translate(table)


# ------------------------------------------------------------------ Cholesky
CHOL_MODES = {"exact": 0}  # HCLIB_HIP_CHOL_EXACT


class NotSPDError(HclibError):
    """hclib_hip_cholesky met a pivot <= 0 (the reference's "Not a symmetric
    positive definite (SPD) matrix"); fail_col is the global column."""

    def __init__(self, msg: str, fail_col: int):
        super().__init__(msg)
        self.fail_col = fail_col


def cholesky(a, tile: int, mode: str = "exact"):
    """Tiled Cholesky of test/cholesky on the device promise DAG
    (hclib_hip_cholesky): a is an n x n float64 array whose lower triangle is
    read; returns (L, stats) with L lower triangular (+0.0 above the diagonal).
    mode "exact" (the one mode) is bit-identical to the reference for every
    tile size."""
    import numpy as np

    if mode not in CHOL_MODES:
        raise ValueError(f"cholesky: mode {mode!r} is not one of {sorted(CHOL_MODES)}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("cholesky: a must be a square matrix")
    out = np.empty_like(a)
    r = CholeskyResult(fail_col=-1)
    rc = lib().hclib_hip_cholesky(a.ctypes.data, a.shape[0], tile, CHOL_MODES[mode], out.ctypes.data, C.byref(r))
    if rc != HCLIB_HIP_OK and r.fail_col >= 0:
        msg = lib().hclib_hip_last_error().decode(errors="replace")
        raise NotSPDError(f"hclib_hip_cholesky failed ({rc}): {msg}", r.fail_col)
    _check(rc, "hclib_hip_cholesky")
    return out, {k: getattr(r, k) for k, _ in CholeskyResult._fields_}


def cholesky_read(path: str, n: int):
    """The reference's input reader (cholesky.cpp:57-61): n * n numbers
    separated by whitespace, row by row."""
    import numpy as np

    with open(path) as f:
        vals = f.read().split()
    if len(vals) < n * n:
        raise ValueError(f"cholesky_read: {path} holds {len(vals)} values, {n}x{n} needs {n * n}")
    return np.array(vals[:n * n], dtype=np.float64).reshape(n, n)


def cholesky_format(L) -> str:
    """The reference's cholesky.out writer (cholesky.cpp:129-147): row by row
    the lower triangle, each value as "%lf " (six decimals), no newlines."""
    n = L.shape[0]
    return "".join("%f " % v for i in range(n) for v in L[i, :i + 1].tolist())


# ---------------------------------------------------------------- BOTS sort
def sort(keys, merge_cutoff: int = 2048, sort_cutoff: int = 2048):
    """BOTS sort (cilksort) on dynamic device dataflow (hclib_hip_sort_i64):
    keys is a one-dimensional array of int64; returns (the sorted keys as a new
    int64 ndarray, stats). merge_cutoff / sort_cutoff are the reference's
    cutoff_value / cutoff_value_1."""
    import numpy as np

    a = np.array(keys, dtype=np.int64, copy=True, order="C")
    if a.ndim != 1:
        raise ValueError("sort: keys must be one-dimensional")
    r = SortResult()
    _check(lib().hclib_hip_sort_i64(a.ctypes.data, a.shape[0], merge_cutoff, sort_cutoff, C.byref(r)),
           "hclib_hip_sort_i64")
    return a, {k: getattr(r, k) for k, _ in SortResult._fields_}


def sort_bounds(n: int, merge_cutoff: int = 2048, sort_cutoff: int = 2048) -> dict:
    """The pool sizes a sort of n keys allocates (hclib_hip_sort_bounds): upper
    bounds on its device tasks, promises (finish scopes) and wait nodes."""
    out = (C.c_uint64 * 3)()
    _check(lib().hclib_hip_sort_bounds(n, merge_cutoff, sort_cutoff, out), "hclib_hip_sort_bounds")
    return {"tasks": out[0], "promises": out[1], "wait_nodes": out[2]}


def sort_last_ticks() -> dict:
    """Wave time of the last sort() by task class, in ticks of the 100 MHz
    device clock (hclib_hip_sort_last_ticks)."""
    out = (C.c_uint64 * 6)()
    lib().hclib_hip_sort_last_ticks(out)
    return dict(zip(("sort_leaf", "sort_split", "merge_leaf", "merge_split", "merge_empty", "merge_phase"), out))


def sort_bots_input(n: int):
    """The reference's input (fill_array + scramble_array, sort.ref.c:425-446):
    0 .. n-1, then for every i a swap with j = rand % n, rand the 64-bit LCG
    rand * 1103515245 + 12345 (:93-97) from seed 1."""
    import numpy as np

    if n < 1:
        raise ValueError("sort_bots_input: n must be positive")
    # rand_i = a^i + c (1 + a + ... + a^(i-1)) mod 2^64 for seed 1: uint64
    # arithmetic wraps, so both series come from cumulative operations
    with np.errstate(over="ignore"):
        pw = np.cumprod(np.full(n, 1103515245, dtype=np.uint64))
        geo = np.cumsum(np.concatenate((np.ones(1, dtype=np.uint64), pw[:-1])))
        js = ((pw + np.uint64(12345) * geo) % np.uint64(n)).tolist()
    a = list(range(n))
    for i, j in enumerate(js):
        a[i], a[j] = a[j], a[i]
    return np.array(a, dtype=np.int64)


# ------------------------------------------------------------ BOTS SparseLU
SPARSELU_KINDS = ("lu0", "fwd", "bdiv", "bmod")  # payload word 0 of a planned task


def _slu_mask(mask):
    import numpy as np

    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("sparselu: mask must be a square matrix of block flags")
    return m


def sparselu_genmat(S: int, B: int):
    """The reference's generator (sparselu.ref.c:86-133, hclib_hip_sparselu_genmat):
    (mask, blocks) with mask an S x S uint8 array and blocks the present blocks
    in row-major (ii, jj) order, float32 of shape (count, B, B)."""
    import numpy as np

    if S < 1 or B < 1:
        raise ValueError("sparselu_genmat: S and B must be positive")
    mask = np.zeros((S, S), dtype=np.uint8)
    _check(lib().hclib_hip_sparselu_genmat(S, B, mask.ctypes.data, None), "hclib_hip_sparselu_genmat")
    blocks = np.empty((int(mask.sum()), B, B), dtype=np.float32)
    _check(lib().hclib_hip_sparselu_genmat(S, B, mask.ctypes.data, blocks.ctypes.data), "hclib_hip_sparselu_genmat")
    return mask, blocks


def sparselu_plan(mask, graph: bool = True) -> dict:
    """The symbolic pass of SparseLU on the host (hclib_hip_sparselu_plan; no
    GPU): the final block structure after fill-in, the task counts and, with
    graph=True, the promise DAG: payload (tasks x 4: kind, kk, ii, jj — the
    task writes block (ii, jj)), await_off (tasks + 1) and await_ids, where
    promise p is the one task p puts."""
    import numpy as np

    m = _slu_mask(mask)
    S = m.shape[0]
    out = np.zeros_like(m)
    counts = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_sparselu_plan(m.ctypes.data, S, out.ctypes.data, counts, None, None, None),
           "hclib_hip_sparselu_plan")
    plan = {"mask_out": out, "blocks_in": counts[4], "blocks_out": counts[5], "tasks": sum(counts[:4])}
    plan.update(zip(SPARSELU_KINDS, counts[:4]))
    if graph:
        n = plan["tasks"]
        payload = np.zeros((n, 4), dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint32)
        ids = np.zeros(3 * n, dtype=np.uint32)
        _check(lib().hclib_hip_sparselu_plan(m.ctypes.data, S, None, None, payload.ctypes.data, off.ctypes.data,
                                             ids.ctypes.data), "hclib_hip_sparselu_plan")
        plan.update(payload=payload, await_off=off, await_ids=ids[:int(off[-1])].copy())
    return plan


def sparselu(mask, blocks, B: int):
    """BOTS SparseLU on the device promise DAG (hclib_hip_sparselu): mask is an
    S x S array of block flags, blocks the present blocks in row-major (ii, jj)
    order (count x B x B float32). Returns (mask_out, blocks_out, stats):
    the structure after fill-in and its blocks, L and U in place, bit-identical
    to the reference's sparselu_seq_call. No pivoting and no pivot check."""
    import numpy as np

    m = _slu_mask(mask)
    S = m.shape[0]
    b = np.ascontiguousarray(blocks, dtype=np.float32)
    if 1 <= B <= 128 and b.size != int(m.sum()) * B * B:
        raise ValueError(f"sparselu: {int(m.sum())} present blocks of {B} x {B} need {int(m.sum()) * B * B} "
                         f"floats, blocks holds {b.size}")
    counts = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_sparselu_plan(m.ctypes.data, S, None, counts, None, None, None), "hclib_hip_sparselu_plan")
    mask_out = np.zeros_like(m)
    out = np.empty((counts[5], max(B, 0), max(B, 0)), dtype=np.float32)
    r = SparseLUResult()
    _check(lib().hclib_hip_sparselu(m.ctypes.data, b.ctypes.data, S, B, mask_out.ctypes.data, out.ctypes.data,
                                    C.byref(r)), "hclib_hip_sparselu")
    return mask_out, out, {k: getattr(r, k) for k, _ in SparseLUResult._fields_}


def sparselu_bmod_rate(B: int, wgs_per_cu: int = 2, reps: int = 64):
    """The bmod body alone on resident blocks (hclib_hip_sparselu_bmod_rate):
    (kernel ms, GFLOP/s), the unfused f32 rate SparseLU's updates can reach."""
    ms, gf = C.c_double(), C.c_double()
    _check(lib().hclib_hip_sparselu_bmod_rate(B, wgs_per_cu, reps, C.byref(ms), C.byref(gf)),
           "hclib_hip_sparselu_bmod_rate")
    return ms.value, gf.value


def sparselu_structure(mask) -> str:
    """The reference's print_structure picture (sparselu.ref.c:141-148): one
    line per block row, "x" for a present block and " " for an absent one."""
    return "".join("".join("x" if v else " " for v in row) + "\n" for row in _slu_mask(mask).tolist())


# ---------------------------------------------------------------- N-Queens
NQUEENS_FORMS = {"bots": 0, "flat": 1}  # HCLIB_HIP_NQUEENS_BOTS / _FLAT


def _nqueens_form(form) -> int:
    if form not in NQUEENS_FORMS:
        raise ValueError(f"nqueens: form {form!r} is not one of {sorted(NQUEENS_FORMS)}")
    return NQUEENS_FORMS[form]


def nqueens(n: int, form: str = "bots", task_depth: int = 0, hist: bool = False) -> dict:
    """N-Queens on the work-stealing scheduler (hclib_hip_nqueens): form "bots"
    (one finish scope per call, sums climbing the scopes) or "flat" (a task per
    valid placement, one counter). task_depth is the BOTS cutoff: calls at that
    depth and below are finished by one lane's serial search; 0 = every call
    spawns. Returns the fields of hclib_hip_nqueens_result_t and, with hist,
    "hist": the number of valid prefixes of each length 0..n."""
    r = NQueensResult()
    h = (C.c_uint64 * (max(n, 0) + 1))() if hist else None
    _check(lib().hclib_hip_nqueens(n, _nqueens_form(form), task_depth, C.byref(r), h), "hclib_hip_nqueens")
    out = {k: getattr(r, k) for k, _ in NQueensResult._fields_}
    if hist:
        out["hist"] = list(h)
    return out


def nqueens_bounds(n: int, form: str = "bots", task_depth: int = 0) -> dict:
    """The reference's task and finish-scope counts for (n, form, task_depth),
    on the host alone (hclib_hip_nqueens_bounds); scopes is what the BOTS
    form's arena is sized from."""
    out = (C.c_uint64 * 2)()
    _check(lib().hclib_hip_nqueens_bounds(n, _nqueens_form(form), task_depth, out), "hclib_hip_nqueens_bounds")
    return {"tasks": out[0], "scopes": out[1]}


# ------------------------------------------------------------ BOTS Strassen
def strassen(a, b, cutoff: int = 0, band_rows: int = 0):
    """BOTS Strassen on dynamic device dataflow (hclib_hip_strassen): a and b
    are square float64 arrays of one power-of-two size; returns (a x b as the
    reference's OptimizedStrassenMultiply computes it, bit for bit, stats).
    cutoff is the reference's (0 = 64), band_rows the rows per band task of the
    two sweeps (0 = the default: 8, or 16 for a tree of 8192 leaf multiplies or
    more)."""
    import numpy as np

    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or b.shape != a.shape:
        raise ValueError("strassen: a and b must be square matrices of the same size")
    c = np.empty_like(a)
    r = StrassenResult()
    _check(lib().hclib_hip_strassen(a.ctypes.data, b.ctypes.data, c.ctypes.data, a.shape[0], cutoff, band_rows,
                                    C.byref(r)), "hclib_hip_strassen")
    return c, {k: getattr(r, k) for k, _ in StrassenResult._fields_}


def strassen_bounds(n: int, cutoff: int = 0, band_rows: int = 0) -> dict:
    """What a strassen() of size n allocates (hclib_hip_strassen_bounds), exact
    and on the host alone: device tasks, finish scopes, wait nodes and the
    bytes of the temporaries."""
    out = (C.c_uint64 * 4)()
    _check(lib().hclib_hip_strassen_bounds(n, cutoff, band_rows, out), "hclib_hip_strassen_bounds")
    return {"tasks": out[0], "scopes": out[1], "wait_nodes": out[2], "workspace_bytes": out[3]}


def strassen_waves_per_cu(n: int, cutoff: int = 0) -> int:
    """The persistent waves per CU a strassen() of this tree launches (the rule
    of hclib_amd/csrc/strassen.hip, str_waves_per_cu, restated: measurements
    divide the last launch's ticks by them): 8 from 8192 leaf multiplies on, 2
    from 1024 on, else 1; HCLIB_HIP_STRASSEN_WAVES_PER_CU overrides it."""
    env = os.environ.get("HCLIB_HIP_STRASSEN_WAVES_PER_CU")
    if env:
        return min(max(int(env), 1), 8)
    cutoff = cutoff or 64
    calls, size = 1, n
    while size > cutoff:
        calls, size = calls * 7, size // 2
    leaves = calls * (size // 64) ** 2 if size > 64 else calls
    return 8 if leaves >= 8192 else (2 if leaves >= 1024 else 1)


def strassen_last_ticks() -> dict:
    """Wave time of the last strassen() by task class, in ticks of the 100 MHz
    device clock (hclib_hip_strassen_last_ticks)."""
    out = (C.c_uint64 * 6)()
    lib().hclib_hip_strassen_last_ticks(out)
    return dict(zip(("multiply", "pre", "combine", "split", "fork", "post"), out))


# ------------------------------------------------------------------ BOTS fft
def fft(x, w=None, cutoff: int = 0, band: int = 0):
    """BOTS fft on dynamic device dataflow (hclib_hip_fft): x is a complex128
    vector of n points; returns (fft_seq's output given the table w, bit for
    bit, stats). w is the twiddle table the transform reads, n + 1 entries as a
    complex128 vector or an (n + 1, 2) float64 array: the reference's own table
    gives the reference's bits; None means fft_twiddles(n). cutoff is the
    largest call that runs as one task (0 = 8192, at least 32), band the
    columns per band task of the two sweeps (0 = 256, or 1024 for n above 2^22; a
    multiple of 64);
    results depend on neither."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.complex128)
    if x.ndim != 1:
        raise ValueError("fft: x must be a vector")
    n = x.shape[0]
    wp = None
    if w is not None:
        w = np.ascontiguousarray(w)
        w = np.ascontiguousarray(w, dtype=np.complex128 if np.iscomplexobj(w) else np.float64)
        if w.size * (2 if np.iscomplexobj(w) else 1) != 2 * (n + 1):
            raise ValueError("fft: w must hold n + 1 (re, im) pairs")
        wp = w.ctypes.data
    out = np.empty_like(x)
    r = FftResult()
    _check(lib().hclib_hip_fft(x.ctypes.data, out.ctypes.data, n, wp, cutoff, band, C.byref(r)), "hclib_hip_fft")
    st = {k: getattr(r, k) for k, _ in FftResult._fields_ if k not in ("factors", "nfactors")}
    st["factors"] = list(r.factors[:r.nfactors])
    return out, st


def fft_factors(n: int) -> list:
    """fft_seq's factor list of n (hclib_hip_fft_factors, host only)."""
    out = (C.c_int * 40)()
    cnt = lib().hclib_hip_fft_factors(n, out)
    if cnt < 0:
        _check(cnt, "hclib_hip_fft_factors")
    return list(out[:cnt])


def fft_twiddles(n: int):
    """The table compute_w_coefficients fills, by the reference's formula and
    write order through this host's cos and sin: (n + 1, 2) float64
    (hclib_hip_fft_twiddles, host only). The reference's binary differs from it
    in the last bit of a few entries, so its own table is an input of fft()."""
    import numpy as np

    if n < 1:
        _check(lib().hclib_hip_fft_twiddles(n, None), "hclib_hip_fft_twiddles")
    w = np.empty((n + 1, 2), dtype=np.float64)
    _check(lib().hclib_hip_fft_twiddles(n, w.ctypes.data), "hclib_hip_fft_twiddles")
    return w


def fft_bounds(n: int, cutoff: int = 0, band: int = 0) -> dict:
    """What an fft() of n points creates (hclib_hip_fft_bounds), exact and on the
    host alone: device tasks, finish scopes, wait nodes, leaf tasks, band tasks
    and the bytes its passes move."""
    out = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_fft_bounds(n, cutoff, band, out), "hclib_hip_fft_bounds")
    return dict(zip(("tasks", "scopes", "nodes", "leaves", "bands", "bytes"), out))


def fft_last_ticks() -> dict:
    """Wave time of the last fft() by task class, in ticks of the 100 MHz device
    clock (hclib_hip_fft_last_ticks)."""
    out = (C.c_uint64 * 6)()
    lib().hclib_hip_fft_last_ticks(out)
    return dict(zip(("leaf", "unsh", "twid", "call", "fork", "post"), out))


# ------------------------------------------------------------ Kastors Jacobi
def jacobi(f, unew0, dx=None, dy=None, block: int = 0, niter: int = 4, fuse: int = 0):
    """Kastors jacobi on the device promise DAG (hclib_hip_jacobi): niter sweeps of
    the 5-point stencil over the (nx, ny) float64 grid unew0 with right-hand side
    and boundary values f; returns (sweep_seq's unew, bit for bit, stats). dx and
    dy default to run()'s 1 / (nx - 1) and 1 / (ny - 1). block (0 = 128, the
    reference's default, which is above what fits: name one with block + 2 fuse
    <= 82) must divide both sides; a task advances its block by up to fuse
    sweeps (0 = the default) from LDS; results depend on neither."""
    import numpy as np

    f = np.ascontiguousarray(f, dtype=np.float64)
    unew0 = np.ascontiguousarray(unew0, dtype=np.float64)
    if f.ndim != 2 or f.shape != unew0.shape:
        raise ValueError("jacobi: f and unew0 must be matrices of one shape")
    nx, ny = f.shape
    dx = 1.0 / (nx - 1) if dx is None else dx
    dy = 1.0 / (ny - 1) if dy is None else dy
    out = np.empty_like(unew0)
    r = JacobiResult()
    _check(lib().hclib_hip_jacobi(f.ctypes.data, unew0.ctypes.data, nx, ny, dx, dy, block, niter, fuse, out.ctypes.data,
                                  C.byref(r)), "hclib_hip_jacobi")
    return out, {k: getattr(r, k) for k, _ in JacobiResult._fields_}


def jacobi_rhs(nx: int, ny: int):
    """(f, unew0) of the reference's rhs() and run() for an (nx, ny) grid, through
    this host's libm (hclib_hip_jacobi_rhs, host only)."""
    import numpy as np

    if nx < 3 or ny < 3:
        _check(lib().hclib_hip_jacobi_rhs(nx, ny, None, None), "hclib_hip_jacobi_rhs")
    f, u = np.empty((nx, ny), dtype=np.float64), np.empty((nx, ny), dtype=np.float64)
    _check(lib().hclib_hip_jacobi_rhs(nx, ny, f.ctypes.data, u.ctypes.data), "hclib_hip_jacobi_rhs")
    return f, u


def jacobi_bounds(nx: int, ny: int, block: int = 0, niter: int = 4, fuse: int = 0) -> dict:
    """What a jacobi() launch creates (hclib_hip_jacobi_bounds), exact and on the
    host alone: tasks, awaits, supersteps and the bytes the tasks move. Raises as
    the launch would for arguments it rejects."""
    out = (C.c_uint64 * 4)()
    _check(lib().hclib_hip_jacobi_bounds(nx, ny, block, niter, fuse, out), "hclib_hip_jacobi_bounds")
    return dict(zip(("tasks", "awaits", "supersteps", "bytes_moved"), out))


# -------------------------------------------------------------- Rodinia BFS
BFS_FORMS = {"level": 0, "async": 1}  # HCLIB_HIP_BFS_LEVEL / _ASYNC


def _bfs_form(form) -> int:
    if form not in BFS_FORMS:
        raise ValueError(f"bfs: form {form!r} is not one of {sorted(BFS_FORMS)}")
    return BFS_FORMS[form]


def bfs_read_input(path) -> dict:
    """A Rodinia BFS graph file (bfs.ref.cpp:84-121) through
    hclib_hip_bfs_read_input, on the host alone: {"starting", "degree", "edges"
    (int32 arrays), "source"}, as bfs() takes it. Nothing is checked here: the
    launch and bfs_bounds refuse a graph that does not hold together."""
    import numpy as np

    counts = (C.c_int64 * 3)()
    _check(lib().hclib_hip_bfs_read_input(os.fsencode(path), None, None, None, counts), "hclib_hip_bfs_read_input")
    g = {"starting": np.empty(counts[0], dtype=np.int32), "degree": np.empty(counts[0], dtype=np.int32),
         "edges": np.empty(counts[1], dtype=np.int32)}
    _check(lib().hclib_hip_bfs_read_input(os.fsencode(path), g["starting"].ctypes.data, g["degree"].ctypes.data,
                                          g["edges"].ctypes.data, counts), "hclib_hip_bfs_read_input")
    g["source"] = int(counts[2])
    return g


def _bfs_graph(graph_or_path):
    import numpy as np

    g = bfs_read_input(graph_or_path) if isinstance(graph_or_path, (str, bytes, os.PathLike)) else graph_or_path
    a = [np.ascontiguousarray(g[k], dtype=np.int32).ravel() for k in ("starting", "degree", "edges")]
    if a[0].size != a[1].size:
        raise ValueError("bfs: starting and degree must have one entry per vertex each")
    return a[0], a[1], a[2], int(g["source"])


def bfs(graph_or_path, form: str = "level", frontier: bool = False, order: bool = False) -> dict:
    """Rodinia BFS on the work-stealing scheduler (hclib_hip_bfs): the hop count
    of every vertex from the source, -1 where there is no path. graph_or_path: a
    graph as bfs_read_input returns it, or a file of Rodinia's format. form
    "level" follows the reference's level-by-level schedule over the frontier
    alone, the wave that finishes a level last opening the next; "async" has no
    levels and lowers costs with atomic minima until none changes. Returns the
    fields of hclib_hip_bfs_result_t, "cost" (int32 array) and, on request,
    "frontier" (vertices per level, `levels` entries) and "order" (level form:
    the vertices in claiming order, level after level, -1 behind the reached)."""
    import numpy as np

    st, dg, ed, src = _bfs_graph(graph_or_path)
    f = _bfs_form(form)
    n = st.size
    cost = np.empty(n, dtype=np.int32)
    fr = np.zeros(n, dtype=np.uint64) if frontier else None
    od = np.empty(n, dtype=np.int32) if order else None
    r = BfsResult()
    _check(lib().hclib_hip_bfs(st.ctypes.data, dg.ctypes.data, n, ed.ctypes.data if ed.size else None, ed.size, src, f,
                               cost.ctypes.data, C.byref(r), fr.ctypes.data if frontier else None,
                               od.ctypes.data if order else None), "hclib_hip_bfs")
    out = {k: getattr(r, k) for k, _ in BfsResult._fields_}
    out["cost"] = cost
    if frontier:
        out["frontier"] = [int(v) for v in fr[:r.levels]]
    if order:
        out["order"] = od
    return out


def bfs_bounds(graph_or_path, form: str = "level") -> dict:
    """What a bfs() launch takes (hclib_hip_bfs_bounds), on the host alone: the
    bytes of device memory and the bound n_nodes + n_edges on the level form's
    items. Raises as the launch would for a graph it refuses."""
    st, dg, ed, src = _bfs_graph(graph_or_path)
    out = (C.c_uint64 * 2)()
    _check(lib().hclib_hip_bfs_bounds(st.ctypes.data, dg.ctypes.data, st.size, ed.ctypes.data if ed.size else None,
                                      ed.size, src, _bfs_form(form), out), "hclib_hip_bfs_bounds")
    return {"arena_bytes": out[0], "items": out[1]}


# -------------------------------------------------------------- Rodinia CFD
CFD_FORMS = {"dag": 0, "phases": 1}  # HCLIB_HIP_CFD_DAG / _PHASES


def cfd_read_input(path) -> dict:
    """A Rodinia CFD mesh file through hclib_hip_cfd_read_input (the reference's
    reader, euler3d_cpu_double.ref.cpp:417-455), on the host alone: {"nel",
    "nelr", "areas" [nelr], "neighbours" [nelr, 4] (int32: an element, -1 wing,
    -2 far field), "normals" [nelr, 4, 3] (negated)}, the rows from nel on
    copies of row nel - 1, as cfd() takes it."""
    import numpy as np

    counts = (C.c_int64 * 2)()
    _check(lib().hclib_hip_cfd_read_input(os.fsencode(path), None, None, None, counts), "hclib_hip_cfd_read_input")
    nelr = int(counts[1])
    m = {"nel": int(counts[0]), "nelr": nelr, "areas": np.empty(nelr, dtype=np.float64),
         "neighbours": np.empty((nelr, 4), dtype=np.int32), "normals": np.empty((nelr, 4, 3), dtype=np.float64)}
    _check(lib().hclib_hip_cfd_read_input(os.fsencode(path), m["areas"].ctypes.data, m["neighbours"].ctypes.data,
                                          m["normals"].ctypes.data, counts), "hclib_hip_cfd_read_input")
    return m


def _cfd_mesh(path_or_arrays):
    import numpy as np

    m = cfd_read_input(path_or_arrays) if isinstance(path_or_arrays, (str, bytes, os.PathLike)) else path_or_arrays
    nel = int(m["nel"])
    nelr = 8 * ((nel + 7) // 8) if nel >= 1 else 0
    ar = np.ascontiguousarray(m["areas"], dtype=np.float64).ravel()
    nb = np.ascontiguousarray(m["neighbours"], dtype=np.int32).ravel()
    nr = np.ascontiguousarray(m["normals"], dtype=np.float64).ravel()
    if nel >= 1 and (ar.size != nelr or nb.size != nelr * 4 or nr.size != nelr * 12):
        raise ValueError(f"cfd: areas, neighbours and normals must hold nelr = {nelr} rows (1, 4 and 4 x 3 entries each)")
    return nel, nelr, ar, nb, nr


def cfd(path_or_arrays, iterations: int = 5, block: int = 0, form: str = "dag", variables0=None):
    """Rodinia CFD on the device promise DAG (hclib_hip_cfd): `iterations`
    iterations of the three-stage Euler solver over the mesh path_or_arrays (a
    file of Rodinia's format, or what cfd_read_input returns); returns
    (variables [nelr, 5] float64, the reference's bits, stats). variables0: the
    initial state, default the far field everywhere. block: elements per task
    (a multiple of 8 in [8, 1024], 0 = the default); form "dag" is one launch
    whose tasks await only the blocks the mesh connects them to, "phases" one
    kernel per stage, the reference's schedule; results depend on neither."""
    import numpy as np

    if form not in CFD_FORMS:
        raise ValueError(f"cfd: form {form!r} is not one of {sorted(CFD_FORMS)}")
    nel, nelr, ar, nb, nr = _cfd_mesh(path_or_arrays)
    v0 = None
    if variables0 is not None:
        v0 = np.ascontiguousarray(variables0, dtype=np.float64).ravel()
        if v0.size != nelr * 5:
            raise ValueError(f"cfd: variables0 must hold nelr x 5 = {nelr * 5} values")
    out = np.empty((nelr, 5), dtype=np.float64)
    r = CfdResult()
    _check(lib().hclib_hip_cfd(nel, ar.ctypes.data, nb.ctypes.data, nr.ctypes.data, None if v0 is None else v0.ctypes.data,
                               iterations, block, CFD_FORMS[form], out.ctypes.data, C.byref(r)), "hclib_hip_cfd")
    return out, {k: getattr(r, k) for k, _ in CfdResult._fields_}


def cfd_bounds(path_or_arrays, iterations: int = 5, block: int = 0) -> dict:
    """What a cfd() launch creates (hclib_hip_cfd_bounds), exact and on the host
    alone: tasks, awaits, stages, the longest waiter list, the bytes of device
    memory and the bytes the tasks move. Raises as the launch would."""
    nel, nelr, ar, nb, nr = _cfd_mesh(path_or_arrays)
    out = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_cfd_bounds(nel, nb.ctypes.data, iterations, block, out), "hclib_hip_cfd_bounds")
    return dict(zip(("tasks", "awaits", "stages", "max_waiters", "arena_bytes", "bytes_moved"), out))


# ------------------------------------------------------------- Rodinia SRAD
SRAD_FORMS = {"dag": 0, "phases": 1}  # HCLIB_HIP_SRAD_DAG / _PHASES


def srad(j0, roi, lam: float = 0.5, niter: int = 2, block: int = 0, form: str = "dag"):
    """Rodinia SRAD on the device promise DAG (hclib_hip_srad): `niter`
    iterations of speckle-reducing anisotropic diffusion over the float32 image
    `j0` (what srad_image returns, or any positive image whose sides are
    multiples of 16). roi = (r1, r2, c1, c2), rows and columns of the region of
    interest, both ends included. Returns (J, stats); stats["q0sqr"] holds each
    iteration's scalar of the serial section, read back from the reduce
    promises' datums. form "dag" is one launch, "phases" a reduce kernel and a
    sweep kernel per iteration; both, and every block (16, 32, 64; 0 = the
    largest that divides both sides), give the bits of the reference built
    without fused multiply-add."""
    if form not in SRAD_FORMS:
        raise ValueError(f"srad: form {form!r} is not one of {sorted(SRAD_FORMS)}")
    import numpy as np

    j0 = np.ascontiguousarray(j0, dtype=np.float32)
    if j0.ndim != 2:
        raise ValueError("srad: j0 must be a matrix")
    r1, r2, c1, c2 = (int(x) for x in roi)
    rows, cols = j0.shape
    out = np.empty_like(j0)
    q = np.zeros(max(int(niter), 0), dtype=np.float32)
    r = SradResult()
    _check(lib().hclib_hip_srad(j0.ctypes.data, rows, cols, r1, r2, c1, c2, float(np.float32(lam)), niter, block,
                                SRAD_FORMS[form], out.ctypes.data, q.ctypes.data, C.byref(r)), "hclib_hip_srad")
    st = {k: getattr(r, k) for k, _ in SradResult._fields_}
    st["q0sqr"] = q
    return out, st


def srad_image(rows: int, cols: int):
    """The reference's input image: random_matrix (srand(7), rand() / RAND_MAX)
    followed by expf (hclib_hip_srad_image, host only). It changes the
    process's rand() state, as the reference does."""
    import numpy as np

    if rows < 1 or cols < 1:
        _check(lib().hclib_hip_srad_image(rows, cols, None), "hclib_hip_srad_image")
    j0 = np.empty((rows, cols), dtype=np.float32)
    _check(lib().hclib_hip_srad_image(rows, cols, j0.ctypes.data), "hclib_hip_srad_image")
    return j0


def srad_bounds(rows: int, cols: int, roi, niter: int = 2, block: int = 0) -> dict:
    """What a srad() launch creates (hclib_hip_srad_bounds), exact and on the
    host alone: tasks, awaits, the block as resolved, the longest waiter list,
    the bytes of device memory and the bytes the tasks move. Raises as the
    launch would."""
    r1, r2, c1, c2 = (int(x) for x in roi)
    out = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_srad_bounds(rows, cols, r1, r2, c1, c2, niter, block, out), "hclib_hip_srad_bounds")
    return dict(zip(("tasks", "awaits", "block", "max_waiters", "arena_bytes", "bytes_moved"), out))


# --------------------------------------------------------------- BOTS Health
HEALTH_PARAMS = tuple(k for k, _ in HealthParams._fields_)
HEALTH_TOTALS = ("population", "hospitals", "personnel", "hosps_visited", "in_village", "waiting", "assess", "inside",
                 "total_time")
HEALTH_LISTS = ("population", "waiting", "assess", "inside")


def _health_params(params) -> HealthParams:
    if isinstance(params, HealthParams):
        return params
    if not isinstance(params, dict):
        params = dict(zip(HEALTH_PARAMS, params))
    if sorted(params) != sorted(HEALTH_PARAMS):
        raise ValueError(f"health: params must give exactly {HEALTH_PARAMS}")
    p = HealthParams()
    for k in HEALTH_PARAMS[:6]:
        setattr(p, k, int(params[k]))
    s = int(params["seed"]) & 0xffffffff  # the low 32 bits of what the reference reads with %ld
    p.seed = s - (1 << 32) if s & 0x80000000 else s
    for k in HEALTH_PARAMS[7:]:
        setattr(p, k, float(params[k]))
    return p


def health_read_input(path):
    """A BOTS health input file (read_input_data, health.ref.c:487-535): 19
    numbers, the ten settings and the nine expected results. Returns (params,
    expected): params a dict for health(), expected the eight totals that
    check_village compares, by health()'s names, and "avg_stay"."""
    f = open(path).read().split()
    if len(f) != 19:
        raise ValueError(f"{path}: {len(f)} numbers, a health input file has 19")
    params = dict(zip(HEALTH_PARAMS, [int(x) for x in f[:7]] + [float(x) for x in f[7:10]]))
    expected = dict(zip(HEALTH_TOTALS[:8], (int(x) for x in f[10:18])))
    expected["avg_stay"] = float(f[18])
    return params, expected


def health_bounds(params) -> dict:
    """What a health() of these settings allocates (hclib_hip_health_bounds),
    exact and on the host alone."""
    out = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_health_bounds(C.byref(_health_params(params)), out), "hclib_hip_health_bounds")
    return dict(zip(("villages", "patients", "tasks", "scopes", "wait_nodes", "arena_bytes"), out))


def health(params, state: bool = False, expected=None) -> dict:
    """BOTS Health on dynamic device dataflow (hclib_hip_health): sim_time
    rounds over the village tree in one launch. params is a dict of
    HEALTH_PARAMS (or the ten values in that order). Returns the fields of
    hclib_hip_health_result_t; with state, "state": the reference's full final
    state as numpy arrays (seed, time, time_left, hosps_visited per patient id;
    village, one row of id, level, free_personnel and the four list lengths per
    village in allocation order; lists, the lists' ids village by village); with
    expected (health_read_input's), "verified": the reference's check_village
    comparison of the eight totals."""
    import numpy as np

    p = _health_params(params)
    st, arrays = None, None
    if state:
        b = health_bounds(p)
        arrays = {k: np.zeros(b["patients"], dtype=np.int32) for k in ("seed", "time", "time_left", "hosps_visited",
                                                                         "lists")}
        arrays["village"] = np.zeros((b["villages"], 7), dtype=np.int32)
        st = HealthState(**{k: a.ctypes.data for k, a in arrays.items()})
    r = HealthResult()
    _check(lib().hclib_hip_health(C.byref(p), C.byref(r), C.byref(st) if st is not None else None), "hclib_hip_health")
    out = {k: getattr(r, k) for k, _ in HealthResult._fields_}
    if state:
        out["state"] = arrays
    if expected is not None:
        out["verified"] = all(out[k] == expected[k] for k in HEALTH_TOTALS[:8])
    return out


def health_last_ticks() -> dict:
    """Wave time of the last health() by task class, in ticks of the 100 MHz
    device clock (hclib_hip_health_last_ticks)."""
    out = (C.c_uint64 * 3)()
    lib().hclib_hip_health_last_ticks(out)
    return dict(zip(("leaf_call", "inner_call", "post"), out))


# ------------------------------------------------------------ BOTS floorplan
FLOORPLAN_NOPRUNE = 1  # HCLIB_HIP_FLOORPLAN_NOPRUNE


def _floorplan_input(cells) -> FloorplanInput:
    """cells: one (shapes, left, above, next) per cell 1..n, shapes a list of
    (rows, cols). What does not fit the struct is left for the library to
    refuse (a count it can see is kept, the surplus is dropped)."""
    if isinstance(cells, FloorplanInput):
        return cells
    inp = FloorplanInput()
    inp.n, inp.solution = len(cells), -1
    for c, (shapes, left, above, nxt) in enumerate(cells[:FLOORPLAN_MAX_CELLS], 1):
        inp.shapes[c] = len(shapes)
        for i, (rows, cols) in enumerate(shapes[:FLOORPLAN_MAX_SHAPES]):
            inp.shape[c][i][0], inp.shape[c][i][1] = rows, cols
        inp.left[c], inp.above[c], inp.next[c] = left, above, nxt
    return inp


def floorplan_read_input(path):
    """A BOTS floorplan input file (read_inputs, floorplan.c:159-195) through
    hclib_hip_floorplan_read_input, on the host alone. Returns (cells,
    solution): cells as floorplan() takes them, solution the file's trailing
    expected minimum area or -1."""
    inp = FloorplanInput()
    _check(lib().hclib_hip_floorplan_read_input(os.fsencode(path), C.byref(inp)), "hclib_hip_floorplan_read_input")
    cells = [([(inp.shape[c][i][0], inp.shape[c][i][1]) for i in range(inp.shapes[c])], inp.left[c], inp.above[c],
              inp.next[c]) for c in range(1, inp.n + 1)]
    return cells, inp.solution


def floorplan(cells_or_path, prune: bool = True, hist: bool = False) -> dict:
    """BOTS floorplan on the work-stealing scheduler (hclib_hip_floorplan): the
    branch-and-bound search for the smallest bounding box of the cells, one
    task per (shape, corner) candidate, pruned against a bound the tasks lower
    while they run. cells_or_path: a cell table (see floorplan_read_input) or
    an input file. prune=False compares against the constant 4096: exhaustive,
    every count deterministic. Returns the fields of
    hclib_hip_floorplan_result_t with "footprint" a list, "placements" one
    [shape, top, lhs] per cell (None without a complete placement), "board"
    the 4096 bytes of the best board and, with hist, "hist": the candidates
    laid down per depth 0..n."""
    cells = floorplan_read_input(cells_or_path)[0] if isinstance(cells_or_path, (str, bytes, os.PathLike)) \
        else cells_or_path
    inp = _floorplan_input(cells)
    r = FloorplanResult()
    board = (C.c_uint8 * 4096)()
    h = (C.c_uint64 * (FLOORPLAN_MAX_CELLS + 1))() if hist else None
    _check(lib().hclib_hip_floorplan(C.byref(inp), 0 if prune else FLOORPLAN_NOPRUNE, C.byref(r), board, h),
           "hclib_hip_floorplan")
    out = {k: getattr(r, k) for k, _ in FloorplanResult._fields_ if k not in ("footprint", "placements")}
    out["footprint"] = list(r.footprint)
    out["placements"] = [[p.shape, p.top, p.lhs] for p in r.placements[:inp.n]] if r.min_area < 4096 else None
    out["board"] = bytes(board)
    if hist:
        out["hist"] = list(h)[:inp.n + 1]
    return out


# ------------------------------------------------------------ BOTS alignment
ALIGNMENT_CODES = "ABCDEFGHIKLMNPQRSTUVWXYZ-"  # a residue's code is its index; '-' is stored as 31
ALIGNMENT_MAX_LEN = 4999
ALIGNMENT_DEFAULT_CUTOFF = 16384
ALIGNMENT_BOUNDS = ("pairs", "tasks", "spawns", "diff_calls", "arena_bytes", "row_bytes")
ALIGNMENT_TICKS = ("root", "pair", "spawn", "leaf")


def alignment_read_input(path):
    """A BOTS alignment input (a Pearson file with the `Number of sequences is
    <n>` line) through hclib_hip_alignment_read_input, on the host alone:
    [(name, codes)], codes a list of residue codes as the reference's readseqs
    leaves them."""
    inp = AlignmentInput()
    _check(lib().hclib_hip_alignment_read_input(os.fsencode(path), C.byref(inp)), "hclib_hip_alignment_read_input")
    try:
        names = C.string_at(inp.names, inp.nseqs * 31)
        return [(names[31 * i:31 * i + 31].split(b"\0")[0].decode("latin-1"),
                 [inp.codes[inp.offset[i] + k] for k in range(inp.length[i])]) for i in range(inp.nseqs)]
    finally:
        lib().hclib_hip_alignment_free_input(C.byref(inp))


def alignment_read_matrix(path):
    """A substitution-matrix file through
    hclib_hip_alignment_read_matrix: (avscore, 32 rows of 32 scores)."""
    m = AlignmentMatrix()
    _check(lib().hclib_hip_alignment_read_matrix(os.fsencode(path), C.byref(m)), "hclib_hip_alignment_read_matrix")
    return m.avscore, [list(row) for row in m.score]


def _alignment_input(seqs):
    """(AlignmentInput, the arrays it points into) of [(name, codes)], [codes] or an input file."""
    if isinstance(seqs, (str, bytes, os.PathLike)):
        seqs = alignment_read_input(seqs)
    codes = [list(q[1]) if isinstance(q, tuple) else list(q) for q in seqs]
    if any(not 0 <= c <= 255 for q in codes for c in q):
        raise ValueError("alignment: residue codes are 0..31")
    n, total = len(codes), sum(len(q) for q in codes)
    length = (C.c_int32 * max(n, 1))(*[len(q) for q in codes])
    offset = (C.c_int32 * max(n, 1))()
    flat = (C.c_uint8 * max(total, 1))()
    at = 0
    for i, q in enumerate(codes):
        offset[i] = at
        flat[at:at + len(q)] = q
        at += len(q)
    inp = AlignmentInput(nseqs=n, total=total, length=length, offset=offset, codes=flat, names=None)
    return inp, (length, offset, flat)


def _alignment_matrix(matrix) -> AlignmentMatrix:
    if isinstance(matrix, AlignmentMatrix):
        return matrix
    if isinstance(matrix, (str, bytes, os.PathLike)):
        matrix = alignment_read_matrix(matrix)
    avscore, rows = matrix
    if len(rows) != 32 or any(len(r) != 32 for r in rows):
        raise ValueError("alignment: the matrix has 32 x 32 scores")
    m = AlignmentMatrix(avscore=avscore)
    for i, row in enumerate(rows):
        for j, v in enumerate(row):
            m.score[i][j] = v
    return m


def alignment_bounds(seqs, cutoff: int = 0) -> dict:
    """What an alignment() of these sequences uses at most
    (hclib_hip_alignment_bounds), on the host alone: ALIGNMENT_BOUNDS."""
    inp, keep = _alignment_input(seqs)
    out = (C.c_uint64 * 6)()
    _check(lib().hclib_hip_alignment_bounds(C.byref(inp), cutoff, out), "hclib_hip_alignment_bounds")
    return dict(zip(ALIGNMENT_BOUNDS, out))


def alignment(seqs, matrix, cutoff: int = 0, pairs: bool = False) -> dict:
    """BOTS alignment on dynamic device dataflow (hclib_hip_alignment): every
    pair of the sequences aligned by Myers-Miller with affine gaps in one
    launch, a task per pair and two per diff of more than `cutoff` cells (0:
    the default). seqs: an input file, [(name, codes)] or [codes]; matrix: a
    matrix file or (avscore, rows). Returns the fields of
    hclib_hip_alignment_result_t with "scores" the nseqs x nseqs matrix the
    reference prints (a list of rows) and, with pairs, a dict per pair
    by the names of hclib_hip_alignment_pair_t
    ("pair_records")."""
    inp, keep = _alignment_input(seqs)
    m = _alignment_matrix(matrix)
    ns = inp.nseqs
    scores = (C.c_int32 * max(ns * ns, 1))()
    r = AlignmentResult(scores=C.addressof(scores))
    npairs = alignment_bounds([list(keep[2][keep[1][i]:keep[1][i] + keep[0][i]]) for i in range(ns)], cutoff)["pairs"] \
        if pairs else 0
    recs = (AlignmentPair * max(npairs, 1))() if pairs else None
    _check(lib().hclib_hip_alignment(C.byref(inp), C.byref(m), cutoff, C.byref(r), recs), "hclib_hip_alignment")
    out = {k: getattr(r, k) for k, _ in AlignmentResult._fields_ if k != "scores"}
    out["scores"] = [list(scores[i * ns:(i + 1) * ns]) for i in range(ns)]
    if pairs:
        out["pair_records"] = [{k: getattr(q, k) for k, _ in AlignmentPair._fields_} for q in recs[:npairs]]
    return out


def alignment_last_ticks() -> dict:
    """Wave time of the last alignment() by task class, in ticks of the 100 MHz
    device clock (hclib_hip_alignment_last_ticks): ALIGNMENT_TICKS."""
    out = (C.c_uint64 * 4)()
    lib().hclib_hip_alignment_last_ticks(out)
    return dict(zip(ALIGNMENT_TICKS, out))


ATOMIC_SCATTER_RET64 = 0  # include/hclib_hip.h
ATOMIC_HOT_WORD = 1
ATOMIC_COALESCED32 = 2


def atomic_calibrate(mode: int, iters: int = 256):
    """Saturated L2 atomic rate of one access shape: (Mops/s, kernel ms)."""
    r, ms = C.c_double(), C.c_double()
    _check(lib().hclib_hip_atomic_calibrate(mode, iters, C.byref(r), C.byref(ms)),
           "hclib_hip_atomic_calibrate")
    return r.value, ms.value


def sha1_calibrate(chains: int = 1, waves_per_cu: int = 8, iters: int = 2000):
    """The chip's UTS SHA-1 issue ceiling (SHA-1/s, kernel ms): the
    rng_spawn stream of k_uts_search back to back on every lane."""
    r, ms = C.c_double(), C.c_double()
    _check(lib().hclib_hip_sha1_calibrate(chains, waves_per_cu, iters, C.byref(r), C.byref(ms)),
           "hclib_hip_sha1_calibrate")
    return r.value, ms.value


def last_phase_counters():
    """HX_PHASES builds: main-loop batch phase cycles of the last launch
    (hclib_hip_last_phase_counters)."""
    out = (C.c_uint64 * 8)()
    lib().hclib_hip_last_phase_counters(out)
    return list(out)


def last_sched_counters():
    """Counters of the last megakernel launch (see include/hclib_hip.h)."""
    out = (C.c_uint64 * 16)()
    lib().hclib_hip_last_sched_counters(out)
    return list(out)


def last_narrow_counters():
    """Narrow-frontier loop of the last launch: batches, cycles, entries."""
    out = (C.c_uint64 * 4)()
    lib().hclib_hip_last_narrow_counters(out)
    return list(out)


def last_shed_counters():
    """The narrow loop's overflow exits of the last launch
    (hclib_hip_last_shed_counters): exits, placed, blocks, items, fallbacks."""
    out = (C.c_uint64 * 8)()
    lib().hclib_hip_last_shed_counters(out)
    return dict(zip(("exits", "placed", "blocks", "items", "fallbacks"), out))


def last_comm_counters():
    """The hand-off waves' counts of the last launch (hclib_hip_last_comm_counters):
    the outbox blocks and items of the main loop's give-away and of the narrow
    loop's overflow exit, the blocks passed on to a deque and to a sibling,
    the claims that found no outbox free, the overflow exits that reached the ring."""
    out = (C.c_uint64 * 8)()
    lib().hclib_hip_last_comm_counters(out)
    return dict(zip(("main_blocks", "main_items", "shed_blocks", "shed_items", "to_deque", "to_sibling", "busy",
                     "ring_exits"), out))


TIMELINE_EVENTS = {1: "start", 2: "busy", 3: "idle", 4: "spill", 5: "term", 6: "end"}


def last_timeline():
    """Worker timelines of the last megakernel launch (a `--variant timeline`
    library run with HCLIB_HIP_TIMELINE=<events per worker>, hx_sched.h
    Timeline): per worker a list of (time in 10 ns ticks, event, value)."""
    per = C.c_uint32()
    nw = lib().hclib_hip_last_timeline(None, 0, C.byref(per))
    if nw <= 0 or per.value == 0:
        return []
    import numpy as np
    buf = np.zeros(nw * per.value, dtype=np.uint64)
    lib().hclib_hip_last_timeline(buf.ctypes.data, buf.size, C.byref(per))
    buf = buf.reshape(nw, per.value)
    out = []
    for w in range(nw):
        row = buf[w][buf[w] != 0]
        out.append([(int(v >> 24), int((v >> 20) & 0xF), int(v & 0xFFFFF)) for v in row])
    return out
