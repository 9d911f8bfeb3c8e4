"""ctypes binding of include/sls_mi355x.h (libsls_mi355x.so).

This is the same marshalling the Julia `ccall` wrapper performs:
SciPy's CSC triplet (indptr, indices, data) is Julia's (colptr, rowval, nzval) with
index_base = 0 instead of 1.

The library is the ONLY compute backend of this package.  If it cannot be loaded the
import fails loudly; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsls_mi355x.so")

# ---- constants (mirror the header) ----
SLS_ABI_VERSION = 2
SLS_EINVAL, SLS_ENOTSF, SLS_EUNSUPPORTED, SLS_EHIP, SLS_ENOMEM, SLS_ENODEVICE = -1, -2, -3, -4, -5, -6
SLS_SOLVE_DEFAULT, SLS_SOLVE_SUM_OF_NORMS = 0, 1
SLS_PLAN_WEIGHTS_UPDATABLE = 2
SLS_PLAN_MULTIPLIERS = 4
SLS_COL_OK, SLS_COL_INFEASIBLE, SLS_COL_NOTCONV, SLS_COL_TRIVIAL, SLS_COL_SKIPPED, SLS_COL_UNSUPPORTED = 0, 1, 2, 3, 4, 5

ERROR_NAMES = {SLS_EINVAL: "SLS_EINVAL", SLS_ENOTSF: "SLS_ENOTSF", SLS_EUNSUPPORTED: "SLS_EUNSUPPORTED",
               SLS_EHIP: "SLS_EHIP", SLS_ENOMEM: "SLS_ENOMEM", SLS_ENODEVICE: "SLS_ENODEVICE"}


class SLSError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


class sls_csc_f64(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("colptr", C.POINTER(C.c_int64)),
                ("rowval", C.POINTER(C.c_int64)), ("nzval", C.POINTER(C.c_double))]


class sls_csc_bool(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("colptr", C.POINTER(C.c_int64)),
                ("rowval", C.POINTER(C.c_int64)), ("nzval", C.POINTER(C.c_uint8))]


class sls_dims(C.Structure):
    _fields_ = [("Nx", C.c_int64), ("Nu", C.c_int64), ("Nz", C.c_int64), ("Nw", C.c_int64), ("T", C.c_int64),
                ("index_base", C.c_int32), ("flags", C.c_uint32)]


class sls_plant(C.Structure):
    _fields_ = [(k, C.POINTER(sls_csc_f64)) for k in ("A", "B1", "B2", "C1", "D11", "D12")]


class sls_stats(C.Structure):
    _fields_ = [("n_subproblems", C.c_int64), ("n_not_ok", C.c_int64), ("n_values_x", C.c_int64),
                ("n_values_u", C.c_int64), ("n_free", C.c_int64), ("max_nx", C.c_int32), ("max_nu", C.c_int32),
                ("max_iters", C.c_int32), ("n_devices", C.c_int32), ("max_residual", C.c_double),
                ("flops_alg", C.c_double), ("bytes_alg", C.c_double), ("t_symbolic_s", C.c_double),
                ("t_upload_s", C.c_double), ("t_solve_s", C.c_double), ("t_download_s", C.c_double), ("n_refined", C.c_int64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class sls_plan_info(C.Structure):
    _fields_ = [("n_subproblems", C.c_int64), ("n_values", C.c_int64), ("n_values_x", C.c_int64),
                ("n_values_u", C.c_int64), ("n_packed", C.c_int64), ("workspace_bytes", C.c_int64),
                ("max_nx", C.c_int32), ("max_nu", C.c_int32), ("T", C.c_int32), ("device", C.c_int32),
                ("flops_alg", C.c_double), ("bytes_alg", C.c_double), ("t_symbolic_s", C.c_double),
                ("t_upload_s", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


EXPORTS = [
    "sls_create", "sls_destroy", "sls_last_error", "sls_abi_version", "sls_device_count",
    "sls_h2_sf_solve", "sls_h2_sf_solve_batch", "sls_set_ridge", "sls_h2_sf_plan", "sls_plan_get_info", "sls_plan_value_offsets",
    "sls_plan_execute", "sls_plan_execute_batch", "sls_plan_refine", "sls_plan_synchronize", "sls_plan_packed_dest", "sls_plan_fetch_status",
    "sls_plan_kernel_time_ms", "sls_plan_alloc_values", "sls_plan_free_values", "sls_plan_download",
    "sls_plan_destroy", "sls_scatter_f64", "sls_shard_groups", "sls_sparsity_dim_reduction",
    "sls_h2_sf_packed_layout", "sls_plan_describe", "sls_localization_masks", "sls_localization_masks_device",
    "sls_index_sets_device", "sls_h2_sf_plan_localized", "sls_h2_sf_solve_localized",
    "sls_closed_loop_plan", "sls_closed_loop_run", "sls_closed_loop_run_host", "sls_closed_loop_last_ms",
    "sls_closed_loop_entries", "sls_closed_loop_destroy",
    "sls_plan_objective", "sls_plan_fetch_objective", "sls_ctx_want_objective", "sls_ctx_last_objective",
    "sls_plan_update_plant", "sls_plan_update_result", "sls_plan_fetch_plant",
    "sls_plan_update_weights", "sls_plan_update_weights_result", "sls_plan_fetch_weights",
    "sls_plan_execute_columns", "sls_plan_track_changes", "sls_plan_execute_dirty", "sls_plan_fetch_dirty", "sls_plan_clear_dirty",
    "sls_plan_residual", "sls_plan_fetch_residual",
    "sls_plan_gradient", "sls_plan_fetch_gradient", "sls_plan_fetch_multipliers",
    "sls_controller_plan", "sls_controller_load", "sls_controller_reset", "sls_controller_step", "sls_controller_info",
    "sls_controller_destroy",
    "sls_rollout_plan", "sls_rollout_load", "sls_rollout_set_plant", "sls_rollout_set_weights", "sls_rollout_reset", "sls_rollout_run",
    "sls_rollout_stats", "sls_rollout_fetch", "sls_rollout_info", "sls_rollout_destroy",
    "sls_margin_plan", "sls_margin_load", "sls_margin_set_plant", "sls_margin_run", "sls_margin_fetch", "sls_margin_info",
    "sls_margin_destroy",
    "sls_margin_fetch_plant", "sls_margin_set_radius", "sls_margin_box_run", "sls_margin_box_fetch", "sls_margin_box_worst_plant", "sls_margin_box_info",
    "sls_norms_plan", "sls_norms_load", "sls_norms_l1", "sls_norms_hinf", "sls_norms_fetch_l1", "sls_norms_fetch_hinf", "sls_norms_info",
    "sls_norms_destroy", "sls_norms_h2", "sls_norms_fetch_h2", "sls_norms_cov_pattern", "sls_norms_cov", "sls_norms_fetch_cov",
]

_lib = None


def load_library(path: str | None = None):
    """dlopen libsls_mi355x.so and declare every prototype.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C systemlevelcontrol.jl_amd/csrc).  There is no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64 under the system runtime's SONAME; whichever copy the process loads
    # first serves both, and torch only finds its GPUs through its own.  A process that also uses torch tensors/streams
    # (tests, bench.py, dist.py) must therefore load torch's copy before this library pulls in /opt/rocm's.
    if "torch" not in sys.modules and not os.environ.get("SLS_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(p)
    vp, i64p, i32p, dp = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    dpp = C.POINTER(C.POINTER(C.c_double))
    lib.sls_create.restype = vp; lib.sls_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_uint32]
    lib.sls_destroy.restype = None; lib.sls_destroy.argtypes = [vp]
    lib.sls_last_error.restype = C.c_char_p; lib.sls_last_error.argtypes = [vp]
    lib.sls_abi_version.restype = C.c_int; lib.sls_abi_version.argtypes = []
    lib.sls_device_count.restype = C.c_int; lib.sls_device_count.argtypes = []
    common = [C.POINTER(sls_dims), C.POINTER(sls_plant), C.POINTER(sls_csc_bool), C.POINTER(sls_csc_bool),
              C.c_int64, i64p, i64p]
    lib.sls_h2_sf_solve.restype = C.c_int
    lib.sls_h2_sf_solve.argtypes = [vp] + common + [dpp, dpp, i32p, C.POINTER(sls_stats)]
    lib.sls_set_ridge.restype = C.c_int; lib.sls_set_ridge.argtypes = [vp, C.c_int64, dp, C.c_int64, dp]
    lib.sls_h2_sf_solve_batch.restype = C.c_int
    lib.sls_h2_sf_solve_batch.argtypes = [vp, C.c_int, C.POINTER(sls_dims), C.POINTER(sls_plant), C.POINTER(C.POINTER(sls_csc_bool)),
                                          C.POINTER(C.POINTER(sls_csc_bool)), C.POINTER(dpp), C.POINTER(dpp), C.POINTER(i32p),
                                          C.POINTER(sls_stats)]
    lib.sls_h2_sf_plan.restype = C.c_int
    lib.sls_h2_sf_plan.argtypes = [vp, C.c_int] + common + [C.c_int64, C.c_int64, C.POINTER(vp)]
    lib.sls_plan_get_info.restype = C.c_int; lib.sls_plan_get_info.argtypes = [vp, C.POINTER(sls_plan_info)]
    lib.sls_plan_value_offsets.restype = C.c_int; lib.sls_plan_value_offsets.argtypes = [vp, i64p, i64p]
    lib.sls_plan_execute.restype = C.c_int; lib.sls_plan_execute.argtypes = [vp, vp, vp, C.c_int]
    lib.sls_plan_synchronize.restype = C.c_int; lib.sls_plan_synchronize.argtypes = [vp, vp]
    lib.sls_plan_refine.restype = C.c_int; lib.sls_plan_refine.argtypes = [vp] + common + [vp, vp, C.c_int, i64p]
    lib.sls_plan_packed_dest.restype = C.c_int; lib.sls_plan_packed_dest.argtypes = [vp, i64p]
    lib.sls_plan_fetch_status.restype = C.c_int; lib.sls_plan_fetch_status.argtypes = [vp, i32p, dp, i32p]
    lib.sls_plan_kernel_time_ms.restype = C.c_int; lib.sls_plan_kernel_time_ms.argtypes = [vp, dp, i64p]
    lib.sls_plan_describe.restype = C.c_int; lib.sls_plan_describe.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.sls_plan_alloc_values.restype = C.c_int; lib.sls_plan_alloc_values.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.sls_plan_free_values.restype = C.c_int; lib.sls_plan_free_values.argtypes = [vp, vp]
    lib.sls_plan_download.restype = C.c_int; lib.sls_plan_download.argtypes = [vp, vp, dpp, dpp]
    lib.sls_plan_destroy.restype = None; lib.sls_plan_destroy.argtypes = [vp]
    lib.sls_scatter_f64.restype = C.c_int; lib.sls_scatter_f64.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp]
    lib.sls_shard_groups.restype = C.c_int; lib.sls_shard_groups.argtypes = common + [C.c_int, i64p]
    lib.sls_h2_sf_packed_layout.restype = C.c_int
    lib.sls_h2_sf_packed_layout.argtypes = common + [C.c_int64, C.c_int64, i64p, i64p, i64p, C.POINTER(sls_plan_info)]
    i64pp = C.POINTER(C.POINTER(C.c_int64))
    lib.sls_localization_masks.restype = C.c_int
    lib.sls_localization_masks.argtypes = [C.POINTER(sls_dims), C.POINTER(sls_csc_f64), C.POINTER(sls_csc_f64), C.c_int64,
                                           C.c_double, i64p, i64p, i64pp, i64pp, i64pp, i64pp]
    lib.sls_localization_masks_device.restype = C.c_int
    lib.sls_localization_masks_device.argtypes = [vp, C.c_int] + lib.sls_localization_masks.argtypes
    lib.sls_sparsity_dim_reduction.restype = C.c_int
    lib.sls_sparsity_dim_reduction.argtypes = [C.POINTER(sls_dims), C.POINTER(sls_csc_f64), C.POINTER(sls_csc_bool),
                                               C.POINTER(sls_csc_bool), i64p, C.c_int64, i64p, i64p, i64p, i64p]
    lib.sls_index_sets_device.restype = C.c_int
    lib.sls_index_sets_device.argtypes = [vp, C.c_int, C.POINTER(sls_dims), C.POINTER(sls_csc_f64), C.POINTER(sls_csc_bool),
                                          C.POINTER(sls_csc_bool), i64p, i64p, i64p, i64p]
    lib.sls_h2_sf_plan_localized.restype = C.c_int
    lib.sls_h2_sf_plan_localized.argtypes = [vp, C.c_int, C.POINTER(sls_dims), C.POINTER(sls_plant), C.c_int64, C.c_double, C.POINTER(vp)]
    lib.sls_h2_sf_solve_localized.restype = C.c_int
    lib.sls_h2_sf_solve_localized.argtypes = [vp, C.POINTER(sls_dims), C.POINTER(sls_plant), C.c_int64, C.c_double, dpp, dpp, i32p,
                                              C.POINTER(sls_stats)]
    lib.sls_closed_loop_plan.restype = C.c_int
    lib.sls_closed_loop_plan.argtypes = [vp, C.c_int, C.POINTER(sls_dims), C.POINTER(sls_plant), C.POINTER(sls_csc_bool),
                                         C.POINTER(sls_csc_bool), C.POINTER(vp)]
    lib.sls_closed_loop_run.restype = C.c_int
    lib.sls_closed_loop_run.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int64, vp, vp]
    lib.sls_closed_loop_run_host.restype = C.c_int
    lib.sls_closed_loop_run_host.argtypes = [vp, vp, dp, C.c_int64, C.c_int64, dp, dp]
    lib.sls_closed_loop_last_ms.restype = C.c_int; lib.sls_closed_loop_last_ms.argtypes = [vp, dp]
    lib.sls_closed_loop_entries.restype = C.c_int; lib.sls_closed_loop_entries.argtypes = [vp, i64p]
    lib.sls_closed_loop_destroy.restype = None; lib.sls_closed_loop_destroy.argtypes = [vp]
    lib.sls_plan_execute_batch.restype = C.c_int
    lib.sls_plan_execute_batch.argtypes = [C.POINTER(vp), C.c_int, vp, C.POINTER(vp), C.c_int]
    lib.sls_plan_objective.restype = C.c_int; lib.sls_plan_objective.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    lib.sls_plan_fetch_objective.restype = C.c_int; lib.sls_plan_fetch_objective.argtypes = [vp, vp, C.c_int, dp, dp]
    lib.sls_ctx_want_objective.restype = C.c_int; lib.sls_ctx_want_objective.argtypes = [vp, C.c_int]
    lib.sls_ctx_last_objective.restype = C.c_int; lib.sls_ctx_last_objective.argtypes = [vp, dp, C.c_int64, dp]
    lib.sls_plan_update_plant.restype = C.c_int; lib.sls_plan_update_plant.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.sls_plan_update_result.restype = C.c_int; lib.sls_plan_update_result.argtypes = [vp, i64p]
    lib.sls_plan_fetch_plant.restype = C.c_int; lib.sls_plan_fetch_plant.argtypes = [vp, dp, dp]
    lib.sls_plan_update_weights.restype = C.c_int; lib.sls_plan_update_weights.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.sls_plan_update_weights_result.restype = C.c_int; lib.sls_plan_update_weights_result.argtypes = [vp, i64p]
    lib.sls_plan_fetch_weights.restype = C.c_int; lib.sls_plan_fetch_weights.argtypes = [vp, dp, dp]
    u8p = C.POINTER(C.c_uint8)
    lib.sls_plan_execute_columns.restype = C.c_int; lib.sls_plan_execute_columns.argtypes = [vp, vp, vp, C.c_int, i64p, C.c_int64, i64p]
    lib.sls_plan_track_changes.restype = C.c_int; lib.sls_plan_track_changes.argtypes = [vp, C.c_int]
    lib.sls_plan_execute_dirty.restype = C.c_int; lib.sls_plan_execute_dirty.argtypes = [vp, vp, vp, C.c_int, i64p]
    lib.sls_plan_fetch_dirty.restype = C.c_int; lib.sls_plan_fetch_dirty.argtypes = [vp, u8p]
    lib.sls_plan_clear_dirty.restype = C.c_int; lib.sls_plan_clear_dirty.argtypes = [vp, vp]
    lib.sls_plan_residual.restype = C.c_int; lib.sls_plan_residual.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.sls_plan_fetch_residual.restype = C.c_int; lib.sls_plan_fetch_residual.argtypes = [vp, vp, C.c_int, dp, dp, dp, dp]
    masks = [C.POINTER(sls_dims), C.POINTER(sls_csc_bool), C.POINTER(sls_csc_bool)]
    lib.sls_controller_plan.restype = C.c_int; lib.sls_controller_plan.argtypes = [vp, C.c_int] + masks + [C.c_int64, C.POINTER(vp)]
    lib.sls_controller_load.restype = C.c_int; lib.sls_controller_load.argtypes = [vp, vp, vp]
    lib.sls_controller_reset.restype = C.c_int; lib.sls_controller_reset.argtypes = [vp, vp]
    lib.sls_controller_step.restype = C.c_int; lib.sls_controller_step.argtypes = [vp, vp, vp, vp, vp]
    lib.sls_controller_info.restype = C.c_int; lib.sls_controller_info.argtypes = [vp, i64p, i64p, i64p]
    lib.sls_controller_destroy.restype = None; lib.sls_controller_destroy.argtypes = [vp]
    planted = [C.POINTER(sls_dims), C.POINTER(sls_plant), C.POINTER(sls_csc_bool), C.POINTER(sls_csc_bool)]
    lib.sls_rollout_plan.restype = C.c_int; lib.sls_rollout_plan.argtypes = [vp, C.c_int] + planted + [C.c_int64, C.POINTER(vp)]
    lib.sls_rollout_load.restype = C.c_int; lib.sls_rollout_load.argtypes = [vp, vp, vp]
    lib.sls_rollout_set_plant.restype = C.c_int; lib.sls_rollout_set_plant.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    lib.sls_rollout_set_weights.restype = C.c_int; lib.sls_rollout_set_weights.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.sls_rollout_reset.restype = C.c_int; lib.sls_rollout_reset.argtypes = [vp, vp, vp]
    lib.sls_rollout_run.restype = C.c_int; lib.sls_rollout_run.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.sls_rollout_stats.restype = C.c_int; lib.sls_rollout_stats.argtypes = [vp, vp, vp, vp, vp]
    lib.sls_rollout_fetch.restype = C.c_int; lib.sls_rollout_fetch.argtypes = [vp, vp, dp, dp, dp, dp]
    lib.sls_rollout_info.restype = C.c_int; lib.sls_rollout_info.argtypes = [vp, i64p, i64p, i64p, i64p]
    lib.sls_rollout_destroy.restype = None; lib.sls_rollout_destroy.argtypes = [vp]
    lib.sls_margin_plan.restype = C.c_int; lib.sls_margin_plan.argtypes = [vp, C.c_int] + planted + [C.c_int64, C.POINTER(vp)]
    lib.sls_margin_load.restype = C.c_int; lib.sls_margin_load.argtypes = [vp, vp, vp]
    lib.sls_margin_set_plant.restype = C.c_int; lib.sls_margin_set_plant.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    lib.sls_margin_run.restype = C.c_int; lib.sls_margin_run.argtypes = [vp, vp, vp, vp, vp]
    lib.sls_margin_fetch.restype = C.c_int; lib.sls_margin_fetch.argtypes = [vp, vp, dp, dp, dp]
    lib.sls_margin_info.restype = C.c_int; lib.sls_margin_info.argtypes = [vp, i64p, i64p, i64p, i64p]
    lib.sls_margin_destroy.restype = None; lib.sls_margin_destroy.argtypes = [vp]
    lib.sls_margin_fetch_plant.restype = C.c_int; lib.sls_margin_fetch_plant.argtypes = [vp, vp, dp, dp]
    lib.sls_margin_set_radius.restype = C.c_int; lib.sls_margin_set_radius.argtypes = [vp, dp, dp, C.c_int]
    lib.sls_margin_box_run.restype = C.c_int; lib.sls_margin_box_run.argtypes = [vp, vp, vp, vp, vp]
    lib.sls_margin_box_fetch.restype = C.c_int; lib.sls_margin_box_fetch.argtypes = [vp, vp, dp, i64p, C.POINTER(C.c_uint8), dp]
    lib.sls_margin_box_worst_plant.restype = C.c_int; lib.sls_margin_box_worst_plant.argtypes = [vp, vp, dp, dp]
    lib.sls_margin_box_info.restype = C.c_int; lib.sls_margin_box_info.argtypes = [vp, i64p, i64p, i64p, i64p]
    lib.sls_norms_plan.restype = C.c_int; lib.sls_norms_plan.argtypes = [vp, C.c_int] + masks + [dp, dp, C.c_int64, C.POINTER(vp)]
    lib.sls_norms_load.restype = C.c_int; lib.sls_norms_load.argtypes = [vp, vp, vp]
    lib.sls_norms_l1.restype = C.c_int; lib.sls_norms_l1.argtypes = [vp, vp, vp, vp, vp]
    lib.sls_norms_hinf.restype = C.c_int; lib.sls_norms_hinf.argtypes = [vp, vp, dp, C.c_int64, C.c_int64, vp, vp]
    lib.sls_norms_fetch_l1.restype = C.c_int; lib.sls_norms_fetch_l1.argtypes = [vp, vp, dp, dp, dp]
    lib.sls_norms_fetch_hinf.restype = C.c_int; lib.sls_norms_fetch_hinf.argtypes = [vp, vp, dp, C.c_int64, C.c_int64, dp, dp]
    lib.sls_norms_info.restype = C.c_int; lib.sls_norms_info.argtypes = [vp, i64p, i64p, i64p]
    lib.sls_norms_destroy.restype = None; lib.sls_norms_destroy.argtypes = [vp]
    lib.sls_norms_h2.restype = C.c_int; lib.sls_norms_h2.argtypes = [vp, vp, vp, vp, vp]
    lib.sls_norms_fetch_h2.restype = C.c_int; lib.sls_norms_fetch_h2.argtypes = [vp, vp, dp, dp, dp]
    lib.sls_norms_cov_pattern.restype = C.c_int; lib.sls_norms_cov_pattern.argtypes = [vp, C.c_int64, i64p, i64p]
    lib.sls_norms_cov.restype = C.c_int; lib.sls_norms_cov.argtypes = [vp, vp, vp]
    lib.sls_norms_fetch_cov.restype = C.c_int; lib.sls_norms_fetch_cov.argtypes = [vp, vp, dp]
    # diagnostics outside the public header
    lib.sls_debug_norms_h2_host.restype = C.c_int
    lib.sls_debug_norms_h2_host.argtypes = masks + [dp, dp, dp, dp, dp, dp]
    lib.sls_debug_norms_cov_host.restype = C.c_int
    lib.sls_debug_norms_cov_host.argtypes = masks + [dp, dp, dp, C.c_int64, i64p, i64p, dp]
    lib.sls_debug_norms_tables.restype = C.c_int
    lib.sls_debug_norms_tables.argtypes = masks + [i64p, i32p, i32p, i32p, i32p, i32p, i32p]
    lib.sls_debug_norms_host.restype = C.c_int
    lib.sls_debug_norms_host.argtypes = masks + [dp, dp, dp, dp, C.c_int64, C.c_int64, dp, dp, dp, dp, dp]
    lib.sls_debug_controller_tables.restype = C.c_int
    lib.sls_debug_controller_tables.argtypes = masks + [i64p, i32p, i32p, i32p, i32p]
    lib.sls_debug_controller_host.restype = C.c_int
    lib.sls_debug_controller_host.argtypes = masks + [dp, C.c_int64, C.c_int64, dp, dp, dp]
    lib.sls_debug_rollout_tables.restype = C.c_int
    lib.sls_debug_rollout_tables.argtypes = planted + [i64p, i64p, i32p, i32p, i32p, i32p, i32p, i32p, C.POINTER(C.c_uint8), i32p]
    lib.sls_debug_margin_tables.restype = C.c_int
    lib.sls_debug_margin_tables.argtypes = planted + [i64p, i64p] + [i32p] * 14
    lib.sls_debug_margin_host.restype = C.c_int
    lib.sls_debug_margin_host.argtypes = planted + [dp, C.c_int64, dp, dp, C.c_int, dp, dp, dp, i64p, i64p, i64p, dp, dp, dp]
    lib.sls_debug_margin_box_host.restype = C.c_int
    lib.sls_debug_margin_box_host.argtypes = planted + [dp, C.c_int64, dp, dp, C.c_int, dp, dp, C.c_int, dp, i64p, C.POINTER(C.c_uint8), dp,
                                                        i64p, dp, dp, dp, i32p, i32p]
    lib.sls_debug_margin_entry_signed.restype = C.c_int
    lib.sls_debug_margin_entry_signed.argtypes = planted + [dp, C.c_int64, dp, dp, C.c_int, i64p, i64p, i64p]
    lib.sls_debug_rollout_host.restype = C.c_int
    lib.sls_debug_rollout_host.argtypes = planted + [dp, C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int64, i64p, C.c_int64, dp, C.c_int64,
                                           dp, dp, dp, dp, dp, dp]
    lib.sls_debug_residual_host.restype = C.c_int
    lib.sls_debug_residual_host.argtypes = common + [dpp, dpp, dp, dp, dp, dp, i64p, dp, i64p, dp, i64p, i32p, C.c_int64]
    lib.sls_plan_gradient.restype = C.c_int; lib.sls_plan_gradient.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.sls_plan_fetch_gradient.restype = C.c_int; lib.sls_plan_fetch_gradient.argtypes = [vp, vp, C.c_int, dp, dp, dp, dp, dp, i64p]
    lib.sls_plan_fetch_multipliers.restype = C.c_int; lib.sls_plan_fetch_multipliers.argtypes = [vp, C.c_int64, dp, C.c_int64]
    lib.sls_debug_gradient_host.restype = C.c_int
    lib.sls_debug_gradient_host.argtypes = common + [i64p, i64p, i32p, i64p, i64p, i32p, dp, dpp, dpp, i32p, dp, dp, dp, dp, dp, i64p, i64p]
    lib.sls_debug_objective_host.restype = C.c_int
    lib.sls_debug_objective_host.argtypes = common + [dp, dp, dpp, dpp, dp, dp, i64p, dp]
    lib.sls_debug_operator_update_host.restype = C.c_int
    lib.sls_debug_operator_update_host.argtypes = [C.POINTER(sls_dims), C.POINTER(sls_csc_f64), C.POINTER(sls_csc_f64), dp, dp, dp, dp, dp, dp,
                                                   i32p, C.POINTER(C.c_uint8)]
    lib.sls_debug_affected_host.restype = C.c_int
    lib.sls_debug_affected_host.argtypes = common + [u8p, u8p, u8p]
    lib.sls_debug_weights_shape_check.restype = C.c_int
    lib.sls_debug_weights_shape_check.argtypes = [C.POINTER(sls_dims), C.POINTER(sls_plant), dp]
    lib.sls_debug_weights_host.restype = C.c_int
    lib.sls_debug_weights_host.argtypes = common + [dp, dp, dp, dp, C.c_int, i64p, i32p, i64p, i32p, i32p, dp, dp, dp, dp, u8p, i64p]
    lib.sls_debug_tile_invert.restype = C.c_int; lib.sls_debug_tile_invert.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_int]
    lib.sls_plan_debug_read_workspace.restype = C.c_int; lib.sls_plan_debug_read_workspace.argtypes = [vp, C.c_int64, C.c_int64, dp]
    lib.sls_plan_debug_twisted4_tables.restype = C.c_int
    lib.sls_plan_debug_twisted4_tables.argtypes = [vp, i64p, i32p, i64p, i32p, i32p, dp, C.POINTER(C.c_uint64)]
    lib.sls_plan_debug_twisted4_static.restype = C.c_int
    lib.sls_plan_debug_twisted4_static.argtypes = [vp, i64p, i32p, i64p, dp, u8p, dp]
    lib.sls_plan_debug_twisted4_images.restype = C.c_int
    lib.sls_plan_debug_twisted4_images.argtypes = [vp, i64p, i64p, i32p, dp]
    lib.sls_debug_plan_tables.restype = C.c_int
    lib.sls_debug_plan_tables.argtypes = [vp, C.c_int, C.POINTER(sls_dims), C.POINTER(sls_plant), C.POINTER(sls_csc_bool),
                                          C.POINTER(sls_csc_bool), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sls_debug_plan_tables_localized.restype = C.c_int
    lib.sls_debug_plan_tables_localized.argtypes = [vp, C.c_int, C.POINTER(sls_dims), C.POINTER(sls_plant), C.c_int64, C.c_double,
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.sls_debug_describe_launches.restype = C.c_int
    lib.sls_debug_describe_launches.argtypes = common + [C.c_int64, C.c_int64, C.c_int, C.c_char_p, C.c_int64]
    if lib.sls_abi_version() != SLS_ABI_VERSION:
        raise ImportError(f"ABI mismatch: library {lib.sls_abi_version()} vs binding {SLS_ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def last_error(ctx=None) -> str:
    s = load_library().sls_last_error(ctx)
    return s.decode("utf-8", "replace") if s else ""


def check(rc: int, ctx=None):
    if rc < 0:
        raise SLSError(rc, last_error(ctx) or last_error(None))
    return rc


# ---------------------------------------------------------------------------
# device arguments of the objects that evaluate a resident Φ
# ---------------------------------------------------------------------------
def _is_tensor(a):
    t = sys.modules.get("torch")
    return t is not None and isinstance(a, t.Tensor)


def _dev_ptr(a, n, what):
    """device pointer of a torch tensor (checked: float64, contiguous, on a GPU, n elements) or a raw pointer / None"""
    if _is_tensor(a):
        t = sys.modules["torch"]
        if not a.is_cuda or a.dtype != t.float64 or not a.is_contiguous() or a.numel() != n:
            raise ValueError(f"{what} must be a contiguous float64 device tensor of {n} elements")
        return a.data_ptr()
    return a


def plant_value_args(A, B2, nnz_A, nnz_B2, nscen, per_scenario):
    """The plant arguments of a `set_plant`: (A pointer, B2 pointer, on_device, arrays to keep alive during the call), or None
    when both are None.  Each of A / B2: None, a host array, or a device tensor; nnz values, or nnz·nscen with per_scenario."""
    given = [(name, v, nnz) for name, v, nnz in (("A", A, nnz_A), ("B2", B2, nnz_B2)) if v is not None]
    if not given:
        return None
    dev = [_is_tensor(v) for _, v, _ in given]
    if any(dev) != all(dev):
        raise ValueError("set_plant: A and B2 must both be host arrays or both be device tensors")
    ptrs, keep = {"A": None, "B2": None}, []
    for name, v, nnz in given:
        n = nnz * (nscen if per_scenario else 1)
        if dev[0]:
            ptrs[name] = _dev_ptr(v, n, f"set_plant: {name}")
        else:
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.size != n:
                raise ValueError(f"set_plant: {name} has {a.size} values, expected {n}")
            keep.append(a)
            ptrs[name] = a.ctypes.data
    return ptrs["A"], ptrs["B2"], int(dev[0]), keep


# ---------------------------------------------------------------------------
# marshalling helpers: keep the numpy arrays alive next to the ctypes structs
# ---------------------------------------------------------------------------
class Marshalled:
    """Holds ctypes views of a problem (plant, masks, groups) plus the arrays backing them."""

    def __init__(self, P, Sx, Su, groups=None, index_base=0, flags=0):
        """index_base = 1 hands every colptr/rowval/group column over exactly as Julia stores them (used by the tests to
        exercise the path the `ccall` binding takes); groups are always given 0-based on the Python side."""
        self.keep = []
        self.base = int(index_base)
        # A, B2, C1 and D12 as handed to the library (references only: struct, colptr, rowval, nzval, nrows), and — once
        # Plan.update_plant or Plan.refine has called own_plant_values — the nzval arrays this object owns and the structs point at
        self.csc, self.nzval = {}, None
        T = len(Sx)
        if len(Su) != T:
            raise ValueError("𝓢x and 𝓢u must have the same length T")
        self.dims = sls_dims(P.Nx, P.Nu, P.Nz, P.Nw, T, self.base, int(flags))
        self.plant = sls_plant()
        for name, attr in (("A", "A"), ("B1", "B1"), ("B2", "B2"), ("C1", "C1"), ("D11", "D11"), ("D12", "D12")):
            M = getattr(P, attr)
            setattr(self.plant, name, C.pointer(self._f64(M, name if name in ("A", "B2", "C1", "D12") else None)) if M is not None else None)
        self.Sx = (sls_csc_bool * T)(*[self._bool(m) for m in Sx])
        self.Su = (sls_csc_bool * T)(*[self._bool(m) for m in Su])
        if groups is None:
            self.ngroups = 0
            self.group_ptr = None
            self.group_cols = None
            self.n_sub = P.Nx
        else:
            ptr = np.zeros(len(groups) + 1, dtype=np.int64)
            ptr[1:] = np.cumsum([len(g) for g in groups])
            cols = np.asarray([c for g in groups for c in g], dtype=np.int64) + self.base
            self.keep += [ptr, cols]
            self.ngroups = len(groups)
            self.group_ptr = ptr.ctypes.data_as(C.POINTER(C.c_int64))
            self.group_cols = cols.ctypes.data_as(C.POINTER(C.c_int64)) if len(cols) else None
            self.n_sub = int(ptr[-1])
        self.nnz_x = [int(sp.csc_matrix(m).nnz) for m in Sx]
        self.nnz_u = [int(sp.csc_matrix(m).nnz) for m in Su]

    @classmethod
    def masks_only(cls, Nx, Nu, Sx, Su, index_base=0):
        """dims and masks without a plant (the stand-alone controller reads Nx, Nu, T, index_base and the masks alone)"""
        self = cls.__new__(cls)
        self.keep, self.base, self.csc, self.nzval = [], int(index_base), {}, None
        T = len(Sx)
        if len(Su) != T:
            raise ValueError("𝓢x and 𝓢u must have the same length T")
        self.dims = sls_dims(int(Nx), int(Nu), int(Nx) + int(Nu), int(Nx), T, self.base, 0)
        self.Sx = (sls_csc_bool * T)(*[self._bool(m) for m in Sx])
        self.Su = (sls_csc_bool * T)(*[self._bool(m) for m in Su])
        self.nnz_x = [int(sp.csc_matrix(m).nnz) for m in Sx]
        self.nnz_u = [int(sp.csc_matrix(m).nnz) for m in Su]
        return self

    def _csc_arrays(self, M):
        M = sp.csc_matrix(M)
        if not M.has_sorted_indices:
            M = M.copy(); M.sort_indices()
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + self.base
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + self.base
        return M, colptr, rowval

    def _f64(self, M, track=None):
        M, colptr, rowval = self._csc_arrays(M)
        nz = np.ascontiguousarray(M.data, dtype=np.float64)
        self.keep += [colptr, rowval, nz]
        s = sls_csc_f64(M.shape[0], M.shape[1], colptr.ctypes.data_as(C.POINTER(C.c_int64)),
                        rowval.ctypes.data_as(C.POINTER(C.c_int64)), nz.ctypes.data_as(C.POINTER(C.c_double)))
        self.keep.append(s)
        if track:
            self.csc[track] = (s, colptr, rowval, nz, M.shape[0])
        return s

    def pattern(self, name):
        """0-based (indptr, indices, nrows) of the stored pattern of A or B2 as the library received it"""
        _, colptr, rowval, _, nrows = self.csc[name]
        return colptr - self.base, rowval - self.base, nrows

    def nnz(self, name):
        return int(self.csc[name][3].size)

    def own_plant_values(self):
        """First Plan.update_plant: from here on the nzval arrays of A and B2 behind the ctypes structs are arrays of this
        object (never the caller's own, which np.ascontiguousarray may have handed through), so that new values can be
        written into them.  Nothing is copied for objects that are never updated."""
        if self.nzval is None:
            self.nzval = {}
            for name, (s, _, _, nz, _) in self.csc.items():
                own = nz.copy()
                s.nzval = own.ctypes.data_as(C.POINTER(C.c_double))
                self.keep.append(own)
                self.nzval[name] = own
        return self.nzval

    def _bool(self, M):
        M, colptr, rowval = self._csc_arrays(M)
        nz = np.ascontiguousarray(M.data != 0, dtype=np.uint8)
        self.keep += [colptr, rowval, nz]
        return sls_csc_bool(M.shape[0], M.shape[1], colptr.ctypes.data_as(C.POINTER(C.c_int64)),
                            rowval.ctypes.data_as(C.POINTER(C.c_int64)), nz.ctypes.data_as(C.POINTER(C.c_uint8)))

    def common_args(self):
        return (C.byref(self.dims), C.byref(self.plant), self.Sx, self.Su, self.ngroups, self.group_ptr,
                self.group_cols)
