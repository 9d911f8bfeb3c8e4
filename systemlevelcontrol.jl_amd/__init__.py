"""MI355X-native engine for the column-separable 𝓗₂ SLS solve of SystemLevelControl.jl.

Public surface mirrors the reference's exports for this path (src/SystemLevelControl.jl:9-23):
    Plant, GeneralizedPlant, StateFeedback, OutputFeedback, SLS_H2 (the reference's SLS_𝓗₂;
    '₂' is not a legal Python identifier character, so the ASCII spelling is the name)
plus the plan/execute split of the C ABI (include/sls_mi355x.h).

The directory is named after the reference (`systemlevelcontrol.jl_amd`), which is not an
importable Python identifier; the repo-root shim `slc_amd.py` loads it as module `slc_amd`.
The compute backend is libsls_mi355x.so (hand-written HIP for gfx950); nothing here falls
back to the CPU.
"""
from .plant import GeneralizedPlant, OutputFeedback, Plant, StateFeedback
from .synthesis import SLS_H2, SLS_H2_batch, SLS_H2_localized, SLS_Hinf_bound, execute_batch, Context, Plan, assemble_phi, default_context, objective_values_host, residual_host, Residual
from .closed_loop import ClosedLoop
from .gradient import gradient_host, gradient_tables, h2_cost
from .controller import Controller, controller_host, controller_tables
from .rollout import Rollout, rollout_host, rollout_tables
from .margin import RobustMargin, margin_box_host, margin_entry_signed_check, margin_host, margin_tables
from .norms import ClosedLoopNorms, covariance_pattern_of, norms_cov_host, norms_h2_host, norms_host, norms_tables
from ._capi import SLSError, load_library
from . import _capi, closed_loop, controller, dist, gradient, margin, norms, rollout, workloads

__all__ = ["Plant", "GeneralizedPlant", "StateFeedback", "OutputFeedback", "SLS_H2", "Context", "Plan",
           "assemble_phi", "default_context", "objective_values_host", "residual_host", "Residual", "SLS_Hinf_bound", "SLS_H2_batch", "SLS_H2_localized", "execute_batch", "ClosedLoop", "Controller", "controller_host", "controller_tables", "Rollout", "rollout_host", "rollout_tables", "RobustMargin", "margin_host", "margin_tables", "margin_box_host", "margin_entry_signed_check", "ClosedLoopNorms", "norms_host", "norms_tables", "norms_h2_host", "norms_cov_host", "covariance_pattern_of", "SLSError", "load_library", "dist", "workloads", "gradient_host", "gradient_tables", "h2_cost"]
