"""SLS_𝓗₂ — host-side mirror of the reference entry point, backed by the HIP engine.

Reference: src/synthesis.jl
  :11      SLS_𝓗₂(P::AbstractGeneralizedPlant, 𝓢::AbstractVector; 𝓘=nothing)
  :13,30   non-StateFeedback plant ⇒ returns `nothing`
  :15      default 𝓘 = [[i] for i in 1:P.Nx]
  :16      static contiguous partition of the groups over nworkers()
  :24-27   @distributed (+) over the chunks; returns eachcol(Φ) → (Φx, Φu)
The per-column work (src/synthesis.jl:34-72, src/reduction.jl:11-27) runs inside
libsls_mi355x.so; this module only marshals.  ('₂' is not a legal Python identifier
character, so the function is spelled `SLS_H2`.)
"""
from __future__ import annotations

import ctypes as C
import sys
import typing
import warnings

import numpy as np
import scipy.sparse as sp

from . import _capi
from .plant import GeneralizedPlant, StateFeedback


class Context:
    """Owns the HIP devices used by a solve — the analogue of the `julia -p N` worker pool."""

    def __init__(self, devices=None):
        lib = _capi.load_library()
        if devices is None:
            devices = [0]
        arr = (C.c_int * len(devices))(*devices)
        self._lib = lib
        self.devices = list(devices)
        self.handle = lib.sls_create(arr, len(devices), 0)
        if not self.handle:
            raise _capi.SLSError(_capi.SLS_ENODEVICE, _capi.last_error(None))

    def set_ridge(self, rx=None, ru=None):
        """Ridge term Σ_t Σ_i rx[i]·Φx[t][i,c]² + Σ_j ru[j]·Φu[t][j,c]² added to every column's cost in later solves on this
        context (sls_set_ridge: the diagonal instance of the reference's L⁺ hook, src/synthesis.jl:21,52).  None/None clears."""
        rx = np.zeros(0) if rx is None else np.ascontiguousarray(rx, dtype=np.float64)
        ru = np.zeros(0) if ru is None else np.ascontiguousarray(ru, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _capi.check(self._lib.sls_set_ridge(self.handle, rx.size, rx.ctypes.data_as(dp) if rx.size else None,
                                            ru.size, ru.ctypes.data_as(dp) if ru.size else None), self.handle)

    def want_objective(self, on=True):
        """sls_ctx_want_objective: later one-shot solves on this context (SLS_H2, SLS_H2_batch, SLS_H2_localized) also evaluate
        every column's objective value on the device, before their download; `last_objective` reads it."""
        _capi.check(self._lib.sls_ctx_want_objective(self.handle, int(bool(on))), self.handle)

    def last_objective(self, n):
        """sls_ctx_last_objective: (per-subproblem objective values in col_status order, their total) of the last one-shot solve
        that ran with `want_objective` on; n = its number of subproblems."""
        col = np.zeros(max(int(n), 1), dtype=np.float64)
        tot = C.c_double()
        _capi.check(self._lib.sls_ctx_last_objective(self.handle, col.ctypes.data_as(C.POINTER(C.c_double)), int(n), C.byref(tot)),
                    self.handle)
        return col[: int(n)], tot.value

    def close(self):
        if getattr(self, "handle", None):
            self._lib.sls_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None or not _default_ctx.handle:
        _default_ctx = Context([0])
    return _default_ctx


class Plan:
    """Symbolic pass + device-resident tables for a shard of the groups (sls_h2_sf_plan)."""

    def __init__(self, ctx: Context, P, S, groups=None, group_range=None, dev_slot=0, objective="h2", updatable_weights=False,
                 multipliers=False):
        """updatable_weights=True builds the plan with SLS_PLAN_WEIGHTS_UPDATABLE: `update_weights` can then give it new LQR
        weights (C1 = [diag(q); 0], D12 = [0; diag(r)], D11 = 0 on the selected rows, no coupled group: SLSError otherwise).
        multipliers=True builds it with SLS_PLAN_MULTIPLIERS: every execute keeps the multipliers of the achievability
        constraints, which `gradient` turns into the derivative of the 𝓗₂ cost in the stored entries of A and B2 (every column
        then runs on the one-wave kernel; SLSError for ñx > 32, dense Hessians, coupled groups and the sum-of-norms objective)."""
        Sx, Su = S
        self.ctx = ctx
        self._lib = ctx._lib
        self.m = _capi.Marshalled(P, Sx, Su, groups, flags=_plan_flags(objective, updatable_weights, multipliers))
        ng = self.m.ngroups if groups is not None else P.Nx
        gb, ge = (0, ng) if group_range is None else group_range
        h = C.c_void_p()
        _capi.check(self._lib.sls_h2_sf_plan(ctx.handle, dev_slot, *self.m.common_args(), gb, ge, C.byref(h)),
                    ctx.handle)
        self.handle = h
        info = _capi.sls_plan_info()
        _capi.check(self._lib.sls_plan_get_info(self.handle, C.byref(info)))
        self.info = info.asdict()
        T = self.info["T"]
        ox = np.zeros(T + 1, dtype=np.int64); ou = np.zeros(T + 1, dtype=np.int64)
        _capi.check(self._lib.sls_plan_value_offsets(self.handle, ox.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     ou.ctypes.data_as(C.POINTER(C.c_int64))))
        self.off_x, self.off_u = ox, ou
        self._owned_values = []

    @classmethod
    def localized(cls, ctx, P, d, T, alpha, dev_slot=0, objective="h2", index_base=0, updatable_weights=False, multipliers=False):
        """sls_h2_sf_plan_localized: the plan of the README's (d, T, α) localization built from the plant alone — level sets,
        index sets, mask slices and destinations computed on the device, no mask array crosses PCIe.  Values come back in the
        CSC order of `workloads.localization_masks_native(P.A, P.B2, d, T, alpha)`.  updatable_weights=True: as in `Plan`; the
        plant may then carry LQR weights other than the identity (D11 must be zero).  multipliers=True: as in `Plan`."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self._lib = ctx._lib
        empty = [sp.csc_matrix((P.Nx, P.Nx), dtype=bool)] * 0
        self.m = _capi.Marshalled(P, empty, empty, None, index_base=index_base, flags=_plan_flags(objective, updatable_weights, multipliers))
        self.m.dims.T = int(T)
        h = C.c_void_p()
        _capi.check(self._lib.sls_h2_sf_plan_localized(ctx.handle, dev_slot, C.byref(self.m.dims), C.byref(self.m.plant), int(d),
                                                       float(alpha), C.byref(h)), ctx.handle)
        self.handle = h
        info = _capi.sls_plan_info()
        _capi.check(self._lib.sls_plan_get_info(self.handle, C.byref(info)))
        self.info = info.asdict()
        ox = np.zeros(T + 1, dtype=np.int64); ou = np.zeros(T + 1, dtype=np.int64)
        _capi.check(self._lib.sls_plan_value_offsets(self.handle, ox.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     ou.ctypes.data_as(C.POINTER(C.c_int64))))
        self.off_x, self.off_u = ox, ou
        self.m.nnz_x = [int(v) for v in np.diff(ox)]
        self.m.nnz_u = [int(v) for v in np.diff(ou)]
        self._owned_values = []
        return self

    # -- device buffers managed by the library (for callers without torch) --
    def alloc_values(self, packed=False):
        p = C.c_void_p()
        _capi.check(self._lib.sls_plan_alloc_values(self.handle, int(packed), C.byref(p)), self.ctx.handle)
        self._owned_values.append(p.value)
        return p.value

    def execute(self, d_values, packed=False, stream=None):
        _capi.check(self._lib.sls_plan_execute(self.handle, stream, d_values, int(packed)), self.ctx.handle)

    def synchronize(self, stream=None):
        _capi.check(self._lib.sls_plan_synchronize(self.handle, stream), self.ctx.handle)

    def refine(self, d_values, packed=False, stream=None):
        """sls_plan_refine: after an execute, re-solve the near-singular columns of the one-wave / twisted kernels on the tile
        kernel and attach that pass to the plan (later executes run it too).  Returns the number of subproblems refined."""
        if getattr(self, "_plant_updated", False):       # after updates: pass the plant the device holds
            own = self.m.own_plant_values()
            own["A"][:], own["B2"][:] = self.plant_values()
            self._plant_updated = False
        if getattr(self, "_weights_updated", False):     # … and the weights it holds
            own = self.m.own_plant_values()
            own["C1"][:], own["D12"][:] = self.weights()
            self._weights_updated = False
        n = C.c_int64()
        _capi.check(self._lib.sls_plan_refine(self.handle, *self.m.common_args(), stream, d_values, int(packed), C.byref(n)), self.ctx.handle)
        return n.value

    def update_plant(self, A=None, B2=None, stream=None):
        """sls_plan_update_plant: new values of A and / or B2 for this plan, enqueued on `stream`; the next `execute` solves
        the new plant without a rebuild.  Each argument is None (unchanged), a scipy sparse matrix whose stored pattern equals
        the plan's (ValueError otherwise), a 1-D float64 NumPy array of nzval in the plan's CSC order, or a CUDA torch tensor
        of nzval, which selects the device path (both arguments must then be tensors, or one of them None; a tensor must stay
        valid and unchanged until the update has run on `stream`, and is not kept beyond the call).  An entry that was exactly
        0.0 when the plan was built must stay 0.0 and every value must be finite: the host path raises SLSError (SLS_EINVAL)
        and leaves the plan untouched, the device path skips such entries and counts them (`update_result`).
        An attached refinement is dropped — call `refine` again.  The marshalled plant of this object follows: the host path
        writes the new values into it at once, and `refine` first reads the plan's own values back from the device
        (`plant_values`), so it always passes the plant the device holds."""
        given = [(name, v) for name, v in (("A", A), ("B2", B2)) if v is not None]
        if not given:
            return
        on_device = [_is_device_tensor(v) for _, v in given]
        if any(on_device) != all(on_device):
            raise ValueError("update_plant: A and B2 must both be host arrays or both be device tensors")
        ptrs, host = {"A": None, "B2": None}, {}
        for name, v in given:
            nnz = self.m.nnz(name)
            if on_device[0]:
                if v.dtype != _torch().float64 or v.dim() != 1 or not v.is_contiguous() or v.device.index != self.info["device"]:
                    raise ValueError(f"update_plant: {name} must be a contiguous 1-D float64 tensor on the plan's device")
                if v.numel() != nnz:
                    raise ValueError(f"update_plant: {name} has {v.numel()} values, the plan's {name} stores {nnz}")
                ptrs[name] = v.data_ptr()
            else:
                host[name] = _nzval_of(name, v, nnz, self.m)
                ptrs[name] = host[name].ctypes.data
        _capi.check(self._lib.sls_plan_update_plant(self.handle, stream, ptrs["A"], ptrs["B2"], int(on_device[0])), self.ctx.handle)
        own = self.m.own_plant_values()
        for name, nz in host.items():
            own[name][:] = nz
        self._plant_updated = True

    def plant_values(self):
        """sls_plan_fetch_plant: (A nzval, B2 nzval) as the plan holds them on the device now — waits for the last
        `update_plant`; entries its device path refused are at their old values."""
        a, b = np.zeros(max(self.m.nnz("A"), 1)), np.zeros(max(self.m.nnz("B2"), 1))
        dp = C.POINTER(C.c_double)
        _capi.check(self._lib.sls_plan_fetch_plant(self.handle, a.ctypes.data_as(dp), b.ctypes.data_as(dp)), self.ctx.handle)
        return a[: self.m.nnz("A")], b[: self.m.nnz("B2")]

    def update_result(self):
        """sls_plan_update_result: waits for the last `update_plant` and returns how many entries its device path refused
        (0: applied in full; always 0 after a host-path update)."""
        n = C.c_int64()
        _capi.check(self._lib.sls_plan_update_result(self.handle, C.byref(n)), self.ctx.handle)
        return n.value

    # -- new LQR weights for a plan built with updatable_weights=True (sls_mi355x.h) --
    def update_weights(self, C1=None, D12=None, stream=None):
        """sls_plan_update_weights: new diagonals of C1 and / or D12, enqueued on `stream`; the next `execute` solves the
        re-weighted problem without a rebuild.  Each argument is None (unchanged), a 1-D float64 array of the diagonal (Nx values
        C1[i, i], Nu values D12[Nx + j, j]), a scipy sparse matrix of the LQR shape ([diag(q); 0] / [0; diag(r)], one stored entry per
        column: ValueError otherwise; the diagonal is taken on the host) or a CUDA torch tensor of the diagonal, which selects
        the device path (both arguments must then be tensors, or one of them None).  A value must be finite and leave the
        Hessian positive (0.0 needs a ridge term): the host path raises SLSError (SLS_EINVAL) and leaves the plan untouched, the
        device path skips such values and counts them (`update_weights_result`).  An attached refinement is dropped — call
        `refine` again; it passes the plant with the weights the device holds (`weights`)."""
        given = [(name, v) for name, v in (("C1", C1), ("D12", D12)) if v is not None]
        if not given:
            raise ValueError("update_weights: give C1, D12 or both")
        on_device = [_is_device_tensor(v) for _, v in given]
        if any(on_device) != all(on_device):
            raise ValueError("update_weights: C1 and D12 must both be host arrays or both be device tensors")
        Nx, Nu = int(self.m.dims.Nx), int(self.m.dims.Nu)
        ptrs, keep = {"C1": None, "D12": None}, []
        for name, v in given:
            n, shift = (Nx, 0) if name == "C1" else (Nu, Nx)
            if on_device[0]:
                if v.dtype != _torch().float64 or v.dim() != 1 or not v.is_contiguous() or v.device.index != self.info["device"]:
                    raise ValueError(f"update_weights: {name} must be a contiguous 1-D float64 tensor on the plan's device")
                if v.numel() != n:
                    raise ValueError(f"update_weights: {name} has {v.numel()} values, the diagonal has {n}")
                ptrs[name] = v.data_ptr()
            else:
                d = _diag_of(name, v, n, shift, Nx + Nu)
                keep.append(d)
                ptrs[name] = d.ctypes.data
        _capi.check(self._lib.sls_plan_update_weights(self.handle, stream, ptrs["C1"], ptrs["D12"], int(on_device[0])), self.ctx.handle)
        self._weights_updated = True

    def update_weights_result(self):
        """sls_plan_update_weights_result: waits for the plan's last update and returns how many values the device path of the
        last `update_weights` refused (0: applied in full; always 0 after a host-path update)."""
        n = C.c_int64()
        _capi.check(self._lib.sls_plan_update_weights_result(self.handle, C.byref(n)), self.ctx.handle)
        return n.value

    def weights(self):
        """sls_plan_fetch_weights: (C1 diagonal, D12 diagonal) as the plan holds them on the device now — waits for the last
        update; values its device path refused are at their old values."""
        Nx, Nu = int(self.m.dims.Nx), int(self.m.dims.Nu)
        a, b = np.zeros(max(Nx, 1)), np.zeros(max(Nu, 1))
        dp = C.POINTER(C.c_double)
        _capi.check(self._lib.sls_plan_fetch_weights(self.handle, a.ctypes.data_as(dp), b.ctypes.data_as(dp)), self.ctx.handle)
        return a[:Nx], b[:Nu]

    # -- partial re-solve: only the columns a local plant change touched (sls_mi355x.h) --
    def execute_columns(self, d_values, subs, packed=False, stream=None):
        """sls_plan_execute_columns: solve only the subproblems `subs` (positions in col_status order, 0-based, strictly
        ascending; ValueError otherwise) into `d_values`; entries and status words of the others are not written.  A coupled
        group is solved as a whole when any of its columns is listed.  Waits for `stream` once, before the solve is enqueued
        (the launch lists are sized on the host).  Returns the number of subproblems solved."""
        s = np.asarray(subs)
        if s.ndim != 1 or (s.size and not np.issubdtype(s.dtype, np.integer)):
            raise ValueError("execute_columns: subs must be a 1-D sequence of integers")
        s = np.ascontiguousarray(s, dtype=np.int64)
        n = self.info["n_subproblems"]
        if s.size and (s[0] < 0 or s[-1] >= n or np.any(np.diff(s) <= 0)):
            raise ValueError(f"execute_columns: subs must be strictly ascending inside 0 .. {n - 1}")
        if s.size == 0:
            return 0
        k = C.c_int64()
        _capi.check(self._lib.sls_plan_execute_columns(self.handle, stream, d_values, int(packed), s.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       s.size, C.byref(k)), self.ctx.handle)
        return k.value

    def track_changes(self, on=True):
        """sls_plan_track_changes: with tracking on, every later `update_plant` also marks the subproblems touched by the
        entries it actually changed (accepted, and different in their bits); turning it on clears the marks."""
        _capi.check(self._lib.sls_plan_track_changes(self.handle, int(bool(on))), self.ctx.handle)

    def execute_dirty(self, d_values, packed=False, stream=None):
        """sls_plan_execute_dirty: `execute_columns` on the marked subproblems, then the marks are cleared on the same stream.
        Returns the number of subproblems solved (0, and nothing is enqueued, when tracking was never on)."""
        k = C.c_int64()
        _capi.check(self._lib.sls_plan_execute_dirty(self.handle, stream, d_values, int(packed), C.byref(k)), self.ctx.handle)
        return k.value

    def dirty(self):
        """sls_plan_fetch_dirty: the marks as a uint8 array in col_status order (waits for the last update and execute)."""
        n = self.info["n_subproblems"]
        d = np.zeros(max(n, 1), dtype=np.uint8)
        _capi.check(self._lib.sls_plan_fetch_dirty(self.handle, d.ctypes.data_as(C.POINTER(C.c_uint8))), self.ctx.handle)
        return d[:n]

    def clear_dirty(self, stream=None):
        _capi.check(self._lib.sls_plan_clear_dirty(self.handle, stream), self.ctx.handle)

    def packed_dest(self):
        d = np.zeros(max(self.info["n_packed"], 1), dtype=np.int64)
        _capi.check(self._lib.sls_plan_packed_dest(self.handle, d.ctypes.data_as(C.POINTER(C.c_int64))))
        return d[: self.info["n_packed"]]

    def fetch_status(self):
        n = self.info["n_subproblems"]
        st = np.zeros(max(n, 1), dtype=np.int32); it = np.zeros(max(n, 1), dtype=np.int32)
        rs = np.zeros(max(n, 1), dtype=np.float64)
        _capi.check(self._lib.sls_plan_fetch_status(self.handle, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    rs.ctypes.data_as(C.POINTER(C.c_double)),
                                                    it.ctypes.data_as(C.POINTER(C.c_int32))), self.ctx.handle)
        return st[:n], rs[:n], it[:n]

    def objective_values(self, d_values, packed=False, stream=None):
        """(col_objective ndarray, total float): the objective value every subproblem of this plan achieved, evaluated on the
        device from the value array an execute wrote (sls_plan_fetch_objective; layout `packed` as in `execute`).  A coupled
        group's joint value sits on its first column, the others report 0.0.  With `stream` the evaluation is enqueued there
        (after the execute the caller put on it) and that stream is waited for."""
        n = self.info["n_subproblems"]
        if stream is not None:
            col, tot = self.objective_values_async(d_values, packed=packed, stream=stream)
            self.synchronize(stream)
            return col.cpu().numpy(), float(tot.item())
        col = np.zeros(max(n, 1), dtype=np.float64)
        tot = C.c_double()
        _capi.check(self._lib.sls_plan_fetch_objective(self.handle, d_values, int(packed), col.ctypes.data_as(C.POINTER(C.c_double)),
                                                       C.byref(tot)), self.ctx.handle)
        return col[:n], tot.value

    def objective_values_async(self, d_values, packed=False, stream=None):
        """sls_plan_objective into fresh torch tensors on the plan's device: (col_objective[n_subproblems], total[1]), enqueued
        on `stream` (None = the null stream) after the execute that wrote `d_values`; nothing waits for the device."""
        import torch
        dev = torch.device("cuda", self.info["device"])
        col = torch.empty(max(self.info["n_subproblems"], 1), dtype=torch.float64, device=dev)
        tot = torch.empty(1, dtype=torch.float64, device=dev)          # written by the call (zeroed there when the plan is empty)
        _capi.check(self._lib.sls_plan_objective(self.handle, stream, d_values, int(packed), col.data_ptr(), tot.data_ptr()),
                    self.ctx.handle)
        return col[: self.info["n_subproblems"]], tot

    def residual(self, d_values, packed=False, stream=None):
        """`Residual` record of the achievability residual of every subproblem of this plan against the FULL plant, evaluated
        on the device from the value array `d_values` (layout `packed` as in `execute`) and the values of A and B2 the plan
        holds now (sls_plan_fetch_residual; definition: include/sls_mi355x.h).  Waits for the plan's last execute
        and last `update_plant`.  With `stream` the evaluation is enqueued there instead (sls_plan_residual, behind what the
        caller put on it) and that stream is waited for."""
        n = self.info["n_subproblems"]
        dp = C.POINTER(C.c_double)
        if stream is not None:
            ri, hi, l1, tot = self.residual_async(d_values, packed=packed, stream=stream)
            self.synchronize(stream)
            tot = tot.cpu().numpy()
            return Residual(ri.cpu().numpy(), hi.cpu().numpy(), l1.cpu().numpy(), float(tot[0]), float(tot[1]))
        out = [np.zeros(max(n, 1), dtype=np.float64) for _ in range(3)]
        tot = np.zeros(2, dtype=np.float64)
        _capi.check(self._lib.sls_plan_fetch_residual(self.handle, d_values, int(packed), *[a.ctypes.data_as(dp) for a in out],
                                                      tot.ctypes.data_as(dp)), self.ctx.handle)
        return Residual(out[0][:n], out[1][:n], out[2][:n], float(tot[0]), float(tot[1]))

    def residual_async(self, d_values, packed=False, stream=None):
        """sls_plan_residual into fresh torch tensors on the plan's device: (res_inf, halo_inf, res_l1 [n_subproblems],
        totals[2] = max res_inf, max res_l1), enqueued on `stream` (None = the null stream); nothing waits for the device
        (the plan's first call builds the halo lists on the host and does wait)."""
        import torch
        dev = torch.device("cuda", self.info["device"])
        n = self.info["n_subproblems"]
        out = [torch.empty(max(n, 1), dtype=torch.float64, device=dev) for _ in range(3)]
        tot = torch.empty(2, dtype=torch.float64, device=dev)          # written by the call (zeroed there when the plan is empty)
        _capi.check(self._lib.sls_plan_residual(self.handle, stream, d_values, int(packed), *[a.data_ptr() for a in out],
                                                tot.data_ptr()), self.ctx.handle)
        return out[0][:n], out[1][:n], out[2][:n], tot

    # -- gradient of the 𝓗₂ cost in A, B2 and the LQR diagonals, for a plan built with multipliers=True --
    def gradient(self, d_values, packed=False, column_weights=None, stream=None, weights=False):
        """sls_plan_gradient into fresh torch tensors on the plan's device: (gA[nnz(A)], gB2[nnz(B2)]) — the derivative of
        Σ_j c_j·J_j (J_j: what `objective_values` reports, c_j = column_weights, default 1) in the stored entries of A and B2, in
        the CSC order of `update_plant` — from the multipliers the last execute left and the values it wrote to `d_values`.
        weights=True (plans with updatable_weights=True) appends (gc1[Nx], gd12[Nu]), the derivatives in the two diagonals.
        column_weights: None, or a float64 tensor on the plan's device with n_subproblems values.  Enqueued on `stream` (None =
        the null stream) behind the plan's last execute and update; nothing waits for the device (the plan's first call
        builds the entry tables on the host and does wait)."""
        import torch
        dev = torch.device("cuda", self.info["device"])
        cw = None
        if column_weights is not None:
            if not _is_device_tensor(column_weights) or column_weights.dtype != torch.float64 or column_weights.dim() != 1 or \
                    not column_weights.is_contiguous() or column_weights.numel() != self.info["n_subproblems"]:
                raise ValueError("gradient: column_weights must be a contiguous float64 tensor of n_subproblems values on the plan's device")
            cw = column_weights.data_ptr()
        sizes = [self.m.nnz("A"), self.m.nnz("B2")] + ([int(self.m.dims.Nx), int(self.m.dims.Nu)] if weights else [])
        out = [torch.empty(max(n, 1), dtype=torch.float64, device=dev) for n in sizes]
        ptrs = [a.data_ptr() for a in out] + [None] * (4 - len(out))
        _capi.check(self._lib.sls_plan_gradient(self.handle, stream, d_values, int(packed), cw, *ptrs), self.ctx.handle)
        return tuple(a[:n] for a, n in zip(out, sizes))

    def gradient_values(self, d_values, packed=False, column_weights=None, weights=False):
        """sls_plan_fetch_gradient: the same on the plan's own stream into host arrays — (gA, gB2, n_skipped), with weights=True
        (gA, gB2, gc1, gd12, n_skipped); n_skipped counts the subproblems that contributed 0 because their status is neither
        SLS_COL_OK nor SLS_COL_TRIVIAL.  column_weights: None or n_subproblems host values."""
        dp = C.POINTER(C.c_double)
        cw = None
        if column_weights is not None:
            cw = np.ascontiguousarray(column_weights, dtype=np.float64)
            if cw.ndim != 1 or cw.size != self.info["n_subproblems"]:
                raise ValueError("gradient_values: column_weights needs n_subproblems values")
        sizes = [self.m.nnz("A"), self.m.nnz("B2")] + ([int(self.m.dims.Nx), int(self.m.dims.Nu)] if weights else [])
        out = [np.zeros(max(n, 1)) for n in sizes]
        ptrs = [a.ctypes.data_as(dp) for a in out] + [None] * (4 - len(out))
        ns = C.c_int64()
        _capi.check(self._lib.sls_plan_fetch_gradient(self.handle, d_values, int(packed), None if cw is None else cw.ctypes.data_as(dp),
                                                      *ptrs, C.byref(ns)), self.ctx.handle)
        return tuple(a[:n] for a, n in zip(out, sizes)) + (ns.value,)

    def multipliers(self, sub):
        """sls_plan_fetch_multipliers: μ of subproblem `sub` (col_status order) as the last execute left it, shape (T + 1, ñx):
        block row k of the achievability constraints, rows in s_x order; Eᵀμ = ∇J on the subproblem's free variables."""
        T = self.info["T"]
        n = self._lib.sls_plan_fetch_multipliers(self.handle, int(sub), None, 0)       # the length the call wants, or an error
        if n < 0:
            _capi.check(n, self.ctx.handle)
        buf = np.zeros(max(n, 1))
        _capi.check(self._lib.sls_plan_fetch_multipliers(self.handle, int(sub), buf.ctypes.data_as(C.POINTER(C.c_double)), n), self.ctx.handle)
        return buf[:n].reshape(T + 1, n // (T + 1)).copy()

    def describe(self):
        buf = C.create_string_buffer(4096)
        _capi.check(self._lib.sls_plan_describe(self.handle, buf, len(buf)))
        return buf.value.decode()

    def twisted4_tables(self):
        """sls_plan_debug_twisted4_tables: the prepared records of the plan's four-wave columns, in col_status order, as a dict —
        `caps` (capA, capAc, capB, capBc), `columns` [n], `counts` [n, 4], `bits` [n, 2] (uint64: upward, downward), and per list
        `arow`, `acol`, `brow`, `bcol` a pair (indices, values) of arrays [n, cap, 32] ([n, cap, 64] for bcol).  Raises SLSError
        when the plan has no four-wave launch."""
        f = self._lib.sls_plan_debug_twisted4_tables
        n = C.c_int64(); caps = np.zeros(4, dtype=np.int32)
        i32p, i64p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        _capi.check(f(self.handle, C.byref(n), caps.ctypes.data_as(i32p), None, None, None, None, None), self.ctx.handle)
        n = n.value
        ne = 32 * int(caps[0] + caps[1] + caps[2]) + 64 * int(caps[3])
        cols = np.zeros(n, dtype=np.int64); counts = np.zeros((n, 4), dtype=np.int32); bits = np.zeros((n, 2), dtype=np.uint64)
        idx = np.zeros((n, max(ne, 1)), dtype=np.int32); val = np.zeros((n, max(ne, 1)), dtype=np.float64)
        _capi.check(f(self.handle, C.byref(C.c_int64()), None, cols.ctypes.data_as(i64p), counts.ctypes.data_as(i32p),
                      idx.ctypes.data_as(i32p), val.ctypes.data_as(dp), bits.ctypes.data_as(C.POINTER(C.c_uint64))), self.ctx.handle)
        out = {"caps": tuple(int(c) for c in caps), "columns": cols, "counts": counts, "bits": bits}
        o = 0
        for name, cap, w in (("arow", caps[0], 32), ("acol", caps[1], 32), ("brow", caps[2], 32), ("bcol", caps[3], 64)):
            sl = slice(o, o + int(cap) * w)
            out[name] = (idx[:, sl].reshape(n, int(cap), w), val[:, sl].reshape(n, int(cap), w))
            o += int(cap) * w
        return out

    def twisted4_static(self):
        """sls_plan_debug_twisted4_static: the plan-time static blocks of the plan's four-wave columns, in col_status order, as a
        dict — `delta` [n], `valid` [n, T + 1] (uint8: slots the prepare kernel filled) and `blocks`, a list of n arrays
        [T + 1, TQ, 64] (slot, stored tile q, lane; layout: include/sls_mi355x_debug.h).  Raises SLSError when the plan has no
        four-wave launch or keeps no pool."""
        f = self._lib.sls_plan_debug_twisted4_static
        i32p, i64p, dp, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        n = C.c_int64(); ns = C.c_int32()
        _capi.check(f(self.handle, C.byref(n), C.byref(ns), None, None, None, None), self.ctx.handle)
        n, ns = n.value, ns.value
        off = np.zeros(n + 1, dtype=np.int64)
        _capi.check(f(self.handle, C.byref(C.c_int64()), None, off.ctypes.data_as(i64p), None, None, None), self.ctx.handle)
        delta = np.zeros(n, dtype=np.float64); valid = np.zeros((n, ns), dtype=np.uint8)
        blocks = np.zeros(max(int(off[-1]), 1), dtype=np.float64)
        _capi.check(f(self.handle, C.byref(C.c_int64()), None, None, delta.ctypes.data_as(dp), valid.ctypes.data_as(u8p),
                      blocks.ctypes.data_as(dp)), self.ctx.handle)
        return {"delta": delta, "valid": valid,
                "blocks": [blocks[off[i]:off[i + 1]].reshape(ns, -1, 64).copy() for i in range(n)]}

    def twisted4_images(self):
        """sls_plan_debug_twisted4_images: the plan-time setup images of the plan's four-wave columns, in col_status order, as a
        dict — `Ad`, a list of n arrays [8·TR, 40] (the dense image of Ã the launch holds in LDS), and `wxt`, a list of n arrays
        [T + 1, 32] (the weight table Wx).  Raises SLSError when the plan has no four-wave launch or keeps no pool."""
        f = self._lib.sls_plan_debug_twisted4_images
        i32p, i64p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        n = C.c_int64()
        _capi.check(f(self.handle, C.byref(n), None, None, None), self.ctx.handle)
        n = n.value
        off = np.zeros(n + 1, dtype=np.int64); ad = np.zeros(n, dtype=np.int32)
        _capi.check(f(self.handle, C.byref(C.c_int64()), off.ctypes.data_as(i64p), ad.ctypes.data_as(i32p), None), self.ctx.handle)
        img = np.zeros(max(int(off[-1]), 1), dtype=np.float64)
        _capi.check(f(self.handle, C.byref(C.c_int64()), None, None, img.ctypes.data_as(dp)), self.ctx.handle)
        return {"Ad": [img[off[i]:off[i] + ad[i]].reshape(-1, 40).copy() for i in range(n)],
                "wxt": [img[off[i] + ad[i]:off[i + 1]].reshape(-1, 32).copy() for i in range(n)]}

    def kernel_time_ms(self):
        avg = C.c_double(); n = C.c_int64()
        _capi.check(self._lib.sls_plan_kernel_time_ms(self.handle, C.byref(avg), C.byref(n)), self.ctx.handle)
        return avg.value, n.value

    def download(self, d_values):
        """D2H of a mask-order value array → (list of T arrays for Φx, list of T arrays for Φu)."""
        T = self.info["T"]
        vx = [np.zeros(max(n, 1), dtype=np.float64) for n in self.m.nnz_x]
        vu = [np.zeros(max(n, 1), dtype=np.float64) for n in self.m.nnz_u]
        px = (C.POINTER(C.c_double) * T)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in vx])
        pu = (C.POINTER(C.c_double) * T)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in vu])
        _capi.check(self._lib.sls_plan_download(self.handle, d_values, px, pu), self.ctx.handle)
        return ([a[:n] for a, n in zip(vx, self.m.nnz_x)], [a[:n] for a, n in zip(vu, self.m.nnz_u)])

    def close(self):
        if getattr(self, "handle", None):
            for p in self._owned_values:
                self._lib.sls_plan_free_values(self.handle, p)
            self._owned_values = []
            self._lib.sls_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        # a plan that is still alive when the interpreter shuts down (kept by the traceback of a failed test, say) is left to
        # the process exit: the HIP runtime may already be unloading, and its context may be gone with the streams it lent
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Residual(typing.NamedTuple):
    """What `Plan.residual` returns: per subproblem, in col_status order, `res_inf` (max |Δ| over local and halo rows), `halo_inf`
    (the same over halo rows only) and `res_l1` (Σ|Δ|); `max_inf` = max res_inf and `e1_norm` = max res_l1, the 𝓔₁ norm of Δ."""
    res_inf: np.ndarray
    halo_inf: np.ndarray
    res_l1: np.ndarray
    max_inf: float
    e1_norm: float


def _torch():
    import torch
    return torch


def _is_device_tensor(v):
    t = sys.modules.get("torch")
    return t is not None and isinstance(v, t.Tensor) and v.is_cuda


def _nzval_of(name, v, nnz, m):
    """The nzval array of a host argument of `Plan.update_plant`: a scipy matrix is checked against the plan's stored pattern."""
    if sp.issparse(v):
        M = sp.csc_matrix(v)
        if not M.has_sorted_indices:
            M = M.copy(); M.sort_indices()
        indptr, indices, nrows = m.pattern(name)
        if M.shape != (nrows, indptr.size - 1) or M.nnz != nnz or not np.array_equal(M.indptr, indptr) or \
                not np.array_equal(M.indices, indices):
            raise ValueError(f"update_plant: the stored pattern of {name} differs from the one the plan was built from")
        v = M.data
    nz = np.ascontiguousarray(v, dtype=np.float64)
    if nz.ndim != 1 or nz.size != nnz:
        raise ValueError(f"update_plant: {name} needs {nnz} nzval entries (1-D), got shape {nz.shape}")
    return nz


def _diag_of(name, v, n, shift, nz):
    """The diagonal a host argument of `Plan.update_weights` stands for: a scipy matrix must have the LQR shape."""
    if sp.issparse(v):
        M = sp.csc_matrix(v)
        if not M.has_sorted_indices:
            M = M.copy(); M.sort_indices()
        if M.shape != (nz, n) or M.nnz != n or not np.array_equal(M.indptr, np.arange(n + 1)) or \
                not np.array_equal(M.indices, np.arange(n) + shift):
            raise ValueError(f"update_weights: {name} must be {nz}×{n} with one stored entry per column, column j on row {shift} + j")
        v = M.data
    d = np.ascontiguousarray(v, dtype=np.float64)
    if d.ndim != 1 or d.size != n:
        raise ValueError(f"update_weights: {name} needs the {n} diagonal values (1-D), got shape {d.shape}")
    return d


class _WantObjective:
    """Turns the context's objective option on for one call and restores `off` afterwards (the option is off by default and
    these wrappers leave it as they found it: only calls that ask for the values pay for the evaluation)."""

    def __init__(self, ctx, on):
        self.ctx, self.on = ctx, bool(on)

    def __enter__(self):
        if self.on:
            self.ctx.want_objective(True)
        return self

    def __exit__(self, *a):
        if self.on:
            self.ctx.want_objective(False)

    def into(self, info, n):
        if self.on:
            info["col_objective"], info["objective_total"] = self.ctx.last_objective(n)


def objective_values_host(P, S, vals_x, vals_u, I=None, *, ridge=None, objective="h2", index_base=0, return_bound=False):
    """Host twin of `Plan.objective_values` (sls_debug_objective_host; needs no device): the host symbolic pass over all groups,
    then the same formulas from host value arrays — vals_x[t] / vals_u[t] in the masks' CSC order, as the C ABI fills them.
    ridge = (rx, ru) as `Context.set_ridge` takes them.  Returns (col_objective, total); with return_bound also, per column,
    the number N of products its value sums and the sum S of their absolute values (a summation in another order differs
    by at most 2·N·2⁻⁵³·S)."""
    lib = _capi.load_library()
    Sx, Su = S
    m = _capi.Marshalled(P, Sx, Su, None if I is None else [list(g) for g in I], index_base=index_base, flags=_objective_flags(objective))
    T = len(Sx)
    dp = C.POINTER(C.c_double)
    vx = [np.ascontiguousarray(v, dtype=np.float64) for v in vals_x]
    vu = [np.ascontiguousarray(v, dtype=np.float64) for v in vals_u]
    if [v.size for v in vx] != m.nnz_x or [v.size for v in vu] != m.nnz_u:
        raise ValueError("value arrays do not match the masks' nnz")
    pad = np.zeros(1)
    px = (dp * T)(*[(a if a.size else pad).ctypes.data_as(dp) for a in vx])
    pu = (dp * T)(*[(a if a.size else pad).ctypes.data_as(dp) for a in vu])
    rx, ru = (None, None) if ridge is None else ridge
    rx = None if rx is None else np.ascontiguousarray(rx, dtype=np.float64)
    ru = None if ru is None else np.ascontiguousarray(ru, dtype=np.float64)
    n = m.n_sub
    col = np.zeros(max(n, 1)); cabs = np.zeros(max(n, 1)); cn = np.zeros(max(n, 1), dtype=np.int64)
    tot = C.c_double()
    _capi.check(lib.sls_debug_objective_host(*m.common_args(), None if rx is None else rx.ctypes.data_as(dp),
                                             None if ru is None else ru.ctypes.data_as(dp), px, pu, col.ctypes.data_as(dp),
                                             C.byref(tot), cn.ctypes.data_as(C.POINTER(C.c_int64)), cabs.ctypes.data_as(dp)))
    if return_bound:
        return col[:n], tot.value, cn[:n], cabs[:n]
    return col[:n], tot.value


def residual_host(P, S, vals_x, vals_u, I=None, *, index_base=0, return_bound=False, return_halo=False):
    """Host twin of `Plan.residual` (sls_debug_residual_host; needs no device): the host symbolic pass over all groups, then the
    same formulas from host value arrays — vals_x[t] / vals_u[t] in the masks' CSC order — against P.A and P.B2, accumulated in
    long double.  Returns a `Residual`; with return_bound also a dict of what a summation-order bound 2·N·2⁻⁵³·S needs, per
    column: `ent_terms` / `ent_abs` (N and S that bound every entry of Δ, hence res_inf and halo_inf) and `l1_terms` / `l1_abs`
    (N and S of res_l1); with return_halo also the list of halo row arrays H(q) (0-based, ascending)."""
    lib = _capi.load_library()
    Sx, Su = S
    m = _capi.Marshalled(P, Sx, Su, None if I is None else [list(g) for g in I], index_base=index_base)
    T = len(Sx)
    dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    vx = [np.ascontiguousarray(v, dtype=np.float64) for v in vals_x]
    vu = [np.ascontiguousarray(v, dtype=np.float64) for v in vals_u]
    if [v.size for v in vx] != m.nnz_x or [v.size for v in vu] != m.nnz_u:
        raise ValueError("value arrays do not match the masks' nnz")
    pad = np.zeros(1)
    px = (dp * T)(*[(a if a.size else pad).ctypes.data_as(dp) for a in vx])
    pu = (dp * T)(*[(a if a.size else pad).ctypes.data_as(dp) for a in vu])
    n = m.n_sub
    out = [np.zeros(max(n, 1)) for _ in range(3)]
    tot = np.zeros(2)
    et, lt = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    ea, la = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    hp = np.zeros(n + 1, dtype=np.int64)

    def call(rows):
        _capi.check(lib.sls_debug_residual_host(*m.common_args(), px, pu, *[a.ctypes.data_as(dp) for a in out], tot.ctypes.data_as(dp),
                                                et.ctypes.data_as(i64p), ea.ctypes.data_as(dp), lt.ctypes.data_as(i64p),
                                                la.ctypes.data_as(dp), hp.ctypes.data_as(i64p),
                                                None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                                0 if rows is None else rows.size))
    call(None)
    res = [Residual(out[0][:n], out[1][:n], out[2][:n], float(tot[0]), float(tot[1]))]
    if return_bound:
        res.append({"ent_terms": et[:n], "ent_abs": ea[:n], "l1_terms": lt[:n], "l1_abs": la[:n]})
    if return_halo:
        rows = np.zeros(max(int(hp[n]), 1), dtype=np.int32)
        call(rows)
        res.append([rows[hp[q]:hp[q + 1]].copy() for q in range(n)])
    return res[0] if len(res) == 1 else tuple(res)


def assemble_phi(Sx, Su, vals_x, vals_u, dropzeros=True):
    """Φx[t] = SparseMatrixCSC(Nx,Nx, 𝓢x[t].colptr, 𝓢x[t].rowval, vals) (+ dropzeros!, which is what the
    reference's sparse `+` accumulation does to numerical zeros: src/synthesis.jl:65-67)."""
    def build(Sm, v):
        Sm = sp.csc_matrix(Sm)
        if not Sm.has_sorted_indices:
            Sm = Sm.copy(); Sm.sort_indices()
        M = sp.csc_matrix((np.asarray(v, dtype=np.float64).copy(), Sm.indices.copy(), Sm.indptr.copy()), shape=Sm.shape)
        if dropzeros:
            M.eliminate_zeros()
        return M
    return [build(s, v) for s, v in zip(Sx, vals_x)], [build(s, v) for s, v in zip(Su, vals_u)]


def execute_batch(plans, d_values, packed=False, stream=None):
    """Several independent plants in one call (sls_plan_execute_batch): plan i writes d_values[i]; the launches overlap on the
    device, `stream` (None = the null stream) sees all results.  The reference's counterpart is one SLS_𝓗₂ call per plant."""
    n = len(plans)
    if n != len(d_values):
        raise ValueError("one value array per plan")
    if n == 0:
        return
    hp = (C.c_void_p * n)(*[p.handle for p in plans])
    dv = (C.c_void_p * n)(*[int(v) for v in d_values])
    _capi.check(plans[0]._lib.sls_plan_execute_batch(hp, n, stream, dv, int(packed)), plans[0].ctx.handle)


def SLS_H2_batch(plants, masks, *, ctx: Context | None = None, return_info=False, dropzeros=True, objective="h2", index_base=0,
                 return_objective=False):
    """[(Φx, Φu) for each plant] = one sls_h2_sf_solve_batch call over independent plants that share T: a loop of reference
    `SLS_𝓗₂(P, 𝓢)` calls (src/synthesis.jl:11) run as ONE set of kernel launches (the block-diagonal composite plant)."""
    n = len(plants)
    if n == 0 or n != len(masks):
        raise ValueError("one [𝓢x, 𝓢u] per plant")
    ctx = ctx or default_context()
    lib = ctx._lib
    ms = [_capi.Marshalled(P, S[0], S[1], None, index_base=index_base, flags=_objective_flags(objective)) for P, S in zip(plants, masks)]
    T = len(masks[0][0])
    dims = (_capi.sls_dims * n)(*[m.dims for m in ms])
    pl = (_capi.sls_plant * n)(*[m.plant for m in ms])
    bp = C.POINTER(_capi.sls_csc_bool)
    sx = (bp * n)(*[C.cast(m.Sx, bp) for m in ms]); su = (bp * n)(*[C.cast(m.Su, bp) for m in ms])
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    dpp = C.POINTER(dp)
    vals, keep = [], []
    pxs, pus, sts = (dpp * n)(), (dpp * n)(), (i32p * n)()
    status = []
    for i, m in enumerate(ms):
        vx = [np.zeros(max(k, 1), dtype=np.float64) for k in m.nnz_x]
        vu = [np.zeros(max(k, 1), dtype=np.float64) for k in m.nnz_u]
        px = (dp * T)(*[a.ctypes.data_as(dp) for a in vx]); pu = (dp * T)(*[a.ctypes.data_as(dp) for a in vu])
        st = np.zeros(max(m.n_sub, 1), dtype=np.int32)
        keep += [px, pu]
        pxs[i] = C.cast(px, dpp); pus[i] = C.cast(pu, dpp); sts[i] = st.ctypes.data_as(i32p)
        vals.append((vx, vu)); status.append(st)
    stats = _capi.sls_stats()
    with _WantObjective(ctx, return_objective) as wo:
        rc = lib.sls_h2_sf_solve_batch(ctx.handle, n, dims, pl, sx, su, pxs, pus, sts, C.byref(stats))
        _capi.check(rc, ctx.handle)
        obj = {}
        wo.into(obj, sum(m.n_sub for m in ms))
    out = []
    for m, S, (vx, vu) in zip(ms, masks, vals):
        out.append(assemble_phi(S[0], S[1], [a[:k] for a, k in zip(vx, m.nnz_x)], [a[:k] for a, k in zip(vu, m.nnz_u)],
                                dropzeros=dropzeros))
    if return_info:
        info = stats.asdict()
        info["col_status"] = [st[: m.n_sub].copy() for st, m in zip(status, ms)]
        info["n_unsolved"] = rc
        if return_objective:          # composite order cut back into one array per plant
            cuts = np.cumsum([0] + [m.n_sub for m in ms])
            info["col_objective"] = [obj["col_objective"][a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
            info["objective_total"] = obj["objective_total"]
        return out, info
    if rc > 0:
        warnings.warn(f"SLS_H2_batch: {rc} subproblems not solved — pass return_info=True for the per-column status",
                      RuntimeWarning, stacklevel=2)
    return out


def SLS_H2_localized(P, d, T, alpha, *, ctx: Context | None = None, return_info=False, dropzeros=True, objective="h2", index_base=0,
                     return_objective=False):
    """Φx, Φu = SLS_𝓗₂(P, [𝓢x, 𝓢u]) for the README's own masks (README.md:52-54), given as (d, T, α) instead of 2T sparse
    matrices: sls_h2_sf_solve_localized builds index sets, mask slices and destinations on the device.  The patterns needed to
    return Φ as sparse matrices are fetched with the device mask recipe (row indices only come down)."""
    if not isinstance(P, GeneralizedPlant) or P.Ts is not StateFeedback:
        return None
    from .workloads import localization_masks_native
    ctx = ctx or default_context()
    lib = ctx._lib
    Sx, Su = localization_masks_native(P.A, P.B2, d, T, alpha, ctx=ctx)
    empty = []
    m = _capi.Marshalled(P, empty, empty, None, index_base=index_base, flags=_objective_flags(objective))
    m.dims.T = int(T)
    nnz_x = [int(M.nnz) for M in Sx]; nnz_u = [int(M.nnz) for M in Su]
    vx = [np.zeros(max(n, 1), dtype=np.float64) for n in nnz_x]
    vu = [np.zeros(max(n, 1), dtype=np.float64) for n in nnz_u]
    px = (C.POINTER(C.c_double) * T)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in vx])
    pu = (C.POINTER(C.c_double) * T)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in vu])
    status = np.zeros(max(P.Nx, 1), dtype=np.int32)
    stats = _capi.sls_stats()
    with _WantObjective(ctx, return_objective) as wo:
        rc = lib.sls_h2_sf_solve_localized(ctx.handle, C.byref(m.dims), C.byref(m.plant), int(d), float(alpha), px, pu,
                                           status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(stats))
        _capi.check(rc, ctx.handle)
        st = stats.asdict()
        wo.into(st, P.Nx)
    if st["n_values_x"] != sum(nnz_x) or st["n_values_u"] != sum(nnz_u):
        raise RuntimeError("device symbolic route and device mask recipe disagree on the pattern sizes")
    Phix, Phiu = assemble_phi(Sx, Su, [a[:n] for a, n in zip(vx, nnz_x)], [a[:n] for a, n in zip(vu, nnz_u)], dropzeros=dropzeros)
    if return_info:
        st["col_status"] = status[: P.Nx].copy()
        st["n_unsolved"] = rc
        return Phix, Phiu, st
    if rc > 0:
        warnings.warn(f"SLS_H2_localized: {rc} of {P.Nx} subproblems not solved — pass return_info=True for the per-column status",
                      RuntimeWarning, stacklevel=2)
    return Phix, Phiu


def _plan_flags(objective, updatable_weights, multipliers=False):
    return _objective_flags(objective) | (_capi.SLS_PLAN_WEIGHTS_UPDATABLE if updatable_weights else 0) | \
        (_capi.SLS_PLAN_MULTIPLIERS if multipliers else 0)


def _objective_flags(objective):
    if objective in ("h2", None):
        return _capi.SLS_SOLVE_DEFAULT
    if objective == "sum_of_norms":
        return _capi.SLS_SOLVE_SUM_OF_NORMS
    raise ValueError(f"unknown objective {objective!r}")


def SLS_Hinf_bound(P, S, I=None, **kw):
    """Φx, Φu minimising, per column, Σ_t ‖[C̃1 D̃12]Φ̃[t]B̃1‖₂ — the column-separable bound of the 𝓗∞ norm — over the same
    localized constraints as SLS_𝓗₂ (SLS_SOLVE_SUM_OF_NORMS).  NOT in the reference: it has no 𝓗∞ synthesis;
    BASELINE.json configs[3] names one.  Diagonal weights, D11 = 0."""
    return SLS_H2(P, S, I, objective="sum_of_norms", **kw)


def SLS_H2(P, S, I=None, *, ctx: Context | None = None, return_info=False, dropzeros=True, index_base=0, objective="h2",
           return_objective=False):
    """Φx, Φu = SLS_𝓗₂(P, [𝓢x, 𝓢u]; 𝓘)   — drop-in for reference src/synthesis.jl:11.

    P : GeneralizedPlant (state feedback).  Any other feedback structure returns None,
        exactly like the reference (src/synthesis.jl:13,30-32).
    S : [𝓢x, 𝓢u], two length-T lists of boolean sparse matrices (Nx×Nx, Nu×Nx).
    I : optional list of column groups (0-based column indices, ascending inside a group).
    index_base : 0, or 1 to marshal every index array the way Julia stores it (what the `ccall` binding hands over).
    return_objective : with return_info, `info` also carries `col_objective` (the objective value every subproblem achieved,
        in col_status order, evaluated on the device before the download) and `objective_total` (their sum: the squared 𝓗₂
        norm of the closed loop).  Not defined for a group list with overlapping groups (SLS_EUNSUPPORTED).
    Returns two length-T lists of scipy CSC matrices (Φx[t] Nx×Nx, Φu[t] Nu×Nx).
    """
    if not isinstance(P, GeneralizedPlant) or P.Ts is not StateFeedback:
        return None
    Sx, Su = S
    ctx = ctx or default_context()
    lib = ctx._lib
    m = _capi.Marshalled(P, Sx, Su, None if I is None else [list(g) for g in I], index_base=index_base,
                         flags=_objective_flags(objective))
    T = len(Sx)
    vx = [np.zeros(max(n, 1), dtype=np.float64) for n in m.nnz_x]
    vu = [np.zeros(max(n, 1), dtype=np.float64) for n in m.nnz_u]
    px = (C.POINTER(C.c_double) * T)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in vx])
    pu = (C.POINTER(C.c_double) * T)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in vu])
    status = np.zeros(max(m.n_sub, 1), dtype=np.int32)
    stats = _capi.sls_stats()
    obj = {}
    with _WantObjective(ctx, return_objective) as wo:
        rc = lib.sls_h2_sf_solve(ctx.handle, *m.common_args(), px, pu,
                                 status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(stats))
        _capi.check(rc, ctx.handle)
        wo.into(obj, m.n_sub)
    Phix, Phiu = assemble_phi(Sx, Su, [a[:n] for a, n in zip(vx, m.nnz_x)],
                              [a[:n] for a, n in zip(vu, m.nnz_u)], dropzeros=dropzeros)
    if return_info:
        info = stats.asdict()
        info["col_status"] = status[: m.n_sub].copy()
        info["n_unsolved"] = rc
        info.update(obj)
        return Phix, Phiu, info
    if rc > 0:
        # the reference never checks Ipopt's status (src/synthesis.jl:62-65); a caller that does not ask for the per-column
        # status words still gets a signal, like julia/SLSMI355X.jl's @warn
        st = status[: m.n_sub]
        n_uns = int((st == _capi.SLS_COL_UNSUPPORTED).sum())
        warnings.warn(f"SLS_H2: {rc} of {m.n_sub} subproblems not solved "
                      f"({int((st == _capi.SLS_COL_INFEASIBLE).sum())} infeasible, "
                      f"{int((st == _capi.SLS_COL_NOTCONV).sum())} not converged, {n_uns} unsupported); "
                      "their columns hold the least-squares point (zeros if unsupported) — "
                      "pass return_info=True for the per-column status", RuntimeWarning, stacklevel=2)
    return Phix, Phiu
