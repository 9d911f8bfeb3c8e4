"""The stand-alone SLS controller: one step from a measured state to u, with the Φ that lives on the device.

    ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
    u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
    β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}

`ClosedLoop` fuses these two sums with one fixed linear plant; here the state comes from the caller, so the plant may be
anything — the design model perturbed, a torch model, a measurement — and Φ may be reloaded under a running controller.
The step runs in libsls_mi355x.so (sls_controller_*: one HIP kernel per step); this module only marshals.  No CPU fallback:
`controller_host` / `controller_tables` are the diagnostic host twin the tests compare against, not a second backend.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import _dev_ptr, _is_tensor


def _dims_of(P_or_dims):
    """(Nx, Nu) of a Plant-like object or of a pair"""
    if hasattr(P_or_dims, "Nx") and hasattr(P_or_dims, "Nu"):
        return int(P_or_dims.Nx), int(P_or_dims.Nu)
    Nx, Nu = P_or_dims
    return int(Nx), int(Nu)


class Controller:
    """Row-oriented FIR operator of the controller built from the masks alone (sls_controller_plan) on one device of `ctx`,
    with its state — β and the history of ŵ — for `nscen` scenarios.  P_or_dims: a Plant (only Nx, Nu are read) or (Nx, Nu)."""

    def __init__(self, ctx, P_or_dims, S, nscen=1, dev_slot=0, index_base=0):
        Sx, Su = S
        self.ctx, self._lib = ctx, ctx._lib
        self.Nx, self.Nu = _dims_of(P_or_dims)
        self.T, self.nscen = len(Sx), int(nscen)
        self.device = ctx.devices[dev_slot] if 0 <= dev_slot < len(ctx.devices) else None
        self.m = _capi.Marshalled.masks_only(self.Nx, self.Nu, Sx, Su, index_base)
        h = C.c_void_p()
        _capi.check(self._lib.sls_controller_plan(ctx.handle, dev_slot, C.byref(self.m.dims), self.m.Sx, self.m.Su, self.nscen,
                                                  C.byref(h)), ctx.handle)
        self.handle = h
        self.n_entries, _, self.state_bytes = self._info()
        self._u = None

    def _info(self):
        n, k, b = C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(self._lib.sls_controller_info(self.handle, C.byref(n), C.byref(k), C.byref(b)))
        return n.value, k.value, b.value

    @property
    def k(self):
        """steps enqueued since the last reset"""
        return self._info()[1]

    def load(self, d_values, stream=None):
        """Φ from the mask-order device array `Plan.execute(packed=False)` fills (tensor or pointer); β, the history and k stay."""
        if _is_tensor(d_values):
            d_values = d_values.data_ptr()
        _capi.check(self._lib.sls_controller_load(self.handle, stream, d_values), self.ctx.handle)

    def reset(self, stream=None):
        """β = 0, history = 0, k = 0"""
        _capi.check(self._lib.sls_controller_reset(self.handle, stream), self.ctx.handle)

    def step(self, x, u=None, what=None, stream=None):
        """x [Nx, nscen] in, u [Nu, nscen] out (and ŵ_k into `what` [Nx, nscen] when given): device torch tensors or raw device
        pointers.  Enqueued on `stream` (a raw stream handle; None = the null stream); nothing waits.  Returns `u`; when none is
        given, a tensor allocated once and reused by later calls."""
        if u is None and self.Nu > 0:
            if self._u is None:
                import torch
                self._u = torch.empty((self.Nu, self.nscen), dtype=torch.float64, device=torch.device("cuda", self.device))
            u = self._u
        _capi.check(self._lib.sls_controller_step(self.handle, stream, _dev_ptr(x, self.Nx * self.nscen, "x"),
                                                  _dev_ptr(u, self.Nu * self.nscen, "u"), _dev_ptr(what, self.Nx * self.nscen, "what")),
                    self.ctx.handle)
        return u

    def close(self):
        if getattr(self, "handle", None):
            self._lib.sls_controller_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def controller_tables(P_or_dims, S, index_base=0):
    """sls_debug_controller_tables (needs no device): (row_ptr [Nx+Nu+1], lag [n], col [n], perm [n]) of the controller's
    operator — β rows then u rows, entries ascending in (lag, col); lag 1-based, col 0-based, perm into the mask-order array."""
    Nx, Nu = _dims_of(P_or_dims)
    m = _capi.Marshalled.masks_only(Nx, Nu, S[0], S[1], index_base)
    lib = _capi.load_library()
    n = C.c_int64()
    _capi.check(lib.sls_debug_controller_tables(C.byref(m.dims), m.Sx, m.Su, C.byref(n), None, None, None, None))
    row_ptr = np.zeros(Nx + Nu + 1, dtype=np.int32)
    lag, col, perm = (np.zeros(max(n.value, 1), dtype=np.int32) for _ in range(3))
    ip = C.POINTER(C.c_int32)
    _capi.check(lib.sls_debug_controller_tables(C.byref(m.dims), m.Sx, m.Su, C.byref(n), row_ptr.ctypes.data_as(ip),
                                                lag.ctypes.data_as(ip), col.ctypes.data_as(ip), perm.ctypes.data_as(ip)))
    return row_ptr, lag[: n.value], col[: n.value], perm[: n.value]


def controller_host(P_or_dims, S, values, x, index_base=0):
    """sls_debug_controller_host (needs no device): the host twin of `len(x)` steps from the reset state.  values: Φ in mask
    order (host); x [steps, Nx, nscen].  Returns (u [steps, Nu, nscen], ŵ [steps, Nx, nscen])."""
    Nx, Nu = _dims_of(P_or_dims)
    m = _capi.Marshalled.masks_only(Nx, Nu, S[0], S[1], index_base)
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] != Nx:
        raise ValueError(f"x must be [steps, Nx={Nx}, nscen], got {x.shape}")
    steps, _, nscen = x.shape
    values = np.ascontiguousarray(values, dtype=np.float64)
    u, what = np.zeros((steps, max(Nu, 1), nscen)), np.zeros((steps, Nx, nscen))
    dp = C.POINTER(C.c_double)
    _capi.check(_capi.load_library().sls_debug_controller_host(C.byref(m.dims), m.Sx, m.Su, values.ctypes.data_as(dp), nscen, steps,
                                                              x.ctypes.data_as(dp), u.ctypes.data_as(dp), what.ctypes.data_as(dp)))
    return u[:, :Nu] if Nu else np.zeros((steps, 0, nscen)), what
