"""Closed-loop rollout of the Φ that lives on the device against an ensemble of plants: how a design behaves on plants that
are not the design model.

    ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
    u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
    β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}
    x_{k+1} = A⁽ˢ⁾·x_k + B₁·w_k + B₂⁽ˢ⁾·u_k
    J⁽ˢ⁾   += Σ_i (q_i·x_k[i])² + Σ_j (r_j·u_k[j])²         peak_x⁽ˢ⁾ = max(peak_x⁽ˢ⁾, max_i |x_k[i]|), peak_u likewise

Every scenario s has its own values of A and B₂ on the plan's non-zero patterns; B₁ and Φ are shared.  `ClosedLoop` keeps one plant
and every step of x, u, ŵ; `Controller` has no plant at all.  Here the plant steps on the device with the controller, the running
cost and the peaks are accumulated there, and memory does not depend on the number of steps.  The rollout runs in
libsls_mi355x.so (sls_rollout_*: one HIP kernel per step); this module only marshals.  No CPU fallback: `rollout_host` /
`rollout_tables` are the diagnostic host twin the tests compare against, not a second backend.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import _dev_ptr, _is_tensor, plant_value_args

_dp = C.POINTER(C.c_double)


class Rollout:
    """sls_rollout_plan on one device of `ctx`: the simulator's operator from the masks, the plant patterns and initial values
    from P (A, B1, B2), and all state for `nscen` scenarios.  Weights start at q = r = 1 (`from_plant` takes them from P)."""

    def __init__(self, ctx, P, S, nscen=1, dev_slot=0, index_base=0):
        Sx, Su = S
        self.ctx, self._lib = ctx, ctx._lib
        self.Nx, self.Nu, self.Nw, self.T, self.nscen = int(P.Nx), int(P.Nu), int(P.Nw), len(Sx), int(nscen)
        self.device = ctx.devices[dev_slot] if 0 <= dev_slot < len(ctx.devices) else None
        self.m = _capi.Marshalled(P, Sx, Su, None, index_base=index_base)
        self.nnz_A, self.nnz_B2 = self.m.nnz("A"), self.m.nnz("B2")
        h = C.c_void_p()
        _capi.check(self._lib.sls_rollout_plan(ctx.handle, dev_slot, C.byref(self.m.dims), C.byref(self.m.plant), self.m.Sx, self.m.Su,
                                               self.nscen, C.byref(h)), ctx.handle)
        self.handle = h
        self.n_entries, _, self.state_bytes, self.plant_bytes = self._info()

    @classmethod
    def from_plant(cls, ctx, P, S, nscen=1, dev_slot=0, index_base=0):
        """A rollout whose weights are the LQR diagonals of P: C1 = [diag(q); 0], D12 = [0; diag(r)] (the shape rule
        of SLS_PLAN_WEIGHTS_UPDATABLE).  ValueError when P does not have that form."""
        m = _capi.Marshalled(P, [], [], None, index_base=index_base)
        diag = np.zeros(max(P.Nx + P.Nu, 1))
        rc = _capi.load_library().sls_debug_weights_shape_check(C.byref(m.dims), C.byref(m.plant), diag.ctypes.data_as(_dp))
        if rc != 0:
            raise ValueError("Rollout.from_plant: the plant is not in the LQR form C1 = [diag(q); 0], D12 = [0; diag(r)]: " + _capi.last_error(None))
        self = cls(ctx, P, S, nscen=nscen, dev_slot=dev_slot, index_base=index_base)
        self.set_weights(diag[: P.Nx], diag[P.Nx: P.Nx + P.Nu])
        return self

    def _info(self):
        n, k, b, pb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(self._lib.sls_rollout_info(self.handle, C.byref(n), C.byref(k), C.byref(b), C.byref(pb)))
        return n.value, k.value, b.value, pb.value

    @property
    def k(self):
        """steps enqueued since the last reset"""
        return self._info()[1]

    def load(self, d_values, stream=None):
        """Φ from the mask-order device array `Plan.execute(packed=False)` fills (tensor or pointer); state, cost and k stay."""
        if _is_tensor(d_values):
            d_values = d_values.data_ptr()
        _capi.check(self._lib.sls_rollout_load(self.handle, stream, d_values), self.ctx.handle)

    def set_plant(self, A=None, B2=None, per_scenario=False, stream=None):
        """New plant values in the CSC nzval order of the plan's A / B2 (what `Plan.plant_values()` returns): each None (kept), a
        host array, or a device tensor (both must then be tensors, or one None).  per_scenario=False: nnz values for all
        scenarios; True: [nnz, nscen].  The values are not validated."""
        args = plant_value_args(A, B2, self.nnz_A, self.nnz_B2, self.nscen, per_scenario)
        if args is None:
            return
        pA, pB2, on_device, _keep = args
        _capi.check(self._lib.sls_rollout_set_plant(self.handle, stream, pA, pB2, on_device, int(bool(per_scenario))), self.ctx.handle)

    def set_weights(self, q=None, r=None, stream=None):
        """q [Nx], r [Nu]: each None (kept), a host array or a device tensor — `Plan.weights()` can be passed as it is"""
        given = [(name, v, n) for name, v, n in (("q", q, self.Nx), ("r", r, self.Nu)) if v is not None]
        if not given:
            return
        dev = [_is_tensor(v) for _, v, _ in given]
        if any(dev) != all(dev):
            raise ValueError("set_weights: q and r must both be host arrays or both be device tensors")
        ptrs, keep = {"q": None, "r": None}, []
        for name, v, n in given:
            if dev[0]:
                ptrs[name] = _dev_ptr(v, n, f"set_weights: {name}")
            else:
                a = np.ascontiguousarray(v, dtype=np.float64)
                if a.size != n:
                    raise ValueError(f"set_weights: {name} has {a.size} values, expected {n}")
                keep.append(a)
                ptrs[name] = a.ctypes.data if n else None
        _capi.check(self._lib.sls_rollout_set_weights(self.handle, stream, ptrs["q"], ptrs["r"], int(dev[0])), self.ctx.handle)

    def reset(self, x0=None, stream=None):
        """ring, β, cost, peaks and k cleared; x0 [Nx, nscen] (device tensor or pointer) or None for 0"""
        _capi.check(self._lib.sls_rollout_reset(self.handle, stream, _dev_ptr(x0, self.Nx * self.nscen, "x0")), self.ctx.handle)

    def run(self, steps, w=None, x=None, u=None, stream=None):
        """`steps` steps from the current state, enqueued on `stream` (None = the null stream); nothing waits.  w [steps, Nw,
        nscen] or None; x [steps, Nx, nscen] / u [steps, Nu, nscen] record x_k, u_k when given (device tensors or pointers)."""
        steps = int(steps)
        _capi.check(self._lib.sls_rollout_run(self.handle, stream, _dev_ptr(w, steps * self.Nw * self.nscen, "w"), steps,
                                              _dev_ptr(x, steps * self.Nx * self.nscen, "x"), _dev_ptr(u, steps * self.Nu * self.nscen, "u")),
                    self.ctx.handle)

    def stats_async(self, cost=None, peak_x=None, peak_u=None, stream=None):
        """sls_rollout_stats into device tensors / pointers of nscen doubles (each optional), enqueued on `stream`"""
        _capi.check(self._lib.sls_rollout_stats(self.handle, stream, *(_dev_ptr(a, self.nscen, n) for a, n in
                                                                      ((cost, "cost"), (peak_x, "peak_x"), (peak_u, "peak_u")))),
                    self.ctx.handle)

    def _fetch(self, stream, want_x, want_stats):
        xs = np.zeros((self.Nx, self.nscen)) if want_x else None
        out = [np.zeros(self.nscen) for _ in range(3)] if want_stats else [None] * 3
        p = lambda a: None if a is None else a.ctypes.data_as(_dp)
        _capi.check(self._lib.sls_rollout_fetch(self.handle, stream, p(xs), p(out[0]), p(out[1]), p(out[2])), self.ctx.handle)
        return xs, out

    def stats(self, stream=None):
        """(cost, peak_x, peak_u): host arrays [nscen] over the steps run since the last reset; waits for `stream`"""
        return tuple(self._fetch(stream, False, True)[1])

    def state(self, stream=None):
        """x_K [Nx, nscen], the current state (host array); waits for `stream`"""
        return self._fetch(stream, True, False)[0]

    def close(self):
        if getattr(self, "handle", None):
            self._lib.sls_rollout_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rollout_tables(P, S, index_base=0):
    """sls_debug_rollout_tables (needs no device): a dict with n_entries, A_ptr / A_idx / A_src, B2_ptr / B2_idx / B2_src (CSR
    entry → position in the CSC nzval array), B2_owner (1 where the entry's row counts u_j) and orphan (actuators with an empty
    B2 column)."""
    m = _capi.Marshalled(P, S[0], S[1], None, index_base=index_base)
    lib = _capi.load_library()
    nA, nB = m.nnz("A"), m.nnz("B2")
    ne, no = C.c_int64(), C.c_int64()
    i32 = lambda n: np.zeros(max(n, 1), dtype=np.int32)
    t = dict(A_ptr=i32(P.Nx + 1), A_idx=i32(nA), A_src=i32(nA), B2_ptr=i32(P.Nx + 1), B2_idx=i32(nB), B2_src=i32(nB),
             B2_owner=np.zeros(max(nB, 1), dtype=np.uint8), orphan=i32(P.Nu))
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    _capi.check(lib.sls_debug_rollout_tables(C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, C.byref(ne), C.byref(no),
                                             *(t[k].ctypes.data_as(bp if k == "B2_owner" else ip) for k in
                                               ("A_ptr", "A_idx", "A_src", "B2_ptr", "B2_idx", "B2_src", "B2_owner", "orphan"))))
    for k, n in (("A_idx", nA), ("A_src", nA), ("B2_idx", nB), ("B2_src", nB), ("B2_owner", nB), ("orphan", no.value)):
        t[k] = t[k][:n]
    t["n_entries"] = ne.value
    return t


def rollout_host(P, S, values, nscen, steps, w=None, A=None, B2=None, per_scenario=False, q=None, r=None, x0=None, chunks=None,
                 switch=None, index_base=0):
    """sls_debug_rollout_host (needs no device): the host twin of plan → load(values) → set_plant(A, B2, per_scenario) →
    set_weights(q, r) → reset(x0) → `steps` steps, as one run or as runs of `chunks` steps.  switch = (k, values2): Φ = values2
    from step k on, state kept.  Host arrays in the layouts of `Rollout`.  Returns a dict: x [steps, Nx, nscen], u [steps, Nu,
    nscen], state [Nx, nscen], cost, peak_x, peak_u [nscen]."""
    m = _capi.Marshalled(P, S[0], S[1], None, index_base=index_base)
    Nx, Nu, Nw = int(P.Nx), int(P.Nu), int(P.Nw)
    keep = []

    def arr(a, n, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != n:
            raise ValueError(f"rollout_host: {what} has {a.size} values, expected {n}")
        keep.append(a)
        return a.ctypes.data_as(_dp)

    per = nscen if per_scenario else 1
    ch = None if chunks is None else np.ascontiguousarray(chunks, dtype=np.int64)
    x, u = np.zeros((steps, Nx, nscen)), np.zeros((steps, max(Nu, 1), nscen))
    xe, cost, px, pu = np.zeros((Nx, nscen)), np.zeros(nscen), np.zeros(nscen), np.zeros(nscen)
    o = lambda a: a.ctypes.data_as(_dp)
    _capi.check(_capi.load_library().sls_debug_rollout_host(
        C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, arr(values, len(np.asarray(values)), "values"), int(nscen),
        arr(A, m.nnz("A") * per, "A"), arr(B2, m.nnz("B2") * per, "B2"), int(bool(per_scenario)), arr(q, Nx, "q"), arr(r, Nu, "r"),
        arr(x0, Nx * nscen, "x0"), arr(w, steps * Nw * nscen, "w"), int(steps),
        None if ch is None else ch.ctypes.data_as(C.POINTER(C.c_int64)), 0 if ch is None else len(ch),
        None if switch is None else arr(switch[1], len(np.asarray(values)), "switch values"), 0 if switch is None else int(switch[0]),
        o(x), o(u), o(xe), o(cost), o(px), o(pu)))
    return dict(x=x, u=u[:, :Nu] if Nu else np.zeros((steps, 0, nscen)), state=xe, cost=cost, peak_x=px, peak_u=pu)
