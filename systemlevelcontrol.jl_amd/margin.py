"""Robust-stability margins of the Φ that lives on the device for an ensemble of plants: for which plants is the loop guaranteed
stable, and how much can it amplify a bounded disturbance.

The controller (`Controller`: ŵ_k = x_k − β_k, Φx[0] taken as I) on plant s, x_{k+1} = A⁽ˢ⁾·x_k + B₂⁽ˢ⁾·u_k + w̃_k, obeys exactly

    ŵ_{k+1} = w̃_k − Σ_{τ=0..T−1} D⁽ˢ⁾[τ]·ŵ_{k−τ}
    D⁽ˢ⁾[τ] = Φx[τ+1] − A⁽ˢ⁾·Φx[τ] − B₂⁽ˢ⁾·Φu[τ]            (0-based slices; Φx[0] := I, Φx[T] := 0)

with x = Φx ∗ ŵ, u = Φu ∗ ŵ.  The loop is internally stable when ‖D⁽ˢ⁾‖ < 1 in an induced norm — ‖D‖_𝓛₁ = max_i Σ_τ Σ_j |D[τ][i,j]|
or ‖D‖_𝓔₁ = max_j Σ_τ Σ_i |D[τ][i,j]| — and then ‖ŵ‖∞ ≤ ‖w̃‖∞ / (1 − ‖D‖_𝓛₁), so every 𝓛₁ bound of `ClosedLoopNorms.l1` degrades by
at most that factor.  `Rollout` shows what happens for given disturbances; this is the certificate.  Every scenario has its own
values of A and B₂ on the plan's non-zero patterns; Φ is shared.  The passes run in libsls_mi355x.so (sls_margin_*: HIP
kernels); this module only marshals.  No CPU fallback: `margin_host` / `margin_tables` are the diagnostic host twin the tests
compare against, not a second backend.

`set_radius` / `box_margins` / `worst_plant` answer the same question for a SET of plants: every stored coefficient known to ± a
radius, the exact worst ‖D‖_𝓛₁ over the box from the vertices of each row (sls_margin_box_*; `margin_box_host` is its twin).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import _dev_ptr, _is_tensor, plant_value_args

_dp = C.POINTER(C.c_double)


class RobustMargin:
    """sls_margin_plan on one device of `ctx`: the patterns and initial values of A and B₂ from P, Φ's pattern from the masks, and
    every buffer for `nscen` scenarios (`device_bytes` in all, the scratch of 8·n_defect·nscen B included)."""

    def __init__(self, ctx, P, S, nscen=1, dev_slot=0, index_base=0):
        Sx, Su = S
        self.ctx, self._lib = ctx, ctx._lib
        self.Nx, self.Nu, self.T, self.nscen = int(P.Nx), int(P.Nu), len(Sx), int(nscen)
        self.device = ctx.devices[dev_slot] if 0 <= dev_slot < len(ctx.devices) else None
        self.m = _capi.Marshalled(P, Sx, Su, None, index_base=index_base)
        self.nnz_A, self.nnz_B2 = self.m.nnz("A"), self.m.nnz("B2")
        h = C.c_void_p()
        _capi.check(self._lib.sls_margin_plan(ctx.handle, dev_slot, C.byref(self.m.dims), C.byref(self.m.plant), self.m.Sx, self.m.Su,
                                              self.nscen, C.byref(h)), ctx.handle)
        self.handle = h
        n, d, b, pb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(self._lib.sls_margin_info(self.handle, C.byref(n), C.byref(d), C.byref(b), C.byref(pb)))
        self.n_entries, self.n_defect, self.device_bytes, self.plant_bytes = n.value, d.value, b.value, pb.value

    def load(self, d_values, stream=None):
        """Φ from the mask-order device array `Plan.execute(packed=False)` fills (tensor or pointer)"""
        if _is_tensor(d_values):
            d_values = d_values.data_ptr()
        _capi.check(self._lib.sls_margin_load(self.handle, stream, d_values), self.ctx.handle)

    def set_plant(self, A=None, B2=None, per_scenario=False, stream=None):
        """New plant values in the CSC nzval order of the plan's A / B2 (what `Plan.plant_values()` returns): each None (kept), a
        host array, or a device tensor (both must then be tensors, or one None).  per_scenario=False: nnz values for all
        scenarios; True: [nnz, nscen].  The values are not validated."""
        args = plant_value_args(A, B2, self.nnz_A, self.nnz_B2, self.nscen, per_scenario)
        if args is None:
            return
        pA, pB2, on_device, _keep = args
        _capi.check(self._lib.sls_margin_set_plant(self.handle, stream, pA, pB2, on_device, int(bool(per_scenario))), self.ctx.handle)

    def run_async(self, row_l1=None, col_l1=None, totals=None, stream=None):
        """sls_margin_run into device tensors / pointers (each optional): row_l1, col_l1 [Nx, nscen], totals [2, nscen] (‖D‖_𝓛₁, then
        ‖D‖_𝓔₁); enqueued on `stream`, nothing waits"""
        n = self.Nx * self.nscen
        _capi.check(self._lib.sls_margin_run(self.handle, stream, _dev_ptr(row_l1, n, "row_l1"), _dev_ptr(col_l1, n, "col_l1"),
                                             _dev_ptr(totals, 2 * self.nscen, "totals")), self.ctx.handle)

    def margins(self, stream=None):
        """dict of host arrays: row_l1, col_l1 [Nx, nscen], l1 = ‖D⁽ˢ⁾‖_𝓛₁ and e1 = ‖D⁽ˢ⁾‖_𝓔₁ [nscen]; waits for `stream`"""
        row, col, tot = np.zeros((self.Nx, self.nscen)), np.zeros((self.Nx, self.nscen)), np.zeros((2, self.nscen))
        p = lambda a: a.ctypes.data_as(_dp)
        _capi.check(self._lib.sls_margin_fetch(self.handle, stream, p(row), p(col), p(tot)), self.ctx.handle)
        return dict(row_l1=row, col_l1=col, l1=tot[0].copy(), e1=tot[1].copy())

    def certified(self, stream=None):
        """bool [nscen]: min(‖D‖_𝓛₁, ‖D‖_𝓔₁) < 1 — the loop on that plant is internally stable"""
        m = self.margins(stream)
        return np.minimum(m["l1"], m["e1"]) < 1.0

    def gain_bound(self, stream=None):
        """[nscen]: 1/(1 − ‖D‖_𝓛₁) where that norm is below 1 — the factor by which ‖ŵ‖∞, and with it every 𝓛₁ bound of the design,
        can grow on that plant — else inf"""
        l1 = self.margins(stream)["l1"]
        out = np.full(self.nscen, np.inf)
        ok = l1 < 1.0
        out[ok] = 1.0 / (1.0 - l1[ok])
        return out

    # ---- the worst case over a box of plants (csrc/sls_margin_box.h) ----

    def set_radius(self, A=None, B2=None, per_scenario=False, relative=None):
        """sls_margin_set_radius: every stored A[i,k], B2[i,m] is known to ± a radius round the centre `set_plant` set.  A / B2:
        host arrays in the CSC nzval order, None = zeros, nnz values or [nnz, nscen].  relative=ε instead: ε·|centre|, per
        scenario, from the centres as they are on the device now (waits for them).  A setup call: allocates and waits."""
        if relative is not None:
            if A is not None or B2 is not None:
                raise ValueError("set_radius: give A / B2 or relative, not both")
            if not (np.isfinite(relative) and relative >= 0):
                raise ValueError("set_radius: relative must be finite and >= 0")
            Ac, Bc = self._centres()
            A, B2, per_scenario = float(relative) * np.abs(Ac), float(relative) * np.abs(Bc), True
        ptrs, keep = [], []
        for name, v, nnz in (("A", A, self.nnz_A), ("B2", B2, self.nnz_B2)):
            if v is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(v, dtype=np.float64)
            n = nnz * (self.nscen if per_scenario else 1)
            if a.size != n:
                raise ValueError(f"set_radius: {name} has {a.size} values, expected {n}")
            keep.append(a)
            ptrs.append(a.ctypes.data_as(_dp))
        _capi.check(self._lib.sls_margin_set_radius(self.handle, ptrs[0], ptrs[1], int(bool(per_scenario))), self.ctx.handle)
        mb, ni, nv, db = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(self._lib.sls_margin_box_info(self.handle, C.byref(mb), C.byref(ni), C.byref(nv), C.byref(db)), self.ctx.handle)
        self.box_max_bits, self.box_inexact_rows, self.box_vertex_sums, self.box_device_bytes = mb.value, ni.value, nv.value, db.value

    def _centres(self):
        """sls_margin_fetch_plant: the plant values on the device, [nnz, nscen] in CSC nzval order; waits"""
        A, B = np.zeros((self.nnz_A, self.nscen)), np.zeros((self.nnz_B2, self.nscen))
        _capi.check(self._lib.sls_margin_fetch_plant(self.handle, None, A.ctypes.data_as(_dp), B.ctypes.data_as(_dp)), self.ctx.handle)
        return A, B

    def box_run_async(self, row_wc=None, row_vertex=None, totals=None, stream=None):
        """sls_margin_box_run into device tensors / pointers (each optional): row_wc [Nx, nscen] float64, row_vertex [Nx, nscen]
        int64, totals [nscen]; enqueued on `stream`, nothing waits"""
        n = self.Nx * self.nscen
        if _is_tensor(row_vertex):
            if not row_vertex.is_cuda or row_vertex.element_size() != 8 or row_vertex.is_floating_point() or not row_vertex.is_contiguous() \
                    or row_vertex.numel() != n:
                raise ValueError(f"row_vertex must be a contiguous int64 device tensor of {n} elements")
            row_vertex = row_vertex.data_ptr()
        _capi.check(self._lib.sls_margin_box_run(self.handle, stream, _dev_ptr(row_wc, n, "row_wc"), row_vertex,
                                                 _dev_ptr(totals, self.nscen, "totals")), self.ctx.handle)

    def box_margins(self, stream=None):
        """dict of host arrays: row_wc [Nx, nscen] = the largest absolute row sum of D over the box, vertex [Nx, nscen] = the sign
        pattern that attains it (bit b set: centre + radius of the row's b-th active coefficient; −1: a bound row), exact [Nx] bool,
        l1_wc [nscen] = the worst ‖D‖_𝓛₁ of the box; waits for `stream`"""
        row, ver = np.zeros((self.Nx, self.nscen)), np.zeros((self.Nx, self.nscen), dtype=np.int64)
        ex, tot = np.zeros(self.Nx, dtype=np.uint8), np.zeros(self.nscen)
        _capi.check(self._lib.sls_margin_box_fetch(self.handle, stream, row.ctypes.data_as(_dp), ver.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   ex.ctypes.data_as(C.POINTER(C.c_uint8)), tot.ctypes.data_as(_dp)), self.ctx.handle)
        return dict(row_wc=row, vertex=ver, exact=ex.astype(bool), l1_wc=tot)

    def box_certified(self, stream=None):
        """bool [nscen]: the worst ‖D‖_𝓛₁ over the box is below 1 — the loop is internally stable on every plant of the box"""
        return self.box_margins(stream)["l1_wc"] < 1.0

    def box_gain_bound(self, stream=None):
        """[nscen]: 1/(1 − l1_wc) where the worst norm is below 1, else inf: `gain_bound` for every plant of the box"""
        l1 = self.box_margins(stream)["l1_wc"]
        out = np.full(self.nscen, np.inf)
        ok = l1 < 1.0
        out[ok] = 1.0 / (1.0 - l1[ok])
        return out

    def worst_plant(self, stream=None):
        """(A_nzval, B2_nzval), each [nnz, nscen] in CSC nzval order: every row at its arg-max vertex (centre ± radius), a bound
        row at centre + radius.  One plant per scenario that attains every exact row's worst case; fit for `set_plant(...,
        per_scenario=True)` here and on a `Rollout`.  Waits for `stream`."""
        A, B = np.zeros((self.nnz_A, self.nscen)), np.zeros((self.nnz_B2, self.nscen))
        _capi.check(self._lib.sls_margin_box_worst_plant(self.handle, stream, A.ctypes.data_as(_dp), B.ctypes.data_as(_dp)), self.ctx.handle)
        return A, B

    def close(self):
        if getattr(self, "handle", None):
            self._lib.sls_margin_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def margin_tables(P, S, index_base=0):
    """sls_debug_margin_tables (needs no device): a dict with n_entries, n_defect, Φ by columns without Sx[0] (phi_seg [Nx·T + 1],
    phi_row, phi_perm), the defect pattern by columns (def_ptr, def_key = τ·Nx + i, def_start) and by rows (row_ptr, row_perm), and
    the plant by rows as `rollout_tables` gives it (A_ptr / A_idx / A_src, B2_ptr / B2_idx / B2_src)."""
    m = _capi.Marshalled(P, S[0], S[1], None, index_base=index_base)
    lib = _capi.load_library()
    Nx, T = int(P.Nx), len(S[0])
    nA, nB = m.nnz("A"), m.nnz("B2")
    ne, nd = C.c_int64(), C.c_int64()
    ip = C.POINTER(C.c_int32)
    head = [C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, C.byref(ne), C.byref(nd)]
    _capi.check(lib.sls_debug_margin_tables(*head, *([None] * 14)))
    ne, nd = ne.value, nd.value
    sizes = dict(phi_seg=Nx * T + 1, phi_row=ne, phi_perm=ne, def_ptr=Nx + 1, def_key=nd, def_start=nd, row_ptr=Nx + 1, row_perm=nd,
                 A_ptr=Nx + 1, A_idx=nA, A_src=nA, B2_ptr=Nx + 1, B2_idx=nB, B2_src=nB)
    t = {k: np.zeros(max(n, 1), dtype=np.int32) for k, n in sizes.items()}
    a, b = C.c_int64(), C.c_int64()
    _capi.check(lib.sls_debug_margin_tables(C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, C.byref(a), C.byref(b),
                                            *(t[k].ctypes.data_as(ip) for k in sizes)))
    t = {k: t[k][:n] for k, n in sizes.items()}
    t["n_entries"], t["n_defect"] = ne, nd
    return t


def margin_host(P, S, values, nscen=1, A=None, B2=None, per_scenario=False, index_base=0):
    """sls_debug_margin_host (needs no device): the host twin of plan → load(values) → set_plant(A, B2, per_scenario) → run.
    Returns a dict: row_l1, col_l1 [Nx, nscen], l1, e1 [nscen], and the error model of each output — row_n / col_n [Nx] and tot_n
    [2]: the number N of terms; row_s / col_s [Nx, nscen] and tot_s [2, nscen]: the sum S of their absolute values.  A double
    evaluation of an output in any order is within 2·N·2⁻⁵³·S of the exact value."""
    m = _capi.Marshalled(P, S[0], S[1], None, index_base=index_base)
    Nx, nscen = int(P.Nx), int(nscen)
    keep = []

    def arr(a, n, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != n:
            raise ValueError(f"margin_host: {what} has {a.size} values, expected {n}")
        keep.append(a)
        return a.ctypes.data_as(_dp)

    per = max(nscen, 1) if per_scenario else 1
    shape = (Nx, max(nscen, 1))
    row, col, tot = np.zeros(shape), np.zeros(shape), np.zeros((2, shape[1]))
    row_s, col_s, tot_s = np.zeros(shape), np.zeros(shape), np.zeros((2, shape[1]))
    row_n, col_n, tot_n = np.zeros(Nx, dtype=np.int64), np.zeros(Nx, dtype=np.int64), np.zeros(2, dtype=np.int64)
    o = lambda x: x.ctypes.data_as(_dp)
    n = lambda x: x.ctypes.data_as(C.POINTER(C.c_int64))
    _capi.check(_capi.load_library().sls_debug_margin_host(
        C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, arr(values, len(np.asarray(values)), "values"), nscen,
        arr(A, m.nnz("A") * per, "A"), arr(B2, m.nnz("B2") * per, "B2"), int(bool(per_scenario)), o(row), o(col), o(tot), n(row_n), n(col_n),
        n(tot_n), o(row_s), o(col_s), o(tot_s)))
    return dict(row_l1=row, col_l1=col, l1=tot[0].copy(), e1=tot[1].copy(), row_n=row_n, col_n=col_n, tot_n=tot_n, row_s=row_s,
                col_s=col_s, tot_s=tot_s)


def margin_box_host(P, S, values, nscen=1, A=None, B2=None, per_scenario=False, A_rad=None, B2_rad=None, rad_per_scenario=False,
                    index_base=0):
    """sls_debug_margin_box_host (needs no device): the host twin of plan → load(values) → set_plant(A, B2, per_scenario) →
    set_radius(A_rad, B2_rad, rad_per_scenario) → box run.  Returns a dict: row_wc, vertex [Nx, nscen], exact [Nx], l1_wc [nscen],
    the worst plant A_worst / B2_worst [nnz, nscen] (CSC order), the active lists act_ptr [Nx + 1] and act_ent (coefficient c <
    nnz(A): CSR entry c of A, else CSR entry c − nnz(A) of B₂), and the error model of row_wc — row_n [Nx]: the number N of terms,
    row_s [Nx, nscen]: the sum S of their absolute values (the ρ·|φ| terms included).  A double evaluation of a vertex sum, or of
    the triangle bound of an inexact row, is within 2·N·2⁻⁵³·S of its exact value."""
    m = _capi.Marshalled(P, S[0], S[1], None, index_base=index_base)
    Nx, nscen = int(P.Nx), int(nscen)
    nA, nB = m.nnz("A"), m.nnz("B2")
    keep = []

    def arr(a, n, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != n:
            raise ValueError(f"margin_box_host: {what} has {a.size} values, expected {n}")
        keep.append(a)
        return a.ctypes.data_as(_dp)

    ns = max(nscen, 1)
    per, rper = (ns if per_scenario else 1), (ns if rad_per_scenario else 1)
    row, row_s, tot = np.zeros((Nx, ns)), np.zeros((Nx, ns)), np.zeros(ns)
    ver, row_n, ex = np.zeros((Nx, ns), dtype=np.int64), np.zeros(Nx, dtype=np.int64), np.zeros(Nx, dtype=np.uint8)
    Aw, Bw = np.zeros((nA, ns)), np.zeros((nB, ns))
    act_ptr, act_ent = np.zeros(Nx + 1, dtype=np.int32), np.zeros(max(nA + nB, 1), dtype=np.int32)
    o = lambda x: x.ctypes.data_as(_dp)
    n = lambda x: x.ctypes.data_as(C.POINTER(C.c_int64))
    i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    _capi.check(_capi.load_library().sls_debug_margin_box_host(
        C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, arr(values, len(np.asarray(values)), "values"), nscen,
        arr(A, nA * per, "A"), arr(B2, nB * per, "B2"), int(bool(per_scenario)), arr(A_rad, nA * rper, "A_rad"), arr(B2_rad, nB * rper, "B2_rad"),
        int(bool(rad_per_scenario)), o(row), n(ver), ex.ctypes.data_as(C.POINTER(C.c_uint8)), o(tot), n(row_n), o(row_s), o(Aw), o(Bw),
        i32(act_ptr), i32(act_ent)))
    return dict(row_wc=row, vertex=ver, exact=ex.astype(bool), l1_wc=tot, row_n=row_n, row_s=row_s, A_worst=Aw, B2_worst=Bw,
                act_ptr=act_ptr, act_ent=act_ent[:act_ptr[-1]])


def margin_entry_signed_check(P, S, values, nscen=1, A=None, B2=None, per_scenario=False):
    """sls_debug_margin_entry_signed (needs no device): (entries compared, entries where fabs(margin_entry_signed) and margin_entry
    differ in a bit, entries whose signed value is negative) over every pattern entry and scenario"""
    m = _capi.Marshalled(P, S[0], S[1], None)
    per = int(nscen) if per_scenario else 1
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (values, A, B2)]
    if keep[1] is not None and keep[1].size != m.nnz("A") * per or keep[2] is not None and keep[2].size != m.nnz("B2") * per:
        raise ValueError("margin_entry_signed_check: wrong number of plant values")
    p = lambda a: None if a is None else a.ctypes.data_as(_dp)
    ne, nm, nn = C.c_int64(), C.c_int64(), C.c_int64()
    _capi.check(_capi.load_library().sls_debug_margin_entry_signed(C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, p(keep[0]), int(nscen),
                                                                   p(keep[1]), p(keep[2]), int(bool(per_scenario)), C.byref(ne), C.byref(nm),
                                                                   C.byref(nn)))
    return ne.value, nm.value, nn.value
