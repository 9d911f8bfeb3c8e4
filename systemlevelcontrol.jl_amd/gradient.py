"""Gradient of the 𝓗₂ cost of a resident plan in the plant's stored entries (include/sls_mi355x.h: sls_plan_gradient).

`gradient_tables` / `gradient_host` are the host side (sls_debug_gradient_host; no device): the entry tables of the device pass
and its serial twin.  `h2_cost` is the solve as a differentiable PyTorch layer on a plan built with `multipliers=True`.
"""
import ctypes as C

import numpy as np

from . import _capi


def _marshal(P, S, I, index_base):
    Sx, Su = S
    return _capi.Marshalled(P, Sx, Su, None if I is None else [list(g) for g in I], index_base=index_base)


def gradient_tables(P, S, I=None, *, index_base=0):
    """The entry tables of `Plan.gradient` for the plan `Plan(ctx, P, S, I)` would build, as a dict: `ent_ptr` [n_sub + 1],
    `ent` [n_slots, 3] = (position, local row, local column) of every stored entry of A / B2 with both indices inside the
    subproblem's index sets — position: CSC position in A's nzval, or nnz(A) + that in B2's — and the inverse map `inv_ptr`
    [nnz(A) + nnz(B2) + 1], `inv_slot`, `inv_sub` [n_slots]: per stored entry its slots and their subproblems, ascending."""
    lib = _capi.load_library()
    m = _marshal(P, S, I, index_base)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    ns = C.c_int64()
    tail = [None] * 11
    _capi.check(lib.sls_debug_gradient_host(*m.common_args(), C.byref(ns), None, None, None, None, None, *tail))
    n, nent = ns.value, m.nnz("A") + m.nnz("B2")
    ent_ptr = np.zeros(m.n_sub + 1, dtype=np.int64); ent = np.zeros((max(n, 1), 3), dtype=np.int32)
    inv_ptr = np.zeros(nent + 1, dtype=np.int64); inv_slot = np.zeros(max(n, 1), dtype=np.int64); inv_sub = np.zeros(max(n, 1), dtype=np.int32)
    _capi.check(lib.sls_debug_gradient_host(*m.common_args(), C.byref(ns), ent_ptr.ctypes.data_as(i64p), ent.ctypes.data_as(i32p),
                                            inv_ptr.ctypes.data_as(i64p), inv_slot.ctypes.data_as(i64p), inv_sub.ctypes.data_as(i32p), *tail))
    return {"ent_ptr": ent_ptr, "ent": ent[:n], "inv_ptr": inv_ptr, "inv_slot": inv_slot[:n], "inv_sub": inv_sub[:n]}


def gradient_host(P, S, mu, vals_x, vals_u, I=None, *, col_status=None, column_weights=None, index_base=0, return_bound=False):
    """Host twin of `Plan.gradient` (needs no device): mu is the list of the subproblems' multipliers, each (T + 1, ñx) as
    `Plan.multipliers` returns them; vals_x[t] / vals_u[t] in the masks' CSC order.  Accumulates in long double in the device's
    order.  Returns (gA, gB2); with return_bound also a dict with, per stored entry, the number N of products (`terms_A`,
    `terms_B2`) and the sum S of their absolute values (`abs_A`, `abs_B2`)."""
    lib = _capi.load_library()
    m = _marshal(P, S, I, index_base)
    Sx, _ = S
    T = len(Sx)
    dp, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    vx = [np.ascontiguousarray(v, dtype=np.float64) for v in vals_x]
    vu = [np.ascontiguousarray(v, dtype=np.float64) for v in vals_u]
    if [v.size for v in vx] != m.nnz_x or [v.size for v in vu] != m.nnz_u:
        raise ValueError("value arrays do not match the masks' nnz")
    if len(mu) != m.n_sub:
        raise ValueError("one multiplier array per subproblem")
    muc = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in mu] + [np.zeros(1)]))
    pad = np.zeros(1)
    px = (dp * T)(*[(a if a.size else pad).ctypes.data_as(dp) for a in vx])
    pu = (dp * T)(*[(a if a.size else pad).ctypes.data_as(dp) for a in vu])
    st = None if col_status is None else np.ascontiguousarray(col_status, dtype=np.int32)
    cw = None if column_weights is None else np.ascontiguousarray(column_weights, dtype=np.float64)
    nA, nB = m.nnz("A"), m.nnz("B2")
    gA, gB, aA, aB = (np.zeros(max(n, 1)) for n in (nA, nB, nA, nB))
    tA, tB = np.zeros(max(nA, 1), dtype=np.int64), np.zeros(max(nB, 1), dtype=np.int64)
    _capi.check(lib.sls_debug_gradient_host(*m.common_args(), None, None, None, None, None, None, muc.ctypes.data_as(dp), px, pu,
                                            None if st is None else st.ctypes.data_as(i32p), None if cw is None else cw.ctypes.data_as(dp),
                                            gA.ctypes.data_as(dp), gB.ctypes.data_as(dp), aA.ctypes.data_as(dp), aB.ctypes.data_as(dp),
                                            tA.ctypes.data_as(i64p), tB.ctypes.data_as(i64p)))
    if return_bound:
        return gA[:nA], gB[:nB], {"terms_A": tA[:nA], "terms_B2": tB[:nB], "abs_A": aA[:nA], "abs_B2": aB[:nB]}
    return gA[:nA], gB[:nB]


def h2_cost(plan, d_values, A=None, B2=None, c1=None, d12=None, column_weights=None, packed=False):
    """The 𝓗₂ cost of the plan's solve as a differentiable function of the plant: a 0-dim float64 tensor Σ_j c_j·J_j.

    plan: built with `multipliers=True` (and `updatable_weights=True` when c1 / d12 are given).  A / B2: float64 CUDA tensors of
    nzval in the plan's CSC order, c1 / d12: of the two LQR diagonals; each may be None (the plan's current values, no
    gradient).  Forward, on torch's current stream: device-side `update_plant` / `update_weights`, execute into `d_values`
    (a device pointer or tensor of the plan's value array), objective.  Raises SLSError-like RuntimeError when an update refused
    entries.  Backward: one `Plan.gradient`, scaled by the incoming gradient."""
    import torch

    dptr = d_values.data_ptr() if isinstance(d_values, torch.Tensor) else d_values

    class _H2Cost(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b2, q, r, cw):
            st = torch.cuda.current_stream().cuda_stream
            av, bv = (None if a is None else a.detach().contiguous()), (None if b2 is None else b2.detach().contiguous())
            if av is not None or bv is not None:
                plan.update_plant(A=av, B2=bv, stream=st)
                if plan.update_result():
                    raise RuntimeError("h2_cost: update_plant refused entries (non-finite, or non-zero where the plan-time value was 0.0)")
            qv, rv = (None if q is None else q.detach().contiguous()), (None if r is None else r.detach().contiguous())
            if qv is not None or rv is not None:
                plan.update_weights(C1=qv, D12=rv, stream=st)
                if plan.update_weights_result():
                    raise RuntimeError("h2_cost: update_weights refused values")
            plan.execute(dptr, packed=packed, stream=st)
            col, tot = plan.objective_values_async(dptr, packed=packed, stream=st)
            ctx.cw = None if cw is None else cw.detach().contiguous()
            ctx.need = (a is not None, b2 is not None, q is not None, r is not None)
            return (tot[0] if cw is None else (col * ctx.cw).sum()).clone()

        @staticmethod
        def backward(ctx, gout):
            st = torch.cuda.current_stream().cuda_stream
            wts = ctx.need[2] or ctx.need[3]
            g = plan.gradient(dptr, packed=packed, column_weights=ctx.cw, stream=st, weights=wts)
            g = list(g) + [None] * (4 - len(g))
            return tuple((gi * gout if (gi is not None and nd) else None) for gi, nd in zip(g, ctx.need)) + (None,)

    return _H2Cost.apply(A, B2, c1, d12, column_weights)
