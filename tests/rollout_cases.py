"""Cases, perturbed plants and the reference shared by tests/test_rollout_host.py and tests/test_gpu_rollout.py (a plain module
like controller_cases.py, which it imports and does not edit; not a conftest, and free of HIP: nothing here loads the library).

The operation under test is the ensemble rollout of csrc/sls_rollout.h: scenario s has its own values A⁽ˢ⁾, B₂⁽ˢ⁾,

    ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
    u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
    β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}
    x_{k+1} = A⁽ˢ⁾·x_k + B₁·w_k + B₂⁽ˢ⁾·u_k
    J⁽ˢ⁾   += Σ_i (q_i·x_k[i])² + Σ_j (r_j·u_k[j])²         peak_x⁽ˢ⁾ = max(peak_x⁽ˢ⁾, max_i |x_k[i]|), peak_u likewise

The operators are those of closed_loop_cases.py / controller_cases.py: the row-length ladder (Nx 24, Nu 6, T 24: ring of 32 slots;
one actuator shared by two states, one orphan, one with an empty operator row) and T1, T2, T4, T5, Nu0 on Nx = 9 (rings of 1, 2, 4
= T, 8 > T).  Perturbed plants scale every stored value of A and B₂ by a factor in [0.8, 1.2] from a fixed seed.

Tolerances.  x, u and the peaks: controller_cases.RTOL = 1e-11 relative to max(1, max|ref|) per scenario, the tolerance the
closed-loop and controller tests use on these cases.  Cost: COST_RTOL = 3e-11 relative to the cost itself — squares double the
relative error, and a sum of ≤ 10⁴ non-negative terms adds about 10⁻¹².  Growth is a condition, not a tolerance:
test_rollout_host.py asserts max|x| < GROWTH_BOUND = 1e6 on every reference used, so that relative errors mean something."""
import numpy as np
import scipy.sparse as sp

import closed_loop_cases as clc
import controller_cases as cc

L = np.longdouble
RTOL = cc.RTOL
COST_RTOL = 3e-11
GROWTH_BOUND = 1e6
ALL = ("ladder", "T1", "T2", "T4", "T5", "Nu0")
RING = ("T1", "T2", "T4", "T5")
LAYOUT_NSCEN = (1, 2, 3, 4, 7, 16, 17, 32, 33, 64, 65, 130)
LAYOUT_STEPS = 60


def case(name):
    return cc.case(name)


def ring_steps(T):
    """chunks 1, 2, R−1, R, R+1 and a rest of 2 need 3R + 5 steps: at least 2R + 4, and 29 for T5"""
    return 3 * cc.ring_slots(T) + 5


def ring_chunks(T):
    R = cc.ring_slots(T)
    return [1, 2, R - 1, R, R + 1, ring_steps(T) - (3 * R + 3)]


def disturbance(name, steps, nscen, seed=0):
    """dense w ~ 0.5·N(0,1), [steps, Nw, nscen]"""
    c = ALL.index(name)
    Nx = clc.LADDER_NX if name == "ladder" else clc.SMALL_NX
    return 0.5 * np.random.default_rng(8000 + 17 * c + seed).standard_normal((steps, Nx, nscen))


def initial_state(name, nscen, seed=0):
    Nx = clc.LADDER_NX if name == "ladder" else clc.SMALL_NX
    return np.random.default_rng(8500 + ALL.index(name) + seed).standard_normal((Nx, nscen))


def weights(case, seed=3):
    """q [Nx], r [Nu] ~ U[0.5, 2]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, case.Nx), rng.uniform(0.5, 2.0, case.Nu)


def csc_values(M):
    M = sp.csc_matrix(M).copy()
    M.sort_indices()
    return np.asarray(M.data, dtype=np.float64)


def perturbed(case, nscen, seed=11):
    """(A_vals [nnz(A), nscen], B2_vals [nnz(B₂), nscen]) in the CSC nzval order: every stored value times a factor in [0.8, 1.2].
    Column s does not depend on nscen (the factors are drawn for 130 scenarios and cut)."""
    rng = np.random.default_rng(seed)
    a, b = csc_values(case.A), csc_values(case.B2)
    fa, fb = rng.uniform(0.8, 1.2, (a.size, 130)), rng.uniform(0.8, 1.2, (b.size, 130))
    assert nscen <= 130
    return np.ascontiguousarray(a[:, None] * fa[:, :nscen]), np.ascontiguousarray(b[:, None] * fb[:, :nscen])


def with_values(M, vals):
    """the CSC matrix M with its stored values replaced (same pattern, nzval order)"""
    M = sp.csc_matrix(M).copy()
    M.sort_indices()
    return sp.csc_matrix((np.asarray(vals, dtype=np.float64), M.indices, M.indptr), shape=M.shape)


def _dense_per_scenario(M, vals, nscen):
    """[nscen, rows, cols] longdouble from the pattern of M and vals [nnz] (shared), [nnz, nscen], or None (M's own values)"""
    M = sp.csc_matrix(M).copy()
    M.sort_indices()
    cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    v = np.asarray(M.data if vals is None else vals, dtype=L)
    if v.ndim == 1:
        v = np.repeat(v[:, None], nscen, axis=1)
    D = np.zeros((nscen,) + M.shape, dtype=L)
    D[:, M.indices, cols] = v.T
    return D


def reference(case, steps, nscen, w=None, A_vals=None, B2_vals=None, x0=None, q=None, r=None, scale=1.0, switch=None,
              weights_from=None):
    """The five lines above in np.longdouble with dense per-scenario plants, all scenarios at once; the controller part is
    controller_cases.Reference.  w [steps, Nw, nscen] or None.  switch = (k, scale'): Φ is multiplied by scale' from step k on.
    weights_from = (k, q', r'): the weights from step k on.  Returns a dict of longdouble arrays: x, u [steps, ·, nscen], state
    [Nx, nscen] (x after the last step), cost, peak_x, peak_u [nscen]."""
    A = _dense_per_scenario(case.A, A_vals, nscen)
    B2 = _dense_per_scenario(case.B2, B2_vals, nscen)
    B1 = np.asarray(sp.csc_matrix(case.B1).toarray(), dtype=L)
    q = np.ones(case.Nx, dtype=L) if q is None else np.asarray(q, dtype=L)
    r = np.ones(case.Nu, dtype=L) if r is None else np.asarray(r, dtype=L)
    ref = cc.Reference(case, scale)
    x = np.zeros((case.Nx, nscen), dtype=L) if x0 is None else np.asarray(x0, dtype=L)
    xs, us = [], []
    cost, px, pu = np.zeros(nscen, dtype=L), np.zeros(nscen, dtype=L), np.zeros(nscen, dtype=L)
    for k in range(steps):
        if switch is not None and k == switch[0]:
            ref.scale = switch[1]
        if weights_from is not None and k == weights_from[0]:
            q, r = np.asarray(weights_from[1], dtype=L), np.asarray(weights_from[2], dtype=L)
        u, _ = ref.step(x)
        xs.append(x); us.append(u)
        cost = cost + ((q[:, None] * x) ** 2).sum(axis=0) + ((r[:, None] * u) ** 2).sum(axis=0)
        px = np.maximum(px, np.abs(x).max(axis=0))
        if case.Nu:
            pu = np.maximum(pu, np.abs(u).max(axis=0))
        xn = np.einsum("sij,js->is", A, x) + np.einsum("sij,js->is", B2, u)
        if w is not None:
            xn = xn + B1 @ np.asarray(w[k], dtype=L)
        x = xn
    return dict(x=np.array(xs, dtype=L).reshape(steps, case.Nx, nscen), u=np.array(us, dtype=L).reshape(steps, case.Nu, nscen), state=x,
                cost=cost, peak_x=px, peak_u=pu)


def check_cost(got, ref, what):
    """every scenario's cost relative to itself; returns the largest relative error"""
    got, ref = np.asarray(got, dtype=L), np.asarray(ref, dtype=L)
    assert got.shape == ref.shape and np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (ref > 0).all(), what
    e = float((np.abs(got - ref) / ref).max())
    assert e < COST_RTOL, (what, e)
    return e


def check_all(got, ref, what):
    """x, u, state, peaks at RTOL (controller_cases.check: per scenario, relative to max(1, max|ref|)), cost at COST_RTOL.
    got: a dict with the keys of `reference` (missing keys are skipped).  Returns {key: largest relative error}."""
    out = {}
    for key in ("x", "u", "state", "peak_x", "peak_u"):
        if key in got and ref[key].size:
            out[key] = cc.check(np.asarray(got[key]), ref[key], f"{what} {key}")
    if "cost" in got:
        out["cost"] = check_cost(got["cost"], ref["cost"], f"{what} cost")
    return out
