"""Plants, masks and a NumPy statement of the achievability residual, shared by tests/test_residual_host.py and
tests/test_gpu_residual.py (a plain module like objective_cases.py; not a conftest).

The quantity under test (include/sls_mi355x.h), per subproblem with global column c and index sets s_x, s_u:
    Δ[0] = Φx[0][:,c] − e_c,   Δ[t+1] = Φx[t+1][:,c] − A·Φx[t][:,c] − B2·Φu[t][:,c]  (t = 0 … T−2),   Δ[T] = −A·Φx[T−1][:,c] − B2·Φu[T−1][:,c]
on all rows of the plant, Φ[:,c] read through the mask restricted to (s_x, s_u); local rows are s_x, the halo H(q) the rows outside
s_x that a stored entry of A[:, s_x] or B2[:, s_u] reaches, plus row c when c ∉ s_x."""
import os

import numpy as np
import scipy.sparse as sp

import objective_cases as oc

GOLDEN = oc.GOLDEN


# ------------------------------------------------------------------ cases: (P, S, groups, vals_x[t], vals_u[t]) or (P, S, groups)

def band(A, k):
    """(A≠0)^k ≠ 0 as a sorted Boolean CSC matrix"""
    Ab = (sp.csc_matrix(A) != 0).astype(np.int32).tocsc()
    R = sp.identity(A.shape[0], dtype=np.int32, format="csc")
    for _ in range(k):
        R = ((Ab @ R) != 0).astype(np.int32).tocsc()
    M = (R != 0).tocsc(); M.sort_indices()
    return M


def halo_chain(slc):
    """12-state chain, T = 4.  𝓢x[t] is the d = 2 band for t < T−1 and the d = 1 band at the last step, so s_x (built from the last
    mask) is narrower than what the earlier steps may fill; actuator 2 (on state 6) has a second entry on state 11, five states
    away: both put A·Φx + B2·Φu on rows the reduced problem never constrained."""
    Pc = slc.workloads.chain_plant(12)
    B2 = sp.lil_matrix(Pc.B2)
    B2[11, 2] = 0.5
    P = slc.Plant(Pc.A, Pc.B1, B2.tocsc())
    T = 4
    Bb = (sp.csc_matrix(P.B2).T != 0).astype(np.int32)
    Sx, Su = [], []
    for t in range(T):
        k = 2 if t < T - 1 else 1
        Sx.append(band(P.A, k))
        U = ((Bb @ band(P.A, k + 1).astype(np.int32)) != 0).tocsc(); U.sort_indices()
        Su.append(U)
    return P, [Sx, Su], None


def grid_strides(slc, which):
    """4-neighbour grids whose ñx + |H| straddles the lane strides: 9×9 at d = 5 — 36 … 77 rows, 64 among them; 12×12 at d = 8 —
    66 … 139 rows, 128 among them."""
    n, d, T = {"grid9": (9, 5, 3), "grid12": (12, 8, 2)}[which]
    P = slc.workloads.grid_plant(n, 2)
    S = slc.workloads.localization_masks(P.A, P.B2, d, T, 8.0)
    return P, [list(S[0]), list(S[1])], None


def dense_rows(slc):
    """16 states, 12 actuators, rows longer than the eight entries the device keeps in registers per row: row 5 of A is full (16
    entries — A alone overflows), row 2 of B2 is full (3 entries of A + 12 of B2 — B2 overflows part way), row 9 of A holds
    exactly 8 and its B2 row one more."""
    Nx, Nu = 16, 12
    A = sp.lil_matrix(slc.workloads.chain_plant(Nx).A)
    A[5, :] = 0.05 * (1.0 + np.arange(Nx) % 3); A[5, 5] = 1.0
    for j in (0, 3, 6, 12, 15):
        A[9, j] = -0.04
    B2 = sp.lil_matrix((Nx, Nu))
    for k in range(Nu):
        B2[k, k] = 1.0
    B2[2, :] = 0.1 * (1.0 + np.arange(Nu) % 2)
    B2[5, 7] = 0.3
    P = slc.Plant(A.tocsc(), sp.identity(Nx, format="csc"), B2.tocsc())
    S = slc.workloads.localization_masks(P.A, P.B2, 2, 3, 1.5)
    return P, [list(S[0]), list(S[1])], None


def short_chain(slc, T):
    P = slc.workloads.chain_plant(23)
    S = slc.workloads.localization_masks(P.A, P.B2, 3, T, 1.5)
    return P, [list(S[0]), list(S[1])], None


def infeasible_golden(slc):
    g = np.load(os.path.join(GOLDEN, "infeasible_chain.npz"))
    P = slc.workloads.chain_plant(int(g["Nx"]))
    S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    S = [list(S[0]), list(S[1])]
    return P, S, None, oc.split(g["vals_x"], S[0]), oc.split(g["vals_u"], S[1])


def grouped_golden(slc):
    """the README chain in three multi-column groups on shared index sets"""
    P, S, _, _, _, _ = oc.readme_golden(slc)
    g = np.load(os.path.join(GOLDEN, "grouped_chain_phi.npz"))
    groups = [list(range(0, 20)), list(range(20, 40)), list(range(40, 59))]
    return P, S, groups, oc.split(g["vals_x"], S[0]), oc.split(g["vals_u"], S[1])


def golden_case(slc, name):
    """the cases whose Φ is a committed golden: (P, S, groups, vals_x[t], vals_u[t])"""
    if name == "infeasible":
        return infeasible_golden(slc)
    if name == "grouped":
        return grouped_golden(slc)
    if name == "readme":
        P, S, I, vx, vu, _ = oc.readme_golden(slc)
    elif name == "weighted":
        P, S, I, vx, vu, _ = oc.weighted_golden(slc)
    elif name == "general":
        P, S, I, vx, vu, _ = oc.general_golden(slc)
    elif name in ("coupled_dense", "coupled_diag"):
        P, S, I, vx, vu, _ = oc.coupled_golden(slc, name.split("_")[1])
    else:
        raise KeyError(name)
    return P, S, I, oc.split(vx, S[0]), oc.split(vu, S[1])


GOLDEN_CASES = ["readme", "infeasible", "weighted", "general", "coupled_dense", "coupled_diag", "grouped"]


def oracle_case(slc, name):
    """the cases whose Φ an oracle computes: (P, S, groups)"""
    if name == "halo":
        return halo_chain(slc)
    if name in ("grid9", "grid12"):
        return grid_strides(slc, name)
    if name in ("T1", "T2"):
        return short_chain(slc, int(name[1]))
    if name == "whole":           # 12-state chain whose index sets are the whole plant: every H(q) is empty
        P = slc.workloads.chain_plant(12)
        S = slc.workloads.localization_masks(P.A, P.B2, 12, 3, 8.0)
        return P, [list(S[0]), list(S[1])], None
    if name == "dense_rows":
        return dense_rows(slc)
    raise KeyError(name)


ORACLE_CASES = ["halo", "grid9", "grid12", "T1", "T2", "whole", "dense_rows"]


def perturbed_A(P, seed=5):
    """the stale-Φ update: three entries of A moved by a few percent, the pattern untouched"""
    A = sp.csc_matrix(P.A, dtype=np.float64).copy(); A.sort_indices()
    rng = np.random.default_rng(seed)
    k = rng.choice(A.nnz, size=3, replace=False)
    A.data[k] *= 1.0 + 0.05 * np.array([1.0, -1.0, 2.0])
    return A


# ------------------------------------------------------------------ the definition, stated with dense columns in np.longdouble

def _pattern(M):
    M = sp.csc_matrix(M)
    return sp.csc_matrix((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape)      # stored entries, zeros included


def halo_sets(oracle, P, S, groups=None):
    """(s_x, s_u, H, c) per subproblem in col_status order; H from Boolean matrix products over the stored patterns"""
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    groups = [[c] for c in range(P.Nx)] if groups is None else groups
    PA, PB = _pattern(P.A), _pattern(P.B2)
    out = []
    for g in groups:
        _, _, _, sx, su = oracle.sparsity_dim_reduction(Po, list(g), S)
        sx, su = np.asarray(sx, dtype=np.int64), np.asarray(su, dtype=np.int64)
        ex = np.zeros(P.Nx, dtype=np.int64); ex[sx] = 1
        eu = np.zeros(P.Nu, dtype=np.int64); eu[su] = 1
        reach = (PA @ ex + PB @ eu) > 0
        for c in g:
            h = reach.copy()
            h[c] = True
            h[sx] = False
            out.append((sx, su, np.flatnonzero(h), int(c)))
    return out


def numpy_residual(oracle, P, S, groups, vals_x, vals_u):
    """(res_inf, halo_inf, res_l1, [H(q)]) straight from the definition: Φ[t][:,c] as a dense column (mask-true entries on s_x / s_u,
    0.0 elsewhere), A and B2 as dense matrices, everything in np.longdouble; the maxima and the sum over the rows s_x ∪ H."""
    ld = np.longdouble
    T = len(S[0])
    A = np.asarray(sp.csc_matrix(P.A).todense()).astype(ld)
    B = np.asarray(sp.csc_matrix(P.B2).todense()).astype(ld)

    def masked(Sm, v):            # stored-true entries carry the value, stored-false ones read as 0.0
        Sm = sp.csc_matrix(Sm)
        return sp.csc_matrix((np.where(Sm.data.astype(bool), np.asarray(v, dtype=np.float64), 0.0), Sm.indices, Sm.indptr), shape=Sm.shape)
    Fx = [masked(m, v) for m, v in zip(S[0], vals_x)]
    Fu = [masked(m, v) for m, v in zip(S[1], vals_u)]
    sets = halo_sets(oracle, P, S, groups)
    ns = len(sets)
    res_inf, halo_inf, res_l1 = np.zeros(ns), np.zeros(ns), np.zeros(ns)
    for q, (sx, su, H, c) in enumerate(sets):
        def col(F, rows, t):
            full = np.asarray(F[t][:, [c]].todense()).ravel()
            z = np.zeros(full.size, dtype=ld)
            z[rows] = full[rows]
            return z
        px = [col(Fx, sx, t) for t in range(T)]
        pu = [col(Fu, su, t) for t in range(T)]
        e = np.zeros(P.Nx, dtype=ld); e[c] = 1
        D = [px[0] - e]
        for t in range(T - 1):
            D.append(px[t + 1] - A @ px[t] - B @ pu[t])
        D.append(-(A @ px[T - 1]) - B @ pu[T - 1])
        D = np.abs(np.stack(D))                                    # [T + 1, Nx]
        rows = np.concatenate([sx, H])
        outside = np.setdiff1d(np.arange(P.Nx), rows)
        assert not D[:, outside].any(), "Δ is non-zero on a row outside s_x ∪ H"
        res_inf[q] = float(D[:, rows].max())
        halo_inf[q] = float(D[:, H].max()) if H.size else 0.0
        res_l1[q] = float(D[:, rows].sum())
    return res_inf, halo_inf, res_l1, [s[2] for s in sets]
