"""Plants and reference formulas shared by tests/test_objective_host.py and tests/test_gpu_objective.py (a plain module like
son_cases.py; not a conftest).

The quantity under test is the reference's objective_value(problem) (src/synthesis.jl:52): per column
Σₜ‖[C̃1 D̃12]·[Φx[t][s_x,c]; Φu[t][s_u,c]]·B̃1 + D̃11‖²_F with the index sets of src/reduction.jl:14."""
import os

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53          # unit round-off of FP64


def split(flat, masks):
    out, o = [], 0
    for M in masks:
        out.append(np.asarray(flat[o:o + M.nnz], dtype=np.float64)); o += M.nnz
    assert o == len(flat)
    return out


def summation_bound(n_terms, abs_sum):
    """Two evaluations of the same sum of N products in different orders differ by at most 2·N·2⁻⁵³·S, S the sum of the
    products' absolute values: each side carries at most (N − 1) additions and a rounding or two per product, i.e. a
    relative error below N·2⁻⁵³ of S."""
    return 2.0 * np.asarray(n_terms, dtype=np.float64) * U * np.asarray(abs_sum, dtype=np.float64)


# ------------------------------------------------------------------ golden plants (as tests/test_gpu_parity.py / test_gpu_tile.py build them)

def readme_golden(slc):
    P, S, _ = slc.workloads.make_workload("readme_chain")
    g = np.load(os.path.join(GOLDEN, "readme_chain_phi.npz"))
    return P, [list(S[0]), list(S[1])], None, g["vals_x"], g["vals_u"], g["col_cost"]


def weighted_golden(slc):
    g = np.load(os.path.join(GOLDEN, "weighted_chain_phi.npz"))
    Nx = int(g["Nx"])
    Pc = slc.workloads.chain_plant(Nx)
    Nu = Pc.Nu
    C1 = sp.vstack([sp.diags(g["q"]), sp.csc_matrix((Nu, Nx))]).tocsc()
    D12 = sp.vstack([sp.csc_matrix((Nx, Nu)), sp.diags(g["r"])]).tocsc()
    D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nx + Nu, Nx))
    P = slc.Plant(Pc.A, sp.diags(g["b"]).tocsc(), Pc.B2, C1, D11, D12)
    S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    return P, [list(S[0]), list(S[1])], None, g["vals_x"], g["vals_u"], g["col_cost"]


def general_golden(slc):
    g = np.load(os.path.join(GOLDEN, "general_weights_phi.npz"))
    Nx = int(g["Nx"])
    Pc = slc.workloads.chain_plant(Nx)
    Nu = Pc.Nu
    W = sp.csc_matrix((g["W_data"], g["W_indices"], g["W_indptr"]), shape=(Nx + Nu, Nx + Nu))
    D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nx + Nu, Nx))
    P = slc.Plant(Pc.A, sp.diags(g["b"]).tocsc(), Pc.B2, W[:, :Nx], D11, W[:, Nx:])
    S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    return P, [list(S[0]), list(S[1])], None, g["vals_x"], g["vals_u"], g["col_cost"]


def coupled_golden(slc, tag):
    """groups of 1–4 columns coupled through B1[c_j, c_j]; `cost` is per GROUP"""
    g = np.load(os.path.join(GOLDEN, "coupled_group_phi.npz"))
    Nx = int(g["Nx"])
    Pc = slc.workloads.chain_plant(Nx)
    Nu = Pc.Nu
    W = sp.csc_matrix((g[f"{tag}_W_data"], g[f"{tag}_W_indices"], g[f"{tag}_W_indptr"]), shape=(Nx + Nu, Nx + Nu))
    B1 = sp.csc_matrix((g["B1_data"], g["B1_indices"], g["B1_indptr"]), shape=(Nx, Nx))
    D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nx + Nu, Nx))
    P = slc.Plant(Pc.A, B1, Pc.B2, W[:, :Nx], D11, W[:, Nx:])
    S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    gp, gc = g["group_ptr"], g["group_cols"]
    groups = [[int(c) for c in gc[gp[i]:gp[i + 1]]] for i in range(len(gp) - 1)]
    return P, [list(S[0]), list(S[1])], groups, g[f"{tag}_vals_x"], g[f"{tag}_vals_u"], g[f"{tag}_group_cost"]


def group_firsts(groups):
    """index (in col_status order) of every group's first column"""
    return np.cumsum([0] + [len(g) for g in groups])[:-1]


# ------------------------------------------------------------------ 23-state chain at T = 6: the cost variants of the formula test

NX, T6, D6 = 23, 6, 3


def chain23_variant(slc, name):
    """(P, S, ridge) — every variant shares the chain's A, B2 and masks, so one Φ serves all of them"""
    Pc = slc.workloads.chain_plant(NX)
    Nu = Pc.Nu
    S = slc.workloads.localization_masks(Pc.A, Pc.B2, D6, T6, 1.5)
    S = [list(S[0]), list(S[1])]
    I = sp.identity(NX + Nu, format="csc")
    ridge = None
    if name == "scale36":            # [C1 D12] = 2I, B1 = 3I: uniform weights, has_w = 0 with scale 36
        P = slc.Plant(Pc.A, (3.0 * sp.identity(NX)).tocsc(), Pc.B2, (2.0 * I[:, :NX]).tocsc(), 0, (2.0 * I[:, NX:]).tocsc())
    elif name == "b_zero":           # one zero on B1's diagonal: that column's cost is constant in Φ
        b = np.ones(NX); b[7] = 0.0
        P = slc.Plant(Pc.A, sp.diags(b).tocsc(), Pc.B2)
    elif name == "d11":              # feed-through: a linear term and a constant
        rng = np.random.default_rng(3)
        D11 = sp.random(NX + Nu, NX, density=0.15, random_state=rng, format="csc")
        P = slc.Plant(Pc.A, sp.diags(np.linspace(0.5, 1.5, NX)).tocsc(), Pc.B2, I[:, :NX], D11, I[:, NX:])
    elif name == "ridge":
        P = slc.Plant(Pc.A, Pc.B1, Pc.B2)
        ridge = (np.linspace(0.1, 0.9, NX), np.linspace(0.3, 0.05, Nu))
    elif name == "default":
        P = slc.Plant(Pc.A, Pc.B1, Pc.B2)
    else:
        raise KeyError(name)
    return P, S, ridge


def reference_formula(oracle, P, S, Phix, Phiu, ridge=None):
    """Per column c (default groups): Σₜ‖L̃·[Φx[t][s_x,c]; Φu[t][s_u,c]]·B̃1 + D̃11‖²_F, index sets from
    oracle.sparsity_dim_reduction — the reference's objective_value, stated with dense NumPy blocks.  `ridge` adds the term
    of sls_set_ridge, Σₜ Σᵢ rx[i]·Φx[t][i,c]² + Σⱼ ru[j]·Φu[t][j,c]²."""
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    out = np.zeros(P.Nx)
    for c in range(P.Nx):
        sub, _, iix, sx, su = oracle.sparsity_dim_reduction(Po, [c], S)
        L = np.hstack([sub["C1"], sub["D12"]])
        Bt = sub["B1"][iix, :]
        if Bt.shape[0] == 0:                      # column outside its own index set: Φ̃·B̃1 is empty, the cost is ‖D̃11‖² per step
            out[c] = len(S[0]) * float(np.sum(sub["D11"] ** 2))
            continue
        J = 0.0
        for t in range(len(S[0])):
            z = np.concatenate([np.asarray(Phix[t][sx][:, [c]].todense()).ravel(), np.asarray(Phiu[t][su][:, [c]].todense()).ravel()])
            J += float(np.sum((L @ z[:, None] @ Bt + sub["D11"]) ** 2))
            if ridge is not None:
                J += float(np.sum(ridge[0][sx] * z[:len(sx)] ** 2) + np.sum(ridge[1][su] * z[len(sx):] ** 2))
        out[c] = J
    return out
