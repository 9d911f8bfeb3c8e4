"""Cases and the reference shared by tests/test_margin_box_host.py and tests/test_gpu_margin_box.py (a plain module like
margin_cases.py, which it imports and does not edit; not a conftest, and free of HIP: nothing here loads the library).

The quantity under test is the worst case of csrc/sls_margin_box.h: every stored A[i,k], B₂[i,m] of scenario s is known to ± a
radius ρ round a centre, and row i of the defect D (margin_cases.defect) has the absolute sum

    f_i(δ) = Σ_τ Σ_j | D⁰[τ][i,j] − Σ_e δ_e·φ_e[τ][j] |,       φ_e = Φx[τ][k,:] for A[i,k], Φu[τ][m,:] for B₂[i,m]  (Φx[0] = I),

convex in δ, so that its maximum over the box |δ_e| ≤ ρ_e is attained at a sign pattern σ.  `reference` is brute force: D⁰ from
margin_cases.defect, the dense rows φ_e from margin_cases.dense_phi, all 2^b sign patterns of the row's b active coefficients as
one long-double matrix product.  It shares no code with the library's twin.  A row with more than MAX_BITS active coefficients
reports the triangle bound Σ|D⁰| + Σ_e ρ_e·Σ|φ_e| (the reference returns that bound for every row as well).

The active list of a row: its stored entries of A in ascending column, then of B₂, whose radius is > 0 in at least one scenario;
bit b of a vertex code set means δ_b = +ρ_b.

No tolerance is picked here.  The twin returns, per row, the number N of terms and the sum S of their absolute values (the
ρ·|φ| terms included); a double evaluation of a vertex sum in any order is within 2·N·2⁻⁵³·S of its exact value,
and margin_cases.bound is that number."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import closed_loop_cases as clc
import margin_cases as mc
import rollout_cases as rc

L = np.longdouble
MAX_BITS = 10
ALL = mc.ALL + ("wide",)

# ------------------------------------------------------------------ the new operator

WIDE_NX, WIDE_NU, WIDE_T = 16, 4, 3
WIDE_A_ROWS = (7, 8, 0, 1, 2, 2, 3, 3, 3, 0, 2, 1, 2, 2, 2, 2)       # stored entries of A per row
WIDE_B2_ROWS = (3, 3, 0, 0, 0, 1, 1, 2, 0, 0, 0, 1, 0, 0, 0, 0)      # stored entries of B₂ per row
# active coefficients per row with the radii of `radii("wide", …)` at nscen ≥ 2: row 0 has exactly MAX_BITS (1 024 vertices, the
# last exact size), row 1 one more (the bound path), rows 2 … 7 have 0 … 5 (both sides of 8 vertices, which one pass of the
# device holds in its vertex lanes), row 8 stores three coefficients whose radii are all 0, row 9 has no defect entry at all, rows
# 10 and 11 are active in one scenario only (scenario 1 and scenario 0), rows 12 … 15 are ordinary
WIDE_ACTIVE = (10, 11, 0, 1, 2, 3, 4, 5, 0, 0, 2, 2, 2, 2, 2, 2)
WIDE_ZERO_RADIUS_ROW, WIDE_EMPTY_ROW, WIDE_ONLY_SCENARIO = 8, 9, {10: 1, 11: 0}


def wide():
    Nx, Nu, T = WIDE_NX, WIDE_NU, WIDE_T
    rng = np.random.default_rng(1609)
    Mx, Mu = np.zeros((T, Nx, Nx), dtype=bool), np.zeros((T, Nu, Nx), dtype=bool)
    Mx[0] = np.eye(Nx, dtype=bool)
    for t in range(1, T):
        Mx[t] = rng.uniform(size=(Nx, Nx)) < 0.4
        Mx[t, WIDE_EMPTY_ROW, :] = False
    for t in range(T):
        Mu[t] = rng.uniform(size=(Nu, Nx)) < 0.6
    Sx = [clc._csc_mask(Mx[t]) for t in range(T)]
    Su = [clc._csc_mask(Mu[t]) for t in range(T)]
    A, B2 = sp.lil_matrix((Nx, Nx)), sp.lil_matrix((Nx, Nu))
    for i in range(Nx):
        for k in rng.choice(Nx, size=WIDE_A_ROWS[i], replace=False):
            A[i, k] = rng.uniform(0.1, 0.4) * (-1) ** int(k)
        for m in rng.choice(Nu, size=WIDE_B2_ROWS[i], replace=False):
            B2[i, m] = rng.uniform(0.5, 1.0)
    A = A.tocsc(); A.sort_indices()
    vals_x, vals_u = clc._values(rng, Sx, Su)
    return clc._finish(A, sp.identity(Nx, format="csc"), B2.tocsc(), Sx, Su, vals_x, vals_u, 0)


def case(name):
    return wide() if name == "wide" else mc.case(name)


def perturbed(case, nscen, seed=11):
    """centres off the design plant, so that D⁰ ≠ 0 and the vertices σ and −σ differ"""
    return mc.perturbed(case, nscen, seed)


def _rows_of(M):
    M = sp.csc_matrix(M).copy(); M.sort_indices()
    return np.asarray(M.indices)


def radii(name, case, nscen):
    """(A_rad [nnz(A), nscen], B2_rad [nnz(B₂), nscen]) in the CSC nzval order; column s does not depend on nscen.  Every stored
    coefficient gets 5 %, 10 % or 15 % of its design value by the scenario; `wide` then clears row 8 and leaves rows 10 and 11 one
    scenario each."""
    a, b = np.abs(rc.csc_values(case.A)), np.abs(rc.csc_values(case.B2))
    f = 0.05 * (1 + np.arange(nscen) % 3)
    Ar, Br = a[:, None] * f[None, :], b[:, None] * f[None, :]
    if name == "wide":
        ra, rb = _rows_of(case.A), _rows_of(case.B2)
        for M, rows in ((Ar, ra), (Br, rb)):
            M[rows == WIDE_ZERO_RADIUS_ROW] = 0.0
            for row, only in WIDE_ONLY_SCENARIO.items():
                keep = M[rows == row, only].copy() if only < nscen else None
                M[rows == row] = 0.0
                if keep is not None:
                    M[rows == row, only] = keep
    return np.ascontiguousarray(Ar), np.ascontiguousarray(Br)


# ------------------------------------------------------------------ the reference

def _stored(M):
    M = sp.csc_matrix(M)
    return np.asarray(sp.csc_matrix((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape).toarray() != 0)


def active_lists(case, nscen, A_rad, B2_rad):
    """per row the list of ("A", k) / ("B2", m) in the order of the header, and the dense radii RA [nscen, Nx, Nx], RB [nscen, Nx, Nu]"""
    RA = rc._dense_per_scenario(case.A, np.zeros(sp.csc_matrix(case.A).nnz) if A_rad is None else A_rad, nscen)
    RB = rc._dense_per_scenario(case.B2, np.zeros(sp.csc_matrix(case.B2).nnz) if B2_rad is None else B2_rad, nscen)
    RB = RB.reshape(nscen, case.Nx, case.Nu)
    hot_a = (RA > 0).any(axis=0) & _stored(case.A)
    hot_b = (RB > 0).any(axis=0) & _stored(case.B2).reshape(case.Nx, case.Nu)
    lists = [[("A", int(k)) for k in np.flatnonzero(hot_a[i])] + [("B2", int(m)) for m in np.flatnonzero(hot_b[i])] for i in range(case.Nx)]
    return lists, RA, RB


def reference(case, nscen, A_vals=None, B2_vals=None, A_rad=None, B2_rad=None, max_bits=MAX_BITS):
    """dict of arrays: row_wc [Nx, nscen] (longdouble: the exact maximum over all vertices, or the triangle bound of a row with
    more than max_bits active coefficients), vertex [Nx, nscen] (the lowest arg-max code, −1 for a bound row), exact [Nx], l1_wc
    [nscen], triangle [Nx, nscen] (the triangle bound of every row), bits [Nx], lists"""
    D0 = mc.defect(case, nscen, A_vals, B2_vals)                # [nscen, T, Nx, Nx]
    Phix, Phiu = mc.dense_phi(case)
    lists, RA, RB = active_lists(case, nscen, A_rad, B2_rad)
    Nx, T = case.Nx, case.T
    row_wc, tri = np.zeros((Nx, nscen), dtype=L), np.zeros((Nx, nscen), dtype=L)
    vertex = np.zeros((Nx, nscen), dtype=np.int64)
    bits = np.array([len(l) for l in lists])
    for i in range(Nx):
        nb = len(lists[i])
        # φ_e as one row vector over (τ, j)
        F = np.zeros((nb, T * Nx), dtype=L)
        for b, (kind, k) in enumerate(lists[i]):
            F[b] = (Phix[:T, k, :] if kind == "A" else Phiu[:, k, :]).reshape(-1)
        if nb <= max_bits:
            codes = np.arange(1 << nb)
            sign = np.where((codes[:, None] >> np.arange(nb)[None, :]) & 1, L(1), L(-1)).astype(L)     # [2^nb, nb]
        for s in range(nscen):
            d0 = D0[s, :, i, :].reshape(-1)
            rho = np.array([(RA if kind == "A" else RB)[s, i, k] for kind, k in lists[i]], dtype=L)
            tri[i, s] = np.abs(d0).sum() + (rho * np.abs(F).sum(axis=1)).sum() if nb else np.abs(d0).sum()
            if nb <= max_bits:
                f = np.abs(d0[None, :] - (sign * rho[None, :]) @ F).sum(axis=1) if nb else np.abs(d0).sum()[None]
                vertex[i, s] = int(np.argmax(f))               # the first maximum: the lowest code
                row_wc[i, s] = f[vertex[i, s]]
            else:
                vertex[i, s], row_wc[i, s] = -1, tri[i, s]
    return dict(row_wc=row_wc, vertex=vertex, exact=bits <= max_bits, l1_wc=row_wc.max(axis=0), triangle=tri, bits=bits, lists=lists)


def row_sum_at(case, nscen, A_vals, B2_vals, A_rad, B2_rad, vertex):
    """f_i at the given vertex codes [Nx, nscen] (longdouble), by the same dense statement — for checking an arg-max that a near-tie
    may have resolved differently"""
    D0 = mc.defect(case, nscen, A_vals, B2_vals)
    Phix, Phiu = mc.dense_phi(case)
    lists, RA, RB = active_lists(case, nscen, A_rad, B2_rad)
    out = np.zeros((case.Nx, nscen), dtype=L)
    for i in range(case.Nx):
        for s in range(nscen):
            v = D0[s, :, i, :].reshape(-1).copy()
            for b, (kind, k) in enumerate(lists[i]):
                rho = (RA if kind == "A" else RB)[s, i, k]
                phi = (Phix[:case.T, k, :] if kind == "A" else Phiu[:, k, :]).reshape(-1)
                v -= (rho if (int(vertex[i, s]) >> b) & 1 else -rho) * phi
            out[i, s] = np.abs(v).sum()
    return out


def check_rows(got_wc, twin, what):
    """row_wc of a double evaluation (or of the long-double reference) against the twin, every row within the twin's own bound;
    returns the largest ratio error / bound met"""
    b = mc.bound(twin["row_n"][:, None], twin["row_s"])
    err = np.abs(np.asarray(got_wc, dtype=L) - np.asarray(twin["row_wc"], dtype=L))
    assert np.isfinite(np.asarray(got_wc, dtype=np.float64)).all(), what
    assert (err <= b).all(), (what, float(err.max()), float(b.max()), np.argwhere(err > b)[:4].tolist())
    return float(np.max(np.where(err > 0, err / np.maximum(b, L(1e-300)), 0)))


def readme_case(P, S, golden):
    """the README chain with the oracle's Φ (tests/golden/readme_chain_phi.npz) as a case record: masks all stored-true"""
    Sx, Su = [sp.csc_matrix(M) for M in S[0]], [sp.csc_matrix(M) for M in S[1]]
    for M in Sx + Su:
        M.sort_indices()
    Nx, Nu, T = int(P.Nx), int(P.Nu), len(Sx)
    values = np.concatenate([golden["vals_x"], golden["vals_u"]]).astype(np.float64)
    Phix, Phiu = np.zeros((T, Nx, Nx)), np.zeros((T, Nu, Nx))
    o = 0
    for D, masks in ((Phix, Sx), (Phiu, Su)):
        for t, M in enumerate(masks):
            cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
            keep = np.asarray(M.data, dtype=bool)
            D[t, M.indices[keep], cols[keep]] = values[o:o + M.nnz][keep]
            o += M.nnz
    assert o == values.size
    return SimpleNamespace(A=sp.csc_matrix(P.A), B1=sp.csc_matrix(P.B1), B2=sp.csc_matrix(P.B2), Sx=Sx, Su=Su, Nx=Nx, Nu=Nu, T=T,
                           Phix=Phix, Phiu=Phiu, values=values)
