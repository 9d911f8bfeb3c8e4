"""Cases, the reference and the Boolean pattern shared by tests/test_margin_host.py and tests/test_gpu_margin.py (a plain module
like rollout_cases.py and controller_cases.py, which it imports and does not edit; not a conftest, and free of HIP: nothing here
loads the library).

The quantity under test is the defect of csrc/sls_margin.h: on plant s the controller's reconstructed disturbance obeys

    ŵ_{k+1} = w̃_k − Σ_{τ=0..T−1} D⁽ˢ⁾[τ]·ŵ_{k−τ}
    D⁽ˢ⁾[τ] = Φx[τ+1] − A⁽ˢ⁾·Φx[τ] − B₂⁽ˢ⁾·Φu[τ]            (0-based slices; Φx[0] := I, Φx[T] := 0)

with row_l1[i] = Σ_τ Σ_j |D[τ][i,j]|, col_l1[j] = Σ_τ Σ_i |D[τ][i,j]|, ‖D‖_𝓛₁ = max_i row_l1 and ‖D‖_𝓔₁ = max_j col_l1.

`reference` evaluates that definition with dense matrices in np.longdouble and shares no code with the library's twin; `pattern`
is the defect pattern from Boolean matrix products.  The operators are the rollout's (ladder, T1, T2, T4, T5, Nu0: an empty A row,
long and short lists, stored-false entries, NaN-poisoned unread values; T1 makes D[0] = −A − B₂·Φu[0] the whole defect, Nu0 has no
B₂ term) plus `edges()` below.

No tolerance is picked here.  The twin returns, per output, the number N of terms and the sum S of their absolute values; a
double evaluation of the output in any order is within 2·N·2⁻⁵³·S of the exact value (the rule of DESIGN §3.9), and `bound` is
that number."""
import numpy as np
import scipy.sparse as sp

import closed_loop_cases as clc
import controller_cases as cc
import rollout_cases as rc

L = np.longdouble
ALL = rc.ALL + ("edges",)
LAYOUT_NSCEN = (1, 2, 3, 4, 7, 16, 17, 33, 64, 65, 130)

# ------------------------------------------------------------------ the new operator

EDGES_NX, EDGES_NU, EDGES_T, EDGES_BLOCK = 24, 4, 6, 6
# defect entries of columns 6 … 23: 0, and on both sides of one and of several turns of the sum pass's eight entry slots
EDGES_COLUMN_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 26, 35, 44, 53, 62)
# stored-true entries of the (j, τ ≥ 1) segments of columns 0 … 5, in turn: on both sides of every halving of the binary search
EDGES_SEGMENT_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
EDGES_A_ROWS = (0, 1, 2, 3, 4, 6)           # stored entries of A rows 0 … 5 (inside the block); rows 6 … 23 are empty
EDGES_B2_ROWS = (0, 1, 2, 0, 4, 0)          # stored entries of B₂ rows 0 … 5; rows 6 … 23 are empty
EDGES_EMPTY_COLUMN, EDGES_EMPTY_ROW = 6, 23


def edges():
    """Nx 24, Nu 4, T 6.  A and B₂ live in rows 0 … 5 (A in the 6 × 6 block), so a defect entry in a row ≥ 6 is fed by Φ alone and
    a column ≥ 6 holds exactly its Φx entries.  What each loop of the passes meets:

    * margin_sums_kernel's slot loop (p = q; p < n; p += 8, eight entry slots): column 6 + n has EDGES_COLUMN_LENGTHS[n] defect
      entries — 0 (column 6: an empty defect list, every slot idle), 1 … 7 (some slots idle), 8, 9, 15, 16, 17 and 26, 35, 44,
      53, 62: every residue mod 8 below one turn and after several.  The row lists do the same (rows 6 … 22 are drawn at
      random, test_margin_host.py asserts the residues met) and row 23 has no entry at all.
    * margin_defect_kernel<SCN> is flat over the pattern entries, NE = 64/SCN per wave: n_defect is no multiple of 64, 32, …, 2
      (asserted by test_margin_host.py), so the last wave of every layout but NE = 1 is cut by the bound d < n_defect.
    * margin_entry's A loop: rows 0 … 5 store 0, 1, 2, 3, 4, 6 entries of A; its B₂ loop: 0, 1, 2, 0, 4, 0 entries; rows ≥ 6: both
      loops are empty.
    * margin_find: the (j, τ) segments of columns 0 … 5 hold EDGES_SEGMENT_LENGTHS entries in turn (state rows 0 … 22 and the four
      input rows) — 0, 1, and 2ᵏ − 1, 2ᵏ, 2ᵏ + 1 up to 17 — with hits at both ends and misses below, between and above; the τ = 0
      segments hold input rows only, 0 … 4 of them.
    * pattern entries fed by Φ alone (every entry in rows 6 … 22) and by the plant alone (τ = 0: A[i,j] stored where Φx[1][i,j]
      is not; asserted by test_margin_host.py); one stored-false entry in a segment that is searched."""
    Nx, Nu, T, nb = EDGES_NX, EDGES_NU, EDGES_T, EDGES_BLOCK
    rng = np.random.default_rng(607)
    Mx, Mu = np.zeros((T, Nx, Nx), dtype=bool), np.zeros((T, Nu, Nx), dtype=bool)
    Mx[0] = np.eye(Nx, dtype=bool)
    for n, count in enumerate(EDGES_COLUMN_LENGTHS):            # columns 6 … 23: Φx in rows 6 … 22, slices 1 … 5
        pick = rng.choice((T - 1) * (Nx - nb - 1), size=count, replace=False)
        Mx[1 + pick // (Nx - nb - 1), nb + pick % (Nx - nb - 1), nb + n] = True
    turn = 0
    for j in range(nb):                                         # columns 0 … 5: segments of the listed lengths
        Mu[0, rng.choice(Nu, size=j % (Nu + 1), replace=False), j] = True
        for t in range(1, T):
            count = EDGES_SEGMENT_LENGTHS[turn % len(EDGES_SEGMENT_LENGTHS)]; turn += 1
            pick = rng.choice(Nx - 1 + Nu, size=count, replace=False)
            Mx[t, pick[pick < Nx - 1], j] = True
            Mu[t, pick[pick >= Nx - 1] - (Nx - 1), j] = True
    Sx = [clc._csc_mask(Mx[t]) for t in range(T)]
    Su = [clc._csc_mask(Mu[t]) for t in range(T)]
    free = np.flatnonzero(~Mx[2][:nb, 1])[0]                    # a stored-false entry among the block rows of segment (1, 2)
    Sx[2] = clc._store_false(Sx[2], int(free), 1)
    A = sp.lil_matrix((Nx, Nx))
    for i, count in enumerate(EDGES_A_ROWS):
        for k in rng.choice(nb, size=count, replace=False):
            A[i, k] = rng.uniform(0.1, 0.4) * (-1) ** k
    B2 = sp.lil_matrix((Nx, Nu))
    for i, count in enumerate(EDGES_B2_ROWS):
        for m in rng.choice(Nu, size=count, replace=False):
            B2[i, m] = rng.uniform(0.5, 1.0)
    A = A.tocsc(); A.sort_indices()
    vals_x, vals_u = clc._values(rng, Sx, Su)
    return clc._finish(A, sp.identity(Nx, format="csc"), B2.tocsc(), Sx, Su, vals_x, vals_u, 0)


def case(name):
    return edges() if name == "edges" else rc.case(name)


def perturbed(case, nscen, seed=11):
    return rc.perturbed(case, nscen, seed)


# ------------------------------------------------------------------ the reference

def dense_phi(case, scale=1.0):
    """(Φx [T+1, Nx, Nx], Φu [T, Nu, Nx]) in longdouble: Φx[0] := I, Φx[T] := 0; `scale` multiplies what is loaded (not the I)"""
    Phix = np.zeros((case.T + 1, case.Nx, case.Nx), dtype=L)
    Phix[1:case.T] = np.asarray(case.Phix[1:], dtype=L) * L(scale)
    Phix[0] = np.eye(case.Nx, dtype=L)
    return Phix, np.asarray(case.Phiu, dtype=L) * L(scale)


def defect(case, nscen, A_vals=None, B2_vals=None, scale=1.0):
    """D [nscen, T, Nx, Nx] in longdouble, straight from the definition with dense per-scenario plants"""
    A = rc._dense_per_scenario(case.A, A_vals, nscen)
    B2 = rc._dense_per_scenario(case.B2, B2_vals, nscen)
    Phix, Phiu = dense_phi(case, scale)
    D = np.zeros((nscen, case.T, case.Nx, case.Nx), dtype=L)
    for t in range(case.T):
        D[:, t] = Phix[t + 1][None] - np.einsum("sik,kj->sij", A, Phix[t])
        if case.Nu:
            D[:, t] -= np.einsum("sim,mj->sij", B2, Phiu[t])
    return D


def reference(case, nscen, A_vals=None, B2_vals=None, scale=1.0):
    """dict of longdouble arrays: row_l1, col_l1 [Nx, nscen], l1, e1 [nscen]"""
    a = np.abs(defect(case, nscen, A_vals, B2_vals, scale))
    row, col = a.sum(axis=(1, 3)).T, a.sum(axis=(1, 2)).T
    return dict(row_l1=row, col_l1=col, l1=row.max(axis=0), e1=col.max(axis=0))


def _true(M):
    M = sp.csc_matrix(M)
    return np.asarray(sp.csc_matrix((np.asarray(M.data, dtype=bool).astype(np.int64), M.indices, M.indptr), shape=M.shape).toarray() != 0)


def _stored(M):
    M = sp.csc_matrix(M)
    return np.asarray(sp.csc_matrix((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape).toarray() != 0)


def boolean_phi(case):
    """(Px [T+1, Nx, Nx], Pu [T, Nu, Nx]): stored-true patterns; Px[0] = I whatever Sx[0] stores, Px[T] = 0"""
    Px = np.zeros((case.T + 1, case.Nx, case.Nx), dtype=bool)
    Px[0] = np.eye(case.Nx, dtype=bool)
    for t in range(1, case.T):
        Px[t] = _true(case.Sx[t])
    Pu = np.zeros((case.T, case.Nu, case.Nx), dtype=bool)
    for t in range(case.T):
        Pu[t] = _true(case.Su[t]).reshape(case.Nu, case.Nx)
    return Px, Pu


def pattern(case):
    """the defect pattern [T, Nx, Nx] (τ, i, j) and its three sources (from Φx[τ+1], through A, through B₂), by Boolean products"""
    Px, Pu = boolean_phi(case)
    PA, PB = _stored(case.A).astype(np.int64), _stored(case.B2).astype(np.int64).reshape(case.Nx, case.Nu)
    own = Px[1:]
    viaA = np.array([(PA @ Px[t].astype(np.int64)) > 0 for t in range(case.T)])
    viaB = np.array([(PB @ Pu[t].astype(np.int64)) > 0 for t in range(case.T)]).reshape(case.T, case.Nx, case.Nx)
    return own | viaA | viaB, own, viaA, viaB


def value_index(case, kind, t, r, c):
    """index of the stored entry (r, c) of Sx[t] (kind "x") or Su[t] (kind "u") in the mask-order value array"""
    o = 0
    for k, masks in (("x", case.Sx), ("u", case.Su)):
        for tt, M in enumerate(masks):
            M = sp.csc_matrix(M)
            if k == kind and tt == t:
                rows = M.indices[M.indptr[c]:M.indptr[c + 1]]
                p = int(np.searchsorted(rows, r))
                assert p < rows.size and rows[p] == r
                return o + M.indptr[c] + p
            o += M.nnz
    raise KeyError((kind, t))


def reach_of_phi(case, kind, t, r, c):
    """(rows, cols) whose sums hold a term from the stored-true Φx[t][r,c] (t ≥ 1) or Φu[t][r,c]: Boolean arrays [Nx]"""
    rows, cols = np.zeros(case.Nx, dtype=bool), np.zeros(case.Nx, dtype=bool)
    cols[c] = True
    if kind == "x":
        rows[r] = True                                          # the start value of entry (t−1, r, c)
        rows |= _stored(case.A)[:, r]                           # A[i,r]·Φx[t][r,c] in entry (t, i, c)
    else:
        rows |= _stored(case.B2).reshape(case.Nx, case.Nu)[:, r]
    return rows, cols


def phi_probe(case):
    """(t, r, c) of a stored-true Φx[t][r,c], t ≥ 1, that feeds a start value and, through a stored A[:, r], products as well"""
    PA = _stored(case.A)
    for t in range(1, case.T):
        hit = np.argwhere(_true(case.Sx[t]) & PA.any(axis=0)[:, None])
        if hit.size:
            return t, int(hit[0][0]), int(hit[0][1])
    raise LookupError("no such entry")


def reach_of_plant(case, which, i, k):
    """(rows, cols) whose sums hold a term from the stored A[i,k] (which "A") or B₂[i,k] ("B2")"""
    Px, Pu = boolean_phi(case)
    rows = np.zeros(case.Nx, dtype=bool)
    rows[i] = True
    cols = (Px[:case.T, k, :] if which == "A" else Pu[:, k, :]).any(axis=0)
    return rows, cols


def scaled_values(case, scale):
    """the mask-order value array with every read value multiplied (NaN poison kept)"""
    return np.where(np.isnan(case.values), np.nan, scale * case.values)


def bound(n, s):
    """2·N·2⁻⁵³·S"""
    return 2.0 * np.asarray(n, dtype=L) * L(2.0) ** -53 * np.asarray(s, dtype=L)


def check_against_twin(got, twin, what):
    """device (or any double evaluation) against the twin, every output within the twin's own bound; returns the largest ratio
    error / bound met (0 where both are exactly equal)"""
    worst = 0.0
    for key, nk, sk in (("row_l1", "row_n", "row_s"), ("col_l1", "col_n", "col_s")):
        b = bound(twin[nk][:, None], twin[sk])
        err = np.abs(np.asarray(got[key], dtype=L) - np.asarray(twin[key], dtype=L))
        assert np.isfinite(np.asarray(got[key])).all(), (what, key)
        assert (err <= b).all(), (what, key, float(err.max()), float(b.max()))
        worst = max(worst, float(np.max(np.where(err > 0, err / np.maximum(b, L(1e-300)), 0))))
    for row, key in enumerate(("l1", "e1")):
        b = bound(twin["tot_n"][row], twin["tot_s"][row])
        err = np.abs(np.asarray(got[key], dtype=L) - np.asarray(twin[key], dtype=L))
        assert (err <= b).all(), (what, key, float(err.max()), float(b.max()))
    return worst
