"""Operators and the reference shared by tests/test_closed_loop_host.py and tests/test_gpu_closed_loop_edges.py (a plain module
like son_cases.py and objective_cases.py; not a conftest, and free of HIP: nothing here loads the library).

The operation under test is the recursion in the header comment of csrc/sls_closed_loop.hip,

    β[:,t+1] = Σ_{τ=1..min(t,T−1)} Φx[τ+1]·(x[:,t+1−τ] − β[:,t+1−τ])
    u[:,t]   = Σ_{τ=1..min(t,T)}   Φu[τ]  ·(x[:,t+1−τ] − β[:,t+1−τ])
    x[:,t+1] = A·x[:,t] + B₁·w(t) + B₂·u[:,t]

None of the operators below comes from a solve: the simulator takes any masks and any values, so the masks are chosen for
what the kernel does with them.  closed_loop_step_kernel<SCN> spreads a row of the operator over NE = 64/SCN entry lanes;
each lane runs a four-way unrolled body while e + 3·NE < end and a tail loop after it, so the code a row takes depends on its
length relative to NE, 3·NE + 1 and 4·NE — a different set of lengths for each of the seven SCN."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

NES = (1, 2, 4, 8, 16, 32, 64)              # entry lanes per scenario slot, NE = 64/SCN for SCN = 64 … 1

# ------------------------------------------------------------------ the row-length ladder

LADDER_NX, LADDER_NU, LADDER_T, LADDER_STEPS = 24, 6, 24, 60
# stored-true entries of operator row i: β rows gather Φx[τ+1], τ = 1…T−1 (capacity (T−1)·Nx = 552), u rows Φu[τ], τ = 1…T (T·Nx = 576)
LADDER_BETA = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257, 515)
LADDER_U = (0, 49, 97, 192, 256, 576)
LADDER_SHARED, LADDER_ORPHAN = 4, 2         # actuator 4 (256 entries) drives two states, actuator 2 (97 entries) drives none
LADDER_EMPTY_A_ROW = 13


def _pick_rows(rng, counts, nlags, Nx):
    """M[lag, row, col]: row i holds counts[i] entries at random (lag, col) positions"""
    M = np.zeros((nlags, len(counts), Nx), dtype=bool)
    for i, n in enumerate(counts):
        pick = rng.choice(nlags * Nx, size=n, replace=False)
        M[pick // Nx, i, pick % Nx] = True
    return M


def _csc_mask(M):
    m = sp.csc_matrix(M.astype(bool))
    m.sort_indices()
    return m


def _store_false(mask, r, c):
    """the mask with a stored-false entry added at the free position (r, c)"""
    assert not mask[r, c]
    d = mask.toarray()
    d[r, c] = True
    m = _csc_mask(d)
    k = m.indptr[c] + int(np.searchsorted(m.indices[m.indptr[c]:m.indptr[c + 1]], r))
    assert m.indices[k] == r
    m.data[k] = False
    return m


def row_lengths(Sx, Su):
    """Stored-TRUE entries per operator row, counted from the masks: (β rows over Sx[1:], u rows over Su)."""
    def count(masks, nrows):
        n = np.zeros(nrows, dtype=np.int64)
        for m in masks:
            m = sp.csc_matrix(m)
            np.add.at(n, m.indices[np.asarray(m.data, dtype=bool)], 1)
        return n
    return count(Sx[1:], Sx[0].shape[0]), count(Su, Su[0].shape[0])


def _values(rng, Sx, Su):
    """Distinct random values, |v| ≤ 0.5/√(length of the entry's operator row); Sx[0] holds Φx[1] = I (not part of the operator)"""
    nb, nu = row_lengths(Sx, Su)
    def draw(m, n):
        return rng.uniform(-1.0, 1.0, m.nnz) * 0.5 / np.sqrt(np.maximum(n[m.indices], 1))
    vals_x = [np.ones(Sx[0].nnz)] + [draw(m, nb) for m in Sx[1:]]
    vals_u = [draw(m, nu) for m in Su]
    flat = np.concatenate(vals_x[1:] + vals_u)
    assert len(np.unique(np.abs(flat))) == len(flat)
    return vals_x, vals_u


def _finish(A, B1, B2, Sx, Su, vals_x, vals_u, steps):
    """The case record.  `values` is the mask-order value array as the device gets it: NaN wherever the operator must not
    read (all of Sx[0], every stored-false entry).  Phix / Phiu are the dense FP64 Φ the reference uses, zero there."""
    Nx, Nu, T = A.shape[0], B2.shape[1], len(Sx)
    Phix, Phiu = np.zeros((T, Nx, Nx)), np.zeros((T, Nu, Nx))
    dev = []
    for D, masks, vals in ((Phix, Sx, vals_x), (Phiu, Su, vals_u)):
        for t in range(T):
            M, v = masks[t], vals[t]
            keep = np.asarray(M.data, dtype=bool)
            cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
            D[t, M.indices[keep], cols[keep]] = v[keep]
            dev.append(np.full(M.nnz, np.nan) if D is Phix and t == 0 else np.where(keep, v, np.nan))
    return SimpleNamespace(A=sp.csc_matrix(A), B1=sp.csc_matrix(B1), B2=sp.csc_matrix(B2), Sx=Sx, Su=Su, Nx=Nx, Nu=Nu,
                           Nw=B1.shape[1], T=T, steps=steps, Phix=Phix, Phiu=Phiu,
                           values=np.concatenate(dev),
                           n_entries=int(sum(np.count_nonzero(m.data) for m in Sx[1:]) + sum(np.count_nonzero(m.data) for m in Su)))


def ladder():
    """Nx = 24, Nu = 6, T = 24: operator row i holds LADDER_BETA[i] (β) / LADDER_U[j] (u) entries at random (lag, column)
    positions.  One mask entry is stored false; actuator LADDER_SHARED drives two states, LADDER_ORPHAN none, actuator 0
    (an empty u row) drives one; state LADDER_EMPTY_A_ROW has an empty A row; B₁ = I."""
    rng = np.random.default_rng(2024)
    Nx, Nu, T = LADDER_NX, LADDER_NU, LADDER_T
    Mx = _pick_rows(rng, LADDER_BETA, T - 1, Nx)
    Mu = _pick_rows(rng, LADDER_U, T, Nx)
    Sx = [sp.identity(Nx, dtype=bool, format="csc")] + [_csc_mask(Mx[t]) for t in range(T - 1)]
    Su = [_csc_mask(Mu[t]) for t in range(T)]
    Sx[5] = _store_false(Sx[5], 10, int(np.flatnonzero(~Mx[4][10])[0]))      # row 10 keeps its 16 stored-true entries
    A = (sp.random(Nx, Nx, 0.2, random_state=np.random.default_rng(1)) * 0.3).tolil()
    A[LADDER_EMPTY_A_ROW, :] = 0.0
    A = A.tocsc(); A.eliminate_zeros(); A.sort_indices()
    B2 = sp.lil_matrix((Nx, Nu))
    B2[3, 0] = 0.8                                              # an actuator whose u row is empty: contributes exactly 0
    B2[8, 1] = 0.7; B2[17, 3] = -0.9; B2[21, 5] = 0.6
    B2[5, LADDER_SHARED] = 1.0; B2[20, LADDER_SHARED] = -0.5
    B2 = B2.tocsc()
    vals_x, vals_u = _values(rng, Sx, Su)
    return _finish(A, sp.identity(Nx, format="csc"), B2, Sx, Su, vals_x, vals_u, LADDER_STEPS)


def ladder_w(nscen):
    """dense random disturbance on every step, [steps, Nw, nscen]"""
    return np.random.default_rng(1000 + 7 * nscen).standard_normal((LADDER_STEPS, LADDER_NX, nscen))


# ------------------------------------------------------------------ small shapes: T = 1, T = 2, Nu = 0

SMALL = ("T1", "T2", "Nu0")
SMALL_NX, SMALL_STEPS = 9, 12


def small_case(name):
    """random masks and values on Nx = 9, steps = 12.  T1: no β entries at all, one u lag.  T2: one β lag.
    Nu0: B₂ is Nx × 0 and every Su[t] is 0 × Nx."""
    Nx = SMALL_NX
    T, Nu = {"T1": (1, 3), "T2": (2, 3), "Nu0": (4, 0)}[name]
    rng = np.random.default_rng(SMALL.index(name) + 40)
    Sx = [sp.identity(Nx, dtype=bool, format="csc")] + [_csc_mask(rng.random((Nx, Nx)) < 0.4) for _ in range(T - 1)]
    Su = [_csc_mask(rng.random((Nu, Nx)) < 0.5) for _ in range(T)]
    A = sp.random(Nx, Nx, 0.3, random_state=np.random.default_rng(5), format="csc") * 0.3
    B2 = sp.lil_matrix((Nx, Nu))
    for j in range(Nu):
        B2[3 * j + 1, j] = 1.0 - 0.3 * j
    vals_x, vals_u = _values(rng, Sx, Su)
    return _finish(A, sp.identity(Nx, format="csc"), B2.tocsc(), Sx, Su, vals_x, vals_u, SMALL_STEPS)


def small_w(nscen):
    return np.random.default_rng(77 + nscen).standard_normal((SMALL_STEPS, SMALL_NX, nscen))


# ------------------------------------------------------------------ the reference

def reference(case, w, steps=None, nscen=None, scale=1.0):
    """The three lines above with dense Φ in np.longdouble, all scenarios at once.  w: [steps, Nw, nscen] or None (then
    `nscen` says how many).  Returns x [steps, Nx, nscen], u [steps, Nu, nscen] as longdouble; row k is the README's
    x[:,k+1], u[:,k+1], so x[0] = 0 and u[steps−1] = 0 (never assigned).  `scale` multiplies Φ."""
    L = np.longdouble
    steps = case.steps if steps is None else steps
    if w is not None:
        w = np.asarray(w, dtype=L)
        assert w.shape[:2] == (steps, case.Nw)
        nscen = w.shape[2]
    A, B1, B2 = (np.asarray(M.toarray(), dtype=L) for M in (case.A, case.B1, case.B2))
    Phix, Phiu = np.asarray(case.Phix, dtype=L) * L(scale), np.asarray(case.Phiu, dtype=L) * L(scale)
    T = case.T
    x = np.zeros((steps, case.Nx, nscen), dtype=L); beta = np.zeros_like(x)
    u = np.zeros((steps, case.Nu, nscen), dtype=L)
    for t in range(1, steps):                                   # the README's 1-based t; x[:,t+1] is row t
        b = np.zeros((case.Nx, nscen), dtype=L)
        for tau in range(1, min(t, T - 1) + 1):
            b += Phix[tau] @ (x[t - tau] - beta[t - tau])       # Φx[τ+1] 1-based = slice τ
        beta[t] = b
        uu = np.zeros((case.Nu, nscen), dtype=L)
        for tau in range(1, min(t, T) + 1):
            uu += Phiu[tau - 1] @ (x[t - tau] - beta[t - tau])
        u[t - 1] = uu
        x[t] = A @ x[t - 1] + B2 @ uu
        if w is not None:
            x[t] += B1 @ w[t - 1]
    return x, u


def sparse_phi(case, scale=1.0):
    """Φ as the lists of sparse matrices oracle.closed_loop takes"""
    return [sp.csc_matrix(scale * M) for M in case.Phix], [sp.csc_matrix(scale * M) for M in case.Phiu]


def rel_err(got, ref):
    """max |got − ref| over everything, relative to max(1, max|ref|)"""
    ref = np.asarray(ref, dtype=np.longdouble)
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / max(1.0, float(np.abs(ref).max())))
