"""Operators, frequency lists and the references shared by tests/test_norms_host.py and tests/test_gpu_norms.py (a plain module
like closed_loop_cases.py; not a conftest, and free of HIP: nothing here loads the library).

The operation under test is the one of csrc/sls_norms.h.  Rows are the Nx state rows followed by the Nu input rows, N = Nx + Nu,

    G[t] = diag(cz) · [Φx[t]; Φu[t]] · diag(b),  t = 0 … T−1        G(ω) = Σ_t G[t] · e^{−iωt}

    row_l1[i] = Σ_t Σ_j |G[t][i,j]|     col_l1[j] = Σ_t Σ_i |G[t][i,j]|     totals = (max row_l1, max col_l1)
    sigma(ω)  = ‖G(ω)·v‖₂ after `iters` steps v ← G(ω)ᴴ·G(ω)·v / ‖·‖₂ from v₀[j] = 1 + (uint32)(j·2654435761)·2⁻³²

The operators are those of closed_loop_cases.py — the row-length ladder (Nx 24, Nu 6, T 24: rows of 0 … 576 entries, every
unroll boundary of the 64 entry slots) and the small cases T1, T2, Nu0 — with one difference: Φx[0] IS part of this operator, so
its diagonal gets finite values (random in [0.5, 1.5]) where the simulator's cases carry NaN.  `values` stays NaN on every
stored-false entry.  HOLES adds what those four lack: a row and a column with no stored-true entry at all.

Tolerances.
* 𝓛₁: a sum of n non-negative terms in any order has relative error ≤ (n − 1)·u, u = 2⁻⁵³; a weighted entry carries two more
  roundings.  L1_RTOL(n) = 4·(n + 2)·u, with n the longest row or column of the case.
* σ against the long-double power iteration at the same iters: HINF_RTOL = max(8 × the worst relative deviation of a plain
  complex128 NumPy run of the same iteration from the long-double one, 64·u).  Measured over every (case, ω) of PARITY below at
  PARITY_ITERS: see HINF_PLAIN_DEVIATION.  test_norms_host.py measures it again on every run and asserts it stays below the bound.
* σ against σ_max of the SVD: relative 1e-9, at an (ω, iters) where the reference's own (σ₂/σ₁)^(2·iters) ≤ 1e-12
  (SVD_OMEGAS / SVD_ITERS; test_norms_host.py asserts the condition for every pair — a clustered pair is replaced here, never
  skipped there)."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import closed_loop_cases as clc

L = np.longdouble
CL = np.clongdouble
U = 2.0 ** -53
SVD_RTOL = 1e-9
SVD_GAP = 1e-12

ALL = ("ladder",) + clc.SMALL + ("HOLES",)
HOLES_NX, HOLES_NU, HOLES_T = 9, 3, 3
HOLES_EMPTY_ROW_X, HOLES_EMPTY_ROW_U, HOLES_EMPTY_COL = 2, 1, 4


def _holes():
    """random masks on Nx 9, Nu 3, T 3 with state row 2, input row 1 and column 4 cleared in every slice (Φx[0] is the
    identity without (2,2) and (4,4)); one stored-false entry sits in the empty column"""
    rng = np.random.default_rng(77)
    Nx, Nu, T = HOLES_NX, HOLES_NU, HOLES_T
    Mx = [np.eye(Nx, dtype=bool)] + [rng.random((Nx, Nx)) < 0.5 for _ in range(T - 1)]
    Mu = [rng.random((Nu, Nx)) < 0.6 for _ in range(T)]
    for M in Mx:
        M[HOLES_EMPTY_ROW_X, :] = False
        M[:, HOLES_EMPTY_COL] = False
    for M in Mu:
        M[HOLES_EMPTY_ROW_U, :] = False
        M[:, HOLES_EMPTY_COL] = False
    Sx, Su = [clc._csc_mask(M) for M in Mx], [clc._csc_mask(M) for M in Mu]
    Sx[1] = clc._store_false(Sx[1], 0, HOLES_EMPTY_COL)
    return Sx, Su


def _from_masks(Sx, Su, rng):
    """values: distinct random numbers, NaN on stored-false entries; G: the dense [T, N, Nx] float64 operator, zero elsewhere"""
    T, Nx, Nu = len(Sx), Sx[0].shape[0], Su[0].shape[0]
    G = np.zeros((T, Nx + Nu, Nx))
    dev = []
    for masks, r0 in ((Sx, 0), (Su, Nx)):
        for t, M in enumerate(masks):
            keep = np.asarray(M.data, dtype=bool)
            cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
            v = rng.uniform(-1.0, 1.0, M.nnz)
            G[t, r0 + M.indices[keep], cols[keep]] = v[keep]
            dev.append(np.where(keep, v, np.nan))
    return G, np.concatenate(dev) if dev else np.zeros(0)


def case(name):
    """Record with Sx, Su, Nx, Nu, N, T, values (mask order, NaN where the operator must not read), G [T, N, Nx] (float64, what
    the values say), n_entries, row_len [N], col_len [Nx]."""
    if name == "HOLES":
        Sx, Su = _holes()
        G, values = _from_masks(Sx, Su, np.random.default_rng(78))
    else:
        c = clc.ladder() if name == "ladder" else clc.small_case(name)
        Sx, Su = c.Sx, c.Su
        Nx = c.Nx
        assert Sx[0].nnz == Nx and not np.isfinite(c.values[:Nx]).any()      # the identity mask, poisoned for the simulator
        d = np.random.default_rng(300 + ALL.index(name)).uniform(0.5, 1.5, Nx)
        values = c.values.copy()
        values[:Nx] = d                                                      # Φx[0]: read here
        G = np.concatenate([c.Phix, c.Phiu], axis=1)
        G[0, :Nx, :Nx] = np.diag(d)
    T, Nx, Nu = len(Sx), Sx[0].shape[0], Su[0].shape[0]
    stored = G != 0
    assert int(stored.sum()) == int(np.isfinite(values).sum())
    values.setflags(write=False); G.setflags(write=False)
    return SimpleNamespace(name=name, Sx=Sx, Su=Su, Nx=Nx, Nu=Nu, N=Nx + Nu, T=T, values=values, G=G, n_entries=int(stored.sum()),
                           row_len=stored.sum(axis=(0, 2)), col_len=stored.sum(axis=(0, 1)))


def from_values(Sx, Su, values):
    """the same record from masks and a mask-order value array — a solved Φ downloaded from the device"""
    Sx, Su = [sp.csc_matrix(m) for m in Sx], [sp.csc_matrix(m) for m in Su]
    T, Nx, Nu = len(Sx), Sx[0].shape[0], Su[0].shape[0]
    G = np.zeros((T, Nx + Nu, Nx))
    stored = np.zeros(G.shape, dtype=bool)
    o = 0
    for masks, r0 in ((Sx, 0), (Su, Nx)):
        for t, M in enumerate(masks):
            M.sort_indices()
            keep = np.asarray(M.data, dtype=bool)
            cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
            v = np.asarray(values[o:o + M.nnz]); o += M.nnz
            G[t, r0 + M.indices[keep], cols[keep]] = v[keep]
            stored[t, r0 + M.indices[keep], cols[keep]] = True
    assert o == len(values)
    return SimpleNamespace(name="solved", Sx=Sx, Su=Su, Nx=Nx, Nu=Nu, N=Nx + Nu, T=T, values=np.asarray(values), G=G,
                           n_entries=int(stored.sum()), row_len=stored.sum(axis=(0, 2)), col_len=stored.sum(axis=(0, 1)))


def weights(c, seed=0):
    """random positive cz [N], b [Nx]"""
    rng = np.random.default_rng(900 + seed)
    return rng.uniform(0.25, 4.0, c.N), rng.uniform(0.25, 4.0, c.Nx)


def prescale(c, cz, b):
    """the mask-order value array times cz[row]·b[col] — the product formed first, as the library's load does — so that a run
    with NULL weights on it must agree with a weighted run on c.values to the rounding of one multiply per entry"""
    out = np.array(c.values)
    o = 0
    for masks, r0 in ((c.Sx, 0), (c.Su, c.Nx)):
        for M in masks:
            cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
            out[o:o + M.nnz] *= cz[r0 + M.indices] * b[cols]
            o += M.nnz
    return out


# ------------------------------------------------------------------ the references (long double)

def dense(c, cz=None, b=None):
    """G [T, N, Nx] in long double, weights applied in long double"""
    G = np.asarray(c.G, dtype=L)
    if cz is not None:
        G = np.asarray(cz, dtype=L)[None, :, None] * G
    if b is not None:
        G = G * np.asarray(b, dtype=L)[None, None, :]
    return G


def l1_reference(G):
    """(row_l1 [N], col_l1 [Nx]) of a dense long-double G"""
    A = np.abs(G)
    return A.sum(axis=(0, 2)), A.sum(axis=(0, 1))


def l1_rtol(c):
    return 4.0 * (max(int(c.row_len.max()), int(c.col_len.max())) + 2) * U


def at_omega(G, omega, dtype=CL):
    """G(ω) = Σ_t G[t]·e^{−iωt}: clongdouble from the long-double angle ω·t, or a plain complex128 evaluation"""
    real = L if dtype == CL else np.float64
    t = np.arange(G.shape[0], dtype=real)
    a = real(omega) * t
    tw = (np.cos(a) - 1j * np.sin(a)).astype(dtype)
    return np.tensordot(tw, np.asarray(G, dtype=real).astype(dtype), axes=(0, 0))


def v0(Nx):
    j = np.arange(Nx, dtype=np.uint64)
    return 1.0 + ((j * np.uint64(2654435761)) % np.uint64(2 ** 32)).astype(np.float64) * 2.0 ** -32


def _norm(x):
    return np.sqrt((x.real * x.real + x.imag * x.imag).sum())


def power_iteration(Gw, iters):
    """sigma after `iters` steps, in the dtype of Gw (clongdouble: the reference; complex128: the plain run HINF_RTOL is
    measured with)"""
    v = v0(Gw.shape[1]).astype(Gw.dtype)
    n = _norm(v)
    if n > 0:
        v = v / n
    H = Gw.conj().T
    for _ in range(iters):
        v = H @ (Gw @ v)
        n = _norm(v)
        if n == 0:
            return float(0.0)
        v = v / n
    return _norm(Gw @ v)


def sigma_reference(c, omegas, iters, cz=None, b=None):
    G = dense(c, cz, b)
    return np.array([power_iteration(at_omega(G, w), iters) for w in omegas], dtype=L)


def svd_top2(c, omega, cz=None, b=None):
    """(σ₁, σ₂) of G(ω) by np.linalg.svd in complex128"""
    s = np.linalg.svd(at_omega(dense(c, cz, b), omega).astype(np.complex128), compute_uv=False)
    return float(s[0]), float(s[1]) if len(s) > 1 else 0.0


def real_matrices(c, cz=None, b=None):
    """(Σ_t G[t], Σ_t (−1)ᵗ G[t]) in long double: G(0) and G(π)"""
    G = dense(c, cz, b)
    sign = np.where(np.arange(G.shape[0]) % 2 == 0, L(1), L(-1))
    return G.sum(axis=0), np.tensordot(sign, G, axes=(0, 0))


def rel(got, ref):
    """largest elementwise |got − ref| / |ref| (entries whose reference is 0 must be 0 exactly)"""
    got, ref = np.asarray(got, dtype=L), np.asarray(ref, dtype=L)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero = ref == 0
    assert not np.any(got[zero] != 0)
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / np.abs(ref[~zero])).max())


# ------------------------------------------------------------------ frequency lists

# parity with the long-double iteration: 0, π, ±ω pairs and generic angles, every case
PARITY_ITERS = 6
PARITY_OMEGAS = (0.0, np.pi, 0.3, -0.3, 1.1, 2.0, -2.0, 2.9, 0.01, 7.5)
# the lane-layout run on the ladder: 65 angles, the first nfreq of them per call
LAYOUT_NFREQ = (1, 2, 3, 5, 9, 17, 33, 64, 65)
LAYOUT_MAX_FREQ = 65
LAYOUT_ITERS = 4
LAYOUT_OMEGAS = tuple(float(x) for x in np.pi * (np.arange(65) * 0.6180339887498949 % 1.0) * np.where(np.arange(65) % 3 == 2, -1.0, 1.0))
MONOTONE_ITERS = (1, 2, 4, 8)
MONOTONE_OMEGAS = (0.0, 0.7, 2.4, np.pi)
# σ_max: (ω list, iters) per case, (σ₂/σ₁)^(2·iters) ≤ SVD_GAP for every pair (asserted in test_norms_host.py)
# (iterations the condition needs at each ω, from the reference's SVD — ladder: 167, 313, 167, 159, 110; T1, whose G(ω) does not
# depend on ω: 453; T2: 249, 263, 156; Nu0: 117, 67, 110; HOLES: 95, 67, 51)
SVD_OMEGAS = {"ladder": (0.0, np.pi, 0.713, 1.2435, 2.1717), "T1": (0.0, 1.0), "T2": (0.0, np.pi, 1.1109),
              "Nu0": (0.0, np.pi, 2.0391), "HOLES": (0.0, np.pi, 1.1109)}
SVD_ITERS = {"ladder": 320, "T1": 460, "T2": 270, "Nu0": 120, "HOLES": 100}
# worst relative deviation of the plain complex128 run from the long-double one over PARITY (all cases, weighted and not):
# measured 3.8e-16 (the weighted ladder); 8× that is below the floor, so the floor 64·u = 7.1e-15 is the tolerance
HINF_PLAIN_DEVIATION = 3.9e-16
HINF_RTOL = max(8.0 * HINF_PLAIN_DEVIATION, 64.0 * U)
