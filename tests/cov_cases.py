"""Pair lists, references and tolerances shared by tests/test_cov_host.py and tests/test_gpu_cov.py (a plain module like
norms_cases.py, whose operators it reuses; not a conftest, and free of HIP: nothing here loads the library).

The operation under test is the one of csrc/sls_norms.h.  With G[t] = diag(cz)·[Φx[t]; Φu[t]]·diag(b), t = 0 … T−1,

    row_h2[i] = Σ_t Σ_j G[t][i,j]²     col_h2[j] = Σ_t Σ_i G[t][i,j]²     totals = (Σ_i row_h2[i], max_i row_h2[i])
    cov[p]    = Σ_t Σ_k G[t][i_p,k]·G[t][j_p,k]                            an entry of Σ = Σ_t G[t]·G[t]ᵀ

Cases: norms_cases.ALL.  `ladder` carries the load (Nx 24, Nu 6, T 24: rows of 0 … 576 entries, so the pairs straddle every
boundary of the 64-entry chunks and either list can be the shorter one); T1, T2, Nu0; HOLES (an empty state row, an empty input
row, an empty column).  The reference is the dense long-double Σ of the case; it shares no code with the library.

Tolerances, derived (u = 2⁻⁵³):
* row_h2 / col_h2: a sum of n non-negative terms in any order has relative error ≤ (n − 1)·u, each term v·v carries one rounding
  (the fma's) and a weighted v two more: relative 4·(n + 2)·u with n the longest row or column of the case — norms_cases.l1_rtol.
* cov[p]: a signed sum of n_p products in an arbitrary order, |error| ≤ (n_p − 1)·u·Σ|terms| to first order, plus the two weight
  roundings of each factor: absolute 4·(n_p + 3)·u·Σ_k |G_i,k·G_j,k|, with n_p the number of shared keys and the sum of
  absolute products taken from the long-double reference.  A pair without a shared key has tolerance 0: exactly 0.0 is required.
* totals[0]: every entry once, then the N row sums: relative 4·(n_entries + N + 2)·u."""
from types import SimpleNamespace

import numpy as np

import norms_cases as nc

L = nc.L
U = nc.U
ALL = nc.ALL


def reference(c, cz=None, b=None):
    """long double: row_h2 [N], col_h2 [Nx], C = Σ_t G[t]·G[t]ᵀ [N, N], Cabs = Σ_t |G[t]|·|G[t]|ᵀ, shared [N, N] (keys in common)"""
    G = nc.dense(c, cz, b)
    S = (np.asarray(c.G) != 0).astype(np.int64)
    A = np.abs(G)
    return SimpleNamespace(row=(G * G).sum(axis=(0, 2)), col=(G * G).sum(axis=(0, 1)), C=np.einsum("tik,tjk->ij", G, G),
                           Cabs=np.einsum("tik,tjk->ij", A, A), shared=np.einsum("tik,tjk->ij", S, S))


def h2_rtol(c):
    return nc.l1_rtol(c)


def total_rtol(c):
    return 4.0 * (c.n_entries + c.N + 2) * U


def cov_atol(ref, pi, pj):
    """absolute tolerance of every pair of a list, long double"""
    return 4.0 * (ref.shared[pi, pj].astype(L) + 3) * L(U) * ref.Cabs[pi, pj]


def cov_error(got, ref, pi, pj):
    """largest |got − ref| / tolerance over a pair list (0 for an empty one); a pair of tolerance 0 must be exactly 0.0"""
    got = np.asarray(got, dtype=L)
    assert got.shape == np.shape(pi) == np.shape(pj)
    err, tol = np.abs(got - ref.C[pi, pj]), cov_atol(ref, pi, pj)
    exact = tol == 0
    assert not np.any(got[exact] != 0), "a pair without a shared key must give exactly 0.0"
    return float((err[~exact] / tol[~exact]).max()) if (~exact).any() else 0.0


# ------------------------------------------------------------------ pair lists (0-based)

def all_pairs(c):
    """all N·(N + 1)/2 unordered pairs, i ≤ j, by rows"""
    i, j = np.triu_indices(c.N)
    return i.astype(np.int64), j.astype(np.int64)


def empty_rows(c):
    return np.flatnonzero(np.asarray(c.row_len) == 0)


def pair_lists(c):
    """name → (pairs_i, pairs_j): all pairs; the same list reversed with (i, j) swapped; one pair; duplicates; (state row, input
    row) pairs; every pair that involves an empty row.  A list a case cannot have (no input rows, no empty row) is left out."""
    i, j = all_pairs(c)
    rng = np.random.default_rng(4000 + ALL.index(c.name) if c.name in ALL else 4099)
    longest, second = (int(x) for x in np.argsort(np.asarray(c.row_len))[::-1][:2])
    dup = rng.integers(0, len(i), 3 * c.N)
    dup[1::3] = dup[0::3]                                               # neighbours in the list that are the same pair
    out = {"all": (i, j), "reversed": (j[::-1].copy(), i[::-1].copy()), "one": (np.array([longest]), np.array([second])),
           "duplicates": (i[dup], j[dup])}
    if c.Nu:
        s, u = np.meshgrid(np.arange(c.Nx), c.Nx + np.arange(c.Nu), indexing="ij")
        out["state_input"] = (s.ravel().astype(np.int64), u.ravel().astype(np.int64))
    e = empty_rows(c)
    if len(e):
        a, o = np.meshgrid(e, np.arange(c.N), indexing="ij")
        out["empty"] = (np.concatenate([a.ravel(), o.ravel()]).astype(np.int64), np.concatenate([o.ravel(), a.ravel()]).astype(np.int64))
    return out
