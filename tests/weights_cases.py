"""Plants, weights and case table shared by tests/test_weights_host.py and tests/test_gpu_weights.py (a plain module like
update_cases.py, which it imports and does not edit; not a conftest).

The feature under test is sls_plan_update_weights: new LQR weights C1 = [diag(c); 0], D12 = [0; diag(d)] for a live plan built with
SLS_PLAN_WEIGHTS_UPDATABLE.  `weighted(P, seed)` draws c and d uniformly from [0.5, 2]; the cases are those of update_cases.CASES
(plants, columns, masks, knobs, route substrings).  The reference is the NumPy oracle with the weights (oracle_c.c_oracle_flat
drops C1 / D12 and cannot serve).  With that oracle, on the CPU: the chain-70 `t4` columns at d 9, T 7 move Φ by 0.83 from identity
weights to seed 11 and by 2.6 from seed 11 to seed 12, the grid-10 `tile` columns by 0.24 and 0.36 — an update that did nothing
cannot pass the 1e-3 "moved" check against TOL = 1e-8.  Feasibility does not depend on the weights: every column of these cases
stays feasible (the oracle's constraint residual is asserted where the reference is computed)."""
import numpy as np
import scipy.sparse as sp

import update_cases as uc
from conftest import flat_phi

SEED_A, SEED_B = 11, 12
GPU_CASES = ("t4", "t4_long", "t4_zeros", "t2", "wave", "tile")       # `son` is compared with a fresh plan only
CASES = {cid: uc.CASES[cid] for cid in GPU_CASES + ("son",)}


def diagonals(P, seed):
    """(c, d): the draws of `weighted` — c first, then d"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, P.Nx), rng.uniform(0.5, 2.0, P.Nu)


def lqr_blocks(Nx, Nu, c, d):
    """C1 = [diag(c); 0] (Nz×Nx) and D12 = [0; diag(d)] (Nz×Nu), Nz = Nx + Nu, one stored entry per column (zeros kept)"""
    C1 = sp.csc_matrix((np.asarray(c, dtype=np.float64), np.arange(Nx), np.arange(Nx + 1)), shape=(Nx + Nu, Nx))
    D12 = sp.csc_matrix((np.asarray(d, dtype=np.float64), Nx + np.arange(Nu), np.arange(Nu + 1)), shape=(Nx + Nu, Nu))
    return C1, D12


def with_weights(P, c, d):
    C1, D12 = lqr_blocks(P.Nx, P.Nu, c, d)
    return type(P)(P.A, P.B1, P.B2, C1, 0, D12)


def weighted(P, seed):
    """Plant(A, B1, B2, C1 = [diag(c); 0], 0, D12 = [0; diag(d)]) with c, d ~ U[0.5, 2] from `seed`"""
    return with_weights(P, *diagonals(P, seed))


_oracle_cache = {}


def oracle_flat(slc, cid, seed):
    """Φ of the NumPy oracle on weighted(P, seed) (seed None: P itself) for the case's columns, in mask order (zeros elsewhere);
    every column's constraint residual is asserted small.  Computed once per (plant, columns, masks, seed), read-only."""
    import sls_oracle as o
    name, cols, dTa = uc.CASES[cid][:3]
    key = (name, cols, dTa, seed)
    if key not in _oracle_cache:
        P, S, groups = uc.case(slc, cid)[:3]
        Q = P if seed is None else weighted(P, seed)
        Po = o.OraclePlant(Q.A, Q.B1, Q.B2, C1=Q.C1, D12=Q.D12)
        ox, ou, diags = o.SLS_H2(Po, S, groups, return_diag=True)
        assert max(dg["resid"] for dg in diags) < 1e-9, [dg["resid"] for dg in diags]
        want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
        want.setflags(write=False)
        _oracle_cache[key] = want
    return _oracle_cache[key]


def index_sets(P, S):
    """(s_x, s_u) per column: the rows of ((𝓢x[end]·(A≠0))[:, c]) and ((𝓢u[end]·(A≠0))[:, c]), ascending (src/reduction.jl:14)"""
    An = (sp.csc_matrix(P.A) != 0).astype(np.int64)
    out = []
    for Sm in (S[0][-1], S[1][-1]):
        M = sp.csc_matrix(sp.csc_matrix(Sm).astype(np.int64) @ An)
        out.append([np.sort(M.indices[M.indptr[c]:M.indptr[c + 1]]) for c in range(M.shape[1])])
    return out[0], out[1]
