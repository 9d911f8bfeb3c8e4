"""Plants, perturbation and case table shared by tests/test_plant_update_host.py and tests/test_gpu_plant_update.py (a plain module
like objective_cases.py; not a conftest).

The feature under test is sls_plan_update_plant: new values of A / B2 for a live plan.  `perturb` scales every stored value by a
factor in [0.8, 1.2]: non-zeros stay non-zero and stored zeros stay zero, so the perturbed plant has the plan's non-zero pattern
and a plan updated to it must be equivalent to a plan built from it.  With this perturbation (seed 5) the C restatement of the
oracle (oracle_c.c_oracle_flat) calls every column of every case below feasible, before and after, and Φ moves by 0.13 to 17.9 —
an update that did nothing cannot pass.  (chain_plant(23) at d 3 is not used: the oracle calls 14 of its columns infeasible.)"""
import numpy as np
import scipy.sparse as sp

NB = 64
BANDED_COLS = tuple(range(20, 44, 3))
T4 = "h2_column_twisted4_kernel<32,12>"


def banded(slc, stored_zeros=False):
    """The banded plant of test_gpu_twisted4_prepared.py (its `_banded`, restated): A = I ± 0.2 on the ±1 and ± 0.1 on the ±2
    diagonals, B2 = I + 0.5 on the −1 and − 0.25 on the −2 diagonal; with `stored_zeros`, explicit 0.0 on the ±3 diagonals of A
    and the −3 diagonal of B2 (rows of 7 / 4 stored entries, 5 / 3 of them non-zero)."""
    def E(k, v):
        return sp.diags(v * np.ones(NB - abs(k)), k)
    A = (sp.identity(NB) + E(1, 0.2) - E(-1, 0.2) + E(2, 0.1) - E(-2, 0.1)).tocoo()
    B2 = (sp.identity(NB) + E(-1, 0.5) - E(-2, 0.25)).tocoo()
    if stored_zeros:
        i = np.arange(NB - 3)
        A = sp.coo_matrix((np.r_[A.data, np.zeros(2 * (NB - 3))], (np.r_[A.row, i, i + 3], np.r_[A.col, i + 3, i])), shape=(NB, NB))
        B2 = sp.coo_matrix((np.r_[B2.data, np.zeros(NB - 3)], (np.r_[B2.row, i + 3], np.r_[B2.col, i])), shape=(NB, NB))
    A, B2 = sp.csc_matrix(A), sp.csc_matrix(B2)          # COO → CSC keeps explicitly stored zeros
    A.sort_indices(); B2.sort_indices()
    return slc.Plant(A, sp.identity(NB, format="csc"), B2)


def perturb(P, seed=5):
    """A and B2 with every stored value scaled by a factor in [0.8, 1.2] (A's draws first, then B2's); same stored pattern."""
    rng = np.random.default_rng(seed)
    A, B2 = sp.csc_matrix(P.A).copy(), sp.csc_matrix(P.B2).copy()
    A.data *= rng.uniform(0.8, 1.2, A.nnz)
    B2.data *= rng.uniform(0.8, 1.2, B2.nnz)
    return type(P)(A, P.B1, B2)


def with_values(P, A_data=None, B2_data=None):
    """The plant with the stored values of A / B2 replaced (same stored pattern, stored zeros kept)."""
    A, B2 = sp.csc_matrix(P.A).copy(), sp.csc_matrix(P.B2).copy()
    if A_data is not None:
        A.data[:] = A_data
    if B2_data is not None:
        B2.data[:] = B2_data
    return type(P)(A, P.B1, B2)


# id: (plant, columns, (d, T, α), environment knobs, substring of Plan.describe() that names the route, objective)
_CHAIN7 = (0, 1, 2, 35, 67, 68, 69)
_CHAIN9 = (0, 1, 2, 3, 35, 66, 67, 68, 69)
CASES = {
    "t4":       ("chain70", _CHAIN7, (9, 7, 1.5), {}, T4, "h2"),
    "t4_long":  ("chain70", _CHAIN9, (9, 29, 1.5), {}, "h2_column_twisted4_kernel", "h2"),
    "t4_zeros": ("banded_zeros", BANDED_COLS, (4, 12, 1.0), {}, "h2_column_twisted4_kernel", "h2"),
    "t2":       ("chain70", _CHAIN7, (9, 7, 1.5), {"SLS_TWISTED4": "0"}, "h2_column_twisted_kernel", "h2"),
    "wave":     ("chain70", tuple(range(70)), (9, 7, 1.5), {"SLS_NO_TWISTED": "1"}, "h2_column_wave_kernel", "h2"),
    "tile":     ("grid10", (0, 9, 45, 55, 90, 99, 4, 50), (3, 4, 8.0), {}, "h2_column_tile_kernel", "h2"),
    "son":      ("chain70", tuple(range(70)), (9, 4, 1.5), {"SLS_NO_TWISTED": "1"}, "h2_column_wave_kernel", "sum_of_norms"),
}
KNOBS = ("SLS_TWISTED4", "SLS_NO_TWISTED")

_plants = {}


def case(slc, cid):
    """(P, S, groups, knobs, route, objective) of a case; plants and masks are built once and never modified."""
    name, cols, (d, T, alpha), knobs, route, objective = CASES[cid]
    key = (name, d, T, alpha)
    if key not in _plants:
        if name == "chain70":
            P = slc.workloads.chain_plant(70); M = P
        elif name == "grid10":
            P = slc.workloads.grid_plant(10, 1); M = P
        else:
            P = banded(slc, stored_zeros=True); M = banded(slc)          # masks of the plain banded plant
        S = slc.workloads.localization_masks(M.A, M.B2, d, T, alpha)
        _plants[key] = (P, [list(S[0]), list(S[1])])
    P, S = _plants[key]
    return P, S, [[c] for c in cols], knobs, route, objective


def set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
