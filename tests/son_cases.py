"""Plants, describe() parsing and the oracle checks of tests/test_gpu_son_classes.py (a plain module like oracle_c.py; not a conftest).

The reference everywhere is the certified CPU oracle oracle/sls_son_oracle.py; the tolerances are the ones test_sum_of_norms.py
states: objective 1e-7 relative, ‖ΔΦ‖∞ ≤ 1e-6·max|Φ| per column, ‖Ez − f‖∞ ≤ 1e-9, objective ≥ oracle objective − oracle gap − 1e-9."""
import re

import numpy as np
import scipy.sparse as sp

NCU = 256                                   # the CU count the launch lists below are recorded for (MI355X)
WAVE_CAPS = (12, 16, 20, 24, 28, 32)        # ñx capacities of the six small one-wave classes (wave_class_of)
WAVE_NAMES = ("h2_column_wave_kernel<16,3>", "h2_column_wave_kernel<16,4>", "h2_column_wave_kernel<32,10>",
              "h2_column_wave_kernel<32,12>", "h2_column_wave_kernel<32,14>", "h2_column_wave_kernel<32,16>")
TILE_LDS = "h2_column_tile_kernel<block_in_LDS,dense_hessian_cg>"
TILE_WS = "h2_column_tile_kernel<block_in_workspace,dense_hessian_cg>"
TILE_BIG = "h2_column_tile_kernel<block_in_workspace,carve_in_workspace,dense_hessian_cg>"

KNOBS = ("SLS_MAX_PER_CU", "SLS_SON_TILE", "SLS_TILE_GLOBAL", "SLS_TILE_BIG", "SLS_NO_TWISTED", "SLS_WAVE64", "SLS_P_LDS",
         "SLS_FORCE_GENERAL", "SLS_TILE", "SLS_ABSORB", "SLS_TWISTED4", "SLS_VEC_GLOBAL", "SLS_VEC_LDS", "SLS_FULL_GRID",
         "SLS_TILE_LDS_MAXNT", "SLS_TILE_ONE_PER_CU", "SLS_GW_TWO", "SLS_TILE_WPE", "SLS_NO_TINY_FIRST", "SLS_TINY_FIRST")


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ plants

def _cut_chain(slc, T):
    """README dynamics on 13 states, an actuator on every state, state 6 cut out of the chain."""
    A = slc.workloads.chain_plant(13).A.tolil()
    for i, j in ((5, 6), (7, 6), (6, 5), (6, 7)):
        A[i, j] = 0.0
    A = A.tocsc(); A.eliminate_zeros()
    I = sp.identity(13, format="csc")
    P = slc.Plant(A, I, I)
    return P, list(slc.workloads.localization_masks(P.A, P.B2, 3, T, 3.0)), None


def _trivial(slc):
    """The plant of test_column_outside_its_own_index_set_is_trivial: A[:, 7] = 0, so column 7 is outside its own index set."""
    Nx = 8
    A = sp.diags(0.5 * np.ones(Nx - 1), -1).tocsc()
    P = slc.Plant(A, sp.identity(Nx, format="csc"), sp.identity(Nx, format="csc")[:, [0, 3]])
    return P, list(slc.workloads.localization_masks(A + sp.identity(Nx), P.B2, 3, 5, 1.0)), [[Nx - 1]]


def _inputless(slc):
    """The plant of test_columns_without_reachable_actuators: two actuators at one end, most columns have ñu = 0."""
    Nx, T, d = 14, 10, 3
    Pc = slc.workloads.chain_plant(Nx)
    P = slc.Plant(Pc.A, Pc.B1, sp.identity(Nx, format="csc")[:, [Nx - 2, Nx - 1]])
    return P, list(slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5)), None


def _localized(make, d, T, alpha):
    def build(slc):
        P = make(slc)
        return P, list(slc.workloads.localization_masks(P.A, P.B2, d, T, alpha)), None
    return build


PLANTS = {
    "chain40": _localized(lambda slc: slc.workloads.chain_plant(40), 7, 12, 1.5),
    "chain70": _localized(lambda slc: slc.workloads.chain_plant(70), 15, 12, 1.5),
    "chain400": _localized(lambda slc: slc.workloads.chain_plant(400), 9, 12, 1.5),
    "mixed400": _localized(lambda slc: slc.workloads.random_plant(400, 2, 2, seed=5), 2, 8, 1.5),
    **{f"cut13_T{T}": (lambda slc, T=T: _cut_chain(slc, T)) for T in (1, 2, 3, 4)},
    "trivial": _trivial,
    "inputless": _inputless,
}

_problems, _oracle = {}, {}
oracle_seconds = {}                         # CPU seconds spent in the oracle, per plant (reported by the GPU tests)


def problem(slc, name):
    """(P, S, groups, column of every mask entry) of a plant of the table; built once."""
    if name not in _problems:
        P, S, groups = PLANTS[name](slc)
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        _problems[name] = (P, S, groups, colidx)
    return _problems[name]


def oracle_column(slc, name, c):
    """The oracle's column c of a plant: dict(E, f, w, tslice, oi, z, dg).  Solved once per session, never modified."""
    if (name, c) not in _oracle:
        import time
        import sls_oracle as o
        import sls_son_oracle as son
        P, S, _, _ = problem(slc, name)
        t0 = time.perf_counter()
        Po = o.OraclePlant(P.A, P.B1, P.B2)
        E, f, w, tslice, oi = son._column_problem(Po, c, S[0], S[1])
        z, dg = son.solve_column(Po, c, S[0], S[1])
        z.setflags(write=False)
        _oracle[(name, c)] = dict(E=E, f=f, w=w, tslice=tslice, oi=oi, z=z, dg=dg)
        oracle_seconds[name] = oracle_seconds.get(name, 0.0) + time.perf_counter() - t0
    return _oracle[(name, c)]


def wave_class_of(n):
    """Index of the small one-wave class that holds an index set of n states, or None (tile kernel)."""
    for k, cap in enumerate(WAVE_CAPS):
        if n <= cap:
            return k
    return None


# ------------------------------------------------------------------ describe() text

_LAUNCH = re.compile(r"(h2_column_[a-z0-9_]+(?:<[^>]*>)?) nsub=(\d+) grid=(\d+) ")


def launches(desc):
    """describe() text → [(kernel with template arguments, nsub, grid)]."""
    out = []
    for seg in [s for s in desc.split(";") if s]:
        m = _LAUNCH.match(seg)
        assert m, (seg, desc)
        out.append((m.group(1), int(m.group(2)), int(m.group(3))))
    return out


def short(desc):
    """The pinned part of a describe(): kernel names with template arguments, nsub= and grid=, in launch order."""
    return ";".join(f"{k} nsub={n} grid={g}" for k, n, g in launches(desc))


# ------------------------------------------------------------------ one column against the oracle

def column_z(P, S, vals, colidx, c, oi):
    """The GPU's column c in the oracle's variable order, from the mask-order value array."""
    T = len(S[0])
    sel = np.flatnonzero(colidx == c)
    # mask order: Φx[0..T-1] then Φu[0..T-1], each CSC; rows of column c per matrix
    rows = np.concatenate([M.indices[M.indptr[c]:M.indptr[c + 1]] for M in S[0] + S[1]])
    which = np.concatenate([np.full(M.indptr[c + 1] - M.indptr[c], k) for k, M in enumerate(S[0] + S[1])])
    assert len(rows) == len(sel)
    lookup = {(int(k), int(r)): float(v) for k, r, v in zip(which, rows, vals[sel])}
    return np.array([lookup[(t + kind * T, int((oi["sx"] if kind == 0 else oi["su"])[r]))] for (t, kind, r, _) in oi["var_index"]])


def check_column(ref, z, stats=None, tag=None):
    """The four tolerances of test_sum_of_norms.py on one feasible column; returns (relative objective error, ‖ΔΦ‖∞/max|Φ|)."""
    E, f, w, tslice, z_o, dg = ref["E"], ref["f"], ref["w"], ref["tslice"], ref["z"], ref["dg"]
    assert np.all(np.isfinite(z)), tag
    res = np.abs(E @ z - f).max() if len(z) else 0.0
    obj = sum(np.linalg.norm((w * z)[idx]) for idx in tslice)
    eo = abs(obj - dg["obj"]) / max(dg["obj"], 1e-30)
    ez = np.abs(z - z_o).max() / max(np.abs(z_o).max(), 1e-300) if len(z) else 0.0
    if stats is not None:
        stats["obj"] = max(stats.get("obj", 0.0), eo); stats["phi"] = max(stats.get("phi", 0.0), ez)
        stats["res"] = max(stats.get("res", 0.0), res); stats["n"] = stats.get("n", 0) + 1
    assert res <= 1e-9, (tag, res)
    assert eo <= 1e-7, (tag, obj, dg["obj"])
    assert obj >= dg["obj"] - dg["gap"] - 1e-9, (tag, obj, dg["obj"], dg["gap"])
    assert ez <= 1e-6, (tag, ez)
    return eo, ez


def achievability(P, S, vals):
    """Φx[1] = I, Φx[t+1] = AΦx[t] + B2Φu[t], AΦx[T] + B2Φu[T] = 0 on the full system: the worst violation."""
    T = len(S[0])
    Phi, o = [], 0
    for M in S[0] + S[1]:
        Phi.append(sp.csc_matrix((vals[o:o + M.nnz], M.indices, M.indptr), shape=M.shape)); o += M.nnz
    Phix, Phiu = Phi[:T], Phi[T:]
    A, B2 = P.A.tocsc(), P.B2.tocsc()
    worst = abs(Phix[0] - sp.identity(P.Nx, format="csc")).max()
    for t in range(T - 1):
        worst = max(worst, abs(Phix[t + 1] - A @ Phix[t] - B2 @ Phiu[t]).max())
    return max(worst, abs(A @ Phix[T - 1] + B2 @ Phiu[T - 1]).max())
