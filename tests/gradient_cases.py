"""The cases and the reference of tests/test_gradient_host.py and tests/test_gpu_gradient.py (a plain module like
objective_cases.py; not a conftest).

The reference shares no code with the library: per column it takes the dense (E, f, M, m₀) of `sls_oracle.assemble_group`,
solves the equality-constrained least squares by the null-space method, takes the multiplier of minimum norm
    μ = lstsq(Eᵀ, 2Mᵀ(Mz + m₀), rcond = 1e-11)
and applies the envelope-theorem formulas of include/sls_mi355x.h (sls_plan_gradient):
    ∂J/∂A[a,b]  = Σ_j c_j Σ_{k=1..T} μ_{j,k}[a]·x_{j,k−1}[b],      ∂J/∂B2[a,m] = Σ_j c_j Σ_{k=1..T} μ_{j,k}[a]·u_{j,k−1}[m]
over the stored entries with both indices inside the column's index sets, and for the diagonals of C1 / D12
    ∂J/∂c1[i] = 2 Σ_j c_j Σ_t r_{j,t}[i]·b_j·x_{j,t}[i]   with r = Mz + m₀ (= 2·c1[i]·b_j²·Σ_t x² when D11 = 0).
A column whose constraints have no solution (‖Ez − f‖∞ > 1e-8) contributes 0 and is counted.

Cases, the smallest shapes at which the code can still go wrong:
  chain17     17-state README-type chain, d = 6, T = 16, α = 1.5, every stored value of A and B2 times U[0.8, 1.2]
  T1, T2      the same A at T = 1 and T = 2 (block row T is the first, or the second, dynamic row).  With the README's six
              actuators and masks no column has a localized Φ at these horizons, whatever d: u_t is confined to fewer rows than
              A·x_t reaches, and a gradient of skipped columns checks nothing.  So these two cases put an actuator on every
              state (B2 = a perturbed identity) and give the input masks one ring more than the state masks,
              Sx[t] = (A≠0)^t, Su[t] = (B2ᵀ≠0)(A≠0)^(t+1): every column is feasible.
  weighted    d = 6, T = 12; diagonal C1, D12 with non-uniform entries, non-unit B1 diagonal and a D11 entry per column: g ≠ 0
  full32      the act_all plant of wave_cases.py, the three ladder columns of the class of 32 states (ñx = 29, 31, 32)
  groups      d = 6, T = 12; two-column groups with diagonal B1
  infeasible  the plant of tests/golden/infeasible_chain.npz: 12 of its 23 columns have no localized Φ
"""
import os

import numpy as np
import scipy.sparse as sp

from conftest import GOLDEN

NAMES = ("chain17", "T1", "T2", "weighted", "full32", "groups", "infeasible")
RCOND = 1e-11
FEAS = 1e-8            # ‖Ez − f‖∞ above which the reference calls a column infeasible

_cases, _refs = {}, {}


def _perturbed_chain(slc, n=17, seed=0):
    P0 = slc.workloads.chain_plant(n)
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(P0.A, dtype=np.float64); A.sort_indices()
    B2 = sp.csc_matrix(P0.B2, dtype=np.float64); B2.sort_indices()
    A.data = A.data * rng.uniform(0.8, 1.2, A.nnz)
    B2.data = B2.data * rng.uniform(0.8, 1.2, B2.nnz)
    return A, B2


def case(slc, name):
    """dict(P, S, I, T): the plant (slc.Plant), the masks [Sx, Su], the groups (None: one per column) of a case; built once."""
    if name in _cases:
        return _cases[name]
    I = None
    if name in ("T1", "T2"):
        A, _ = _perturbed_chain(slc)
        B2 = sp.diags(np.random.default_rng(7).uniform(0.8, 1.2, 17)).tocsc()
        P = slc.Plant(A, sp.identity(17, format="csc"), B2)
        Ab = (A != 0).astype(np.int64).tocsc()
        pw = [sp.identity(17, dtype=np.int64, format="csc")]
        for _ in range(3):
            pw.append(((pw[-1] @ Ab) != 0).astype(np.int64).tocsc())
        T = int(name[1])
        S = ([_csc(pw[t]).astype(bool) for t in range(T)], [_csc(pw[t + 1]).astype(bool) for t in range(T)])
    elif name in ("chain17", "groups"):
        A, B2 = _perturbed_chain(slc)
        P = slc.Plant(A, sp.identity(17, format="csc"), B2)
        d, T = {"chain17": (6, 16), "groups": (6, 12)}[name]
        S = slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5)
        if name == "groups":
            rng = np.random.default_rng(5)
            P = slc.Plant(A, sp.diags(rng.uniform(0.5, 1.5, 17)).tocsc(), B2)
            I = [[2 * k, 2 * k + 1] for k in range(8)] + [[16]]
    elif name == "weighted":
        A, B2 = _perturbed_chain(slc, seed=1)
        nx, nu = 17, B2.shape[1]
        rng = np.random.default_rng(2)
        q, r, b = rng.uniform(0.5, 2.0, nx), rng.uniform(0.5, 2.0, nu), rng.uniform(0.5, 1.5, nx)
        C1 = sp.vstack([sp.diags(q), sp.csc_matrix((nu, nx))]).tocsc()
        D12 = sp.vstack([sp.csc_matrix((nx, nu)), sp.diags(r)]).tocsc()
        D11 = sp.lil_matrix((nx + nu, nx))
        for c in range(nx):                                  # one feed-through entry on the column's own state row
            D11[c, c] = 0.1 * (1 + c % 3)
        P = slc.Plant(A, sp.diags(b).tocsc(), B2, C1, D11.tocsc(), D12)
        S = slc.workloads.localization_masks(P.A, P.B2, 6, 12, 1.5)
    elif name == "full32":
        import wave_cases as wc
        pr = wc.problem(slc, "act_all")
        P, S = pr["P"], pr["S"]
        I = wc.groups_of(slc, wc.CLASS_TARGETS[32])
    elif name == "infeasible":
        g = np.load(os.path.join(GOLDEN, "infeasible_chain.npz"))
        P = slc.workloads.chain_plant(int(g["Nx"]))
        S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    else:
        raise KeyError(name)
    S = [list(S[0]), list(S[1])]
    _cases[name] = dict(P=P, S=S, I=I, T=len(S[0]))
    return _cases[name]


def oracle_plant(P):
    import sls_oracle as o
    return o.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)


def _csc(M):
    M = sp.csc_matrix(M, dtype=np.float64).copy()
    M.sort_indices()
    return M


def _solve(E, f, M, m0, want_mu=True):
    """(z, μ, ‖Ez − f‖∞) of  min ‖Mz + m₀‖²  s.t.  Ez = f  (least-squares z where E z = f has no solution)."""
    if E.shape[1] == 0:
        return np.zeros(0), np.zeros(E.shape[0]), float(np.abs(f).max(initial=0.0))
    U, s, Vt = np.linalg.svd(E, full_matrices=True)
    r = int((s > RCOND * s[0]).sum()) if len(s) else 0
    zp = Vt[:r].T @ ((U[:, :r].T @ f) / s[:r])
    N = Vt[r:].T
    z = zp + N @ np.linalg.lstsq(M @ N, -(M @ zp + m0), rcond=None)[0] if N.shape[1] else zp
    mu = np.linalg.lstsq(E.T, 2.0 * M.T @ (M @ z + m0), rcond=RCOND)[0] if want_mu else None
    return z, mu, float(np.abs(E @ z - f).max())


def column_problems(P, S, I=None):
    """Per subproblem, in col_status order (group by group, column by column): dict(col, sx, su, E, f, M, m0, x_of, u_of, b, n, m)
    with E's rows block-row major (k, then the rows of s_x ASCENDING) — the order of `Plan.multipliers`."""
    import sls_oracle as o
    Po = oracle_plant(P)
    Sx, Su = S
    T = len(Sx)
    groups = [[c] for c in range(Po.Nx)] if I is None else [list(g) for g in I]
    out = []
    for cj in groups:
        E, f, M, m0, info = o.assemble_group(Po, cj, Sx, Su)
        n, m, w = info["n"], info["m"], info["w"]
        nz = info["W"].shape[0]
        vcol = np.array([c for (_, _, _, c) in info["var_index"]], dtype=np.int64)
        ox, ou = np.argsort(info["sx"]), np.argsort(info["su"])          # the oracle keeps first-appearance order
        for c in range(w):
            vsel = np.flatnonzero(vcol == c)
            rsel = np.concatenate([(k * w + c) * n + ox for k in range(T + 1)])
            msel = np.concatenate([np.arange((t * w + c) * nz, (t * w + c + 1) * nz) for t in range(T)])
            B1t = info["B1t"]
            assert np.count_nonzero(B1t - np.diag(np.diag(B1t))) == 0, "the reference takes diagonal B1[c_j, c_j] only"
            var = [info["var_index"][q] for q in vsel]
            rank_x, rank_u = np.argsort(ox), np.argsort(ou)               # oracle local row → ascending position
            out.append(dict(col=cj[c], sx=info["sx"][ox], su=info["su"][ou], n=n, m=m, T=T, b=float(B1t[c, c]),
                            E=E[np.ix_(rsel, vsel)], f=f[rsel], M=M[np.ix_(msel, vsel)], m0=m0[msel], nz=nz,
                            var=[(t, kind, int(rank_x[r] if kind == 0 else rank_u[r])) for (t, kind, r, _) in var],
                            zrow_x=ox, zrow_u=n + ou))
    return out


def _dense_xu(cp, z):
    x, u = np.zeros((cp["T"], cp["n"])), np.zeros((cp["T"], cp["m"]))
    for q, (t, kind, r) in enumerate(cp["var"]):
        (x if kind == 0 else u)[t, r] = z[q]
    return x, u


def gradient_from(P, cps, mus, zs, live, column_weights=None):
    """The formulas, from per-column multipliers (T + 1, ñx) and solutions: (gA, gB2, gc1, gd12) in the CSC order of P.A / P.B2."""
    A, B2 = _csc(P.A), _csc(P.B2)
    Nx, Nu = A.shape[0], B2.shape[1]
    gA, gB, gq, gr = np.zeros(A.nnz), np.zeros(B2.nnz), np.zeros(Nx), np.zeros(Nu)
    for j, cp in enumerate(cps):
        if not live[j]:
            continue
        cw = 1.0 if column_weights is None else float(column_weights[j])
        mu = np.asarray(mus[j]).reshape(cp["T"] + 1, cp["n"])
        x, u = _dense_xu(cp, zs[j])
        GA = cw * (mu[1:].T @ x)                                   # [a, b] = Σ_k μ_k[a]·x_{k−1}[b]
        GB = cw * (mu[1:].T @ u)
        lx = {int(g): i for i, g in enumerate(cp["sx"])}
        lu = {int(g): i for i, g in enumerate(cp["su"])}
        for Mx, loc, G, out in ((A, lx, GA, gA), (B2, lu, GB, gB)):
            for gc, b in loc.items():
                for k in range(Mx.indptr[gc], Mx.indptr[gc + 1]):
                    a = lx.get(int(Mx.indices[k]))
                    if a is not None:
                        out[k] += G[a, b]
        r = (cp["M"] @ zs[j] + cp["m0"]).reshape(cp["T"], cp["nz"])
        gq[cp["sx"]] += 2.0 * cw * cp["b"] * (r[:, cp["zrow_x"]] * x).sum(axis=0)
        gr[cp["su"]] += 2.0 * cw * cp["b"] * (r[:, cp["zrow_u"]] * u).sum(axis=0)
    return gA, gB, gq, gr


def reference(slc, name):
    """dict of a case, computed once and never modified: cps (column_problems), z, mu (lists), resid, live (feasible columns),
    J (per column) and total, stationarity = max_j ‖Eᵀμ − ∇J‖∞ / max|∇J| over the live columns, gA, gB2, gc1, gd12."""
    if name not in _refs:
        cs = case(slc, name)
        cps = column_problems(cs["P"], cs["S"], cs["I"])
        zs, mus, resid, J, stat = [], [], [], [], 0.0
        for cp in cps:
            z, mu, rs = _solve(cp["E"], cp["f"], cp["M"], cp["m0"])
            zs.append(z); mus.append(mu.reshape(cp["T"] + 1, cp["n"])); resid.append(rs)
            rr = cp["M"] @ z + cp["m0"]
            J.append(float(rr @ rr))
            if rs <= FEAS and z.size:
                g = 2.0 * cp["M"].T @ rr
                stat = max(stat, float(np.abs(cp["E"].T @ mu - g).max() / max(np.abs(g).max(), 1e-300)))
        resid = np.array(resid)
        live = resid <= FEAS
        gA, gB, gq, gr = gradient_from(cs["P"], cps, mus, zs, live)
        ref = dict(cps=cps, z=zs, mu=mus, resid=resid, live=live, J=np.array(J), total=float(np.sum(np.array(J)[live])),
                   stationarity=stat, gA=gA, gB2=gB, gc1=gq, gd12=gr)
        for a in (resid, live, gA, gB, gq, gr):
            a.setflags(write=False)
        _refs[name] = ref
    return _refs[name]


def total_cost(slc, name, A_data=None, B2_data=None, c1=None, d12=None):
    """Σ_j J_j over the feasible columns of the case (the live set of `reference`), for other values of the stored entries of A /
    B2 or of the diagonals of C1 / D12: the function the finite differences difference."""
    cs = case(slc, name)
    P = cs["P"]
    A, B2, C1, D12 = _csc(P.A), _csc(P.B2), _csc(P.C1), _csc(P.D12)
    if A_data is not None:
        A.data = np.asarray(A_data, dtype=np.float64)
    if B2_data is not None:
        B2.data = np.asarray(B2_data, dtype=np.float64)
    if c1 is not None:
        C1.data = np.asarray(c1, dtype=np.float64)
    if d12 is not None:
        D12.data = np.asarray(d12, dtype=np.float64)
    P2 = slc.Plant(A, P.B1, B2, C1, P.D11, D12)
    live = reference(slc, name)["live"]
    tot = 0.0
    for j, cp in enumerate(column_problems(P2, cs["S"], cs["I"])):
        if live[j]:
            z, _, _ = _solve(cp["E"], cp["f"], cp["M"], cp["m0"], want_mu=False)
            rr = cp["M"] @ z + cp["m0"]
            tot += float(rr @ rr)
    return tot


def brute_tables(P, cps):
    """[(subproblem, position, local row, local column)] by enumeration over every stored entry and every subproblem; the
    position counts B2's entries behind A's."""
    A, B2 = _csc(P.A), _csc(P.B2)
    out = []
    for j, cp in enumerate(cps):
        sx, su = list(map(int, cp["sx"])), list(map(int, cp["su"]))
        for Mx, cols, first in ((A, sx, 0), (B2, su, A.nnz)):
            for c in range(Mx.shape[1]):
                for k in range(Mx.indptr[c], Mx.indptr[c + 1]):
                    r = int(Mx.indices[k])
                    if r in sx and c in cols:
                        out.append((j, first + k, sx.index(r), cols.index(c)))
    return out


def mask_order_values(slc, name, zs=None):
    """(vals_x, vals_u): the reference's Φ (or the solutions `zs`) of a case in the masks' CSC order, per time step — the layout
    `Plan.download` returns and `gradient_host` takes.  Entries of the mask outside every subproblem stay 0."""
    cs, ref = case(slc, name), reference(slc, name)
    zs = ref["z"] if zs is None else zs
    out = []
    for kind, masks in ((0, cs["S"][0]), (1, cs["S"][1])):
        per_t = []
        for t, Sm in enumerate(masks):
            Sm = _csc(Sm)
            v = np.zeros(Sm.nnz)
            for cp, z in zip(ref["cps"], zs):
                rows = Sm.indices[Sm.indptr[cp["col"]]:Sm.indptr[cp["col"] + 1]]
                glob = cp["sx"] if kind == 0 else cp["su"]
                dense = _dense_xu(cp, z)[kind][t]
                where = {int(g): i for i, g in enumerate(glob)}
                for k, r in enumerate(rows):
                    if int(r) in where:
                        v[Sm.indptr[cp["col"]] + k] = dense[where[int(r)]]
            per_t.append(v)
        out.append(per_t)
    return out[0], out[1]


def solutions_from_values(slc, name, vals_x, vals_u):
    """The inverse of `mask_order_values`: per subproblem the vector of its free variables (the order of column_problems' E and
    M) read from value arrays in the masks' CSC order, as `Plan.download` returns them."""
    cs, ref = case(slc, name), reference(slc, name)
    masks = [[_csc(m) for m in cs["S"][0]], [_csc(m) for m in cs["S"][1]]]
    vals = [vals_x, vals_u]
    out = []
    for cp in ref["cps"]:
        z = np.zeros(len(cp["var"]))
        for q, (t, kind, r) in enumerate(cp["var"]):
            Sm = masks[kind][t]
            g = int((cp["sx"] if kind == 0 else cp["su"])[r])
            lo, hi = Sm.indptr[cp["col"]], Sm.indptr[cp["col"] + 1]
            k = lo + int(np.searchsorted(Sm.indices[lo:hi], g))
            assert k < hi and Sm.indices[k] == g
            z[q] = vals[kind][t][k]
        out.append(z)
    return out


def stationarity(cp, mu, z):
    """‖Eᵀμ − ∇J‖∞ / max|∇J| of one column, ∇J = 2Mᵀ(Mz + m₀)."""
    g = 2.0 * cp["M"].T @ (cp["M"] @ z + cp["m0"])
    return float(np.abs(cp["E"].T @ np.asarray(mu).reshape(-1) - g).max() / max(np.abs(g).max(), 1e-300))
