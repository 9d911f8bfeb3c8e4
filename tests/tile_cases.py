"""The size ladder of tests/test_gpu_tile_ladder.py and its host twin tests/test_tile_cases_host.py (a plain module like
son_cases.py; not a conftest).

One plant, chain_plant(260), and one COMPOSITE mask: column c of the mask is column c of localization_masks(A, B2, d_c, 8, 16)
with its own d_c, so that the 27 ladder columns have ñx = 15, 16, 17, 31, 32, 33, …, 143, 144, 145 — one below, one on and one
above every multiple of the tile kernel's 16×16 tile from NT = 1 to NT = 10.  With α = 16 the mask widens by 16 hops per step and reaches every d_c ≤ 96 before the last step.
The two neighbours of a ladder column carry the same d_c (ñx of column c is the row count of (𝓢x[T]·(A≠0))[:, c], which reads
the mask columns c − 1, c, c + 1), so the index set is the column's d_c-neighbourhood plus its boundary ring, as on a
uniform mask; the ladder columns are three apart.  (d_c, c) of every target is found by a search over the actual patterns, and
the host twin asserts the sizes with the oracle's reduction and with the library's."""
import time

import numpy as np
import scipy.sparse as sp

from conftest import flat_phi
from son_cases import set_knobs  # noqa: F401  (re-exported: every routing knob is cleared before a case sets its own)

NCU = 256                                   # the CU count the launch lists are recorded for (MI355X)
NX, T, ALPHA = 260, 8, 16.0
TARGETS = tuple(16 * k + o for k in range(1, 10) for o in (-1, 0, 1))
D_MAX = 96                                  # the search's bound on d_c
TOL = 1e-8                                  # the suite's bound on |Φ − Φ_oracle| (header of test_gpu_parity.py)

_K = "h2_column_tile_kernel"
PROBLEMS = ("act_all", "readme_act", "weighted", "dense")


def nt_of(n):
    """Pivot tiles of an index set of n states (npad = 16·NT)."""
    return (n + 15) // 16


# ------------------------------------------------------------------ the composite mask

_pick = {}


def pick_columns(slc):
    """[(target ñx, column c, d_c)] in target order, by search: sizes[d][c] is the row count of (A≠0)^(d+1)[:, c], the index set
    a column gets when it and its two neighbours carry d.  Candidate columns are 1, 4, 7, … (three apart, each used once); an
    even size exists only next to an end of the chain (c + d + 2 rows; an interior column has 2d + 3), so ñx = 16k is looked for
    from the left end, 16k + 1 from the right end and 16k − 1 from the middle: edge and interior columns on every tile count."""
    if not _pick:
        Ab = (slc.workloads.chain_plant(NX).A != 0).astype(np.int32).tocsc()
        R = Ab.copy()
        sizes = {}
        for d in range(1, D_MAX + 1):
            R = ((R @ Ab) != 0).astype(np.int32).tocsc()
            sizes[d] = np.diff(R.indptr)
        used, out = set(), []
        order = {0: range(1, 130, 3), 1: range(256, 130, -3), 15: range(130, 1, -3)}
        for n in TARGETS:
            hit = next(((c, d) for c in order[n % 16] if c not in used for d in range(1, D_MAX + 1) if sizes[d][c] == n), None)
            assert hit is not None, f"no (column, d) of the chain gives an index set of {n} states"
            used.add(hit[0])
            out.append((n, hit[0], hit[1]))
        _pick["cols"] = out
    return _pick["cols"]


def composite_masks(slc, A, B2, picks, T, alpha):
    """[𝓢x, 𝓢u] of the mask whose columns c − 1, c, c + 1 carry d_c for every (ñx, c, d_c) of picks (shared with wave_cases.py)."""
    by_d = {}
    for _, c, d in picks:
        by_d.setdefault(d, []).extend([c - 1, c, c + 1])
    owner = np.ones(A.shape[0], dtype=np.int64)                  # d of every column; 1 for those that no ladder column reads
    for d, cs in by_d.items():
        owner[cs] = d
    Sx, Su = [0] * T, [0] * T
    for d in sorted(set(owner.tolist())):
        mx, mu = slc.workloads.localization_masks(A, B2, d, T, alpha)
        take = sp.diags((owner == d).astype(np.int32)).tocsc()   # keeps the columns that carry this d
        for t in range(T):
            Sx[t] = Sx[t] + mx[t].astype(np.int32) @ take
            Su[t] = Su[t] + mu[t].astype(np.int32) @ take
    out = []
    for L in (Sx, Su):
        ms = []
        for M in L:
            M = sp.csc_matrix(M); M.eliminate_zeros()
            M = (M != 0).tocsc(); M.sort_indices()
            ms.append(M)
        out.append(ms)
    return out


def _composite_masks(slc, A, B2, T=T, alpha=ALPHA):
    return composite_masks(slc, A, B2, pick_columns(slc), T, alpha)


# ------------------------------------------------------------------ problems

def _banded_weight(rng, Nz):
    """The recipe of tests/golden/make_golden_general.py: a diagonal in [0.8, 1.6] plus off-diagonals at +1 and −2."""
    return sp.csc_matrix(sp.diags(rng.uniform(0.8, 1.6, Nz)) + sp.diags(rng.uniform(-0.3, 0.3, Nz - 1), 1)
                         + sp.diags(rng.uniform(-0.3, 0.3, Nz - 2), -2))


def _plant(slc, name):
    Pc = slc.workloads.chain_plant(NX)
    I = sp.identity(NX, format="csc")
    B2 = Pc.B2 if name in ("readme_act", "dense") else I
    Nu = B2.shape[1]
    if name in ("act_all", "readme_act"):
        return slc.Plant(Pc.A, I, B2)
    if name == "weighted":                                       # as test_tile_kernel_weighted_and_wide_inputs
        rng = np.random.default_rng(3)
        q = rng.uniform(0.5, 2.0, NX); r = rng.uniform(0.5, 2.0, Nu); b = rng.uniform(0.5, 1.5, NX)
        C1 = sp.vstack([sp.diags(q), sp.csc_matrix((Nu, NX))]).tocsc()
        D12 = sp.vstack([sp.csc_matrix((NX, Nu)), sp.diags(r)]).tocsc()
        D11 = sp.random(NX + Nu, NX, density=0.02, random_state=4, format="csc") * 0.1
        return slc.Plant(Pc.A, sp.diags(b).tocsc(), B2, C1, D11, D12)
    assert name == "dense"
    rng = np.random.default_rng(11)
    W = _banded_weight(rng, NX + Nu)
    b = rng.uniform(0.5, 1.5, NX)
    D11 = sp.random(NX + Nu, NX, density=0.02, random_state=5, format="csc") * 0.3
    return slc.Plant(Pc.A, sp.diags(b).tocsc(), B2, W[:, :NX], D11, W[:, NX:])


_problems, _refs = {}, {}
oracle_seconds = {}                         # CPU seconds spent in the reference, per problem (reported by the GPU tests)


def problem(slc, name):
    """dict(P, S, cols, groups, colidx, targets) of a ladder problem; built once.  cols is in target order."""
    if name not in _problems:
        P = _plant(slc, name)
        S = _composite_masks(slc, P.A, P.B2)
        cols = [c for _, c, _ in pick_columns(slc)]
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        _problems[name] = dict(P=P, S=S, cols=cols, groups=[[c] for c in cols], colidx=colidx, targets=list(TARGETS))
    return _problems[name]


def short_problem(slc, Th):
    """act_all with the horizon cut to Th steps (α = 128: the first step after t = 0 already has the full width, so the index
    sets are the ladder's): the columns with ñx = 97 and 113, the two smallest blocks that live in the workspace by default."""
    key = f"short_T{Th}"
    if key not in _problems:
        P = _plant(slc, "act_all")
        S = _composite_masks(slc, P.A, P.B2, Th, 128.0)
        cols = [c for n, c, _ in pick_columns(slc) if n in (97, 113)]
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        _problems[key] = dict(P=P, S=S, cols=cols, groups=[[c] for c in cols], colidx=colidx, targets=[97, 113])
    return _problems[key]


def oracle_plant(slc, name):
    import sls_oracle as o
    P = problem(slc, name)["P"]
    return o.OraclePlant(P.A, P.B1, P.B2) if name in ("act_all", "readme_act") else o.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)


def index_sets(slc, name):
    """[(s_x, s_u)] of the ladder columns by the oracle's reduction (reference src/reduction.jl:11-27)."""
    import sls_oracle as o
    pr = problem(slc, name)
    Po = oracle_plant(slc, name)
    return [o.sparsity_dim_reduction(Po, [c], pr["S"])[3:5] for c in pr["cols"]]


def library_index_sets(slc, name):
    """The same by the library's own host reduction (sls_sparsity_dim_reduction)."""
    pr = problem(slc, name)
    return library_index_sets_of(slc, pr["P"], pr["S"], pr["cols"])


def library_index_sets_of(slc, P, S, cols):
    """[(s_x, s_u)] of the given columns of (P, S) by sls_sparsity_dim_reduction (shared with wave_cases.py)."""
    import ctypes as C
    lib, cap = slc.load_library(), slc._capi
    i64p = C.POINTER(C.c_int64)
    keep = []

    def csc(M, cls, dt):
        M = sp.csc_matrix(M); M.sort_indices()
        cp = M.indptr.astype(np.int64); rv = M.indices.astype(np.int64); nz = np.ascontiguousarray(M.data, dtype=dt)
        keep.extend([cp, rv, nz])
        return cls(M.shape[0], M.shape[1], cp.ctypes.data_as(i64p), rv.ctypes.data_as(i64p),
                   nz.ctypes.data_as(C.POINTER(C.c_double if dt == np.float64 else C.c_uint8)))
    A = csc(P.A, cap.sls_csc_f64, np.float64)
    sxm = csc(S[0][-1], cap.sls_csc_bool, np.uint8); sum_ = csc(S[1][-1], cap.sls_csc_bool, np.uint8)
    dims = cap.sls_dims(P.Nx, P.Nu, P.Nz, P.Nw, 1, 0, 0)
    out = []
    for c in cols:
        cj = np.asarray([c], dtype=np.int64)
        sx = np.zeros(P.Nx, dtype=np.int64); su = np.zeros(max(P.Nu, 1), dtype=np.int64)
        nsx, nsu = C.c_int64(), C.c_int64()
        rc = lib.sls_sparsity_dim_reduction(C.byref(dims), C.byref(A), C.byref(sxm), C.byref(sum_), cj.ctypes.data_as(i64p), 1,
                                            sx.ctypes.data_as(i64p), C.byref(nsx), su.ctypes.data_as(i64p), C.byref(nsu))
        assert rc == 0, rc
        out.append((sx[:nsx.value].copy(), su[:nsu.value].copy()))
    return out


def reference(slc, name):
    """dict(flat, resid, status) of a problem: Φ of the 27 ladder columns in mask order (zeros elsewhere) with the residual
    ‖Ez − f‖∞ of every column, in target order.  The C restatement of the oracle for the default weights (it knows no others);
    the NumPy oracle (dense SVD null-space method) for "weighted" and "dense".  Computed once per session, never modified."""
    if name not in _refs:
        import sls_oracle as o
        pr = problem(slc, name)
        S = pr["S"]
        Po = oracle_plant(slc, name)
        t0 = time.perf_counter()
        if name in ("act_all", "readme_act"):
            import sls_oracle_cport as cp
            ox, ou, info = cp.SLS_H2(Po, S, cols=pr["cols"], nthreads=8)
            resid, status = np.asarray(info["resid"], dtype=np.float64), np.asarray(info["status"]).astype(np.int64)
        else:
            ox, ou, dg = o.SLS_H2(Po, S, pr["groups"], return_diag=True)
            resid = np.array([d["resid"] for d in dg])
            status = np.zeros(len(dg), dtype=np.int64)           # the NumPy oracle has no status word: its verdict is the residual
        flat = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
        oracle_seconds[name] = time.perf_counter() - t0
        for a in (flat, resid, status):
            a.setflags(write=False)
        _refs[name] = dict(flat=flat, resid=resid, status=status)
    return _refs[name]


def residual_bound(name):
    """What "feasible in the reference" means: 1e-12 for the C restatement, 1e-9 for the NumPy oracle (the bound
    test_non_diagonal_cost_weights_match_golden uses)."""
    return 1e-12 if name in ("act_all", "readme_act") else 1e-9


def column_errors(slc, name, got):
    """max |Φ_gpu − Φ_ref| of every ladder column, and max |Φ_ref| of every ladder column, in target order."""
    pr = problem(slc, name)
    want = reference(slc, name)["flat"]
    err, big = [], []
    for c in pr["cols"]:
        sel = pr["colidx"] == c
        err.append(np.abs(got[sel] - want[sel]).max()); big.append(np.abs(want[sel]).max())
    return np.array(err), np.array(big)


def worst_per_nt(err):
    """{NT: worst error} of a per-target error array."""
    out = {}
    for n, e in zip(TARGETS, err):
        out[nt_of(n)] = max(out.get(nt_of(n), 0.0), float(e))
    return out


# ------------------------------------------------------------------ describe() text

def short(desc):
    """The pinned part of a describe(): kernel name with template arguments, nsub=, nmax= and per_cu= of every launch."""
    import re
    out = []
    for seg in [s for s in desc.split(";") if s]:
        m = re.match(r"(h2_column_[a-z0-9_]+(?:<[^>]*>)?) nsub=(\d+) ", seg)
        assert m, (seg, desc)
        nmax, per_cu = re.search(r"nmax=(\d+)", seg), re.search(r"per_cu=(\d+)", seg)
        assert nmax and per_cu, (seg, desc)
        out.append(f"{m.group(1)} nsub={m.group(2)} nmax={nmax.group(1)} per_cu={per_cu.group(1)}")
    return ";".join(out)


def launch_sizes(desc):
    """[(kernel, nsub, nmax)] of a short or full describe()."""
    import re
    return [(m.group(1), int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"(h2_column_[a-z0-9_]+(?:<[^>]*>)?) nsub=(\d+) .*?nmax=(\d+)", desc)]


# ------------------------------------------------------------------ cases

_G = {"SLS_FORCE_GENERAL": "1"}
ENV_LDS = dict(_G)
ENV_LDS9 = {**_G, "SLS_TILE_LDS_MAXNT": "9", "SLS_TILE_ONE_PER_CU": "1"}
ENV_WS = {**_G, "SLS_TILE_GLOBAL": "1"}
ENV_BIG = {**_G, "SLS_TILE_BIG": "all"}
_LDS, _WS, _BIG = f"{_K}<block_in_LDS>", f"{_K}<block_in_workspace>", f"{_K}<block_in_workspace,carve_in_workspace>"
_LDS_CG, _WS_CG = f"{_K}<block_in_LDS,dense_hessian_cg>", f"{_K}<block_in_workspace,dense_hessian_cg>"
_BIG_CG = f"{_K}<block_in_workspace,carve_in_workspace,dense_hessian_cg>"


def _case(id, prob, env, pinned):
    return dict(id=id, problem=prob, env=dict(env), pinned=pinned)


def _plain(prob):
    """The four homes of the plain build.  SLS_FORCE_GENERAL keeps the columns with ñx ≤ 32 off the twisted kernels.  By default
    a block of up to 6 tiles (ñx ≤ 96) lives in LDS, two workgroups per CU; SLS_TILE_LDS_MAXNT=9 with one workgroup per CU
    (whole Ã·Q image in LDS) takes the LDS block to ñx = 144 in two launches, and only ñx = 145 (NT = 10) stays outside."""
    return [
        _case(f"{prob}-lds", prob, ENV_LDS, f"{_WS} nsub=10 nmax=145 per_cu=2;{_LDS} nsub=17 nmax=96 per_cu=2"),
        _case(f"{prob}-lds9", prob, ENV_LDS9, f"{_WS} nsub=1 nmax=145 per_cu=1;{_LDS} nsub=9 nmax=144 per_cu=1;{_LDS} nsub=17 nmax=96 per_cu=1"),
        _case(f"{prob}-workspace", prob, ENV_WS, f"{_WS} nsub=27 nmax=145 per_cu=2"),
        _case(f"{prob}-carve", prob, ENV_BIG, f"{_BIG} nsub=27 nmax=145 per_cu=1"),
    ]


CASES = _plain("act_all") + _plain("readme_act") + _plain("weighted") + [
    # the CG build (dense cost Hessian): no routing knob needed, every such column is the tile kernel's
    _case("dense-default", "dense", {}, f"{_WS_CG} nsub=10 nmax=145 per_cu=1;{_LDS_CG} nsub=17 nmax=96 per_cu=1"),
    _case("dense-workspace", "dense", {"SLS_TILE_GLOBAL": "1"}, f"{_WS_CG} nsub=27 nmax=145 per_cu=1"),
    _case("dense-carve", "dense", {"SLS_TILE_BIG": "all"}, f"{_BIG_CG} nsub=27 nmax=145 per_cu=1"),
]
IDS = [c["id"] for c in CASES]


def get(cid):
    return CASES[IDS.index(cid)]


SHORT_T = (2, 3)                            # horizons of the short-horizon cases (both columns feasible at both: host twin)
SHORT_PINNED = f"{_WS} nsub=2 nmax=113 per_cu=2"
