"""The size ladder of tests/test_gpu_wave_ladder.py and its host twin tests/test_wave_cases_host.py (a plain module like
tile_cases.py; not a conftest).

The one-wave, two-wave and four-wave column kernels size their lane grid, LDS carve and pivot tiles by a class (NPL, RPL) of
capacity (64/NPL)·RPL = 12, 16, 20, 24, 28, 32, 40, 48, 64 states (wave_class, sls_device.h), and a merged launch runs every
column in its largest class: only a column with ñx equal to the capacity has no padding row.  One plant, chain_plant(120), and
one COMPOSITE mask as in tile_cases.py (column c and its two neighbours carry their own d_c, ladder columns three apart, (c, d_c)
found by search) whose ladder columns have ñx = capacity − 1, capacity, capacity + 1 for the nine capacities, and 62 and a
second 63 for the ñu ≤ 64 fence (LABELS below).  An interior column of the chain has 2d + 3 states, an end column c + d + 2: even
sizes come from columns next to either end (taken alternately), odd sizes from the middle.

A case is (problem, T, family); it holds one plan per class, of that class's ladder columns alone (capacity + 1 of the class
below, capacity − 1, capacity), so that the merged class of the launch is the class under test and its largest column fills it."""
import time

import numpy as np
import scipy.sparse as sp

import son_cases
import tile_cases
from conftest import flat_phi
from oracle_c import TOL  # noqa: F401  (the suite's bound on |Φ − Φ_oracle|, header of test_gpu_parity.py; not restated here)
from son_cases import set_knobs  # noqa: F401  (re-exported: every routing knob is cleared before a case sets its own)

NCU = 256                                   # the CU count the launch lists are recorded for (MI355X)
NX, T, ALPHA = 120, 8, 16.0
CLASSES = ((16, 3), (16, 4), (32, 10), (32, 12), (32, 14), (32, 16), (64, 40), (64, 48), (64, 64))    # wave_class, sls_device.h
CAPS = tuple((64 // npl) * rpl for npl, rpl in CLASSES)
TARGETS = tuple(cap + o for cap in CAPS for o in (-1, 0, 1)) + (62,)
SMALL = TARGETS[:18]                        # the targets of the six classes with NPL ≤ 32
# One more column for the ñu ≤ 64 fence of wave_class_of.  With B2 = I an interior column has ñu = ñx + 2 and an end column
# ñu = ñx + 1 (the input set is the index set plus one ring, clipped by the same end), so ñx = 62 has ñu = 63 and the interior
# ñx = 63 has ñu = 65: ñu = 64 itself exists only on an END column with ñx = 63 (odd sizes exist at an end too).  "63e" is that
# column; LABELS names the 29 ladder columns, size_of gives their ñx.
LABELS = TARGETS + ("63e",)
D_MAX = 40                                  # the search's bound on d_c
CUT_T, CUT_ALPHA = (2, 3, 4, 31, 32), 128.0  # the horizon cut (act_all): with α = 128 the first step after t = 0 has the full width
PROBLEMS = ("act_all", "readme_act", "weighted")
LEFT_OUT = {"act_all": (), "weighted": (), "readme_act": (11,)}    # ñx of the columns the reference must flag, per problem

# the ladder columns of every class, by capacity
CLASS_TARGETS = {12: (11, 12), 16: (13, 15, 16), 20: (17, 19, 20), 24: (21, 23, 24), 28: (25, 27, 28), 32: (29, 31, 32),
                 40: (33, 39, 40), 48: (41, 47, 48), 64: (49, 63, 64)}


# ------------------------------------------------------------------ the composite mask

_pick = {}


def size_of(label):
    return 63 if label == "63e" else int(label)


def pick_columns(slc):
    """[(label, column c, d_c)] in LABELS order, by search: sizes[d][c] is the row count of (A≠0)^(d+1)[:, c], the index set
    a column gets when it and its two neighbours carry d.  Candidate columns are three apart and used once: an even size exists
    only where the chain's end clips the neighbourhood (c ≤ d + 1 from that end), so the even targets are looked for from the
    left end and from the right end in turn, inward; the odd targets from the middle outward.  The right end's candidates start
    at column 112: the README actuators sit on states 6k and 6k + 1, the last four states have none, and a column next to them
    is solved by the reference to a residual of 1e-10 only (2.3e-10 at column 118), above its feasibility bound."""
    if not _pick:
        Ab = (slc.workloads.chain_plant(NX).A != 0).astype(np.int32).tocsc()
        R = Ab.copy()
        sizes = {}
        for d in range(1, D_MAX + 1):
            R = ((R @ Ab) != 0).astype(np.int32).tocsc()
            sizes[d] = np.diff(R.indptr)
        middle = [61] + [61 + s * 3 * k for k in range(1, 10) for s in (-1, 1)]
        ends = (list(range(1, 31, 3)), list(range(112, 90, -3)))
        assert not {c + o for c in middle for o in (-1, 0, 1)} & {c + o for e in ends for c in e for o in (-1, 0, 1)}
        used, out, n_even = set(), [], 0
        for label in LABELS:
            n = size_of(label)
            if label == "63e":
                order = ends[0]                                  # c ≤ 28 < d + 1 for every d that gives 63 there: clipped
            elif n % 2:
                order = middle
            else:
                order = ends[n_even % 2]; n_even += 1
            hit = next(((c, d) for c in order if c not in used for d in range(1, D_MAX + 1) if sizes[d][c] == n), None)
            assert hit is not None, f"no (column, d ≤ {D_MAX}) of the chain gives an index set of {n} states"
            used.add(hit[0])
            out.append((label, hit[0], hit[1]))
        _pick["cols"] = out
    return _pick["cols"]


def column_of(slc, label):
    """The ladder column of a label (its ñx, or "63e")."""
    return next(c for m, c, _ in pick_columns(slc) if m == label)


# ------------------------------------------------------------------ problems

def _plant(slc, name):
    """The recipes of tile_cases._plant at NX = 120."""
    Pc = slc.workloads.chain_plant(NX)
    I = sp.identity(NX, format="csc")
    if name == "act_all":
        return slc.Plant(Pc.A, I, I)
    if name == "readme_act":
        return slc.Plant(Pc.A, I, Pc.B2)
    assert name == "weighted"
    rng = np.random.default_rng(3)
    q = rng.uniform(0.5, 2.0, NX); r = rng.uniform(0.5, 2.0, NX); b = rng.uniform(0.5, 1.5, NX)
    C1 = sp.vstack([sp.diags(q), sp.csc_matrix((NX, NX))]).tocsc()
    D12 = sp.vstack([sp.csc_matrix((NX, NX)), sp.diags(r)]).tocsc()
    D11 = sp.random(2 * NX, NX, density=0.02, random_state=4, format="csc") * 0.1
    return slc.Plant(Pc.A, sp.diags(b).tocsc(), I, C1, D11, D12)


_problems, _refs = {}, {}
oracle_seconds = {}                         # CPU seconds spent in the reference, per (problem, T) (reported by the GPU tests)


def problem(slc, name, Th=T):
    """dict(P, S, colidx, targets, cols) of a ladder problem at horizon Th (α = 16 at the base horizon, 128 at every other);
    built once.  targets are the labels that are compared at this (problem, horizon): all 29 on act_all and the 28 sizes on
    readme_act at T = 8, the 18 small ones otherwise; cols their columns, in target order."""
    if (name, Th) not in _problems:
        P = _plant(slc, name)
        S = tile_cases.composite_masks(slc, P.A, P.B2, pick_columns(slc), Th, ALPHA if Th == T else CUT_ALPHA)
        targets = SMALL if Th != T or name == "weighted" else LABELS if name == "act_all" else TARGETS
        cols = [column_of(slc, n) for n in targets]
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        _problems[(name, Th)] = dict(P=P, S=S, colidx=colidx, targets=list(targets), cols=cols)
    return _problems[(name, Th)]


def oracle_plant(slc, name):
    import sls_oracle as o
    P = problem(slc, name)["P"]
    return o.OraclePlant(P.A, P.B1, P.B2) if name != "weighted" else o.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)


def index_sets(slc, name, Th=T):
    """[(s_x, s_u)] of all 29 ladder columns, in LABELS order, by the oracle's reduction (reference src/reduction.jl:11-27)."""
    import sls_oracle as o
    pr = problem(slc, name, Th)
    Po = oracle_plant(slc, name)
    return [o.sparsity_dim_reduction(Po, [c], pr["S"])[3:5] for _, c, _ in pick_columns(slc)]


def library_index_sets(slc, name, Th=T):
    """The same by the library's own host reduction (sls_sparsity_dim_reduction)."""
    pr = problem(slc, name, Th)
    return tile_cases.library_index_sets_of(slc, pr["P"], pr["S"], [c for _, c, _ in pick_columns(slc)])


def reference(slc, name, Th=T):
    """dict(flat, resid, status, feasible, big) of a problem: Φ of its compared columns in mask order (zeros elsewhere), and per
    column, in problem(...)["targets"] order, the residual ‖Ez − f‖∞, the status, whether the column is feasible in the reference
    (status 0 and residual under tile_cases.residual_bound) and max |Φ|.  The C restatement of the oracle for the default weights
    (it knows no others), the NumPy oracle for "weighted".  Computed once per session, never modified."""
    if (name, Th) not in _refs:
        import sls_oracle as o
        pr = problem(slc, name, Th)
        S = pr["S"]
        Po = oracle_plant(slc, name)
        t0 = time.perf_counter()
        if name != "weighted":
            import sls_oracle_cport as cp
            ox, ou, info = cp.SLS_H2(Po, S, cols=pr["cols"], nthreads=8)
            resid, status = np.asarray(info["resid"], dtype=np.float64), np.asarray(info["status"]).astype(np.int64)
        else:
            ox, ou, dg = o.SLS_H2(Po, S, [[c] for c in pr["cols"]], return_diag=True)
            resid = np.array([d["resid"] for d in dg])
            status = np.zeros(len(dg), dtype=np.int64)           # the NumPy oracle has no status word: its verdict is the residual
        flat = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
        oracle_seconds[(name, Th)] = time.perf_counter() - t0
        feasible = (status == 0) & (resid < tile_cases.residual_bound(name))
        big = np.array([np.abs(flat[pr["colidx"] == c]).max() for c in pr["cols"]])
        for a in (flat, resid, status, feasible, big):
            a.setflags(write=False)
        _refs[(name, Th)] = dict(flat=flat, resid=resid, status=status, feasible=feasible, big=big)
    return _refs[(name, Th)]


# ------------------------------------------------------------------ cases

FAMILIES = {"four": {}, "two": {"SLS_TWISTED4": "0"}, "one": {"SLS_NO_TWISTED": "1"}, "two_plds": {"SLS_P_LDS": "1"},
            "wave64": {"SLS_WAVE64": "1"}}
_ONE, _TWO, _FOUR, _TILE = "h2_column_wave_kernel", "h2_column_twisted_kernel", "h2_column_twisted4_kernel", "h2_column_tile_kernel"


def _cls(cap):
    return "%d,%d" % CLASSES[CAPS.index(cap)]


def _whole(kernel, cap):
    """The pinned list of a plan whose columns all run in one launch: kernel with template arguments, nsub, grid == nsub."""
    n = len(CLASS_TARGETS[cap])
    return f"{kernel} nsub={n} grid={n}"


def _pins(family, Th):
    """{capacity: pinned launch list} of a family at a horizon, as observed on all three problems (the host twin holds every
    entry to the live routing).  The default route is the four-wave kernel for the four NPL = 32 classes and the two-wave kernel,
    P in the workspace, for the two NPL = 16 classes; SLS_TWISTED4=0 gives the two-wave kernel everywhere, SLS_NO_TWISTED=1 the
    one-wave kernel.  "two_plds" pins what routing gives under SLS_P_LDS=1 alone: the knob takes the NPL = 32 classes off the
    four-wave kernel too, so all six classes run on the two-wave kernel with P in LDS.  Below T = 3 the twisted kernels hand over
    to the one-wave kernel, whatever the family."""
    small = CAPS[:6]
    if family == "wave64":
        return {cap: _whole(f"{_ONE}<{_cls(cap)}>", cap) for cap in CAPS[6:]}
    if family == "one" or Th < 3:
        return {cap: _whole(f"{_ONE}<{_cls(cap)}>", cap) for cap in small}
    if family in ("two", "two_plds"):
        p_home = "P_in_LDS" if family == "two_plds" else "P_in_workspace"
        return {cap: _whole(f"{_TWO}<{_cls(cap)},{p_home}>", cap) for cap in small}
    return {cap: _whole(f"{_TWO}<{_cls(cap)},P_in_workspace>" if cap <= 16 else f"{_FOUR}<{_cls(cap)}>", cap) for cap in small}


def _case(prob, Th, family, pins=None):
    pins = pins or _pins(family, Th)
    return dict(id=f"{prob}-T{Th}-{family}", problem=prob, T=Th, family=family, env=dict(FAMILIES[family]),
                plans=[dict(cap=cap, targets=CLASS_TARGETS[cap], pinned=pinned) for cap, pinned in pins.items()])


# act_all under SLS_WAVE64=1: B2 = I gives ñu = ñx + 1 or + 2, so the columns with ñx = 63 and 64 (ñu = 65) are past the
# ñu ≤ 64 fence of wave_class_of and run on the tile kernel; the column with ñx = 49 then runs in its own class <64,64>, alone
_ACT_ALL_WAVE64 = {40: _whole(f"{_ONE}<64,40>", 40), 48: _whole(f"{_ONE}<64,48>", 48),
                   64: f"{_TILE}<block_in_LDS> nsub=2 grid=2;{_ONE}<64,64> nsub=1 grid=1"}

CASES = ([_case(p, T, f) for p in PROBLEMS for f in ("four", "two", "one")]
         + [_case("act_all", T, "two_plds"), _case("act_all", T, "wave64", _ACT_ALL_WAVE64), _case("readme_act", T, "wave64")]
         + [_case("act_all", Th, f) for Th in CUT_T for f in ("four", "two", "one")])
IDS = [c["id"] for c in CASES]

# the fences: one column stays in a wave class, the next leaves for the tile kernel.  nu is ñu of the plan's columns where the
# fence is the ñu ≤ 64 one: (63, 65) on the columns (62, 63), and (64, 65) — the fence pair itself — on the two columns with
# ñx = 63, the end column and the interior one.
_FENCE = f"{_TILE}<block_in_LDS> nsub=1 grid=1;{_ONE}<64,64> nsub=1 grid=1"
FENCES = [
    dict(id="act_all-nu_fence_62_63", problem="act_all", T=T, env={"SLS_WAVE64": "1"}, targets=(62, 63), nu=(63, 65), pinned=_FENCE),
    dict(id="act_all-nu_fence_64_65", problem="act_all", T=T, env={"SLS_WAVE64": "1"}, targets=("63e", 63), nu=(64, 65),
         pinned=f"{_ONE}<64,64> nsub=1 grid=1;{_TILE}<block_in_LDS> nsub=1 grid=1"),
    dict(id="readme_act-nx_fence", problem="readme_act", T=T, env={"SLS_WAVE64": "1"}, targets=(64, 65), nu=None, pinned=_FENCE),
]
FENCE_IDS = [f["id"] for f in FENCES]


def get(cid):
    return (CASES + FENCES)[(IDS + FENCE_IDS).index(cid)]


def plans_of(case):
    """[dict(cap, targets, pinned)] of a case or of a fence (whose one plan has no class of its own: cap is None)."""
    return case["plans"] if "plans" in case else [dict(cap=None, targets=case["targets"], pinned=case["pinned"])]


def groups_of(slc, targets):
    """The single-column groups of a plan, in target order."""
    return [[column_of(slc, n)] for n in targets]


def short(desc):
    """The pinned part of a describe(): kernel names with template arguments, nsub= and grid=, in launch order."""
    return son_cases.short(desc)
