"""The sum-of-norms loop (SLS_SOLVE_SUM_OF_NORMS) per size class, on column reuse, on short horizons and on a second execute.

This objective does not run the 𝓗₂ kernels: it runs `h2_column_wave_kernel<NPL,RPL,true,true>` (ADMM loop, block soft threshold,
warm-started multipliers and Anderson ring inside `wave_solve_column`), one instantiation per small class <16,3> <16,4> <32,10>
<32,12> <32,14> <32,16>, and the CG / ADMM build of `h2_column_tile_kernel` for everything else (and for every column under
SLS_SON_TILE=1).  A workgroup of these builds keeps y, u, v, the linear term, F and g of the previous step, five difference pairs
of Anderson history and the multipliers λ in its workspace slice, and draws its columns from an atomic work counter that the
host clears before every execute.  Each of these is a place where one column can leak into the next or where a second execute
can silently do nothing; test_sum_of_norms.py pins no size class and test_gpu_column_reuse.py has no sum-of-norms case.

The reference is the certified CPU oracle (oracle/sls_son_oracle.py: `_column_problem`, `solve_column`, `certificate`); the
tolerances are those test_sum_of_norms.py states (tests/son_cases.py: check_column): objective 1e-7 relative, ‖ΔΦ‖∞ ≤
1e-6·max|Φ| per column, ‖Ez − f‖∞ ≤ 1e-9, objective ≥ oracle objective − oracle gap − 1e-9.  Routing is steered with
`monkeypatch.setenv` and a fresh `slc.Context([0])` per case.  One table (`CASES`) drives the GPU tests and their host twin
`test_son_launch_lists_on_256_cus`, which holds `dist.describe_launches(..., 256, objective="sum_of_norms")` of every case to
the pinned text (kernel names with template arguments, nsub=, grid=); the GPU tests hold the live `plan.describe()` to the same
host view.  The shapes are sized for 256 CUs; another CU count fails with a message (it does not skip).

1. classes (chain_plant(40) masks (7, 12, 1.5): ñx 9…17; chain_plant(70) masks (15, 12, 1.5): ñx 17…33): a column on each side
   of every class boundary 12|13, 16|17, 20|21, 24|25, 28|29, 32|33, and ñx = 33 on the tile kernel; default home and
   SLS_SON_TILE=1.  Every launch's nsub equals the number of columns whose ORACLE index set falls into that class by the
   capacities 12, 16, 20, 24, 28, 32 — a column in the wrong class fails.  Columns 0…17, their mirror images and two interior
   ones against the oracle (38 per plant); every column passes the achievability identities on the full system to 1e-9.
2. reuse (chain_plant(400) masks (9, 12, 1.5), interior ñx = 21, class <32,12>, SLS_MAX_PER_CU=1: `nsub=380 grid=236`, so 144
   workgroups draw a second column).  One-wave home: the plan with the knob lifted differs in nothing but `grid=` and values,
   residuals, iteration counts and statuses of all 400 columns are bit-identical — a column's arithmetic depends neither on the
   workgroup that drew it nor on what that workgroup solved before, so any differing bit is state carried across columns.  48
   columns against the oracle: the 20 edge columns, the last ten of the interior launch's queue (columns 380…389: the queue is
   in descending ñx, ties in column order) and 18 spread over the interior.  Tile home (block in LDS, block in the workspace,
   and the carve in the workspace, `grid=256` of 400): statuses 0 and achievability on all columns, the same 48 against the
   oracle, Φ of every column within 2e-6·max|Φ| of the one-wave home's (each home is held to 1e-6 of the same unique optimum).
   Mixed statuses (random_plant(400, 2, 2, seed=5) masks (2, 8, 1.5); every 8th column on the oracle: 18 feasible, 32
   infeasible): oracle infeasible ⇒ status ≠ 0; feasible and the GPU's 𝓗₂ status 0 ⇒ status 0 and the four tolerances;
   feasible but flagged by the 𝓗₂ solve ⇒ status ≠ 0; both kinds present; at least 10 full value checks.  In the default home
   this plant's largest one-wave launch has 201 columns, so at 256 CUs no workgroup of it draws a second column whatever the
   knob: the case pins the six classes side by side next to a tile launch and bit equality with the lifted plan on every
   one-wave column (the tile launch's LDS plan changes with the knob: statuses only).  The tile home of the same plant
   (`nsub=400 grid=256`) is what hands feasible columns to workgroups that have just flagged an infeasible one.
3. short horizons: README dynamics on 13 states, B2 = I, state 6 cut out of the chain, masks (3, T, 3.0), T = 1…4, both homes.
   At T = 1 only column 6 is feasible (objective √2); from T = 2 on all 13 are, and the response is dead-beat in two steps: the
   time blocks t ≥ 2 are exactly zero (the zero branch of the soft threshold, the guard on 1/(ρ‖v‖)) — they must be below
   1e-6·max|Φ| on the GPU.  Statuses equal the oracle's exactly.  The trivial column (A[:, c] = 0) gives SLS_COL_TRIVIAL and
   Φ = 0; the plant with ñu = 0 columns (no column of it is feasible) gives a non-zero status on every column.
4. a plan executed twice, the second time into a separately allocated array pre-filled with NaN: status, residuals,
   iteration counts and values bit-identical, no NaN left — what the per-execute clearing of the work counters rests on.

Cost, measured on an MI355X (wall time of the test body: context, plan, execute, download, and the plant's oracle columns when
the case is the first to need them; in brackets the oracle's share, CPU seconds on that host — each plant's reference is
computed once per session, shared by the plant's cases and never modified; a slower 16-core host needed 5.2 s for the 38
chain-40 columns, 3.6 s for the 38 chain-70 columns and 1.9 s for every 8th column of the random plant):
  classes40_wave 1.00 s [0.62 s]   classes40_tile 0.04 s   classes70_wave 1.12 s [1.05 s]   classes70_tile 0.06 s
  reuse_wave 1.03 s, two plans [0.99 s]   reuse_tile_lds 0.06 s   reuse_tile_workspace 0.05 s   reuse_tile_carve 0.06 s
  mixed_wave 1.13 s, two plans and the 𝓗₂ solve [0.79 s]   mixed_tile 0.03 s
  short_T1…T4 0.02 – 0.05 s one-wave, < 0.01 s tile   trivial < 0.01 s   inputless 0.19 s and < 0.01 s   twice_wave, twice_tile 0.03 s
24 GPU cases, 7 s for the module; 39 – 70 ADMM steps per chain column in either home.  Worst errors against the oracle over all
cases: objective 5.1e-10 relative (short_T4), ‖ΔΦ‖∞ / max|Φ| 2.6e-9 (the chains), ‖Ez − f‖∞ 1.3e-14; the two homes agree to
5.4e-15·max|Φ| on every chain-400 column.
"""
import re
import time

import numpy as np
import pytest

import son_cases as sc
from son_cases import NCU, TILE_BIG, TILE_LDS, TILE_WS, WAVE_NAMES

_R1 = {"SLS_MAX_PER_CU": "1"}
_TILE = {"SLS_SON_TILE": "1"}
_W = "h2_column_wave_kernel"


def _case(id, kind, plant, env, pinned, lift=False):
    return dict(id=id, kind=kind, plant=plant, env=dict(env), pinned=pinned, lift=lift)


CASES = [
    # 1. every size class
    _case("classes40_wave", "classes", "chain40", {}, f"{_W}<32,10> nsub=24 grid=24;{_W}<16,4> nsub=8 grid=8;{_W}<16,3> nsub=8 grid=8"),
    _case("classes40_tile", "classes", "chain40", _TILE, f"{TILE_LDS} nsub=40 grid=40"),
    _case("classes70_wave", "classes", "chain70", {}, f"{TILE_LDS} nsub=38 grid=38;{_W}<32,16> nsub=8 grid=8;{_W}<32,14> nsub=8 grid=8;"
                                                      f"{_W}<32,12> nsub=8 grid=8;{_W}<32,10> nsub=8 grid=8"),
    _case("classes70_tile", "classes", "chain70", _TILE, f"{TILE_LDS} nsub=70 grid=70"),
    # 2. a second column per workgroup
    _case("reuse_wave", "reuse_wave", "chain400", _R1, f"{_W}<32,12> nsub=380 grid=236;{_W}<32,10> nsub=8 grid=8;{_W}<16,4> nsub=8 grid=8;"
                                                       f"{_W}<16,3> nsub=4 grid=4", lift=True),
    _case("reuse_tile_lds", "reuse_tile", "chain400", {**_R1, **_TILE}, f"{TILE_LDS} nsub=400 grid=256"),
    _case("reuse_tile_workspace", "reuse_tile", "chain400", {**_R1, **_TILE, "SLS_TILE_GLOBAL": "1"}, f"{TILE_WS} nsub=400 grid=256"),
    _case("reuse_tile_carve", "reuse_tile", "chain400", {**_R1, **_TILE, "SLS_TILE_BIG": "all"}, f"{TILE_BIG} nsub=400 grid=256"),
    _case("mixed_wave", "mixed", "mixed400", _R1, f"{TILE_LDS} nsub=32 grid=32;{_W}<32,16> nsub=13 grid=13;{_W}<32,14> nsub=24 grid=24;"
                                                  f"{_W}<32,12> nsub=31 grid=31;{_W}<32,10> nsub=44 grid=44;{_W}<16,4> nsub=55 grid=55;"
                                                  f"{_W}<16,3> nsub=201 grid=201", lift=True),
    _case("mixed_tile", "mixed", "mixed400", {**_R1, **_TILE}, f"{TILE_LDS} nsub=400 grid=256"),
    # 3. short horizons, the trivial column, ñu = 0
    *[_case(f"short_T{T}_{home}", "short", f"cut13_T{T}", env, f"{k} nsub=13 grid=13")
      for T in (1, 2, 3, 4) for home, env, k in (("wave", {}, WAVE_NAMES[0]), ("tile", _TILE, TILE_LDS))],
    _case("trivial_wave", "trivial", "trivial", {}, f"{TILE_LDS} nsub=1 grid=1"),
    _case("trivial_tile", "trivial", "trivial", _TILE, f"{TILE_LDS} nsub=1 grid=1"),
    _case("inputless_wave", "inputless", "inputless", {}, f"{WAVE_NAMES[0]} nsub=14 grid=14"),
    _case("inputless_tile", "inputless", "inputless", _TILE, f"{TILE_LDS} nsub=14 grid=14"),
    # 4. a plan executed twice
    _case("twice_wave", "twice", "chain40", {}, f"{_W}<32,10> nsub=24 grid=24;{_W}<16,4> nsub=8 grid=8;{_W}<16,3> nsub=8 grid=8"),
    _case("twice_tile", "twice", "chain40", _TILE, f"{TILE_LDS} nsub=40 grid=40"),
]
_IDS = [c["id"] for c in CASES]


def _ids(kind):
    return [c["id"] for c in CASES if c["kind"] == kind]


def _get(cid):
    return CASES[_IDS.index(cid)]


def _host_describe(slc, case, monkeypatch, env=None):
    P, S, groups, _ = sc.problem(slc, case["plant"])
    sc.set_knobs(monkeypatch, case["env"] if env is None else env)
    return slc.dist.describe_launches(P, S, groups, None, NCU, objective="sum_of_norms")


def _lifted_env(case):
    return {k: v for k, v in case["env"].items() if k != "SLS_MAX_PER_CU"}


def _strip_grid(desc, also_per_cu=False):
    """describe() without `grid=` (and, for a plan with a tile launch, without the `per_cu=` the knob caps)."""
    return re.sub(r"grid=\d+|per_cu=\d+" if also_per_cu else r"grid=\d+", "", desc)


def _check_classes(slc, case, desc):
    """nsub of every launch = the number of columns whose oracle index set falls into that launch's class."""
    import sls_oracle as o
    P, S, _, _ = sc.problem(slc, case["plant"])
    Po = o.OraclePlant(P.A, P.B1, P.B2)
    want = {}
    for c in range(P.Nx):
        _, _, _, sx, su = o.sparsity_dim_reduction(Po, [c], S)
        k = sc.wave_class_of(len(sx)) if len(su) <= 64 and "SLS_SON_TILE" not in case["env"] else None
        name = TILE_LDS if k is None else WAVE_NAMES[k]
        want[name] = want.get(name, 0) + 1
    got = {k: n for k, n, _ in sc.launches(desc)}
    assert len(got) == len(sc.launches(desc)) and got == want, (case["id"], got, want)


# ------------------------------------------------------------------ host twin: runs without a GPU

@pytest.mark.parametrize("cid", _IDS)
def test_son_launch_lists_on_256_cus(slc, cid, monkeypatch):
    """Kernel selection alone, for 256 CUs: every case of the table gets the pinned launch list, so the shapes are proven before
    a GPU is used and a later routing change cannot quietly move a case to another kernel or back to grid == nsub."""
    case = _get(cid)
    desc = _host_describe(slc, case, monkeypatch)
    assert sc.short(desc) == case["pinned"], desc
    if case["kind"] == "classes":
        _check_classes(slc, case, desc)
    if case["kind"] in ("reuse_wave", "reuse_tile") or cid == "mixed_tile":
        assert any(g < n for _, n, g in sc.launches(desc)), desc
    if case["lift"]:
        lifted = _host_describe(slc, case, monkeypatch, _lifted_env(case))
        tile = case["kind"] == "mixed"
        assert _strip_grid(lifted, tile) == _strip_grid(desc, tile), (desc, lifted)
        assert all(n == g for _, n, g in sc.launches(lifted)), lifted


def test_son_table_names_every_build():
    """The six one-wave sum-of-norms instantiations and the tile build's LDS and workspace variants each appear by name in at
    least one pinned (and therefore asserted) launch list."""
    pinned = ";".join(c["pinned"] for c in CASES)
    for name in WAVE_NAMES + (TILE_LDS, TILE_WS, TILE_BIG):
        assert name + " " in pinned, name


# ------------------------------------------------------------------ GPU

_runs = {}


def _device_ncu():
    import torch
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert ncu == NCU, f"the cases of this module are sized for {NCU} compute units; this device reports {ncu}: their launch lists " \
                       "(grid < nsub) have to be re-derived for it"
    return ncu


def _run(slc, case, monkeypatch, env=None, twice=False):
    """A fresh context and plan under the case's knobs, one execute (two with `twice`): describe(), mask-order values, status."""
    P, S, groups, _ = sc.problem(slc, case["plant"])
    sc.set_knobs(monkeypatch, case["env"] if env is None else env)
    ctx = slc.Context([0])
    try:
        plan = slc.Plan(ctx, P, S, groups, objective="sum_of_norms")
        try:
            out = dict(desc=plan.describe())
            d = plan.alloc_values()
            plan.execute(d); plan.synchronize()
            out["vals"] = np.concatenate(sum(plan.download(d), []))
            out["st"], out["rs"], out["it"] = (a.copy() for a in plan.fetch_status())
            if twice:
                import torch
                second = torch.full((max(plan.info["n_values"], 1),), float("nan"), dtype=torch.float64, device="cuda:0")
                torch.cuda.synchronize()
                plan.execute(second.data_ptr()); plan.synchronize()
                out["vals2"] = np.concatenate(sum(plan.download(second.data_ptr()), []))
                out["st2"], out["rs2"], out["it2"] = (a.copy() for a in plan.fetch_status())
                out["vals1_again"] = np.concatenate(sum(plan.download(d), []))
        finally:
            plan.close()
    finally:
        ctx.close()
    return out


def _live_list(slc, case, run, monkeypatch):
    """The live describe() is the host view for this device and the pinned text."""
    _device_ncu()
    assert run["desc"] == _host_describe(slc, case, monkeypatch), run["desc"]
    assert sc.short(run["desc"]) == case["pinned"], run["desc"]


def _check_columns(slc, case, run, cols, stats):
    P, S, _, colidx = sc.problem(slc, case["plant"])
    for c in cols:
        ref = sc.oracle_column(slc, case["plant"], c)
        assert ref["dg"]["feasible"], (case["id"], c)
        sc.check_column(ref, sc.column_z(P, S, run["vals"], colidx, c, ref["oi"]), stats, (case["id"], c))


def _steps(run):
    return f"ADMM steps {int(run['it'].min())}…{int(run['it'].max())}"


def _report(cid, t0, stats, extra=""):
    print(f"{cid}: {time.perf_counter() - t0:.2f} s (oracle of {_get(cid)['plant']} so far {sc.oracle_seconds.get(_get(cid)['plant'], 0.0):.2f} s); {stats.get('n', 0)} columns against the oracle, worst objective error "
          f"{stats.get('obj', 0.0):.2e}, worst ‖ΔΦ‖∞/max|Φ| {stats.get('phi', 0.0):.2e}, worst ‖Ez − f‖∞ {stats.get('res', 0.0):.2e} {extra}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("classes"))
def test_son_every_size_class(slc, oracle, cid, monkeypatch):
    """Part 1 of the module docstring."""
    case = _get(cid)
    P, S, _, _ = sc.problem(slc, case["plant"])
    t0 = time.perf_counter()
    run = _run(slc, case, monkeypatch)
    print(f"{cid}: {run['desc']}")
    _live_list(slc, case, run, monkeypatch)
    _check_classes(slc, case, run["desc"])
    assert np.all(run["st"] == 0), run["st"]
    stats = {}
    edge = list(range(18))
    cols = edge + [P.Nx - 1 - c for c in edge] + [P.Nx // 2 - 1, P.Nx // 2]
    assert len(set(cols)) == 38
    _check_columns(slc, case, run, cols, stats)
    worst = sc.achievability(P, S, run["vals"])
    assert worst <= 1e-9, worst
    _report(cid, t0, stats, f"achievability {worst:.1e}, {_steps(run)}")


_SPREAD48 = sorted(set(range(10)) | set(range(390, 400)) | set(range(380, 390)) | {int(c) for c in np.linspace(15, 372, 18)})


def _one_wave_answer(slc, monkeypatch):
    """The one-wave home's run of chain-400 under SLS_MAX_PER_CU=1: computed once, shared, never modified."""
    if "reuse_wave" not in _runs:
        run = _run(slc, _get("reuse_wave"), monkeypatch)
        for a in run.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _runs["reuse_wave"] = run
    return _runs["reuse_wave"]


def _bit_equal(run, twin, colidx, cols=None):
    sel = slice(None) if cols is None else cols
    vsel = slice(None) if cols is None else np.isin(colidx, cols)
    for k in ("st", "it", "rs"):
        assert np.array_equal(run[k][sel], twin[k][sel]), (k, np.flatnonzero(run[k] != twin[k])[:20])
    a, b = run["vals"][vsel], twin["vals"][vsel]
    diff = np.flatnonzero(a != b)
    assert np.array_equal(a, b), (len(diff), np.unique(colidx[vsel][diff])[:20], np.abs(a - b).max())


@pytest.mark.gpu
def test_son_second_column_one_wave(slc, oracle, monkeypatch):
    """Part 2, one-wave home: 144 workgroups of the <32,12> launch draw a second column; bit equality with the lifted plan."""
    assert len(_SPREAD48) == 48
    case = _get("reuse_wave")
    P, S, _, colidx = sc.problem(slc, case["plant"])
    t0 = time.perf_counter()
    run = _one_wave_answer(slc, monkeypatch)
    print(f"reuse_wave: {run['desc']}")
    _live_list(slc, case, run, monkeypatch)
    k, nsub, grid = sc.launches(run["desc"])[0]
    assert k == WAVE_NAMES[3] and grid < nsub and nsub - grid > 100, run["desc"]
    twin = _run(slc, case, monkeypatch, _lifted_env(case))
    assert _strip_grid(twin["desc"]) == _strip_grid(run["desc"]) and twin["desc"] != run["desc"], (run["desc"], twin["desc"])
    assert all(n == g for _, n, g in sc.launches(twin["desc"])), twin["desc"]
    assert np.all(run["st"] == 0), np.flatnonzero(run["st"])
    _bit_equal(run, twin, colidx)
    stats = {}
    _check_columns(slc, case, run, _SPREAD48, stats)
    worst = sc.achievability(P, S, run["vals"])
    assert worst <= 1e-9, worst
    _report("reuse_wave", t0, stats, f"achievability {worst:.1e}, {_steps(run)}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("reuse_tile"))
def test_son_second_column_tile(slc, oracle, cid, monkeypatch):
    """Part 2, tile home: 144 workgroups draw a second column from the queue; the oracle, and the one-wave home's answer."""
    case = _get(cid)
    P, S, _, colidx = sc.problem(slc, case["plant"])
    t0 = time.perf_counter()
    run = _run(slc, case, monkeypatch)
    print(f"{cid}: {run['desc']}")
    _live_list(slc, case, run, monkeypatch)
    (_, nsub, grid), = sc.launches(run["desc"])
    assert grid < nsub and nsub - grid > 100, run["desc"]
    assert np.all(run["st"] == 0), np.flatnonzero(run["st"])
    worst = sc.achievability(P, S, run["vals"])
    assert worst <= 1e-9, worst
    stats = {}
    _check_columns(slc, case, run, _SPREAD48, stats)
    wave = _one_wave_answer(slc, monkeypatch)
    assert np.all(wave["st"] == 0)
    far = 0.0
    for c in range(P.Nx):
        sel = colidx == c
        far = max(far, np.abs(run["vals"][sel] - wave["vals"][sel]).max() / np.abs(wave["vals"][sel]).max())
    assert far <= 2e-6, far
    _report(cid, t0, stats, f"achievability {worst:.1e}, farthest column from the one-wave home {far:.2e}, {_steps(run)}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("mixed"))
def test_son_mixed_statuses(slc, oracle, cid, monkeypatch):
    """Part 2, mixed statuses: feasible and infeasible columns side by side, every 8th column on the oracle."""
    case = _get(cid)
    P, S, _, colidx = sc.problem(slc, case["plant"])
    t0 = time.perf_counter()
    run = _run(slc, case, monkeypatch)
    print(f"{cid}: {run['desc']}")
    _live_list(slc, case, run, monkeypatch)
    assert np.all(np.isfinite(run["vals"]))
    sc.set_knobs(monkeypatch, {})
    ctx = slc.Context([0])
    try:
        _, _, info_h2 = slc.SLS_H2(P, S, ctx=ctx, return_info=True, dropzeros=False)
    finally:
        ctx.close()
    stats, n_feasible, n_infeasible = {}, 0, 0
    for c in range(0, P.Nx, 8):
        ref = sc.oracle_column(slc, case["plant"], c)
        if not ref["dg"]["feasible"]:
            n_infeasible += 1
            assert run["st"][c] != 0, c
            continue
        n_feasible += 1
        if info_h2["col_status"][c] != 0:
            assert run["st"][c] != 0, c
            continue
        assert run["st"][c] == 0, (c, run["st"][c])
        sc.check_column(ref, sc.column_z(P, S, run["vals"], colidx, c, ref["oi"]), stats, (cid, c))
    assert n_feasible > 0 and n_infeasible > 0, (n_feasible, n_infeasible)
    assert stats.get("n", 0) >= 10, stats
    if case["lift"]:
        twin = _run(slc, case, monkeypatch, _lifted_env(case))
        assert _strip_grid(twin["desc"], True) == _strip_grid(run["desc"], True), (run["desc"], twin["desc"])
        assert np.array_equal(run["st"], twin["st"]), np.flatnonzero(run["st"] != twin["st"])
        import sls_oracle as o
        Po = o.OraclePlant(P.A, P.B1, P.B2)
        small = np.array([c for c in range(P.Nx) if len(o.sparsity_dim_reduction(Po, [c], S)[3]) <= sc.WAVE_CAPS[-1]])
        assert len(small) == sum(n for k, n, _ in sc.launches(run["desc"]) if k in WAVE_NAMES)
        _bit_equal(run, twin, colidx, small)
    else:
        (_, nsub, grid), = sc.launches(run["desc"])
        assert grid < nsub and nsub - grid > 100, run["desc"]
    _report(cid, t0, stats, f"{n_feasible} feasible and {n_infeasible} infeasible in the sample")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("short"))
def test_son_short_horizons(slc, oracle, cid, monkeypatch):
    """Part 3: T = 1…4, statuses exactly the oracle's, feasible columns at the tolerances, the oracle's zero blocks zero."""
    case = _get(cid)
    P, S, _, colidx = sc.problem(slc, case["plant"])
    T = len(S[0])
    t0 = time.perf_counter()
    run = _run(slc, case, monkeypatch)
    print(f"{cid}: {run['desc']}")
    _live_list(slc, case, run, monkeypatch)
    assert np.all(np.isfinite(run["vals"]))
    refs = [sc.oracle_column(slc, case["plant"], c) for c in range(P.Nx)]
    feasible = np.array([bool(r["dg"]["feasible"]) for r in refs])
    assert feasible.tolist() == ([c == 6 for c in range(13)] if T == 1 else [True] * 13)
    assert abs(refs[6]["dg"]["obj"] - np.sqrt(2.0)) < 1e-9
    assert np.array_equal(run["st"] == 0, feasible), run["st"]
    stats, n_zero = {}, 0
    for c in np.flatnonzero(feasible):
        ref = refs[c]
        z = sc.column_z(P, S, run["vals"], colidx, c, ref["oi"])
        sc.check_column(ref, z, stats, (cid, c))
        zmax = np.abs(ref["z"]).max()
        for t, idx in enumerate(ref["tslice"]):
            if len(idx) and np.abs(ref["z"][idx]).max() <= 1e-9 * zmax:
                n_zero += 1
                assert np.abs(z[idx]).max() <= 1e-6 * zmax, (cid, c, t, np.abs(z[idx]).max())
            else:
                assert t < 2                                      # dead-beat in two steps: every later block is an oracle zero
    assert n_zero == (12 * (T - 2) + (T - 1) if T >= 2 else 0), n_zero     # column 6 (cut off, ñx = 1) is at rest after one step
    _report(cid, t0, stats, f"{n_zero} zero blocks, {_steps(run)}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("trivial"))
def test_son_trivial_column(slc, cid, monkeypatch):
    """Part 3: a column outside its own index set gives SLS_COL_TRIVIAL and Φ = 0 under this objective too."""
    case = _get(cid)
    run = _run(slc, case, monkeypatch)
    _live_list(slc, case, run, monkeypatch)
    assert run["st"].tolist() == [slc._capi.SLS_COL_TRIVIAL] and np.all(run["vals"] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("inputless"))
def test_son_columns_without_inputs(slc, oracle, cid, monkeypatch):
    """Part 3: columns with ñu = 0.  Statuses equal the oracle's feasible flags; feasible columns at the tolerances."""
    case = _get(cid)
    P, S, _, colidx = sc.problem(slc, case["plant"])
    run = _run(slc, case, monkeypatch)
    _live_list(slc, case, run, monkeypatch)
    assert np.all(np.isfinite(run["vals"]))
    refs = [sc.oracle_column(slc, case["plant"], c) for c in range(P.Nx)]
    assert min(len(r["oi"]["su"]) for r in refs) == 0
    feasible = np.array([bool(r["dg"]["feasible"]) for r in refs])
    assert np.array_equal(run["st"] == 0, feasible), (run["st"], feasible)
    stats = {}
    _check_columns(slc, case, run, np.flatnonzero(feasible), stats)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids("twice"))
def test_son_plan_executed_twice(slc, oracle, cid, monkeypatch):
    """Part 4: the second execute, into a NaN-filled array of its own, repeats the first bit for bit."""
    case = _get(cid)
    P, S, _, colidx = sc.problem(slc, case["plant"])
    t0 = time.perf_counter()
    run = _run(slc, case, monkeypatch, twice=True)
    _live_list(slc, case, run, monkeypatch)
    assert np.all(run["st"] == 0) and np.all(run["st2"] == 0)
    assert not np.isnan(run["vals2"]).any() and np.all(np.isfinite(run["vals"]))
    for k in ("st", "rs", "it", "vals"):
        assert np.array_equal(run[k], run[k + "2"]), (k, np.flatnonzero(run[k] != run[k + "2"])[:20])
    assert np.array_equal(run["vals"], run["vals1_again"])          # and the first array was left alone
    stats = {}
    _check_columns(slc, case, dict(vals=run["vals2"]), [0, 3, 8, 20, 36, 39], stats)
    _report(cid, t0, stats)
