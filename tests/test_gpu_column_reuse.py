"""Workgroups that solve several columns in a row, and the throughput regime of the one-wave kernel, at small shapes.

Every column kernel takes its columns in a loop (`for (s = blockIdx.x; s < nsub; s += gridDim.x)` in the one-wave, twisted and
round-1 workgroup kernels, a work queue in the tile kernel).  The second trip through that loop is where LDS lists, padded rows,
register tiles, flags and factor slots left by the previous column can leak into the next one.  The other quick GPU tests build
plans with grid == nsub; here `SLS_MAX_PER_CU` caps the occupancy so that 300 – 400 columns on 256 CUs give every workgroup a
second (differently sized) column, and 1040 columns reach the throughput regime (merge_cls < 0: more than 4·ncu columns) that
otherwise only chain-4096 sees.

Per case (the table `CASES` below, read by the GPU test and by its host twin):
  1. statuses: `info["col_status"] == 0` exactly where the C restatement of the oracle reports status 0, on EVERY column;
  2. values on the feasible columns within TOL = 1e-8 of the oracle (the bound and its derivation: header of test_gpu_parity.py);
  3. independence from the schedule (one-wave and twisted kernels): the same plan built with the knob lifted (grid == nsub; the
     two describe() strings differ in nothing but `grid=`) must give bit-identical values, residuals, iteration counts and
     statuses — a column's arithmetic does not depend on which workgroup ran it or what ran before, so any differing bit is state
     carried from one column to the next.  The tile and workgroup kernels change their LDS plan with the knob (oth_rows, per_cu)
     or cannot be lifted (one workgroup per CU by LDS): statuses exactly and values against the oracle only;
  4. the live `plan.describe()` equals `dist.describe_launches` for the device's CU count and names the expected kernel with
     grid < nsub.  The shapes are sized for 256 CUs; another CU count fails the test with a message (it does not skip).
The throughput chain cases (every column feasible) also pass the three achievability identities of test_chain_full_size_properties.

The four-wave twisted kernel cannot be given a second column: routing admits it only for nsub ≤ ncu with one column per CU and
as a plan's only launch, so its grid always equals nsub.  `test_four_wave_kernel_never_gets_a_second_column` pins exactly that,
over every recorded launch list and every case here — that invariant is what the kernel's correctness on reuse currently rests
on (its column loop has never run twice).

What each plant of the table is there for:
  * chain_plant(300), d = 9, T = 12 (NPL = 32, class <32,12>): interior ñx = 21 and 18 edge columns of ñx 11…20 at the end of the
    descending order, so the last workgroups go from an interior column to a smaller edge column.  Every column is feasible.
  * d = 20, T = 14 (NPL = 64, class <64,48>): the largest index set has 39 states; at T = 10 it has 27 and the class is <32,16>.
  * d = 2, T = 6 and T = 3 (NPL = 16, class <16,3>; T = 3 is the `twisted_middle` edge): no column is feasible at these
    horizons (`statuses="none"`), so these cases check that every column is flagged and that statuses, residuals, iteration
    counts and values are bit-equal between the schedules.  d = 6, T = 14 (ñx ≤ 15, class <16,4>, every column feasible) carries
    the NPL = 16 value parity.
  * P_in_LDS at T = 12 takes 88 760 B of LDS: one column per CU with or without the knob, so 300 columns on 256 CUs have no
    grid == nsub plan.  Its schedule-independent twin is the pair of half-range plans [0,150) + [150,300) (grid == nsub == 150
    each; describe() equal up to `nsub=` and `grid=`).
  * random_plant(400, 2, 1, seed=5), masks (2, 8, 1.5) — the plant of test_random_sparse_plant_ragged_classes: ñx 1…52, ñu up to
    97, an actuator on every state, so all 400 columns are feasible.  It gives the tile queue and the round-1 kernel 144 second
    columns of ragged size.
  * random_plant(400, 2, 2, seed=5), same masks (`statuses="mixed"`): an actuator on every other state, ñx 1…25; 58 columns are
    feasible (ñx ≤ 7, oracle residual ≤ 8.7e-11) and 342 infeasible (oracle residual ≥ 1.9e-4).  The descending size order hands
    the small index sets out last: 54 of the 58 feasible columns are among the last 144, the second columns of a launch, each
    after an infeasible first column whose flags or reduction words, if left behind, would flip or perturb it.  The mixed cases
    assert 0 < #feasible < Nx on the oracle's statuses, so that a change to the workload generator cannot turn them into
    single-status cases.
  * chain_plant(1040), d = 9, T = 10: more than 4·256 columns, four size classes (<16,3>, <16,4>, <32,10>, <32,12>), three rounds
    of 347 at two columns per CU.
  * random_plant(1040, 2, 2, seed=1), masks (2, 8, 1.5) (`statuses="mixed"`): the tile launch and six one-wave classes in one
    plan; 133 feasible (oracle residual ≤ 2.1e-14), 907 infeasible (oracle residual ≥ 1.2e-5).

Oracle cost (C restatement, nthreads = 8, measured on a 16-core host; nearly all of it is the Python front end that builds the
dense per-column inputs, the C solve is < 0.4 s everywhere): chain 1100 / T 12 takes 11.6 s and random 1200 takes 14.6 s, over
the 10 s that a reference may cost; chain 1040 / T 10 takes 10.5 s and random 1040 takes 9.7 s.  Chain 300: 1.8 – 3 s per (d, T);
random 400: 3.6 – 4 s.  Each reference is computed once per session and shared by the cases of that plant.
"""
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, flat_phi
from oracle_c import TOL, c_oracle_flat

NCU = 256                                   # the CU count the shapes below are sized for (MI355X)


def _case(id, plant, env, kernel, launch=None, n_launches=None, lift=None, also=(), spare=0, near=None, statuses="some"):
    """plant: ("chain", Nx, d, T) | ("random", Nx, act_every, seed, d, T).  env: the knobs of the reuse run.  kernel: name (with
    template arguments) that the launches under test start with; launch: their exact `nsub= grid=` text; n_launches: how many of
    them.  lift: how the schedule-independent twin is built — "knob" (same plan without SLS_MAX_PER_CU), "halves" (two half-range
    plans), None (oracle only).  also: kernel names that must appear beside it.  spare: the least Σnsub − Σgrid (workgroups that
    are handed a second column).  near: (case id, bound) — Φ equal to that case's within the bound.  statuses: what the oracle
    must report for the plant — "mixed" (feasible and infeasible columns), "none" (no feasible column), "some" (at least one
    feasible column)."""
    return dict(id=id, plant=plant, env=dict(env), kernel=kernel, launch=launch, n_launches=n_launches, lift=lift, also=tuple(also),
                spare=spare, near=near, statuses=statuses)


_R1 = {"SLS_MAX_PER_CU": "1"}
_RANDOM400 = ("random", 400, 1, 5, 2, 8)            # the plant of test_random_sparse_plant_ragged_classes: ñx 1…52, ñu up to 97
_MIXED400 = ("random", 400, 2, 5, 2, 8)             # 58 feasible columns, 342 infeasible
_THROUGHPUT = ("chain", 1040, 9, 10)
CASES = [
    # --- reuse within a workgroup: 300 (400) columns on 256 workgroups ---
    _case("wave32", ("chain", 300, 9, 12), {**_R1, "SLS_NO_TWISTED": "1"}, "h2_column_wave_kernel<32,12>", "nsub=300 grid=150", lift="knob"),
    _case("wave16_T6", ("chain", 300, 2, 6), {**_R1, "SLS_NO_TWISTED": "1"}, "h2_column_wave_kernel<16,3>", "nsub=300 grid=150", lift="knob", statuses="none"),
    _case("wave16_feasible", ("chain", 300, 6, 14), {**_R1, "SLS_NO_TWISTED": "1"}, "h2_column_wave_kernel<16,4>", "nsub=300 grid=150", lift="knob"),
    _case("wave64", ("chain", 300, 20, 14), {**_R1, "SLS_WAVE64": "1"}, "h2_column_wave_kernel<64,48>", "nsub=300 grid=150", lift="knob"),
    _case("twisted32", ("chain", 300, 9, 12), _R1, "h2_column_twisted_kernel<32,12,P_in_workspace>", "nsub=300 grid=150 block=128", lift="knob"),
    _case("twisted16_T6", ("chain", 300, 2, 6), _R1, "h2_column_twisted_kernel<16,3,P_in_workspace>", "nsub=300 grid=150", lift="knob", statuses="none"),
    _case("twisted16_T3", ("chain", 300, 2, 3), _R1, "h2_column_twisted_kernel<16,3,P_in_workspace>", "nsub=300 grid=150", lift="knob", statuses="none"),
    _case("twisted16_feasible", ("chain", 300, 6, 14), _R1, "h2_column_twisted_kernel<16,4,P_in_workspace>", "nsub=300 grid=150", lift="knob"),
    _case("twisted32_P_in_LDS", ("chain", 300, 9, 12), {**_R1, "SLS_P_LDS": "1"}, "h2_column_twisted_kernel<32,12,P_in_LDS>", "nsub=300 grid=150", lift="halves"),
    *[_case(name + tag, plant, {**_R1, "SLS_FORCE_GENERAL": "1", **env}, kernel, "nsub=400 grid=256", spare=100, statuses=statuses)
      for tag, plant, statuses in (("", _RANDOM400, "some"), ("_mixed", _MIXED400, "mixed"))
      for name, env, kernel in (("tile_block_in_LDS", {}, "h2_column_tile_kernel<block_in_LDS>"),
                                ("tile_block_in_workspace", {"SLS_TILE_GLOBAL": "1"}, "h2_column_tile_kernel<block_in_workspace>"),
                                ("tile_carve_in_workspace", {"SLS_TILE_BIG": "all"}, "h2_column_tile_kernel<block_in_workspace,carve_in_workspace>"),
                                ("workgroup_round1", {"SLS_TILE": "0"}, "h2_column_general_kernel"))],
    # --- throughput regime (merge_cls < 0): automatic VG placement, absorb rule, one launch per class ---
    _case("throughput_absorbed", _THROUGHPUT, {}, "h2_column_wave_kernel<32,12>", "nsub=1040 grid=1040", n_launches=1),
    _case("throughput_per_class", _THROUGHPUT, {"SLS_ABSORB": "0"}, "h2_column_wave_kernel", n_launches=4, near=("throughput_absorbed", 1e-10),
          also=("h2_column_wave_kernel<32,12> nsub=1020", "h2_column_wave_kernel<32,10>", "h2_column_wave_kernel<16,4>", "h2_column_wave_kernel<16,3>")),
    _case("throughput_reuse", _THROUGHPUT, {"SLS_MAX_PER_CU": "2"}, "h2_column_wave_kernel<32,12>", "nsub=1040 grid=347", n_launches=1, lift="knob"),
    _case("throughput_ragged", ("random", 1040, 2, 1, 2, 8), {}, "h2_column_wave_kernel", n_launches=6, also=("h2_column_tile_kernel",), statuses="mixed"),
]
_IDS = [c["id"] for c in CASES]
_GRID_EQUALS_NSUB = {"throughput_absorbed", "throughput_per_class", "throughput_ragged"}      # what these pin is the launch list, not reuse

_LAUNCH = re.compile(r"(h2_column_[a-z0-9_]+?)(<[^>]*>)? nsub=(\d+) grid=(\d+) ")


def _launches(desc):
    """describe() text → [(kernel, kernel with template arguments, nsub, grid, the launch's own text)]."""
    out = []
    for seg in [s for s in desc.split(";") if s]:
        m = _LAUNCH.match(seg)
        assert m, (seg, desc)
        out.append((m.group(1), m.group(1) + (m.group(2) or ""), int(m.group(3)), int(m.group(4)), seg))
    return out


def _check_launch_list(case, desc):
    """The case's launch list is what the table says: the kernel, its launch count, grid < nsub (or the stated launch count),
    and no four-wave launch that shares a plan or has grid ≠ nsub."""
    L = _launches(desc)
    mine = [l for l in L if l[1].startswith(case["kernel"])]
    assert mine, (case["id"], desc)
    if case["n_launches"] is not None:
        assert len(mine) == case["n_launches"], (case["id"], desc)
    if case["launch"] is not None:
        assert all(case["launch"] in l[4] for l in mine), (case["id"], desc)
    for other in case["also"]:
        assert other in desc, (case["id"], other, desc)
    nsub, grid = sum(l[2] for l in mine), sum(l[3] for l in mine)
    if case["id"] in _GRID_EQUALS_NSUB:
        assert grid == nsub, (case["id"], desc)
    else:
        assert grid < nsub and nsub - grid >= case["spare"], (case["id"], desc)
    _check_four_wave_invariant(case["id"], desc)


def _check_four_wave_invariant(name, desc):
    L = _launches(desc)
    for kernel, _, nsub, grid, _ in L:
        if kernel == "h2_column_twisted4_kernel":
            assert grid == nsub and len(L) == 1, (name, desc)


_problems, _oracle = {}, {}


def _problem(slc, plant):
    if plant not in _problems:
        wl = slc.workloads
        if plant[0] == "chain":
            _, Nx, d, T = plant
            P = wl.chain_plant(Nx)
        else:
            _, Nx, act, seed, d, T = plant
            P = wl.random_plant(Nx, 2, act, seed=seed)
        S = list(wl.localization_masks(P.A, P.B2, d, T, 1.5))
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        _problems[plant] = (P, S, colidx)
    return _problems[plant]


def _reference(slc, plant):
    """Φ of every column from the C restatement (mask order) + its per-column status; computed once per plant, never modified."""
    if plant not in _oracle:
        P, S, _ = _problem(slc, plant)
        want, oinfo = c_oracle_flat(slc, P, S, list(range(P.Nx)))
        want.setflags(write=False)
        status = np.array(oinfo["status"]); status.setflags(write=False)
        _oracle[plant] = (want, status)
    return _oracle[plant]


def _knobs(monkeypatch, env):
    for k in ("SLS_MAX_PER_CU", "SLS_NO_TWISTED", "SLS_WAVE64", "SLS_P_LDS", "SLS_FORCE_GENERAL", "SLS_TILE", "SLS_TILE_GLOBAL",
              "SLS_TILE_BIG", "SLS_ABSORB", "SLS_TWISTED4", "SLS_VEC_GLOBAL", "SLS_VEC_LDS", "SLS_FULL_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ host twin: runs without a GPU

@pytest.mark.parametrize("cid", _IDS)
def test_case_launch_lists_on_256_cus(slc, cid, monkeypatch):
    """Kernel selection alone, for 256 CUs: every case of the table gets the kernel it names with grid < nsub (or its launch
    count), so the shapes are proven before a GPU is used and a later routing change cannot quietly turn the GPU tests below back
    into grid == nsub tests.  For the cases compared bit for bit, the lifted plan differs in nothing but `grid=` and has
    grid == nsub."""
    case = CASES[_IDS.index(cid)]
    P, S, _ = _problem(slc, case["plant"])
    _knobs(monkeypatch, case["env"])
    desc = slc.dist.describe_launches(P, S, None, None, NCU)
    _check_launch_list(case, desc)
    if case["lift"] == "knob":
        monkeypatch.delenv("SLS_MAX_PER_CU")
        _check_lifted(desc, [slc.dist.describe_launches(P, S, None, None, NCU)], r"grid=\d+")
    elif case["lift"] == "halves":
        h = P.Nx // 2
        _check_lifted(desc, [slc.dist.describe_launches(P, S, None, r, NCU) for r in ((0, h), (h, P.Nx))], r"nsub=\d+ grid=\d+")


def _check_lifted(desc, lifted, what):
    for d2 in lifted:
        assert re.sub(what, "", d2) == re.sub(what, "", desc), (desc, d2)
        assert all(l[2] == l[3] for l in _launches(d2)), d2
        assert d2 != desc


def test_four_wave_kernel_never_gets_a_second_column(slc, monkeypatch):
    """Every h2_column_twisted4_kernel launch has grid == nsub and is its plan's only launch: over the recorded launch list of
    every case of tests/golden/make_golden_launch_lists.py (tests/test_host.py holds those strings, and their set of
    names, to the live routing character for character) and over every case of this module.  The kernel's column loop is never taken twice; this
    invariant, not a test of that loop, is what its correctness on reuse rests on."""
    with open(os.path.join(GOLDEN, "launch_lists.json")) as f:
        golden = json.load(f)["cases"]
    assert any("h2_column_twisted4_kernel" in d for d in golden.values())
    for name, desc in golden.items():
        _check_four_wave_invariant(name, desc)
    for case in CASES:
        P, S, _ = _problem(slc, case["plant"])
        _knobs(monkeypatch, case["env"])
        for ncu in (NCU, 304, 64):
            _check_four_wave_invariant(case["id"], slc.dist.describe_launches(P, S, None, None, ncu))


# ------------------------------------------------------------------ GPU

def _run_plan(slc, ctx, P, S, group_range=None):
    """One execute of a fresh plan: describe(), the mask-order values, fetch_status()."""
    plan = slc.Plan(ctx, P, S, None, group_range)
    try:
        desc = plan.describe()
        d = plan.alloc_values()
        plan.execute(d); plan.synchronize()
        vals = np.concatenate(sum(plan.download(d), []))
        st, rs, it = (a.copy() for a in plan.fetch_status())
    finally:
        plan.close()
    return dict(desc=desc, vals=vals, st=st, rs=rs, it=it)


def _device_ncu():
    import torch
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert ncu == NCU, f"the cases of this module are sized for {NCU} compute units; this device reports {ncu}: their launch lists " \
                       "(grid < nsub, the 4·ncu threshold of the throughput regime) have to be re-derived for it"
    return ncu


def _achievability(P, Phix, Phiu):
    """The identities of test_chain_full_size_properties: Φx[1] = I, Φx[t+1] = AΦx[t] + B2Φu[t], AΦx[T] + B2Φu[T] = 0, and shift
    invariance of interior chain columns 6 states apart."""
    T = len(Phix)
    assert abs(Phix[0] - sp.identity(P.Nx)).max() < 1e-12
    worst = 0.0
    for t in range(T - 1):
        worst = max(worst, abs(Phix[t + 1] - (P.A @ Phix[t] + P.B2 @ Phiu[t])).max())
    worst = max(worst, abs(P.A @ Phix[T - 1] + P.B2 @ Phiu[T - 1]).max())
    assert worst < 1e-11, worst
    j = P.Nx // 2
    for t in sorted({1, T // 2, T - 1}):
        a = Phix[t][:, j].toarray().ravel(); b = Phix[t][:, j + 6].toarray().ravel()
        assert np.abs(a[:-6] - b[6:]).max() < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _IDS)
def test_column_reuse_and_throughput_regime(slc, gpu_ctx, cid, monkeypatch):
    """See the module docstring: statuses and values of every column against the C restatement, the launch list, and — for the
    one-wave and twisted kernels — bit equality with the grid == nsub schedule."""
    case = CASES[_IDS.index(cid)]
    P, S, colidx = _problem(slc, case["plant"])
    want, ostatus = _reference(slc, case["plant"])
    feasible = ostatus == 0
    ncu = _device_ncu()
    _knobs(monkeypatch, case["env"])

    # (4) the live launch list
    run = _run_plan(slc, gpu_ctx, P, S)
    desc = run["desc"]
    print(f"{cid}: {desc}")
    assert desc == slc.dist.describe_launches(P, S, None, None, ncu)
    _check_launch_list(case, desc)

    # (1), (2) the drop-in call under the same knobs, every column against the oracle
    Phix, Phiu, info = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    st = info["col_status"]
    uns = st == slc._capi.SLS_COL_UNSUPPORTED                  # round-1 workgroup kernel only: compared as zeros
    assert not uns.any() or case["kernel"] == "h2_column_general_kernel"
    assert np.all(got[np.isin(colidx, np.flatnonzero(uns))] == 0.0)
    assert np.array_equal((st == 0)[~uns], feasible[~uns]), np.flatnonzero((st == 0) != feasible)
    assert np.array_equal((run["st"] == 0)[~uns], feasible[~uns]), np.flatnonzero((run["st"] == 0) != feasible)
    ok = np.isin(colidx, np.flatnonzero(feasible & ~uns))
    err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
    err_plan = np.abs(run["vals"][ok] - want[ok]).max() if ok.any() else 0.0
    print(f"{cid}: {int(feasible.sum())} feasible of {P.Nx}, max |Φ − Φ_oracle| = {err:.2e} (plan.execute: {err_plan:.2e}), "
          f"max residual {info['max_residual']:.1e}")
    if case["statuses"] == "mixed":
        assert 0 < feasible.sum() < P.Nx, int(feasible.sum())
    elif case["statuses"] == "none":
        assert not feasible.any()
    assert ok.any() == (case["statuses"] != "none")
    assert err < TOL and err_plan < TOL
    assert info["n_unsolved"] == int((~feasible | uns).sum())
    if case["plant"][0] == "random":
        assert info["max_residual"] < 1e-9
    elif case["plant"] == _THROUGHPUT:
        assert feasible.all() and info["max_residual"] < 1e-11
        _achievability(P, Phix, Phiu)

    # (3) independence from the schedule
    if case["lift"] == "knob":
        monkeypatch.delenv("SLS_MAX_PER_CU")
        twin = _run_plan(slc, gpu_ctx, P, S)
        _check_lifted(desc, [twin["desc"]], r"grid=\d+")
    elif case["lift"] == "halves":
        h = P.Nx // 2
        a, b = _run_plan(slc, gpu_ctx, P, S, (0, h)), _run_plan(slc, gpu_ctx, P, S, (h, P.Nx))
        _check_lifted(desc, [a["desc"], b["desc"]], r"nsub=\d+ grid=\d+")
        assert not np.any((a["vals"] != 0) & (b["vals"] != 0))
        twin = dict(vals=a["vals"] + b["vals"], **{k: np.concatenate([a[k], b[k]]) for k in ("st", "rs", "it")})
    else:
        twin = None
    if twin is not None:
        diff = np.flatnonzero(run["vals"] != twin["vals"])
        assert np.array_equal(run["st"], twin["st"]), np.flatnonzero(run["st"] != twin["st"])
        assert np.array_equal(run["it"], twin["it"]), np.flatnonzero(run["it"] != twin["it"])
        assert np.array_equal(run["rs"], twin["rs"]), np.flatnonzero(run["rs"] != twin["rs"])
        assert np.array_equal(run["vals"], twin["vals"]), (len(diff), np.unique(colidx[diff])[:20], np.abs(run["vals"] - twin["vals"]).max())
    if case["near"] is not None:
        other, bound = case["near"]
        oc = CASES[_IDS.index(other)]
        assert oc["plant"] == case["plant"]
        _knobs(monkeypatch, oc["env"])
        ref = _run_plan(slc, gpu_ctx, P, S)
        _check_launch_list(oc, ref["desc"])
        assert np.abs(run["vals"] - ref["vals"]).max() < bound
