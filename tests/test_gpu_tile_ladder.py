"""The tile kernel's whole column solve (build of Ã·Q, sweep, substitution, residual passes, multiplier iteration) at every tile
count and in every home of the block, against the oracle.

`h2_column_tile_kernel` is the only kernel whose arithmetic depends on how ñx sits against a grid of 16×16 tiles: the block is
padded to 16·NT with a −1 pad diagonal, a workspace block is swept with pairs of pivot tiles (the last one alone when NT is odd),
the look-ahead stops at the last pivot, Ã·Q is built in 64-column chunks and in row strips, and every launch is carved by the
maxima over its bin, so most columns run inside a carve sized for another column.  The stock workloads reach the column solve at
ñx = 85, 171, 181 and 576 only.  Here (tests/tile_cases.py): chain_plant(260) under a composite mask whose 27 ladder columns have
ñx = 16k − 1, 16k, 16k + 1 for k = 1…9 (NT = 1…10), as the problems
  act_all     B2 = I (ñu = ñx + 1 or + 2: 17…146)
  readme_act  the README actuators (ñu = 5…50)
  weighted    act_all with diagonal LQR weights, B1 = diag(b) and a sparse D11 (the weight record together with the padding)
  dense       readme_act with a banded [C1 D12], D11 ≠ 0, B1 = diag(b) (the CG build)
in the homes LDS (ñx ≤ 96 by default, two workgroups per CU; ≤ 144 under SLS_TILE_LDS_MAXNT=9 with one per CU and the whole Ã·Q
image in LDS), workspace (SLS_TILE_GLOBAL=1) and carve (SLS_TILE_BIG=all).  One table (tile_cases.CASES) drives these tests and
their host twin tests/test_tile_cases_host.py, which proves without a GPU that every size is hit, that the reference is feasible
on every ladder column and that every case's launch list for 256 CUs is the pinned one.

The reference is the C restatement of the oracle for the default weights and the NumPy oracle (dense SVD null-space method) for
"weighted" and "dense" (the C restatement knows the default weights only); it is computed once per session per problem and
never modified.  Every column is compared: |Φ_gpu − Φ_ref| < TOL = 1e-8 absolute (max |Φ_ref| of every column is between 1 and
a few units), status 0, max_residual < 1e-9.

1. test_ladder_in_one_call: the 27 columns as 27 single-column groups of one call, so that the small columns run inside the
   carve of the launch's largest column.
2. test_each_size_alone: each column as a call of its own (readme_act), so that every size also runs in a carve that is tight.
3. test_homes_agree: LDS (MAXNT=9), workspace and carve give the same Φ to 1e-10·max(1, max|Φ|).
4. test_short_horizons_with_the_block_in_the_workspace: T = 2, 3 at ñx = 97, 113 (test_short_horizons[tile] stops at ñx ≤ 13).

Largest |Φ_gpu − Φ_ref| per (case, NT), measured on an MI355X:
                        NT = 1        2        3        4        5        6        7        8        9       10
  act_all    (4 homes)  5.6e-17  5.6e-17  1.1e-16  5.6e-17  5.6e-17  5.6e-17  5.6e-17  5.6e-17  5.6e-17  5.6e-17
  readme_act (4 homes)  1.9e-14  2.2e-14  1.6e-14  2.8e-14  1.4e-14  1.9e-14  1.4e-14  2.2e-14  1.5e-14  1.8e-15
  weighted   (4 homes)  7.8e-16  1.3e-15  1.3e-15  7.8e-16  8.9e-16  6.7e-16  8.9e-16  1.0e-15  1.1e-15  1.1e-15
  dense      (3 homes)  4.2e-09  1.1e-10  2.8e-11  1.0e-09  2.5e-10  5.7e-11  6.4e-12  1.7e-11  3.1e-11  1.4e-11
The homes of a problem give the same figure to the two digits shown (they agree with each other to 4.4e-16 at the most, most pairs
bit for bit), and each column alone gives the figures of readme_act again.  The plain build ends at max_residual 1.7e-16
(act_all, weighted) and 2.2e-14 (readme_act); the CG build stops at its own tolerance (max_residual 9.6e-13), which is what the
dense row shows.  Short horizons: 5.6e-17 (T = 2) and 2.8e-17 (T = 3).
Cost on that host: 11 s for the module, of which the NumPy oracle 4.0 s ("weighted") and 2.1 s ("dense") once per session and the
first context 0.5 s; every other case is 0.01 – 0.1 s.

What the ladder sees, shown once with value-only edits to a scratch copy of sls_tile_kernel.hip (never committed):
  * the second panel's term dropped from the look-ahead tile (`if (two) rank16(Y1, qn, qn, …)`): 11 of these tests fail (readme_act
    and dense in the lds, workspace and carve homes, in one call and alone, and test_homes_agree; columns from ñx = 49 on come back
    flagged); the LDS-only lds9 cases pass, as they must (single panels).  test_gpu_tile.py as it stood also fails (5 tests).
  * the first panel's term dropped instead: 7 fail (the LDS homes of readme_act and dense, from ñx = 31 on); the workspace homes
    still pass with max_residual < 1e-9 (the multiplier iteration absorbs the damaged inverse there).  test_gpu_tile.py fails too (17).
  * `wc[ch] = wprev[cc]` read from `min(cc, n − 2)`: 10 fail (LDS homes of readme_act, weighted, dense).  test_gpu_tile.py fails (12).
  * the pad diagonal of −P_0 set to −2: nothing fails anywhere and every figure above is reproduced digit for digit — the edit
    changes no result: pad rows carry zero weights in Q = W + W N W and no coupling to the real rows, so any finite negative pad
    value gives the same Φ (the same holds for the `1.0` pad diagonal of D′, whose pivots are clamped at pivmin anyway).
  act_all passes under all four edits (with every state actuated the residual passes evidently repair what these edits damage), so
  the sweep and the build are guarded by readme_act, weighted and dense; act_all adds the largest ñu and the carve they need.
"""
import time

import numpy as np
import pytest

import tile_cases as tc
from conftest import flat_phi
from tile_cases import TOL

pytestmark = pytest.mark.gpu

_runs = {}


def _device_ncu():
    import torch
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert ncu == tc.NCU, f"the cases of this module are pinned for {tc.NCU} compute units; this device reports {ncu}"


def _flat(Phix, Phiu, S):
    return np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])


def _run(slc, cid, monkeypatch):
    """The ladder of a case in one call, on a fresh context set up after the knobs: describe(), host view of the same, mask-order
    values, statuses, info.  Computed once per session and shared (test_homes_agree); never modified."""
    if cid not in _runs:
        case = tc.get(cid)
        pr = tc.problem(slc, case["problem"])
        tc.set_knobs(monkeypatch, case["env"])
        host = slc.dist.describe_launches(pr["P"], pr["S"], pr["groups"], None, tc.NCU)
        ctx = slc.Context([0])
        try:
            plan = slc.Plan(ctx, pr["P"], pr["S"], pr["groups"])
            try:
                desc = plan.describe()
            finally:
                plan.close()
            Phix, Phiu, info = slc.SLS_H2(pr["P"], pr["S"], pr["groups"], ctx=ctx, return_info=True, dropzeros=False)
        finally:
            ctx.close()
        got = _flat(Phix, Phiu, pr["S"])
        got.setflags(write=False)
        _runs[cid] = dict(desc=desc, host=host, got=got, st=info["col_status"].copy(), info=info)
    return _runs[cid]


def _per_nt_text(err):
    return "  ".join(f"NT={nt}: {e:.1e}" for nt, e in sorted(tc.worst_per_nt(err).items()))


def _check_against_reference(slc, name, got, st, tag):
    ref = tc.reference(slc, name)
    assert np.all(ref["status"] == 0) and ref["resid"].max() < tc.residual_bound(name)      # no column is left out below
    assert len(st) == 27
    err, big = tc.column_errors(slc, name, got)
    print(f"{tag}: worst |ΔΦ| per tile count  {_per_nt_text(err)}")
    assert len(err) == 27 and big.min() > 0.1
    # the messages are plain strings naming every offending size with its tile count (pytest shortens tuples and dicts)
    flagged = ", ".join(f"ñx={n} (NT={tc.nt_of(n)}): {s}" for n, s in zip(tc.TARGETS, st.tolist()) if s != 0)
    assert not flagged, f"{tag}: col_status ≠ 0 at {flagged}"
    bad = ", ".join(f"ñx={n} (NT={tc.nt_of(n)}): {e:.2e}" for n, e in zip(tc.TARGETS, err) if not e < TOL)
    assert not bad, f"{tag}: |Φ_gpu − Φ_ref| ≥ {TOL:g} at {bad}; worst per tile count {_per_nt_text(err)}"
    return err


@pytest.mark.parametrize("cid", tc.IDS)
def test_ladder_in_one_call(slc, oracle, cid, monkeypatch):
    """Part 1 of the module docstring."""
    _device_ncu()
    case = tc.get(cid)
    t0 = time.perf_counter()
    run = _run(slc, cid, monkeypatch)
    t_gpu = time.perf_counter() - t0
    print(f"{cid}: {run['desc']}")
    assert run["desc"] == run["host"], (run["desc"], run["host"])
    assert tc.short(run["desc"]) == case["pinned"], run["desc"]
    _check_against_reference(slc, case["problem"], run["got"], run["st"], cid)
    assert run["info"]["max_residual"] < 1e-9, run["info"]["max_residual"]
    print(f"{cid}: GPU side {t_gpu:.2f} s, reference of {case['problem']} {tc.oracle_seconds[case['problem']]:.2f} s (once per session), "
          f"max_residual {run['info']['max_residual']:.1e}")


_ALONE = {"lds": tc.ENV_LDS, "lds9": tc.ENV_LDS9, "workspace": tc.ENV_WS, "carve": tc.ENV_BIG}


@pytest.mark.parametrize("home", list(_ALONE))
def test_each_size_alone(slc, oracle, home, monkeypatch):
    """Part 2: 27 one-column calls on one context, so that nmax, mmax and the list capacities of the carve are the column's own.
    The home is checked on every plan: LDS up to ñx = 96 ("lds") or 144 ("lds9") and the workspace beyond, else as the knob says."""
    pr = tc.problem(slc, "readme_act")
    P, S = pr["P"], pr["S"]
    tc.set_knobs(monkeypatch, _ALONE[home])
    got = np.zeros(len(pr["colidx"]))
    st = np.zeros(27, dtype=np.int64)
    worst_res = 0.0
    ctx = slc.Context([0])
    try:
        for k, (n, c) in enumerate(zip(tc.TARGETS, pr["cols"])):
            plan = slc.Plan(ctx, P, S, [[c]])
            try:
                (kern, nsub, nmax), = tc.launch_sizes(plan.describe())
            finally:
                plan.close()
            in_lds = home == "lds" and n <= 96 or home == "lds9" and n <= 144
            assert (nsub, nmax) == (1, n) and ("block_in_LDS" in kern) == in_lds and ("carve_in_workspace" in kern) == (home == "carve"), (n, kern)
            Phix, Phiu, info = slc.SLS_H2(P, S, [[c]], ctx=ctx, return_info=True, dropzeros=False)
            one = _flat(Phix, Phiu, S)
            sel = pr["colidx"] == c
            assert np.all(one[~sel] == 0.0), n
            got[sel] = one[sel]
            st[k] = info["col_status"][0]
            worst_res = max(worst_res, info["max_residual"])
    finally:
        ctx.close()
    _check_against_reference(slc, "readme_act", got, st, f"alone-{home}")
    assert worst_res < 1e-9, worst_res


@pytest.mark.parametrize("name,homes", [(p, ("lds9", "workspace", "carve")) for p in ("act_all", "readme_act", "weighted")]
                         + [("dense", ("default", "workspace", "carve"))])
def test_homes_agree(slc, name, homes, monkeypatch):
    """Part 3: the same mathematics in three homes of the block; pairwise to 1e-10·max(1, max|Φ|), the bound of
    test_carve_in_workspace_variant_equals_the_lds_variants."""
    runs = [_run(slc, f"{name}-{h}", monkeypatch) for h in homes]
    for r in runs:
        assert np.all(r["st"] == 0), r["st"]
    scale = max(1.0, np.abs(runs[0]["got"]).max())
    for i in range(3):
        for j in range(i + 1, 3):
            far = np.abs(runs[i]["got"] - runs[j]["got"]).max()
            print(f"{name}: {homes[i]} vs {homes[j]}: {far:.2e} (max|Φ| {scale:.2f})")
            assert far < 1e-10 * scale, (name, homes[i], homes[j], far)


@pytest.mark.parametrize("Th", tc.SHORT_T)
def test_short_horizons_with_the_block_in_the_workspace(slc, oracle, Th, monkeypatch):
    """Part 4: T + 1 = 3 and 4 block rows on blocks of 7 and 8 tiles swept in pairs in the workspace; statuses and values
    against the C restatement, which finds both columns feasible at both horizons (host twin)."""
    import sls_oracle_cport as cp
    pr = tc.short_problem(slc, Th)
    P, S = pr["P"], pr["S"]
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ox, ou, oinfo = cp.SLS_H2(Po, S, cols=pr["cols"], nthreads=2)
    want = _flat(ox, ou, S)
    feasible = (oinfo["status"] == 0) & (oinfo["resid"] < 1e-12)
    assert feasible.all(), oinfo
    tc.set_knobs(monkeypatch, tc.ENV_LDS)
    ctx = slc.Context([0])
    try:
        plan = slc.Plan(ctx, P, S, pr["groups"])
        try:
            desc = plan.describe()
        finally:
            plan.close()
        Phix, Phiu, info = slc.SLS_H2(P, S, pr["groups"], ctx=ctx, return_info=True, dropzeros=False)
    finally:
        ctx.close()
    assert tc.short(desc) == tc.SHORT_PINNED, desc
    assert np.array_equal(info["col_status"] == 0, feasible), info["col_status"]
    got = _flat(Phix, Phiu, S)
    for n, c in zip(pr["targets"], pr["cols"]):
        sel = pr["colidx"] == c
        err = np.abs(got[sel] - want[sel]).max()
        print(f"T={Th} ñx={n}: |ΔΦ| {err:.1e}, max|Φ| {np.abs(want[sel]).max():.2f}")
        assert np.abs(want[sel]).max() > 0.1 and err < TOL, (Th, n, err)
    assert info["max_residual"] < 1e-9
