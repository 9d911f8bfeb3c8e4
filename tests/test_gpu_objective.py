"""Objective value of every column, evaluated on the device from Φ (csrc/sls_objective.hip) — against the host twin fed the
SAME downloaded Φ, against the project's anchors, and against the oracles.

Same-Φ parity sums the same doubles in two orders, so its bound is derived, not measured: |Δ| ≤ 2·N·2⁻⁵³·S per column, N the
number of products the column sums and S the sum of their absolute values (both from the host twin; objective_cases.summation_bound);
for the total, the columns' bounds plus one more summation over the column values.  Measured on an MI355X: worst |Δ|/bound over
all parity cases 0.082 (23-state chain at T = 2), 0.001 – 0.05 elsewhere, 0 at T = 1 (`-s` prints every case)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import objective_cases as oc
from conftest import GOLDEN, flat_phi

pytestmark = pytest.mark.gpu


def _total_bound(col_bound, col):
    return float(np.sum(col_bound) + 2 * len(col) * oc.U * np.abs(col).sum())


def _run_plan(slc, ctx, P, S, groups=None, objective="h2", ridge=None, refine=False):
    """execute → device objective + download → host twin on the downloaded values; everything a parity check needs"""
    plan = slc.Plan(ctx, P, S, groups, objective=objective)
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        if refine:
            plan.refine(dv)
        col, tot = plan.objective_values(dv)
        col2, tot2 = plan.objective_values(dv)
        assert np.array_equal(col, col2) and tot == tot2                       # two calls in a row: the same bits
        vx, vu = plan.download(dv)
        status = plan.fetch_status()[0]
        desc = plan.describe()
        info = dict(plan.info)
    finally:
        plan.close()
    hcol, htot, n_terms, abs_sum = slc.objective_values_host(P, S, vx, vu, groups, ridge=ridge, objective=objective, return_bound=True)
    return dict(col=col, tot=tot, hcol=hcol, htot=htot, bound=oc.summation_bound(n_terms, abs_sum), vx=vx, vu=vu, status=status,
                desc=desc, info=info)


def _assert_parity(r, tag):
    d = np.abs(r["col"] - r["hcol"])
    print(tag, "worst |Δ|/bound", float((d / np.maximum(r["bound"], 1e-300)).max()), "total Δ", abs(r["tot"] - r["htot"]))
    assert np.all(np.isfinite(r["col"]))
    assert np.all(d <= r["bound"]), (tag, np.flatnonzero(d > r["bound"]))
    assert abs(r["tot"] - r["htot"]) <= _total_bound(r["bound"], r["hcol"])
    assert abs(r["tot"] - r["col"].sum()) <= 2 * len(r["col"]) * oc.U * np.abs(r["col"]).sum()   # the device total IS the sum of its array


@pytest.fixture(scope="module")
def readme_run(slc, gpu_ctx):
    P, S, I, _, _, cost = oc.readme_golden(slc)
    return _run_plan(slc, gpu_ctx, P, S), cost


def test_readme_chain_parity_and_anchors(readme_run):
    """59 columns, T = 29 + 1 slices: ñx+ñu < 64 with ragged masks along the ramp; then the project's anchors through `Plan`."""
    r, cost = readme_run
    assert r["info"]["max_nx"] + r["info"]["max_nu"] < 64
    _assert_parity(r, "readme")
    assert np.abs(r["col"] - cost).max() < 1e-8
    assert abs(r["tot"] - 893.3262819770) < 1e-7


def test_grid_columns_beyond_one_stride(slc, gpu_ctx):
    """10×10 grid at d = 3: ñx+ñu > 64 and no multiple of 64 — several strides per lane, on tile-kernel columns."""
    P = slc.workloads.grid_plant(10, 2)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 3, 8, 1.5))
    r = _run_plan(slc, gpu_ctx, P, S)
    nm = r["info"]["max_nx"] + r["info"]["max_nu"]
    assert nm > 64 and nm % 64 != 0 and "h2_column_tile_kernel" in r["desc"], (nm, r["desc"])
    _assert_parity(r, "grid10")


@pytest.mark.parametrize("weighted", [False, True])
def test_columns_beyond_the_weight_registers(slc, gpu_ctx, weighted):
    """16×16 grid, an actuator per state, d = 7: ñx+ñu up to 314 > 256 — beyond the four weight registers per lane, where the
    diagonal build re-reads hinv / g (weighted) or needs no weights at all (identity cost); five strides per lane."""
    base = slc.workloads.grid_plant(16, 1)
    P = base
    if weighted:
        rng = np.random.default_rng(2)
        C1 = sp.vstack([sp.diags(rng.uniform(0.5, 2.0, base.Nx)), sp.csc_matrix((base.Nu, base.Nx))]).tocsc()
        D12 = sp.vstack([sp.csc_matrix((base.Nx, base.Nu)), sp.diags(rng.uniform(0.5, 2.0, base.Nu))]).tocsc()
        D11 = sp.random(base.Nx + base.Nu, base.Nx, density=0.01, random_state=rng, format="csc")
        P = slc.Plant(base.A, sp.diags(rng.uniform(0.7, 1.3, base.Nx)).tocsc(), base.B2, C1, D11, D12)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 7, 3, 8.0))
    r = _run_plan(slc, gpu_ctx, P, S)
    assert r["info"]["max_nx"] + r["info"]["max_nu"] > 256
    _assert_parity(r, "grid16_weighted" if weighted else "grid16")


def test_coupled_group_larger_than_the_lds_stage(slc, gpu_ctx):
    """One coupled group of 40 columns on a 10×10 grid (ñx+ñu = 170): 40·170 doubles do not fit the 48 KiB stage of the general
    build, which then reads z through L2; four single columns beside it."""
    base = slc.workloads.grid_plant(10, 1)
    B1 = sp.lil_matrix(sp.identity(base.Nx))
    for c in range(39):
        B1[c, c + 1] = 0.3; B1[c + 1, c] = -0.2
    P = slc.Plant(base.A, B1.tocsc(), base.B2)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 3, 4, 8.0))
    groups = [list(range(40))] + [[c] for c in range(40, 44)]
    r = _run_plan(slc, gpu_ctx, P, S, groups)
    assert 40 * (r["info"]["max_nx"] + r["info"]["max_nu"]) > 6144
    _assert_parity(r, "coupled40")
    assert np.all(r["col"][1:40] == 0.0) and r["col"][0] > 0.0


@pytest.mark.parametrize("T", [1, 2])
def test_single_step_sums(slc, gpu_ctx, T):
    P = slc.workloads.chain_plant(23)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 3, T, 1.5))
    _assert_parity(_run_plan(slc, gpu_ctx, P, S), f"chain23_T{T}")


def test_weighted_golden_plant(slc, gpu_ctx):
    """diagonal record with g ≠ 0 (D11 ≠ 0), B1 = diag(b); and the oracle's own cost of the same columns"""
    P, S, I, _, _, cost = oc.weighted_golden(slc)
    r = _run_plan(slc, gpu_ctx, P, S)
    _assert_parity(r, "weighted")
    ok = r["status"] == 0
    assert ok.all() and (np.abs(r["col"] - cost) <= 1e-7 * np.maximum(1.0, cost)).all()


def test_general_weights_golden_plant(slc, gpu_ctx):
    """dense W: the general build, one column per work item; feasible columns also against the oracle's cost"""
    P, S, I, _, _, cost = oc.general_golden(slc)
    r = _run_plan(slc, gpu_ctx, P, S)
    _assert_parity(r, "general")
    ok = r["status"] == 0
    assert ok.sum() >= 8 and (np.abs(r["col"] - cost)[ok] <= 1e-7 * np.maximum(1.0, cost[ok])).all()


@pytest.mark.parametrize("tag", ["dense", "diag"])
def test_coupled_groups_first_column_carries_the_value(slc, gpu_ctx, tag):
    P, S, I, _, _, gcost = oc.coupled_golden(slc, tag)
    assert sorted({len(g) for g in I}) == [1, 2, 3, 4]
    r = _run_plan(slc, gpu_ctx, P, S, I)
    _assert_parity(r, "coupled_" + tag)
    first = oc.group_firsts(I)
    rest = np.setdiff1d(np.arange(len(r["col"])), first)
    assert np.all(r["col"][rest] == 0.0) and not np.any(np.signbit(r["col"][rest]))      # exactly 0.0
    assert (np.abs(r["col"][first] - gcost) <= 1e-7 * np.maximum(1.0, gcost)).all()


def test_multi_column_groups_on_a_shared_index_set(slc, gpu_ctx):
    P, S, _, _, _, _ = oc.readme_golden(slc)
    groups = [list(range(0, 20)), list(range(20, 40)), list(range(40, 59))]
    r = _run_plan(slc, gpu_ctx, P, S, groups)
    assert r["info"]["max_nx"] == 40
    _assert_parity(r, "grouped")
    g = np.load(os.path.join(GOLDEN, "grouped_chain_phi.npz"))
    gsum = np.array([r["col"][0:20].sum(), r["col"][20:40].sum(), r["col"][40:59].sum()])
    assert (np.abs(gsum - g["group_cost"]) <= 1e-7 * np.maximum(1.0, g["group_cost"])).all()


def test_ridge_term_is_part_of_the_value(slc, oracle):
    P, S, ridge = oc.chain23_variant(slc, "ridge")
    with slc.Context([0]) as ctx:                       # a context of its own: the ridge stays on the context it is set on
        ctx.set_ridge(*ridge)
        r = _run_plan(slc, ctx, P, S, ridge=ridge)
    _assert_parity(r, "ridge")
    Phix, Phiu = slc.assemble_phi(S[0], S[1], r["vx"], r["vu"], dropzeros=False)
    want = oc.reference_formula(oracle, P, S, Phix, Phiu, ridge)
    assert np.all(np.abs(r["col"] - want) <= r["bound"])
    plain = oc.reference_formula(oracle, P, S, Phix, Phiu, None)
    assert np.all(want > plain)


def test_infeasible_plant_reports_the_written_point(slc, gpu_ctx):
    g = np.load(os.path.join(GOLDEN, "infeasible_chain.npz"))
    P = slc.workloads.chain_plant(int(g["Nx"]))
    S = list(slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"])))
    r = _run_plan(slc, gpu_ctx, P, S)
    assert (r["status"] != 0).sum() == 12
    _assert_parity(r, "infeasible")


def test_attached_refinement_is_reflected(slc, monkeypatch):
    """tools/fuzz_h2.py seed 77, column 21 (tests/test_gpu_parity.py::test_resident_plan_refine_attaches_tile_pass): after
    Plan.refine the array holds the refined column, and the value is the one of that array."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, _ = ns["problem"](77)
    S = [list(S[0]), list(S[1])]
    groups = [[21], [22]]
    with slc.Context([0]) as ctx:
        before = _run_plan(slc, ctx, P, S, groups)
        after = _run_plan(slc, ctx, P, S, groups, refine=True)
    _assert_parity(before, "unrefined"); _assert_parity(after, "refined")
    moved = max(np.abs(a - b).max() for a, b in zip(before["vx"] + before["vu"], after["vx"] + after["vu"]))
    assert moved > 1e-6 and before["col"][0] != after["col"][0]


def test_layouts_shards_and_determinism(slc, gpu_ctx, readme_run):
    """A group_range shard in both layouts: packed and mask-order results are bit-equal; two shards' totals add up to the whole
    plan's within the summation bound."""
    import torch
    whole, _ = readme_run
    P, S, _, _, _, _ = oc.readme_golden(slc)
    tots = []
    for rng in ((0, 30), (30, 59)):
        plan = slc.Plan(gpu_ctx, P, S, None, group_range=rng)
        try:
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize()
            col_m, tot_m = plan.objective_values(dv)
            pk = torch.zeros(plan.info["n_packed"], dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            plan.execute(pk.data_ptr(), packed=True); plan.synchronize()
            col_p, tot_p = plan.objective_values(pk.data_ptr(), packed=True)
            assert np.array_equal(col_m, col_p) and tot_m == tot_p
            st = torch.cuda.current_stream().cuda_stream                          # the stream form, device outputs
            col_a, tot_a = plan.objective_values(pk.data_ptr(), packed=True, stream=st)
            assert np.array_equal(col_a, col_p) and tot_a == tot_p
            assert np.array_equal(col_m, whole["col"][rng[0]:rng[1]])
            tots.append(tot_m)
        finally:
            plan.close()
    assert abs(tots[0] + tots[1] - whole["tot"]) <= _total_bound(whole["bound"], whole["col"])


def test_anchors_through_the_one_shot_calls(slc, gpu_ctx):
    P, S, _, _, _, cost = oc.readme_golden(slc)
    _, _, info = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, return_objective=True)
    assert np.abs(info["col_objective"] - cost).max() < 1e-8 and abs(info["objective_total"] - 893.3262819770) < 1e-7
    _, _, info = slc.SLS_H2_localized(P, 9, 29, 1.5, ctx=gpu_ctx, return_info=True, return_objective=True)
    assert np.abs(info["col_objective"] - cost).max() < 1e-8 and abs(info["objective_total"] - 893.3262819770) < 1e-7
    _, info = slc.SLS_H2_batch([P] * 4, [S] * 4, ctx=gpu_ctx, return_info=True, return_objective=True)
    assert len(info["col_objective"]) == 4 and all(np.abs(c - cost).max() < 1e-8 for c in info["col_objective"])
    assert abs(info["objective_total"] - 4 * 893.3262819770) < 4e-7
    # option off: nothing new in info
    _, _, info0 = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True)
    assert "col_objective" not in info0 and "objective_total" not in info0
    assert set(info0) == set(slc._capi.sls_stats().asdict()) | {"col_status", "n_unsolved"}


def test_sum_of_norms_against_the_oracle(slc, gpu_ctx, oracle):
    """The 23-state chain of tests/test_sum_of_norms.py, three of its columns: within 1e-7 relative of the certified oracle's
    primal objective, through the plan and through SLS_Hinf_bound."""
    import sls_son_oracle as son
    P = slc.workloads.chain_plant(23)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 6, 18, 1.5))
    cols = [0, 11, 22]
    _, _, dg = son.SLS_SON(oracle.OraclePlant(P.A, P.B1, P.B2), S, cols=cols)
    want = np.array([d["obj"] for d in dg])
    r = _run_plan(slc, gpu_ctx, P, S, [[c] for c in cols], objective="sum_of_norms")
    assert np.all(r["status"] == 0)
    assert np.all(np.abs(r["col"] - want) <= 1e-7 * want)
    # same Φ, two summation orders: every step's norm is the root of a sum of at most 64 products (relative error ≤ 66·2⁻⁵³/2 + 2⁻⁵³),
    # the T = 18 norms are then added — per side below (64 + 18 + 4)·2⁻⁵³ of the (all-positive) value
    assert np.all(np.abs(r["col"] - r["hcol"]) <= 2 * (64 + 18 + 4) * oc.U * r["hcol"])
    _, _, info = slc.SLS_Hinf_bound(P, S, [[c] for c in cols], ctx=gpu_ctx, return_info=True, return_objective=True)
    assert np.all(np.abs(info["col_objective"] - want) <= 1e-7 * want)
    assert abs(info["objective_total"] - want.sum()) <= 1e-7 * want.sum()


def test_context_contract(slc):
    P, S, _, _, _, _ = oc.readme_golden(slc)
    C = slc._capi
    with slc.Context([0]) as ctx:
        with pytest.raises(slc.SLSError) as ei:                                  # before any opted-in solve
            ctx.last_objective(P.Nx)
        assert ei.value.code == C.SLS_EINVAL
        slc.SLS_H2(P, S, ctx=ctx)                                                # option off: still nothing to report
        with pytest.raises(slc.SLSError) as ei:
            ctx.last_objective(P.Nx)
        assert ei.value.code == C.SLS_EINVAL
        ctx.want_objective(True)
        slc.SLS_H2(P, S, [[5], [40]], ctx=ctx)
        col, tot = ctx.last_objective(2)
        assert col.shape == (2,) and abs(col.sum() - tot) < 1e-12
        with pytest.raises(slc.SLSError) as ei:                                  # wrong n
            ctx.last_objective(3)
        assert ei.value.code == C.SLS_EINVAL
        slc.SLS_H2(P, S, [[5], [5, 6]], ctx=ctx)                                 # column 5 in two groups: a sum of layers
        with pytest.raises(slc.SLSError) as ei:
            ctx.last_objective(3)
        assert ei.value.code == C.SLS_EUNSUPPORTED
        with pytest.raises(slc.SLSError) as ei:
            slc.SLS_H2(P, S, [[5], [5, 6]], ctx=ctx, return_info=True, return_objective=True)
        assert ei.value.code == C.SLS_EUNSUPPORTED


def test_column_sharded_objective_on_one_rank(slc, readme_run):
    whole, _ = readme_run
    P, S, _, _, _, _ = oc.readme_golden(slc)
    sh = slc.dist.ColumnShardedH2(P, S, None, device="cuda:0")
    try:
        sh.step()
        col, tot = sh.objective_values()
        assert np.array_equal(col, whole["col"]) and tot == whole["tot"]
        sh._direct = lambda: False                                               # the packed buffer + unpack route of N > 1
        sh.step()
        col, tot = sh.objective_values()
        assert np.array_equal(col, whole["col"]) and tot == whole["tot"]
    finally:
        sh.local.plan.close(); sh.ctx.close()
