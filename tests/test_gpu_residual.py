"""Achievability residual of every column against the full plant, evaluated on the device from Φ (csrc/sls_residual.hip) —
against the host twin (csrc/sls_residual.cpp, itself held to a NumPy statement by tests/test_residual_host.py) fed the SAME Φ and
the SAME plant values.

The bound is derived, not measured: device and twin evaluate the same sums in two orders and precisions, so per column
|Δ| ≤ 2·N·2⁻⁵³·S (objective_cases.summation_bound) with the N and S the twin reports — the largest term count / absolute sum of one
entry of Δ for res_inf and halo_inf, those of the whole column for res_l1.  halo_inf of a column without halo rows is exactly 0.0.
`-s` prints the worst |Δ|/bound of every case."""
import ctypes

import numpy as np
import pytest

import objective_cases as oc
import residual_cases as rc

pytestmark = pytest.mark.gpu

CERT = 1e-9            # the suite's certificate level of a solve (tests/test_gpu_fullsize.py, tests/son_cases.py)


def _assert_twin(slc, r, P, S, I, vx, vu, tag):
    """device record `r` against the twin on (P, Φ = vx, vu); returns the twin's record and halo lists"""
    h, b, halo = slc.residual_host(P, S, vx, vu, I, return_bound=True, return_halo=True)
    eb = oc.summation_bound(b["ent_terms"], b["ent_abs"])
    lb = oc.summation_bound(b["l1_terms"], b["l1_abs"])
    worst = [float((np.abs(x - y) / np.maximum(bd, 1e-300)).max()) for x, y, bd in
             ((r.res_inf, h.res_inf, eb), (r.halo_inf, h.halo_inf, eb), (r.res_l1, h.res_l1, lb))]
    print(tag, "worst |Δ|/bound: res_inf %.3g halo_inf %.3g res_l1 %.3g" % tuple(worst), "| max_inf", r.max_inf, "E1", r.e1_norm)
    assert r.res_inf.shape == h.res_inf.shape == r.halo_inf.shape == r.res_l1.shape
    assert np.all(np.isfinite(r.res_l1))
    assert np.all(np.abs(r.res_inf - h.res_inf) <= eb), (tag, np.flatnonzero(np.abs(r.res_inf - h.res_inf) > eb))
    assert np.all(np.abs(r.halo_inf - h.halo_inf) <= eb), (tag, np.flatnonzero(np.abs(r.halo_inf - h.halo_inf) > eb))
    assert np.all(np.abs(r.res_l1 - h.res_l1) <= lb), (tag, np.flatnonzero(np.abs(r.res_l1 - h.res_l1) > lb))
    empty = np.array([x.size == 0 for x in halo])
    assert np.all(r.halo_inf[empty] == 0.0) and not np.any(np.signbit(r.halo_inf[empty]))
    assert r.max_inf == r.res_inf.max() and r.e1_norm == r.res_l1.max()                 # the totals ARE the maxima of the arrays
    return h, halo


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def _solve_and_check(slc, ctx, P, S, I=None, objective="h2", tag=""):
    """execute → device residual (twice: same bits) + download → twin on the downloaded Φ"""
    plan = slc.Plan(ctx, P, S, I, objective=objective)
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        r = plan.residual(dv)
        assert _same_bits(r, plan.residual(dv))
        vx, vu = plan.download(dv)
        status = plan.fetch_status()[0]
    finally:
        plan.close()
    h, halo = _assert_twin(slc, r, P, S, I, vx, vu, tag)
    return r, h, halo, status


@pytest.fixture(scope="module")
def readme_run(slc, gpu_ctx):
    P, S, _, _, _ = rc.golden_case(slc, "readme")
    return _solve_and_check(slc, gpu_ctx, P, S, tag="readme")


def test_readme_chain_certificate_layouts_and_determinism(slc, gpu_ctx, readme_run):
    """59 columns.  By pattern every column has halo rows, but the masks keep Φ off the outermost rows of s_x: halo_inf is exactly
    0.0; res_inf sits at the certificate level; mask-order, packed, the stream form and the golden Φ uploaded as it is."""
    import torch
    r, h, halo, status = readme_run
    assert np.all(status == 0) and len(r.res_inf) == 59
    assert np.all(r.halo_inf == 0.0) and r.max_inf <= CERT and np.all(r.res_inf <= CERT)
    P, S, _, gx, gu = rc.golden_case(slc, "readme")
    plan = slc.Plan(gpu_ctx, P, S)
    try:
        pk = torch.zeros(plan.info["n_packed"], dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        plan.execute(pk.data_ptr(), packed=True); plan.synchronize()
        rp = plan.residual(pk.data_ptr(), packed=True)
        assert _same_bits(rp, r)                                                       # packed ≡ mask order, plan to plan
        st = torch.cuda.current_stream().cuda_stream                                   # the stream form, device outputs
        assert _same_bits(plan.residual(pk.data_ptr(), packed=True, stream=st), r)
        # no execute needed: the golden Φ, uploaded in mask order, against the twin on the same numbers
        dv = torch.from_numpy(np.concatenate(gx + gu)).to("cuda:0")
        torch.cuda.synchronize()
        rg = plan.residual(dv.data_ptr())
        _assert_twin(slc, rg, P, S, None, gx, gu, "readme golden Φ")
        assert rg.max_inf <= CERT
    finally:
        plan.close()


def test_halo_rows_show_what_the_status_cannot(slc, gpu_ctx):
    """12-state chain, T = 4, last mask narrower than the earlier ones and an actuator with a far second entry: columns that
    report SLS_COL_OK and are no closed-loop map (tests/test_residual_host.py asserts the same of the oracle's Φ)."""
    P, S, I = rc.oracle_case(slc, "halo")
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, tag="halo")
    assert any(x.size for x in halo)
    assert ((status == 0) & (r.halo_inf > 1e-3)).any()


@pytest.mark.parametrize("name", ["grid9", "grid12"])
def test_rows_beyond_one_lane_stride(slc, gpu_ctx, name):
    """ñx + |H| on both sides of 64 (9×9 grid, 64 included) and of 128 (12×12 grid, 128 included)"""
    P, S, I = rc.oracle_case(slc, name)
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, tag=name)
    n = np.array([len(x) for x in slc_index_sets(slc, P, S)]) + np.array([x.size for x in halo])
    edge = 64 if name == "grid9" else 128
    assert n.min() < edge < n.max() and edge in n


def slc_index_sets(slc, P, S):
    import sls_oracle as o
    Po = o.OraclePlant(P.A, P.B1, P.B2)
    return [o.sparsity_dim_reduction(Po, [c], S)[3] for c in range(P.Nx)]


@pytest.mark.parametrize("name", ["T1", "T2", "whole"])
def test_short_horizons_and_empty_halos(slc, gpu_ctx, name):
    """T = 1: no propagation step between Δ[0] and Δ[T]; T = 2: one.  `whole`: index sets that are the whole plant — every H(q)
    empty, halo_inf exactly 0.0."""
    P, S, I = rc.oracle_case(slc, name)
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, tag=name)
    if name == "whole":
        assert all(x.size == 0 for x in halo) and np.all(r.halo_inf == 0.0)


def test_rows_longer_than_the_register_cache(slc, gpu_ctx):
    """rows of A and B2 with more than the eight entries a lane keeps in registers: A alone past eight, A and B2 together past
    eight, exactly eight and one (tests/residual_cases.py: dense_rows) — the rest of such a row is searched again at every step"""
    P, S, I = rc.oracle_case(slc, "dense_rows")
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, tag="dense_rows")
    assert np.diff(P.A.tocsr().indptr).max() == 16 and np.diff(P.B2.tocsr().indptr).max() == 12


def test_infeasible_columns_report_the_written_point(slc, gpu_ctx):
    """tests/golden/infeasible_chain.npz: the least-squares points of the 12 infeasible columns, above the acceptance level"""
    import torch
    P, S, _, gx, gu = rc.golden_case(slc, "infeasible")
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, tag="infeasible")
    bad = status != 0
    assert bad.sum() == 12 and np.all(r.res_inf[bad] > CERT) and np.all(r.res_inf[~bad] <= CERT)
    assert r.max_inf == r.res_inf[bad].max()
    plan = slc.Plan(gpu_ctx, P, S)
    try:
        dv = torch.from_numpy(np.concatenate(gx + gu)).to("cuda:0")
        torch.cuda.synchronize()
        rg = plan.residual(dv.data_ptr())
    finally:
        plan.close()
    hg, _ = _assert_twin(slc, rg, P, S, None, gx, gu, "infeasible golden Φ")
    assert np.all(hg.res_inf[bad] > CERT)


def test_stale_phi_after_a_plant_update(slc, gpu_ctx):
    """execute → update_plant (A perturbed on three entries) → residual WITHOUT a re-solve: the twin's value on (new plant, old Φ);
    the re-solve restores the certificate; with tracking on, execute_dirty does too."""
    P, S, _, _, _ = rc.golden_case(slc, "readme")
    A2 = rc.perturbed_A(P)
    P2 = slc.Plant(A2, P.B1, P.B2)
    plan = slc.Plan(gpu_ctx, P, S)
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        vx, vu = plan.download(dv)
        assert plan.residual(dv).max_inf <= CERT
        plan.update_plant(A=A2)
        stale = plan.residual(dv)                              # waits for the update, reads the operator it wrote
        _assert_twin(slc, stale, P2, S, None, vx, vu, "stale Φ, new plant")
        assert stale.max_inf > 1e-6
        plan.execute(dv); plan.synchronize()
        fresh = plan.residual(dv)
        vx2, vu2 = plan.download(dv)
        _assert_twin(slc, fresh, P2, S, None, vx2, vu2, "re-solved")
        assert fresh.max_inf <= CERT
        # back to the first plant with tracking on: stale again, then only the marked columns are solved
        plan.track_changes(True)
        plan.update_plant(A=sp_sorted(P.A))
        stale2 = plan.residual(dv)
        _assert_twin(slc, stale2, P, S, None, vx2, vu2, "stale Φ, first plant")
        assert stale2.max_inf > 1e-6
        n = plan.execute_dirty(dv); plan.synchronize()
        assert 0 < n < 59
        assert plan.residual(dv).max_inf <= CERT
    finally:
        plan.close()


def sp_sorted(A):
    import scipy.sparse as sp
    A = sp.csc_matrix(A, dtype=np.float64).copy(); A.sort_indices()
    return A


@pytest.mark.parametrize("name", ["weighted", "general", "coupled_dense", "coupled_diag", "grouped"])
def test_weighted_dense_and_group_plans_report_per_column(slc, gpu_ctx, name):
    """diagonal weights, a dense Hessian, coupled groups (non-diagonal B1 block) and multi-column groups on a shared index set:
    the constraints are the same, every column of every group carries its own three numbers"""
    P, S, I, gx, gu = rc.golden_case(slc, name)
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, I, tag=name)
    assert len(r.res_inf) == P.Nx
    ok = status == 0
    assert ok.any() and np.all(r.res_inf[ok] <= CERT)
    if I is not None:
        assert max(len(g) for g in I) > 1 and len(np.unique(r.res_l1)) > len(I)         # members differ: not one value per group


def test_sum_of_norms_plan(slc, gpu_ctx):
    P = slc.workloads.chain_plant(23)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 6, 18, 1.5))
    r, h, halo, status = _solve_and_check(slc, gpu_ctx, P, S, [[0], [11], [22]], objective="sum_of_norms", tag="sum of norms")
    assert np.all(status == 0) and len(r.res_inf) == 3 and r.max_inf <= CERT


def test_attached_refinement_is_read_like_any_other_write(slc, monkeypatch):
    """tools/fuzz_h2.py seed 77, column 21 (tests/test_gpu_objective.py::test_attached_refinement_is_reflected): the pass reads what
    was written last — the refined column after Plan.refine, and again after a later execute, which runs the attached pass."""
    import os
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, _ = ns["problem"](77)
    S = [list(S[0]), list(S[1])]
    groups = [[21], [22]]
    runs = []
    with slc.Context([0]) as ctx:
        plan = slc.Plan(ctx, P, S, groups)
        try:
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize()
            runs.append((plan.residual(dv), plan.download(dv)))
            assert plan.refine(dv) >= 1
            runs.append((plan.residual(dv), plan.download(dv)))
            plan.execute(dv); plan.synchronize()
            runs.append((plan.residual(dv), plan.download(dv)))
        finally:
            plan.close()
    for tag, (r, (vx, vu)) in zip(("unrefined", "refined", "refined, next execute"), runs):
        _assert_twin(slc, r, P, S, groups, vx, vu, tag)
    moved = max(np.abs(a - b).max() for a, b in zip(runs[0][1][0] + runs[0][1][1], runs[1][1][0] + runs[1][1][1]))
    assert moved > 1e-6 and runs[0][0].res_l1[0] != runs[1][0].res_l1[0]


def test_shard_plans_and_column_sharded_on_one_rank(slc, readme_run):
    whole = readme_run[0]
    P, S, _, _, _ = rc.golden_case(slc, "readme")
    with slc.Context([0]) as ctx:
        for rng in ((0, 30), (30, 59)):
            plan = slc.Plan(ctx, P, S, None, group_range=rng)
            try:
                dv = plan.alloc_values()
                plan.execute(dv); plan.synchronize()
                r = plan.residual(dv)
            finally:
                plan.close()
            assert len(r.res_inf) == rng[1] - rng[0]                                   # its own subproblems only
            assert all(np.array_equal(x, y[rng[0]:rng[1]]) for x, y in zip(r[:3], whole[:3]))
            assert r.max_inf == whole.res_inf[rng[0]:rng[1]].max() and r.e1_norm == whole.res_l1[rng[0]:rng[1]].max()
    sh = slc.dist.ColumnShardedH2(P, S, None, device="cuda:0")
    try:
        sh.step()
        assert _same_bits(sh.residual(), whole)
        sh._direct = lambda: False                                                     # the packed buffer + unpack route of N > 1
        sh.step()
        assert _same_bits(sh.residual(), whole)
    finally:
        sh.local.plan.close(); sh.ctx.close()


def test_contract_null_values_and_localized_plans(slc, readme_run):
    import torch
    whole = readme_run[0]
    P, S, _, _, _ = rc.golden_case(slc, "readme")
    with slc.Context([0]) as ctx:
        plan = slc.Plan(ctx, P, S)
        try:
            with pytest.raises(slc.SLSError) as ei:
                plan.residual(None)
            assert ei.value.code == slc._capi.SLS_EINVAL
            with pytest.raises(slc.SLSError) as ei:
                plan.residual_async(None, stream=torch.cuda.current_stream().cuda_stream)
            assert ei.value.code == slc._capi.SLS_EINVAL
            ws = plan.info["workspace_bytes"]
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize()
            plan.residual(dv)
            info = slc._capi.sls_plan_info()
            slc._capi.check(plan._lib.sls_plan_get_info(plan.handle, ctypes.byref(info)))
            assert info.workspace_bytes == ws                                          # the halo buffers are the feature's own
        finally:
            plan.close()
    with slc.Context([0]) as ctx:
        # device-resident symbolic route: its tables never were on the host, the residual reads them where they are
        plan = slc.Plan.localized(ctx, P, 9, len(S[0]), 1.5)
        try:
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize()
            r = plan.residual(dv)
            vx, vu = plan.download(dv)
        finally:
            plan.close()
    _assert_twin(slc, r, P, S, None, vx, vu, "localized")
    assert r.max_inf <= CERT and np.all(r.halo_inf == 0.0) and len(r.res_inf) == len(whole.res_inf)
