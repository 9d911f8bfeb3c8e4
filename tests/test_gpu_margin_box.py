"""GPU tests of the worst-case 𝓛₁ margin over a box of plants (csrc/sls_margin_box.hip behind sls_margin_set_radius /
sls_margin_box_*): one wave per (row, scenario) parks d⁰ and the factors of the row's active coefficients in LDS once per entry
and sums every vertex in the one order of sls_margin_run; rows with more than 10 active coefficients report the triangle bound.

References.  (1) The library's host twin (margin_box_host): the same tables and active lists, every vertex in long double —
every device row within the twin's own derived bound 2·N·2⁻⁵³·S (test_margin_box_host.py holds the twin to a brute force over
dense long-double matrices within the same bound).  (2) Bit equality wherever the contract promises it: all radii zero against
sls_margin_run, scenario s against an object of its own, run against run.  (3) The object's own sampled margins() on
worst_plant().  (4) On the README chain solved on the device: the verdicts at ε = 0.013 and ε = 0.02, and a Rollout on the worst
plant against the gain bound — an inequality.

Values are compared, never arg-max codes: near-ties may resolve differently.  (The tests print each figure before they assert:
run with -s.)"""
import numpy as np
import pytest
import scipy.sparse as sp

import margin_box_cases as bc
import margin_cases as mc
import rollout_cases as rc

pytestmark = pytest.mark.gpu
L = np.longdouble
NSCEN = (1, 3, 8, 9, 65)


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(_dev())        # a copy: fixtures are read-only


def _plant(slc, case):
    return slc.Plant(case.A, case.B1, case.B2)


def _margin(slc, ctx, case, nscen, values=None):
    mg = slc.RobustMargin(ctx, _plant(slc, case), [case.Sx, case.Su], nscen=nscen)
    mg._keep = _to_dev(case.values if values is None else values)
    mg.load(mg._keep)
    return mg


@pytest.fixture(scope="module")
def cases():
    return {name: bc.case(name) for name in bc.ALL}


@pytest.fixture(scope="module")
def inputs(cases):
    """centres and radii of every case at the largest nscen; column s does not depend on nscen"""
    out = {}
    for name, case in cases.items():
        arrs = bc.perturbed(case, max(NSCEN)) + bc.radii(name, case, max(NSCEN))
        for a in arrs:
            a.setflags(write=False)
        out[name] = arrs
    return out


def _cut(arrs, n):
    return tuple(np.ascontiguousarray(a[:, :n]) for a in arrs)


def _twin(slc, case, nscen, Av, Bv, Ar, Br, values=None):
    return slc.margin_box_host(_plant(slc, case), [case.Sx, case.Su], case.values if values is None else values, nscen, A=Av, B2=Bv,
                               per_scenario=True, A_rad=Ar, B2_rad=Br, rad_per_scenario=True)


def _boxed(slc, ctx, case, nscen, Av, Bv, Ar, Br):
    mg = _margin(slc, ctx, case, nscen)
    mg.set_plant(Av, Bv, per_scenario=True)
    mg.set_radius(Ar, Br, per_scenario=True)
    return mg


# ------------------------------------------------------------------ 1. every case against the twin

@pytest.mark.parametrize("nscen", NSCEN)
@pytest.mark.parametrize("name", bc.ALL)
def test_device_against_the_twin(slc, gpu_ctx, cases, inputs, name, nscen):
    """Per-scenario perturbed centres and radii; 8 and 9 scenarios sit on both sides of a chunk of the totals pass, 65 is a ninth
    chunk.  `wide` has a row of 1 024 vertices (16 passes), a row on the bound path and rows of 1, 2, 4, 8, 16, 32 vertices."""
    case = cases[name]
    Av, Bv, Ar, Br = _cut(inputs[name], nscen)
    tw = _twin(slc, case, nscen, Av, Bv, Ar, Br)
    mg = _boxed(slc, gpu_ctx, case, nscen, Av, Bv, Ar, Br)
    got = mg.box_margins()
    worst = bc.check_rows(got["row_wc"], tw, f"{name} nscen {nscen}")
    print(name, nscen, "largest error / bound", f"{worst:.3f}", "bits", mg.box_max_bits, "bound rows", mg.box_inexact_rows)
    assert np.array_equal(got["exact"], tw["exact"]) and np.array_equal(got["vertex"] < 0, ~tw["exact"][:, None] & np.ones((1, nscen), bool))
    assert np.array_equal(got["l1_wc"], got["row_wc"].max(axis=0))
    bits = np.diff(tw["act_ptr"])
    assert ((got["vertex"] < (1 << np.minimum(bits, 10))[:, None]) | ~tw["exact"][:, None]).all()
    assert mg.box_max_bits == bits.max() and mg.box_inexact_rows == int((~tw["exact"]).sum())
    assert mg.box_vertex_sums == int((1 << bits[tw["exact"]]).sum()) and mg.box_device_bytes > 0
    assert not got["row_wc"][tw["row_n"] == 0].any()
    if name == "wide":
        assert not got["row_wc"][bc.WIDE_EMPTY_ROW].any() and mg.box_inexact_rows == 1 and mg.box_max_bits == 11
    mg.close()


# ------------------------------------------------------------------ 2. what must be equal bit for bit

@pytest.mark.parametrize("name", ["ladder", "edges", "wide"])
def test_all_radii_zero_is_the_sampled_margin(slc, gpu_ctx, cases, inputs, name):
    case = cases[name]
    nscen = 3
    Av, Bv, Ar, Br = _cut(inputs[name], nscen)
    mg = _margin(slc, gpu_ctx, case, nscen)
    mg.set_plant(Av, Bv, per_scenario=True)
    m = mg.margins()
    for kw in (dict(), dict(A=np.zeros_like(Ar), B2=np.zeros_like(Br), per_scenario=True), dict(relative=0.0)):
        mg.set_radius(**kw)
        got = mg.box_margins()
        assert np.array_equal(got["row_wc"], m["row_l1"]) and np.array_equal(got["l1_wc"], m["l1"]), kw
        assert not got["vertex"].any() and got["exact"].all() and mg.box_max_bits == 0
    assert float(m["l1"].max()) > 0.05
    A, B = mg.worst_plant()
    assert np.array_equal(A, Av) and np.array_equal(B, Bv)
    assert all(np.array_equal(mg.margins()[k], m[k]) for k in m)      # the sampled pass is untouched
    mg.close()


@pytest.mark.parametrize("name", ["edges", "wide"])
def test_a_scenario_equals_an_object_of_its_own(slc, gpu_ctx, cases, inputs, name):
    """Values only: the codes depend on which scenarios made a coefficient active (rows 10 and 11 of `wide`)."""
    case = cases[name]
    full = {}
    for nscen in (9, 65):
        mg = _boxed(slc, gpu_ctx, case, nscen, *_cut(inputs[name], nscen))
        full[nscen] = mg.box_margins()
        mg.close()
    Av, Bv, Ar, Br = inputs[name]
    one = _margin(slc, gpu_ctx, case, 1)
    for s in (0, 1, 4, 8, 64):
        one.set_plant(Av[:, s], Bv[:, s])
        one.set_radius(Ar[:, s], Br[:, s])
        m = one.box_margins()
        for nscen in (9, 65):
            if s < nscen:
                assert np.array_equal(full[nscen]["row_wc"][:, s], m["row_wc"][:, 0]), (name, nscen, s)
                assert full[nscen]["l1_wc"][s] == m["l1_wc"][0]
    one.close()


def test_two_runs_and_the_device_outputs(slc, gpu_ctx, cases, inputs):
    import torch
    case = cases["wide"]
    nscen = 9
    mg = _boxed(slc, gpu_ctx, case, nscen, *_cut(inputs["wide"], nscen))
    a, b = mg.box_margins(), mg.box_margins()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    row = torch.full((case.Nx, nscen), float("nan"), dtype=torch.float64, device=_dev())
    ver = torch.full((case.Nx, nscen), -7, dtype=torch.int64, device=_dev())
    tot = torch.full((nscen,), float("nan"), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    mg.box_run_async(row, ver, tot)
    mg.box_run_async(None, None, None)
    torch.cuda.synchronize()
    assert np.array_equal(row.cpu().numpy(), a["row_wc"]) and np.array_equal(ver.cpu().numpy(), a["vertex"])
    assert np.array_equal(tot.cpu().numpy(), a["l1_wc"])
    assert np.array_equal(mg.box_certified(), a["l1_wc"] < 1)
    gb = mg.box_gain_bound()
    assert np.array_equal(np.isinf(gb), a["l1_wc"] >= 1) and (gb[a["l1_wc"] < 1] >= 1).all()
    mg.close()


# ------------------------------------------------------------------ 3. the worst plant through the sampled margin

@pytest.mark.parametrize("name", ["ladder", "T5", "edges", "wide"])
def test_worst_plant_through_the_sampled_margin(slc, gpu_ctx, cases, inputs, name):
    """margins() on worst_plant() gives row_wc back on the exact rows and stays below it on the bound rows.  Room: the derived
    bound of the box twin, that of the sampled twin on the same plant, and the rounding of centre ± radius — one ulp of each
    coefficient, at most 2⁻⁵³·S of the sampled twin."""
    case = cases[name]
    nscen = 5
    Av, Bv, Ar, Br = _cut(inputs[name], nscen)
    mg = _boxed(slc, gpu_ctx, case, nscen, Av, Bv, Ar, Br)
    box = mg.box_margins()
    Aw, Bw = mg.worst_plant()
    for W, V, R in ((Aw, Av, Ar), (Bw, Bv, Br)):                  # inside the box, up to the rounding of centre ± radius
        assert (np.abs(W - V) <= R + 2.0 ** -52 * (np.abs(V) + R)).all()
    mg.set_plant(Aw, Bw, per_scenario=True)
    m = mg.margins()
    tw = _twin(slc, case, nscen, Av, Bv, Ar, Br)
    th = slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, nscen, A=Aw, B2=Bw, per_scenario=True)
    room = mc.bound(tw["row_n"][:, None], tw["row_s"]) + mc.bound(th["row_n"][:, None], th["row_s"]) + L(2.0) ** -53 * th["row_s"].astype(L)
    gap = m["row_l1"].astype(L) - box["row_wc"].astype(L)
    ex = box["exact"]
    print(name, "largest |gap| / room on exact rows", float(np.max(np.abs(gap[ex]) / np.maximum(room[ex], L(1e-300)))))
    assert (np.abs(gap[ex]) <= room[ex]).all() and (gap[~ex] <= room[~ex]).all()
    mg.set_plant(Av, Bv, per_scenario=True)
    centre = mg.margins()
    assert (centre["row_l1"].astype(L) <= box["row_wc"].astype(L) + room).all()      # the centre is the mean of σ and −σ
    mg.close()


# ------------------------------------------------------------------ 4. NaN

def test_a_nan_in_one_centre_value_of_one_scenario(slc, gpu_ctx, cases, inputs):
    case = cases["edges"]
    nscen = 6
    Av, Bv, Ar, Br = _cut(inputs["edges"], nscen)
    mg = _boxed(slc, gpu_ctx, case, nscen, Av, Bv, Ar, Br)
    clean = mg.box_margins()
    Acsc = sp.csc_matrix(case.A); Acsc.sort_indices()
    nz = Acsc.nnz // 2
    i = int(Acsc.indices[nz])
    bad = Av.copy(); bad[nz, 3] = np.nan
    mg.set_plant(A=bad, per_scenario=True)
    got = mg.box_margins()
    hit = np.zeros((case.Nx, nscen), dtype=bool); hit[i, 3] = True
    assert np.isposinf(got["row_wc"][hit]).all() and np.array_equal(got["row_wc"][~hit], clean["row_wc"][~hit])
    assert np.isposinf(got["l1_wc"][3]) and np.array_equal(np.delete(got["l1_wc"], 3), np.delete(clean["l1_wc"], 3))
    assert not mg.box_certified()[3] and np.isinf(mg.box_gain_bound()[3])
    mg.close()


@pytest.mark.parametrize("name", ["edges", "wide"])
def test_a_nan_in_one_read_phi_value(slc, gpu_ctx, cases, inputs, name):
    """+inf in the rows margin_cases.reach_of_phi names (the row of the start value and every row with a stored A[i, r]), the rest
    bitwise unchanged; on `wide` the reach holds exact rows and may hold the bound row."""
    case = cases[name]
    nscen = 3
    mg = _boxed(slc, gpu_ctx, case, nscen, *_cut(inputs[name], nscen))
    clean = mg.box_margins()
    t, r, c = mc.phi_probe(case)
    vals = case.values.copy(); vals[mc.value_index(case, "x", t, r, c)] = np.nan
    bad = _to_dev(vals)
    mg.load(bad)
    got = mg.box_margins()
    rows, _ = mc.reach_of_phi(case, "x", t, r, c)
    assert rows.sum() >= 2 and not rows.all()
    assert np.isposinf(got["row_wc"][rows]).all() and np.array_equal(got["row_wc"][~rows], clean["row_wc"][~rows])
    assert np.isposinf(got["l1_wc"]).all()
    mg.close()


# ------------------------------------------------------------------ 5. errors

def test_error_paths_leave_the_object_usable(slc, gpu_ctx, cases, inputs):
    case = cases["T2"]
    nscen = 3
    EINVAL = slc._capi.SLS_EINVAL
    Av, Bv, Ar, Br = _cut(inputs["T2"], nscen)
    mg = slc.RobustMargin(gpu_ctx, _plant(slc, case), [case.Sx, case.Su], nscen=nscen)
    mg.set_plant(Av, Bv, per_scenario=True)

    def refused(call):
        with pytest.raises(slc.SLSError) as e:
            call()
        assert e.value.code == EINVAL

    refused(lambda: mg.box_margins())                            # before the first load and the first set_radius
    d = _to_dev(case.values)
    mg.load(d)
    for call in (lambda: mg.box_margins(), lambda: mg.box_run_async(), lambda: mg.worst_plant()):   # loaded, still no radii
        refused(call)
    mg.set_radius(Ar, Br, per_scenario=True)
    want = mg.box_margins()
    for bad in (-1e-300, -1.0, np.inf, -np.inf, np.nan):
        x = Ar.copy(); x[1, 2] = bad
        refused(lambda: mg.set_radius(x, Br, per_scenario=True))
        y = Br[:, 0].copy(); y[0] = bad
        refused(lambda: mg.set_radius(None, y))
        got = mg.box_margins()                                    # the object is unchanged
        assert all(np.array_equal(got[k], want[k]) for k in want), bad
    with pytest.raises(ValueError):
        mg.set_radius(A=np.zeros(2))
    with pytest.raises(ValueError):
        mg.set_radius(A=Ar, relative=0.1)
    bc.check_rows(want["row_wc"], _twin(slc, case, nscen, Av, Bv, Ar, Br), "after the refusals")
    mg.set_radius(relative=0.05)                                  # ε·|centre| of every scenario
    rel = mg.box_margins()
    tw = _twin(slc, case, nscen, Av, Bv, 0.05 * np.abs(Av), 0.05 * np.abs(Bv))
    bc.check_rows(rel["row_wc"], tw, "relative")
    mg.close(); mg.close()


# ------------------------------------------------------------------ 6. the README chain through a Plan

@pytest.fixture(scope="module")
def solved_readme(slc, gpu_ctx, readme):
    P, S, _ = readme
    plan = slc.Plan(gpu_ctx, P, S)
    d = plan.alloc_values()
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == 0)
    yield P, S, plan, d
    plan.close()


def test_readme_box_certificate_worst_plant_and_rollout(slc, gpu_ctx, solved_readme):
    """ε·|a⁰| round the design plant.  ε = 0.013: certified by the exact number (0.946 on the oracle's Φ) where the triangle bound
    is not (1.034); ε = 0.02: not certified (1.455).  Then 200 steps on the worst plant of ε = 0.013 with |w| ≤ 1 stay below
    ‖Φx‖_𝓛₁ · 1/(1 − l1_wc)."""
    import torch
    P, S, plan, d = solved_readme
    mg = slc.RobustMargin(gpu_ctx, P, S, nscen=1)
    mg.load(d)
    out = {}
    for eps in (0.013, 0.02):
        mg.set_radius(relative=eps)
        out[eps] = mg.box_margins()
        print("ε", eps, "worst ‖D‖_𝓛₁ over the box", out[eps]["l1_wc"], "bits", mg.box_max_bits, "vertex sums", mg.box_vertex_sums,
              "certified", mg.box_certified(), "gain bound", mg.box_gain_bound())
        assert out[eps]["exact"].all() and mg.box_max_bits <= 4
    assert out[0.013]["l1_wc"][0] < 1 and out[0.02]["l1_wc"][0] >= 1
    mg.set_radius(relative=0.02)
    assert not mg.box_certified()[0] and np.isinf(mg.box_gain_bound()[0])
    mg.set_radius(relative=0.013)
    assert mg.box_certified()[0]
    gain = mg.box_gain_bound()[0]
    Aw, Bw = mg.worst_plant()
    a0, b0 = rc.csc_values(P.A), rc.csc_values(P.B2)
    assert (np.abs(np.abs(Aw[:, 0] - a0) - 0.013 * np.abs(a0)) <= 2.0 ** -50 * np.abs(a0)).all()      # every coefficient at a vertex
    assert (np.abs(np.abs(Bw[:, 0] - b0) - 0.013 * np.abs(b0)) <= 2.0 ** -50 * np.abs(b0)).all()
    mg.set_plant(Aw, Bw, per_scenario=True)
    m = mg.margins()
    vx, vu = plan.download(d)
    values = np.concatenate(vx + vu)
    tw = slc.margin_box_host(P, S, values, 1, A_rad=0.013 * np.abs(a0), B2_rad=0.013 * np.abs(b0))
    th = slc.margin_host(P, S, values, 1, A=Aw, B2=Bw, per_scenario=True)
    bc.check_rows(out[0.013]["row_wc"], tw, "README ε = 0.013")
    room = mc.bound(tw["row_n"][:, None], tw["row_s"]) + mc.bound(th["row_n"][:, None], th["row_s"]) + L(2.0) ** -53 * th["row_s"].astype(L)
    gap = np.abs(m["row_l1"].astype(L) - out[0.013]["row_wc"].astype(L))
    print("sampled margin of the worst plant", m["l1"], "box", out[0.013]["l1_wc"], "largest gap", float(gap.max()), "room", float(room.min()))
    assert (gap <= room).all()
    assert (abs(sp.csc_matrix(P.B1) - sp.identity(P.Nx)) > 0).nnz == 0          # w̃ = B₁·w = w, so |w̃| ≤ 1
    nrm = slc.ClosedLoopNorms((P.Nx, P.Nu), S, ctx=gpu_ctx).load(d)
    row, _, _ = nrm.l1()
    phix_l1 = row[: P.Nx].max()
    steps = 200
    w = np.random.default_rng(5).uniform(-1.0, 1.0, (steps, P.Nw, 1))
    ro = slc.Rollout(gpu_ctx, P, S, nscen=1)
    ro.load(d)
    ro.set_plant(Aw, Bw, per_scenario=True)
    d_w = _to_dev(w)
    ro.run(steps, w=d_w)
    torch.cuda.synchronize()
    _, peak_x, _ = ro.stats()
    print("peak_x", peak_x, "bound", phix_l1 * gain)
    assert (peak_x > 0).all() and (peak_x <= phix_l1 * gain).all()
    ro.close(); nrm.close(); mg.close()
