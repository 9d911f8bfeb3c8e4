"""GPU tests of the robust-stability margins (csrc/sls_margin.hip, sls_margin_*): |D⁽ˢ⁾| of every pattern entry by a pass that is
flat over (entry, scenario) in the rollout's seven lane layouts, then the row and column sums in one fixed order and the two
maxima per scenario.

References.  (1) The library's host twin (margin_host): the same tables and the same fma chain per entry, so the entries agree
bit for bit and only the sums differ — every device output is held within the twin's own derived bound 2·N·2⁻⁵³·S
(margin_cases.bound; test_margin_host.py holds the twin to the dense long-double definition within the same bound).  (2) Bit
equality wherever the contract promises it: scenario s against an object of its own, shared against replicated values, host
against device path, run against run.  (3) On the README chain solved on the device: Plan.residual for the 𝓔₁ half on the design
plant, and a Rollout for the gain bound — an inequality.

(The tests print each figure before they assert: run with -s.)"""
import numpy as np
import pytest
import scipy.sparse as sp

import margin_cases as mc
import rollout_cases as rc

pytestmark = pytest.mark.gpu
NSCEN_MAX = 130
KEYS = ("row_l1", "col_l1", "l1", "e1")


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
    assert mg.n_entries == case.n_entries and mg.device_bytes >= 8 * mg.n_defect * nscen + mg.plant_bytes
    mg._keep = _to_dev(case.values if values is None else values)
    mg.load(mg._keep)
    return mg


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def _cut(twin, n):
    """the first n scenarios of a twin record (term counts do not depend on the scenario)"""
    return {k: (v if k.endswith("_n") else v[..., :n]) for k, v in twin.items()}


@pytest.fixture(scope="module")
def cases():
    return {name: mc.case(name) for name in mc.ALL}


@pytest.fixture(scope="module")
def twins(slc, cases):
    """One twin per case for all layouts, at 130 scenarios: column s of the perturbed plants does not depend on nscen, and
    test_margin_host.py shows that scenario s of the twin does not either"""
    out = {}
    for name, case in cases.items():
        Av, Bv = mc.perturbed(case, NSCEN_MAX)
        tw = slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, NSCEN_MAX, A=Av, B2=Bv, per_scenario=True)
        for a in (Av, Bv) + tuple(tw.values()):
            a.setflags(write=False)
        out[name] = (Av, Bv, tw)
    return out


# ------------------------------------------------------------------ 1. every case at every lane layout

@pytest.mark.parametrize("nscen", mc.LAYOUT_NSCEN)
@pytest.mark.parametrize("name", mc.ALL)
def test_device_against_the_twin(slc, gpu_ctx, cases, twins, name, nscen):
    """Per-scenario perturbed plants; nscen 1 … 64 take the seven lane layouts, 65 and 130 a second and a third chunk.  Rows and
    columns without a pattern entry report exactly 0.0."""
    case = cases[name]
    Av, Bv, tw = twins[name]
    mg = _margin(slc, gpu_ctx, case, nscen)
    mg.set_plant(Av[:, :nscen], Bv[:, :nscen], per_scenario=True)
    got = mg.margins()
    worst = mc.check_against_twin(got, _cut(tw, nscen), f"{name} nscen {nscen}")
    print(name, nscen, "largest error / bound", f"{worst:.3f}")
    assert np.array_equal(got["l1"], got["row_l1"].max(axis=0)) and np.array_equal(got["e1"], got["col_l1"].max(axis=0))
    for key, n in (("row_l1", "row_n"), ("col_l1", "col_n")):
        assert not got[key][tw[n] == 0].any()
    if name == "edges":
        assert not got["row_l1"][mc.EDGES_EMPTY_ROW].any() and not got["col_l1"][mc.EDGES_EMPTY_COLUMN].any()
    mg.close()


# ------------------------------------------------------------------ 2. what must be equal bit for bit

@pytest.mark.parametrize("name", ["ladder", "edges"])
def test_a_scenario_equals_an_object_of_its_own(slc, gpu_ctx, cases, twins, name):
    case = cases[name]
    Av, Bv, _ = twins[name]
    full = {}
    for nscen in (7, 65):
        mg = _margin(slc, gpu_ctx, case, nscen)
        mg.set_plant(Av[:, :nscen], Bv[:, :nscen], per_scenario=True)
        full[nscen] = mg.margins()
        mg.close()
    one = _margin(slc, gpu_ctx, case, 1)
    for s in (0, 3, 6, 64):
        one.set_plant(Av[:, s], Bv[:, s])
        m = one.margins()
        for nscen in (7, 65):
            if s < nscen:
                assert all(np.array_equal(full[nscen][k][..., s], m[k][..., 0]) for k in KEYS), (name, nscen, s)
    one.close()


def test_shared_replicated_host_device_and_null(slc, gpu_ctx, cases, twins):
    """One shared array = per-scenario copies of it; host arrays = device tensors; None keeps what is there; two runs and the
    device-tensor outputs of run_async carry the same bits."""
    import torch
    case = cases["ladder"]
    Av, Bv, _ = twins["ladder"]
    nscen = 5
    mg = _margin(slc, gpu_ctx, case, nscen)
    design = mg.margins()
    assert _same(design, mg.margins())
    mg.set_plant(Av[:, 2], Bv[:, 2])
    shared = mg.margins()
    assert not _same(shared, design)
    mg.set_plant(np.repeat(Av[:, 2:3], nscen, axis=1), np.repeat(Bv[:, 2:3], nscen, axis=1), per_scenario=True)
    assert _same(mg.margins(), shared)
    mg.set_plant(rc.csc_values(case.A), rc.csc_values(case.B2))
    assert _same(mg.margins(), design)
    mg.set_plant(_to_dev(Av[:, 2]), _to_dev(Bv[:, 2]))
    assert _same(mg.margins(), shared)
    mg.set_plant(Av[:, :nscen], Bv[:, :nscen], per_scenario=True)
    host = mg.margins()
    mg.set_plant(rc.csc_values(case.A), rc.csc_values(case.B2))
    mg.set_plant(_to_dev(Av[:, :nscen]), _to_dev(Bv[:, :nscen]), per_scenario=True)
    assert _same(mg.margins(), host) and not _same(host, shared)
    mg.set_plant(None, None)
    mg.set_plant(A=Av[:, :nscen], per_scenario=True)                # B2 kept
    mg.set_plant(B2=_to_dev(Bv[:, :nscen]), per_scenario=True)      # A kept
    assert _same(mg.margins(), host)
    row = torch.full((case.Nx, nscen), float("nan"), dtype=torch.float64, device=_dev())
    col, tot = torch.full_like(row, float("nan")), torch.full((2, nscen), float("nan"), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    mg.run_async(row, col, tot)
    mg.run_async(None, None, None)
    torch.cuda.synchronize()
    assert np.array_equal(row.cpu().numpy(), host["row_l1"]) and np.array_equal(col.cpu().numpy(), host["col_l1"])
    assert np.array_equal(tot.cpu().numpy(), np.stack([host["l1"], host["e1"]]))
    assert np.array_equal(mg.certified(), np.minimum(host["l1"], host["e1"]) < 1)
    gb = mg.gain_bound()
    assert np.array_equal(np.isinf(gb), host["l1"] >= 1) and (gb[host["l1"] < 1] >= 1).all()
    mg.close()


@pytest.mark.parametrize("name", ["T5", "edges"])
def test_a_second_load_of_scaled_phi(slc, gpu_ctx, cases, twins, name):
    case = cases[name]
    Av, Bv, tw = twins[name]
    nscen = 3
    mg = _margin(slc, gpu_ctx, case, nscen)
    mg.set_plant(Av[:, :nscen], Bv[:, :nscen], per_scenario=True)
    first = mg.margins()
    half = _to_dev(mc.scaled_values(case, 0.5))
    mg.load(half)
    got = mg.margins()
    want = slc.margin_host(_plant(slc, case), [case.Sx, case.Su], mc.scaled_values(case, 0.5), nscen, A=Av[:, :nscen], B2=Bv[:, :nscen],
                           per_scenario=True)
    print(name, "scaled: largest error / bound", f"{mc.check_against_twin(got, want, name):.3f}")
    assert not _same(got, first)
    mg.load(mg._keep)
    assert _same(mg.margins(), first)
    mg.close()


# ------------------------------------------------------------------ 3. NaN

def test_a_nan_in_one_plant_value_of_one_scenario(slc, gpu_ctx, cases, twins):
    case = cases["edges"]
    Av, Bv, _ = twins["edges"]
    nscen = 6
    mg = _margin(slc, gpu_ctx, case, nscen)
    mg.set_plant(Av[:, :nscen], Bv[:, :nscen], per_scenario=True)
    clean = mg.margins()
    Acsc = sp.csc_matrix(case.A); Acsc.sort_indices()
    nz = Acsc.nnz // 2
    k, i = int(np.searchsorted(Acsc.indptr, nz, side="right") - 1), int(Acsc.indices[nz])
    bad = np.array(Av[:, :nscen]); bad[nz, 3] = np.nan
    mg.set_plant(A=bad, per_scenario=True)
    got = mg.margins()
    rows, cols = mc.reach_of_plant(case, "A", i, k)
    assert rows.any() and cols.any() and not cols.all()
    for key, hit in (("row_l1", rows), ("col_l1", cols)):
        assert np.isposinf(got[key][hit, 3]).all() and np.array_equal(got[key][~hit, 3], clean[key][~hit, 3]), key
    assert np.isposinf(got["l1"][3]) and np.isposinf(got["e1"][3])
    others = [s for s in range(nscen) if s != 3]
    assert all(np.array_equal(got[k2][..., others], clean[k2][..., others]) for k2 in KEYS)
    assert not mg.certified()[3] and np.isinf(mg.gain_bound()[3])
    mg.close()


def test_a_nan_in_one_read_phi_value(slc, gpu_ctx, cases, twins):
    case = cases["edges"]
    Av, Bv, _ = twins["edges"]
    nscen = 3
    mg = _margin(slc, gpu_ctx, case, nscen)
    mg.set_plant(Av[:, :nscen], Bv[:, :nscen], per_scenario=True)
    clean = mg.margins()
    t, r, c = mc.phi_probe(case)
    vals = case.values.copy(); vals[mc.value_index(case, "x", t, r, c)] = np.nan
    bad = _to_dev(vals)
    mg.load(bad)
    got = mg.margins()
    rows, cols = mc.reach_of_phi(case, "x", t, r, c)
    assert rows.sum() >= 2 and cols.sum() == 1
    for key, hit in (("row_l1", rows), ("col_l1", cols)):
        assert np.isposinf(got[key][hit]).all() and np.array_equal(got[key][~hit], clean[key][~hit]), key
    assert np.isposinf(got["l1"]).all() and np.isposinf(got["e1"]).all()
    mg.close()


# ------------------------------------------------------------------ 4. errors

def test_error_paths_leave_the_object_usable(slc, gpu_ctx, cases):
    case = cases["T2"]
    EINVAL = slc._capi.SLS_EINVAL
    mg = slc.RobustMargin(gpu_ctx, _plant(slc, case), [case.Sx, case.Su], nscen=3)
    for call in (lambda: mg.run_async(), lambda: mg.margins()):   # before the first load
        with pytest.raises(slc.SLSError) as e:
            call()
        assert e.value.code == EINVAL
    for kw in (dict(nscen=0), dict(nscen=-2), dict(nscen=1, dev_slot=5), dict(nscen=1, dev_slot=-1)):
        with pytest.raises(slc.SLSError) as e:
            slc.RobustMargin(gpu_ctx, _plant(slc, case), [case.Sx, case.Su], **kw)
        assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        mg.set_plant(A=np.zeros(2))
    with pytest.raises(ValueError):
        mg.set_plant(A=rc.csc_values(case.A), B2=_to_dev(rc.csc_values(case.B2)))
    d = _to_dev(case.values)
    mg.load(d)
    want = slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, 3)
    mc.check_against_twin(mg.margins(), want, "after the refusals")
    mg.close(); mg.close()


# ------------------------------------------------------------------ 5. the README chain through a Plan

EPS_DRAWS = 8


def _epsilon_draws(P, eps, n=EPS_DRAWS, seed=11):
    """every stored value of A and B₂ times U[1 − ε, 1 + ε]: ([nnz(A), n], [nnz(B₂), n]) in the CSC nzval order"""
    rng = np.random.default_rng(seed)
    a, b = rc.csc_values(P.A), rc.csc_values(P.B2)
    return a[:, None] * rng.uniform(1 - eps, 1 + eps, (a.size, n)), b[:, None] * rng.uniform(1 - eps, 1 + eps, (b.size, n))


@pytest.fixture(scope="module")
def solved_readme(slc, gpu_ctx, readme):
    P, S, _ = readme
    plan = slc.Plan(gpu_ctx, P, S)
    d = plan.alloc_values()
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == 0)
    yield P, S, plan, d
    plan.close()


def test_readme_design_plant_against_the_plans_residual(slc, gpu_ctx, solved_readme):
    """col_l1[j] is the plan's res_l1[j] without the Δ[0] = Φx[0][:,j] − e_j block: they agree up to Σ_i |Φx[0][i,j] − δ_ij| of the
    downloaded Φ plus the two derived bounds."""
    P, S, plan, d = solved_readme
    mg = slc.RobustMargin(gpu_ctx, P, S, nscen=1)
    mg.load(d)
    got = mg.margins()
    res = plan.residual(d)
    vx, vu = plan.download(d)
    values = np.concatenate(vx + vu)
    tw = slc.margin_host(P, S, values, 1)
    mc.check_against_twin(got, tw, "README design plant")
    _, rb = slc.residual_host(P, S, vx, vu, return_bound=True)
    assert res.res_l1.shape == (P.Nx,)
    M0 = sp.csc_matrix(S[0][0]); M0.sort_indices()
    X0 = sp.csc_matrix((np.where(np.asarray(M0.data, dtype=bool), vx[0][: M0.nnz], 0.0), M0.indices, M0.indptr), shape=M0.shape).toarray()
    first = np.abs(X0.astype(np.longdouble) - np.eye(P.Nx)).sum(axis=0)
    room = first + mc.bound(tw["col_n"], tw["col_s"][:, 0]) + mc.bound(rb["l1_terms"], rb["l1_abs"])
    gap = np.abs(got["col_l1"][:, 0].astype(np.longdouble) - res.res_l1)
    print("README design plant: l1", got["l1"], "e1", got["e1"], "plan e1", res.e1_norm, "largest gap", float(gap.max()), "room", float(room.min()),
          "Σ|Φx[0] − I|", float(first.max()))
    assert (gap <= room).all()
    assert mg.certified().all() and got["l1"][0] < 1e-9
    mg.close()


def test_readme_ensemble_certificate_and_gain_bound(slc, gpu_ctx, solved_readme):
    """8 plants at ε = 0.01 and 8 at ε = 0.2: the first eight are certified, the others are not (on the oracle's Φ the norms are at
    most 0.63 and at least 5.9).  For the certified ones a 200-step rollout with |w| ≤ 1 stays below ‖Φx‖_𝓛₁ / (1 − ‖D⁽ˢ⁾‖_𝓛₁)."""
    import torch
    P, S, plan, d = solved_readme
    A1, B1 = _epsilon_draws(P, 0.01)
    A2, B2 = _epsilon_draws(P, 0.2)
    mg = slc.RobustMargin(gpu_ctx, P, S, nscen=2 * EPS_DRAWS)
    mg.load(d)
    mg.set_plant(np.hstack([A1, A2]), np.hstack([B1, B2]), per_scenario=True)
    m = mg.margins()
    print("ε = 0.01: l1", m["l1"][:EPS_DRAWS].min(), "–", m["l1"][:EPS_DRAWS].max(), "e1", m["e1"][:EPS_DRAWS].min(), "–", m["e1"][:EPS_DRAWS].max())
    print("ε = 0.2:  l1", m["l1"][EPS_DRAWS:].min(), "–", m["l1"][EPS_DRAWS:].max(), "e1", m["e1"][EPS_DRAWS:].min(), "–", m["e1"][EPS_DRAWS:].max())
    cert = mg.certified()
    assert cert[:EPS_DRAWS].all() and not cert[EPS_DRAWS:].any()
    gain = mg.gain_bound()[:EPS_DRAWS]
    assert np.isfinite(gain).all()
    assert (abs(sp.csc_matrix(P.B1) - sp.identity(P.Nx)) > 0).nnz == 0          # w̃ = B₁·w = w, so |w̃| ≤ 1
    nrm = slc.ClosedLoopNorms((P.Nx, P.Nu), S, ctx=gpu_ctx).load(d)
    row, _, _ = nrm.l1()
    phix_l1 = row[: P.Nx].max()
    steps = 200
    w = np.random.default_rng(5).uniform(-1.0, 1.0, (steps, P.Nw, EPS_DRAWS))
    ro = slc.Rollout(gpu_ctx, P, S, nscen=EPS_DRAWS)
    ro.load(d)
    ro.set_plant(A1, B1, per_scenario=True)
    d_w = _to_dev(w)
    ro.run(steps, w=d_w)
    torch.cuda.synchronize()
    _, peak_x, _ = ro.stats()
    print("peak_x", peak_x, "bound", phix_l1 * gain)
    assert (peak_x > 0).all() and (peak_x <= phix_l1 * gain).all()
    ro.close(); nrm.close(); mg.close()
