"""GPU tests of the ensemble rollout (csrc/sls_rollout.hip, sls_rollout_*): one kernel launch per step, the plant stepped on the
device with the controller, a plant of its own per scenario, cost and peaks accumulated on the device.

References.  (1) The closed-loop simulator on the same device: the step kernel is the simulator's restated on the controller's
ring — same entries, same lanes, same order — so with the plant the simulator was planned with x and u must equal its rows BIT
FOR BIT.  (2) The long-double statement of the recursion in tests/rollout_cases.py with dense per-scenario plants, at the project's
RTOL = 1e-11 relative to max(1, max|reference|) per scenario for x, u, state and peaks and 3e-11 relative for the cost
(test_rollout_host.py shows max|x| < 4 on every reference used here).  (3) The solver's own objective value of a column, for the
cost of that column's impulse response.

Largest relative error against the long-double reference on an MI355X, against the tolerances of 1e-11 (x, u, state, peaks) and
3e-11 (cost): lane layouts x 2.2e-16 (nscen 7), u 3.2e-16 (nscen 130), state 2.5e-16, peaks 2.8e-16, cost 5.6e-16 (nscen ≥ 32); ring
and chunks x 1.6e-16, cost 2.6e-16; run sequence x 2.2e-16, cost 3.8e-16; Nu = 0 x 1.4e-16.  Cost against the solver's objective:
3.0e-15 on the design plant and 1.7e-15 after update and reload (bound 1e-8); 0.37 with the stale Φ.  (The tests print each figure
before they assert: run with -s.)"""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import closed_loop_cases as clc
import controller_cases as cc
import rollout_cases as rc
import weights_cases as wc

pytestmark = pytest.mark.gpu
NSCEN_MAX = 130


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(_dev())        # a copy: fixtures are read-only


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device=_dev())


def _plant(slc, case, A=None, B2=None):
    return slc.Plant(case.A if A is None else A, case.B1, case.B2 if B2 is None else B2)


def _rollout(slc, ctx, case, nscen, values=None):
    ro = slc.Rollout(ctx, _plant(slc, case), [case.Sx, case.Su], nscen=nscen)
    assert ro.n_entries == case.n_entries and ro.k == 0
    d_vals = _to_dev(case.values if values is None else values)
    ro.load(d_vals)
    ro._keep = d_vals
    return ro


def _run(ro, steps, w=None, stream=None, record=True):
    """one run of `steps` steps: dict of host arrays x, u (recorded rows) — nothing waits before the final synchronise"""
    import torch
    d_w = None if w is None else _to_dev(w)
    d_x = _nan(steps, ro.Nx, ro.nscen) if record else None
    d_u = _nan(steps, ro.Nu, ro.nscen) if record and ro.Nu else None
    torch.cuda.synchronize()
    ro.run(steps, w=d_w, x=d_x, u=d_u, stream=stream)
    torch.cuda.synchronize()
    out = {}
    if record:
        out["x"] = d_x.cpu().numpy()
        out["u"] = d_u.cpu().numpy() if ro.Nu else np.zeros((steps, 0, ro.nscen))
    return out


def _collect(ro, out=None):
    out = {} if out is None else out
    out["state"] = ro.state()
    out["cost"], out["peak_x"], out["peak_u"] = ro.stats()
    return out


def _simulate(slc, ctx, case, w, A=None, B2=None):
    """ClosedLoop.run on device tensors with the plant (A, B2): host arrays x, u [steps, ·, nscen]"""
    import torch
    steps, _, nscen = w.shape
    loop = slc.ClosedLoop(ctx, _plant(slc, case, A, B2), [case.Sx, case.Su])
    d_vals, d_w = _to_dev(case.values), _to_dev(w)
    d_x, d_u = _nan(steps, case.Nx, nscen), _nan(steps, max(case.Nu, 1), nscen)
    torch.cuda.synchronize()
    loop.run(d_vals.data_ptr(), d_w.data_ptr(), steps, nscen, d_x.data_ptr(), d_u.data_ptr() if case.Nu else None,
             stream=torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    loop.close()
    return d_x.cpu().numpy(), d_u.cpu().numpy()[:, : case.Nu]


# ------------------------------------------------------------------ 1. bit for bit against the simulator

@pytest.mark.parametrize("nscen", [1, 5, 64, 130])
@pytest.mark.parametrize("name", ["ladder", "T1", "T2"])
def test_bit_for_bit_against_the_simulator(slc, gpu_ctx, name, nscen):
    """Design plant, x_0 = 0, dense w, one run of S − 1 steps: recorded x rows 0 … S−2 plus the fetched state are rows 0 … S−1 of
    sls_closed_loop_run, the u rows 0 … S−2 are equal too."""
    case = rc.case(name)
    w = clc.ladder_w(nscen) if name == "ladder" else clc.small_w(nscen)
    S = case.steps
    xs, us = _simulate(slc, gpu_ctx, case, w)
    ro = _rollout(slc, gpu_ctx, case, nscen)
    got = _collect(ro, _run(ro, S - 1, w=w[: S - 1]))
    assert ro.k == S - 1
    assert np.isfinite(got["x"]).all() and np.abs(xs).max() > 0.1 and np.abs(us[: S - 1]).max() > 0
    assert np.array_equal(got["x"], xs[: S - 1]) and np.array_equal(got["state"], xs[S - 1])
    assert np.array_equal(got["u"], us[: S - 1])
    assert np.array_equal(got["peak_x"], np.abs(xs[: S - 1]).max(axis=(0, 1)))          # peaks are exact: max of the recorded rows
    assert np.array_equal(got["peak_u"], np.abs(us[: S - 1]).max(axis=(0, 1)))
    ro.close()


# ------------------------------------------------------------------ 2. every lane layout

@pytest.fixture(scope="module")
def ladder():
    return clc.ladder()


@pytest.fixture(scope="module")
def layout_run(ladder):
    """One input and one reference for all layouts: scenarios do not interact, and column s of the perturbed plants does not
    depend on nscen"""
    Av, Bv = rc.perturbed(ladder, NSCEN_MAX)
    x0, w = rc.initial_state("ladder", NSCEN_MAX), rc.disturbance("ladder", rc.LAYOUT_STEPS, NSCEN_MAX)
    q, r = rc.weights(ladder)
    ref = rc.reference(ladder, rc.LAYOUT_STEPS, NSCEN_MAX, w=w, A_vals=Av, B2_vals=Bv, x0=x0, q=q, r=r)
    assert float(np.abs(ref["x"]).max()) < rc.GROWTH_BOUND
    for a in (Av, Bv, x0, w, q, r) + tuple(ref.values()):
        a.setflags(write=False)
    return Av, Bv, x0, w, q, r, ref


@pytest.mark.parametrize("nscen", rc.LAYOUT_NSCEN)
def test_every_lane_layout_on_the_ladder(slc, gpu_ctx, ladder, layout_run, nscen):
    """SCN = 1 … 64, each with all scenario slots live and with dead lanes in the last chunk; 130 scenarios are three chunks in
    grid.y.  Per-scenario perturbed plants (set from the device), a non-zero x_0, weights other than 1, 60 steps: the ring of 32
    slots wraps.  Tolerances: x, u, state, peaks 1e-11, cost 3e-11."""
    Av, Bv, x0, w, q, r, ref = layout_run
    ro = _rollout(slc, gpu_ctx, ladder, nscen)
    dA, dB = _to_dev(Av[:, :nscen]), _to_dev(Bv[:, :nscen])
    ro.set_plant(dA, dB, per_scenario=True)
    ro.set_weights(q, r)
    ro.reset(_to_dev(x0[:, :nscen]))
    got = _collect(ro, _run(ro, rc.LAYOUT_STEPS, w=w[:, :, :nscen]))
    cut = {k: (v[..., :nscen]) for k, v in ref.items()}
    errs = rc.check_all(got, cut, f"ladder nscen={nscen}")
    print(f"ladder nscen={nscen}:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.abs(got["u"][:, 0]).max() == 0                        # the actuator with an empty operator row: exactly 0
    assert np.abs(got["u"][:, clc.LADDER_ORPHAN]).max() > 0
    assert np.array_equal(got["x"][0], x0[:, :nscen])
    ro.close()


# ------------------------------------------------------------------ 3. ensemble against the simulator

@pytest.mark.parametrize("nscen", [5, 65])
def test_ensemble_column_equals_a_simulator_built_from_that_plant(slc, gpu_ctx, ladder, nscen):
    """For three scenarios s: an sls_closed_loop built from plant s, run with the same nscen and the same w — its column s of x
    and u is the ensemble's column s bit for bit (same layout, same order)."""
    Av, Bv = rc.perturbed(ladder, nscen)
    w = clc.ladder_w(nscen)
    S = ladder.steps
    ro = _rollout(slc, gpu_ctx, ladder, nscen)
    ro.set_plant(Av, Bv, per_scenario=True)
    got = _collect(ro, _run(ro, S - 1, w=w[: S - 1]))
    for s in (0, nscen // 2, nscen - 1):
        xs, us = _simulate(slc, gpu_ctx, ladder, w, A=rc.with_values(ladder.A, Av[:, s]), B2=rc.with_values(ladder.B2, Bv[:, s]))
        assert np.array_equal(got["x"][:, :, s], xs[: S - 1, :, s]) and np.array_equal(got["state"][:, s], xs[S - 1, :, s]), s
        assert np.array_equal(got["u"][:, :, s], us[: S - 1, :, s]), s
    assert np.abs(got["x"][:, :, 0] - got["x"][:, :, nscen - 1]).max() > 1e-3      # the plants do differ
    ro.close()


# ------------------------------------------------------------------ 4. ring and chunks

@pytest.mark.parametrize("name", rc.RING)
def test_ring_and_chunks(slc, gpu_ctx, name):
    """Rings of 1, 2, 4 (= T: the slot written is the one just below the oldest read) and 8 > T = 5 slots, 3R + 5 steps: chunk
    lengths 1, 2, R−1, R, R+1 and the rest in sequence give x, u, state, cost and peaks bit-identical to one call; reset and rerun
    gives the same bits; stats called twice is bit-identical; and the single run is within tolerance of the reference."""
    case = rc.case(name)
    steps, nscen = rc.ring_steps(case.T), 3
    R = cc.ring_slots(case.T)
    assert steps >= 2 * R + 4 and (name != "T5" or steps >= 20)
    Av, Bv = rc.perturbed(case, nscen)
    x0, w = rc.initial_state(name, nscen), rc.disturbance(name, steps, nscen)
    ref = rc.reference(case, steps, nscen, w=w, A_vals=Av, B2_vals=Bv, x0=x0)
    ro = _rollout(slc, gpu_ctx, case, nscen)
    ro.set_plant(Av, Bv, per_scenario=True)
    d_x0 = _to_dev(x0)
    ro.reset(d_x0)
    one = _collect(ro, _run(ro, steps, w=w))
    again = _collect(ro)
    assert all(np.array_equal(one[k], again[k]) for k in again)                         # stats twice
    print(f"{name}:", {k: f"{v:.2e}" for k, v in rc.check_all(one, ref, name).items()})
    ro.reset(d_x0)                                                                       # reset and rerun
    two = _collect(ro, _run(ro, steps, w=w))
    assert all(np.array_equal(one[k], two[k]) for k in one)
    ro.reset(d_x0)                                                                       # chunks
    xs, us, done = [], [], 0
    for n in rc.ring_chunks(case.T):
        part = _run(ro, n, w=w[done:done + n])
        xs.append(part["x"]); us.append(part["u"]); done += n
    assert done == steps and ro.k == steps
    many = _collect(ro, dict(x=np.concatenate(xs), u=np.concatenate(us)))
    for k in one:
        assert np.array_equal(one[k], many[k]), (name, k)
    ro.close()


# ------------------------------------------------------------------ 5. one object through a sequence

def test_one_rollout_through_a_sequence(slc, gpu_ctx, ladder):
    """On a non-default stream: (a) shared plant values from the host, with NULL for B₂, equal the plan's own; (b) per-scenario
    values from the device, A alone, then B₂ alone from the host; (c) load of 0.5·Φ at step 20 without reset against the
    reference that switches at that step; (d) set_weights changes the cost and not x or u; (e) recording off while the cost still
    accumulates; (f) stats into device tensors."""
    import torch
    steps, nscen = 40, 3
    stream = torch.cuda.Stream(device=_dev())
    s = stream.cuda_stream
    Av, Bv = rc.perturbed(ladder, nscen)
    w, x0 = rc.disturbance("ladder", steps, nscen, seed=1), rc.initial_state("ladder", nscen, seed=1)
    with torch.cuda.stream(stream):
        d_w, d_x0, d_vals = _to_dev(w), _to_dev(x0), _to_dev(ladder.values)
        d_half = d_vals * 0.5
        dA, dB = _to_dev(Av), _to_dev(Bv)
    stream.synchronize()
    ro = slc.Rollout(gpu_ctx, _plant(slc, ladder), [ladder.Sx, ladder.Su], nscen=nscen)
    ro.load(d_vals, stream=s)

    def go(n, w_rows, record=True):
        d_x = _nan(n, ro.Nx, nscen) if record else None
        d_u = _nan(n, ro.Nu, nscen) if record else None
        stream.synchronize()
        ro.run(n, w=w_rows, x=d_x, u=d_u, stream=s)
        stream.synchronize()
        return (d_x.cpu().numpy(), d_u.cpu().numpy()) if record else (None, None)

    def stats():
        out = dict(state=ro.state(stream=s))
        out["cost"], out["peak_x"], out["peak_u"] = ro.stats(stream=s)
        return out

    # (a) the design plant, as planned and as set from the host with NULL for B₂
    ro.reset(d_x0, stream=s)
    xa, ua = go(steps, d_w)
    a = stats()
    ref = rc.reference(ladder, steps, nscen, w=w, x0=x0)
    print("(a)", {k: f"{v:.2e}" for k, v in rc.check_all(dict(a, x=xa, u=ua), ref, "(a)").items()})
    ro.set_plant(A=rc.csc_values(ladder.A), stream=s)
    ro.reset(d_x0, stream=s)
    xa2, ua2 = go(steps, d_w)
    assert np.array_equal(xa, xa2) and np.array_equal(ua, ua2) and all(np.array_equal(a[k], v) for k, v in stats().items())
    # (b) per-scenario values: A from the device, B₂ alone from the host
    ro.set_plant(A=dA, per_scenario=True, stream=s)
    ro.set_plant(B2=Bv, per_scenario=True, stream=s)
    ro.reset(d_x0, stream=s)
    xb, ub = go(steps, d_w)
    b = stats()
    ref_b = rc.reference(ladder, steps, nscen, w=w, A_vals=Av, B2_vals=Bv, x0=x0)
    print("(b)", {k: f"{v:.2e}" for k, v in rc.check_all(dict(b, x=xb, u=ub), ref_b, "(b)").items()})
    assert np.abs(xb - xa).max() > 1e-3
    # shared again: scenario 0's values for all, both from the device
    ro.set_plant(A=dA[:, 0].contiguous(), B2=dB[:, 0].contiguous(), stream=s)
    ro.reset(d_x0, stream=s)
    xs0, us0 = go(steps, d_w)
    ref_s = rc.reference(ladder, steps, nscen, w=w, A_vals=Av[:, 0], B2_vals=Bv[:, 0], x0=x0)
    print("(b') shared", {k: f"{v:.2e}" for k, v in rc.check_all(dict(stats(), x=xs0, u=us0), ref_s, "(b')").items()})
    assert np.array_equal(xs0[:, :, 0], xb[:, :, 0])
    # (c) Φ switched at step 20, state kept
    ro.set_plant(A=dA, B2=dB, per_scenario=True, stream=s)
    ro.reset(d_x0, stream=s)
    x1, u1 = go(20, d_w[:20])
    ro.load(d_half, stream=s)
    assert ro.k == 20
    x2, u2 = go(steps - 20, d_w[20:])
    c = dict(stats(), x=np.concatenate([x1, x2]), u=np.concatenate([u1, u2]))
    ref_c = rc.reference(ladder, steps, nscen, w=w, A_vals=Av, B2_vals=Bv, x0=x0, switch=(20, 0.5))
    print("(c)", {k: f"{v:.2e}" for k, v in rc.check_all(c, ref_c, "(c)").items()})
    assert np.array_equal(c["x"][:21], xb[:21]) and np.abs(c["x"][21:] - xb[21:]).max() > 1e-3
    ro.load(d_vals, stream=s)
    # (d) weights change the cost, not the trajectory; (e) recording off
    q, r = rc.weights(ladder)
    ro.set_weights(q, r, stream=s)
    ro.reset(d_x0, stream=s)
    xd, ud = go(steps, d_w)
    d = stats()
    assert np.array_equal(xd, xb) and np.array_equal(ud, ub) and np.array_equal(d["peak_x"], b["peak_x"])
    ref_d = rc.reference(ladder, steps, nscen, w=w, A_vals=Av, B2_vals=Bv, x0=x0, q=q, r=r)
    print("(d) cost", rc.check_cost(d["cost"], ref_d["cost"], "(d)"))
    assert (np.abs(d["cost"] - b["cost"]) > 1e-3 * b["cost"]).all()
    ro.set_weights(_to_dev(q), None, stream=s)                     # device path, r kept
    ro.reset(d_x0, stream=s)
    go(steps, d_w, record=False)                                   # (e)
    e = stats()
    assert all(np.array_equal(d[k], e[k]) for k in d)
    d_c, d_px, d_pu = _nan(nscen), _nan(nscen), _nan(nscen)        # (f)
    ro.stats_async(d_c, d_px, d_pu, stream=s)
    ro.stats_async(None, None, None, stream=s)
    stream.synchronize()
    assert np.array_equal(d_c.cpu().numpy(), e["cost"]) and np.array_equal(d_px.cpu().numpy(), e["peak_x"])
    assert np.array_equal(d_pu.cpu().numpy(), e["peak_u"])
    ro.close()


def test_no_actuators_accepts_a_null_u(slc, gpu_ctx):
    """Nu = 0: d_u = NULL, peak_u = 0, x against the reference"""
    case = rc.case("Nu0")
    steps, nscen = 30, 5
    Av, _ = rc.perturbed(case, nscen)
    w, x0 = rc.disturbance("Nu0", steps, nscen), rc.initial_state("Nu0", nscen)
    ro = _rollout(slc, gpu_ctx, case, nscen)
    ro.set_plant(A=Av, per_scenario=True)
    ro.reset(_to_dev(x0))
    got = _collect(ro, _run(ro, steps, w=w))
    ref = rc.reference(case, steps, nscen, w=w, A_vals=Av, x0=x0)
    print("Nu0:", {k: f"{v:.2e}" for k, v in rc.check_all(got, ref, "Nu0").items()})
    assert not got["peak_u"].any() and got["u"].shape[1] == 0
    ro.close()


# ------------------------------------------------------------------ 6. cost against the solver

def test_cost_of_impulse_scenarios_against_the_solvers_objective(slc, gpu_ctx):
    """A chain of 23 states in LQR form with B₁ = I, solved on a plan.  nscen = Nx impulse scenarios (w_0 = e_j) for T + 2 steps on
    the design plant: cost[j] agrees with Plan.objective_values[j] to 1e-8 relative (the bound test_readme_chain_end_to_end uses
    between a trajectory and the solver's Φ).  After set_plant with plant_values of the updated plan and the stale Φ the cost
    differs; after re-execute and load it agrees again."""
    import torch
    P0 = slc.workloads.chain_plant(23)
    P = wc.weighted(P0, wc.SEED_A)
    T = 18
    S = list(slc.workloads.localization_masks(P.A, P.B2, 6, T, 1.5))      # the smoke run's localization: every column feasible
    plan = slc.Plan(gpu_ctx, P, S)
    d = plan.alloc_values()
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == 0)
    obj, _ = plan.objective_values(d)
    Nx = P.Nx
    ro = slc.Rollout.from_plant(gpu_ctx, P, S, nscen=Nx)
    ro.load(d)
    w = np.zeros((T + 2, Nx, Nx)); w[0] = np.eye(Nx)
    d_w = _to_dev(w)

    def cost():
        ro.reset()
        torch.cuda.synchronize()
        ro.run(T + 2, w=d_w)
        return ro.stats()[0]

    c0 = cost()
    e0 = float((np.abs(c0 - obj) / obj).max())
    print(f"cost vs objective: {e0:.3e}")
    assert e0 < 1e-8 and obj.min() > 0.1
    A2 = P.A.copy(); A2.data = A2.data * np.where(A2.data == 1.0, 1.0, 1.1)       # the couplings 0.2 → 0.22
    plan.update_plant(A=A2)
    ro.set_plant(*plan.plant_values())
    c1 = cost()                                                    # new plant, stale Φ
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == 0)
    obj2, _ = plan.objective_values(d)
    assert float((np.abs(c1 - obj2) / obj2).max()) > 1e-4
    ro.load(d)
    c2 = cost()
    e2 = float((np.abs(c2 - obj2) / obj2).max())
    print(f"after update: stale {float((np.abs(c1 - obj2) / obj2).max()):.3e}, reloaded {e2:.3e}")
    assert e2 < 1e-8 and float(np.abs(obj2 - obj).max()) > 1e-4
    with pytest.raises(ValueError):
        slc.Rollout.from_plant(gpu_ctx, slc.Plant(P.A, P.B1, P.B2, sp.csc_matrix(np.ones((Nx + P.Nu, Nx))), 0, P.D12), S)
    ro.close(); plan.close()


# ------------------------------------------------------------------ 7. error paths

def test_error_paths_leave_the_rollout_usable(slc, gpu_ctx):
    import torch
    case = rc.case("T2")
    EINVAL, EUNSUP = slc._capi.SLS_EINVAL, slc._capi.SLS_EUNSUPPORTED
    nscen, steps = 3, 8
    ro = slc.Rollout(gpu_ctx, _plant(slc, case), [case.Sx, case.Su], nscen=nscen)
    w = rc.disturbance("T2", steps, nscen)
    d_w = _to_dev(w)
    with pytest.raises(slc.SLSError) as e:                          # run before the first load
        ro.run(1, w=d_w[:1])
    assert e.value.code == EINVAL and ro.k == 0
    d_vals = _to_dev(case.values)
    ro.load(d_vals)
    with pytest.raises(slc.SLSError) as e:
        slc.Rollout(gpu_ctx, _plant(slc, case), [case.Sx, case.Su], nscen=0)
    assert e.value.code == EINVAL
    with pytest.raises(slc.SLSError) as e:
        slc.Rollout(gpu_ctx, _plant(slc, case), [case.Sx, case.Su], nscen=1, dev_slot=5)
    assert e.value.code == EINVAL
    with pytest.raises(slc.SLSError) as e:
        ro.run(-1)
    assert e.value.code == EINVAL
    ro.run(0, w=None)                                               # steps = 0: a no-op
    assert ro.k == 0
    stream = torch.cuda.Stream(device=_dev())                       # a capturing stream
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # torch warns that the graph is empty: the run was refused
        with torch.cuda.graph(g, stream=stream):
            code = ro._lib.sls_rollout_run(ro.handle, stream.cuda_stream, d_w.data_ptr(), 1, None, None)
    assert code == EUNSUP and ro.k == 0
    torch.cuda.synchronize()
    ro.reset(None)                                                  # null d_x0
    got = _collect(ro, _run(ro, steps, w=w))
    ref = rc.reference(case, steps, nscen, w=w)
    rc.check_all(got, ref, "after refusals")
    assert ro.k == steps
    ro.close()
