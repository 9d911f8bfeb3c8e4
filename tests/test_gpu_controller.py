"""GPU tests of the stand-alone controller (csrc/sls_controller.hip, sls_controller_*): one kernel launch per step, the state
fed from outside.

References.  (1) The long-double statement of the recursion in tests/controller_cases.py, for every scenario, at the project's
RTOL = 1e-11 relative to max(1, max|reference|) (test_controller_host.py shows max|ŵ| ≤ 10 on every sequence used here).
(2) The closed-loop simulator on the same device: fed the simulator's x, the controller evaluates the same entries on the same
lanes in the same order, so u must equal the simulator's BIT FOR BIT in rows 0 … steps−2 (the simulator's last u row is the
README's never-assigned zero).

Shapes (controller_cases.py): the row-length ladder (Nx 24, Nu 6, T 24: ring of 32 slots) at every lane layout; T = 1, 2 (rings of
1 and 2 slots), T = 4 (ring exactly full), T = 5 (ring of 8), Nu = 0; the README chain end to end.

Largest relative error against the long-double reference on an MI355X, against the tolerance of 1e-11: lane layouts u 5.8e-16
(nscen 130), ŵ 1.8e-16; ring edges 1.6e-16; run sequence 1.8e-16; interleaved loops 1.3e-16; README chain with the mismatched
plant 3.5e-16; README replay 4.3e-15 absolute from the committed fixture (bound 1e-8).  (The tests print each figure before they
assert: run with -s.)"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import closed_loop_cases as clc
import controller_cases as cc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
NSCEN_MAX = 130
LAYOUT_STEPS = 70


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(_dev())        # a copy: fixtures are read-only


def _controller(slc, ctx, case, nscen, values=None):
    ctl = slc.Controller(ctx, (case.Nx, case.Nu), [case.Sx, case.Su], nscen=nscen)
    assert ctl.n_entries == case.n_entries and ctl.k == 0
    d_vals = _to_dev(case.values if values is None else values)
    ctl.load(d_vals)
    ctl._keep = d_vals
    return ctl


def _feed(ctl, d_x, stream=None, what=True):
    """every row of the device tensor d_x [steps, Nx, nscen] through ctl.step, nothing waits in between: (u, ŵ) device tensors"""
    import torch
    steps, nscen = d_x.shape[0], d_x.shape[2]
    d_u = torch.full((steps, ctl.Nu, nscen), float("nan"), dtype=torch.float64, device=d_x.device)
    d_w = torch.full((steps, ctl.Nx, nscen), float("nan"), dtype=torch.float64, device=d_x.device) if what else None
    torch.cuda.synchronize()
    for k in range(steps):
        ctl.step(d_x[k], u=d_u[k] if ctl.Nu else None, what=d_w[k] if what else None, stream=stream)
    return d_u, d_w


@pytest.fixture(scope="module")
def ladder():
    return clc.ladder()


@pytest.fixture(scope="module")
def ladder_run(ladder):
    """One input and one reference for all layouts: scenarios do not interact"""
    x = cc.random_x("ladder", LAYOUT_STEPS, NSCEN_MAX)
    u, w = cc.reference(ladder, x)
    for a in (x, u, w):
        a.setflags(write=False)
    return x, u, w


@pytest.mark.parametrize("nscen", [1, 2, 3, 4, 7, 16, 17, 32, 33, 64, 65, 130])
def test_every_lane_layout_on_the_ladder(slc, gpu_ctx, ladder, ladder_run, nscen):
    """SCN = 1 … 64, each with all scenario slots live and with dead lanes in the last chunk; 130 scenarios are three chunks in
    grid.y.  70 steps of random x: the ring of 32 slots wraps twice.  Every row length of the ladder, every scenario."""
    import torch
    x, ur, wr = ladder_run
    ctl = _controller(slc, gpu_ctx, ladder, nscen)
    d_u, d_w = _feed(ctl, _to_dev(x[:, :, :nscen]))
    torch.cuda.synchronize()
    assert ctl.k == LAYOUT_STEPS
    u, w = d_u.cpu().numpy(), d_w.cpu().numpy()
    eu, ew = cc.check(u, ur[:, :, :nscen], f"ladder nscen={nscen} u"), cc.check(w, wr[:, :, :nscen], f"ladder nscen={nscen} ŵ")
    print(f"ladder nscen={nscen}: rel err u {eu:.3e} ŵ {ew:.3e}")
    assert np.abs(u[:, 0]).max() == 0                              # the actuator with an empty operator row: exactly 0
    assert np.abs(u[:, clc.LADDER_ORPHAN]).max() > 0
    ctl.close()


def _simulate(slc, ctx, case, w):
    """ClosedLoop.run on device tensors: (x, u) device tensors [steps, ·, nscen]"""
    import torch
    steps, _, nscen = w.shape
    loop = slc.ClosedLoop(ctx, slc.Plant(case.A, case.B1, case.B2), [case.Sx, case.Su])
    d_vals, d_w = _to_dev(case.values), _to_dev(w)
    d_x = torch.full((steps, case.Nx, nscen), float("nan"), dtype=torch.float64, device=_dev())
    d_u = torch.full((steps, max(case.Nu, 1), nscen), float("nan"), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    loop.run(d_vals.data_ptr(), d_w.data_ptr(), steps, nscen, d_x.data_ptr(), d_u.data_ptr() if case.Nu else None,
             stream=torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    loop.close()
    return d_x, d_u


@pytest.mark.parametrize("nscen", [1, 5, 64, 130])
@pytest.mark.parametrize("name", ["ladder", "T1", "T2"])
def test_bit_for_bit_against_the_simulator(slc, gpu_ctx, name, nscen):
    """The simulator's x tensor fed step by step on the device: same entries, same lanes, same order — the same bits."""
    import torch
    case = cc.case(name)
    w = clc.ladder_w(nscen) if name == "ladder" else clc.small_w(nscen)
    d_x, d_usim = _simulate(slc, gpu_ctx, case, w)
    ctl = _controller(slc, gpu_ctx, case, nscen)
    d_u, _ = _feed(ctl, d_x, stream=torch.cuda.current_stream(_dev()).cuda_stream, what=False)
    torch.cuda.synchronize()
    u, usim = d_u.cpu().numpy(), d_usim.cpu().numpy()
    steps = case.steps
    assert np.isfinite(u).all() and np.abs(usim[: steps - 1]).max() > 0
    assert np.array_equal(u[: steps - 1], usim[: steps - 1])
    assert not usim[steps - 1].any()
    ctl.close()


def test_no_actuators_accepts_a_null_u(slc, gpu_ctx):
    """Nu = 0: d_u = NULL is accepted and ŵ equals x − β of the reference, on the simulator's x"""
    import torch
    case = cc.case("Nu0")
    d_x, _ = _simulate(slc, gpu_ctx, case, clc.small_w(5))
    ctl = _controller(slc, gpu_ctx, case, 5)
    d_u, d_w = _feed(ctl, d_x)
    torch.cuda.synchronize()
    x = d_x.cpu().numpy()
    ur, wr = cc.reference(case, x)
    assert d_u.shape[1] == 0 and ur.shape[1] == 0
    print("Nu0: rel err ŵ", cc.check(d_w.cpu().numpy(), wr, "Nu0 ŵ"))
    assert np.abs(wr - x).max() > 1e-3                                # β is at work
    ctl.close()


@pytest.mark.parametrize("name", ["T1", "T2", "T4", "T5"])
def test_ring_edges(slc, gpu_ctx, name):
    """Rings of 1, 2, 4 (exactly full: the slot written is the one just beyond the oldest read) and 8 > T = 5 slots, for more than
    three turns"""
    import torch
    case = cc.case(name)
    steps = 40
    assert steps >= 3 * cc.ring_slots(case.T) + 2
    x = cc.random_x(name, steps, 3)
    ur, wr = cc.reference(case, x)
    ctl = _controller(slc, gpu_ctx, case, 3)
    d_u, d_w = _feed(ctl, _to_dev(x))
    torch.cuda.synchronize()
    eu, ew = cc.check(d_u.cpu().numpy(), ur, f"{name} u"), cc.check(d_w.cpu().numpy(), wr, f"{name} ŵ")
    print(f"{name}: rel err u {eu:.3e} ŵ {ew:.3e}")
    assert np.abs(ur).max() > 0.1
    ctl.close()


def test_one_controller_through_a_sequence(slc, gpu_ctx, ladder):
    """On a non-default stream, no host wait between steps: (a) 40 steps, one synchronise; (b) reset and the same inputs again —
    the same bits; (c) load of 0.5·Φ at step 20 WITHOUT reset (exact in FP64; the reference switches Φ at the same step and
    keeps its history); (d) after a run with |x| ~ 1e6, reset and compare with a fresh controller: the first T + 2 steps are
    bitwise equal, no stale slot shows."""
    import torch
    steps, nscen = 40, 3
    stream = torch.cuda.Stream(device=_dev())
    s = stream.cuda_stream
    x = cc.random_x("ladder", steps, nscen, seed=1)
    with torch.cuda.stream(stream):
        d_x = _to_dev(x)
        d_vals = _to_dev(ladder.values)
        d_half = d_vals * 0.5
        d_big = d_x * 1e6
    stream.synchronize()
    ctl = slc.Controller(gpu_ctx, slc.Plant(ladder.A, ladder.B1, ladder.B2), [ladder.Sx, ladder.Su], nscen=nscen)
    ctl.load(d_vals, stream=s)

    def fetch(d_u, d_w):
        stream.synchronize()
        return d_u.cpu().numpy(), d_w.cpu().numpy()

    ua, wa = fetch(*_feed(ctl, d_x, stream=s))                      # (a)
    assert ctl.k == steps
    ur, wr = cc.reference(ladder, x)
    print("(a) rel err u", cc.check(ua, ur, "(a) u"), "ŵ", cc.check(wa, wr, "(a) ŵ"))
    ctl.reset(stream=s)                                            # (b)
    assert ctl.k == 0
    ub, wb = fetch(*_feed(ctl, d_x, stream=s))
    assert np.array_equal(ua, ub) and np.array_equal(wa, wb)
    ctl.reset(stream=s)                                            # (c)
    d_u, d_w = _feed(ctl, d_x[:20], stream=s)
    ctl.load(d_half, stream=s)
    assert ctl.k == 20
    d_u2, d_w2 = _feed(ctl, d_x[20:], stream=s)
    uc = np.concatenate([fetch(d_u, d_w)[0], fetch(d_u2, d_w2)[0]]); wc = np.concatenate([d_w.cpu().numpy(), d_w2.cpu().numpy()])
    ur, wr = cc.reference(ladder, x, switch=(20, 0.5))
    print("(c) rel err u", cc.check(uc, ur, "(c) u"), "ŵ", cc.check(wc, wr, "(c) ŵ"))
    assert np.array_equal(uc[:20], ua[:20]) and np.abs(uc[20:] - ua[20:]).max() > 1e-3
    ctl.load(d_vals, stream=s)                                     # (d)
    ctl.reset(stream=s)
    fetch(*_feed(ctl, d_big, stream=s))
    ctl.reset(stream=s)
    n = ladder.T + 2
    ud, wd = fetch(*_feed(ctl, d_x[:n], stream=s))
    fresh = slc.Controller(gpu_ctx, (ladder.Nx, ladder.Nu), [ladder.Sx, ladder.Su], nscen=nscen)
    fresh.load(d_vals, stream=s)
    uf, wf = fetch(*_feed(fresh, d_x[:n], stream=s))
    assert np.array_equal(ud, uf) and np.array_equal(wd, wf) and np.array_equal(ud, ua[:n])
    assert np.abs(ud).max() < 100                                  # nothing of the 1e6 run is left
    ctl.close(); fresh.close()


def _interleaved(ctl, Ad, Bd, x0, w):
    """step → synchronise → host float64 plant → upload, per step: x, u, ŵ as host arrays"""
    import torch
    d_x = _to_dev(x0)
    d_w = torch.empty_like(d_x)
    x = np.array(x0, dtype=np.float64)
    xs, us, ws = [], [], []
    for k in range(w.shape[0]):
        d_u = ctl.step(d_x, what=d_w)
        torch.cuda.synchronize()
        u = d_u.cpu().numpy()
        xs.append(x); us.append(u); ws.append(d_w.cpu().numpy())
        x = cc.plant_step(Ad, Bd, x, u, w[k])
        d_x.copy_(torch.from_numpy(x))
    return np.array(xs), np.array(us), np.array(ws)


@pytest.mark.parametrize("name", ["T2", "ladder"])
def test_interleaved_loop_with_a_nonlinear_plant(slc, gpu_ctx, name):
    """x⁺ = A·x + 0.25·tanh(x) + w + B₂·u on the host in float64, x_0 random: a plant the simulator cannot hold, against the
    long-double loop with the same plant"""
    case = cc.case(name)
    x0, w = cc.loop_inputs(name, cc.LOOP_STEPS[name])
    xr, ur, wr = cc.reference_loop(case, x0, w)
    ctl = _controller(slc, gpu_ctx, case, 3)
    x, u, what = _interleaved(ctl, *cc.dense_plant(case, np.float64), x0, w)
    print(f"{name} loop: rel err x {cc.check(x, xr, 'x'):.3e} u {cc.check(u, ur, 'u'):.3e} ŵ {cc.check(what, wr, 'ŵ'):.3e}, "
          f"max|x| {float(np.abs(xr).max()):.3f}")
    assert np.abs(ur).max() > 0.1
    ctl.close()


def test_readme_chain_end_to_end(slc, gpu_ctx, readme):
    """Plan.execute → Controller.load of that same device array.  The x of the simulator's impulse run (250 steps,
    w = δ(t−50)·e₃₀) replayed: u is the simulator's bit for bit in rows 0 … 248 and within 1e-8 of the committed fixture.  Then a
    plant that differs from the design model (A's super-diagonal 0.25 instead of 0.2) in the interleaved loop for 120 steps,
    against the long-double loop with the downloaded Φ."""
    import torch
    P, S, _ = readme
    plan = slc.Plan(gpu_ctx, P, S)
    d = plan.alloc_values()
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == 0)
    ctl = slc.Controller(gpu_ctx, P, S, nscen=1)
    ctl.load(d)
    loop = slc.ClosedLoop(gpu_ctx, P, S)
    assert ctl.n_entries == loop.n_entries
    steps = 250
    w = np.zeros((steps, P.Nw, 1)); w[49, 29, 0] = 1.0
    d_w = _to_dev(w)
    d_x = torch.full((steps, P.Nx, 1), float("nan"), dtype=torch.float64, device=_dev())
    d_usim = torch.full((steps, P.Nu, 1), float("nan"), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    loop.run(d, d_w.data_ptr(), steps, 1, d_x.data_ptr(), d_usim.data_ptr())
    torch.cuda.synchronize()
    d_u, _ = _feed(ctl, d_x, what=False)
    torch.cuda.synchronize()
    u, usim = d_u.cpu().numpy(), d_usim.cpu().numpy()
    assert np.array_equal(u[: steps - 1], usim[: steps - 1]) and np.abs(u).max() > 0.1
    g = np.load(os.path.join(GOLDEN, "readme_closed_loop.npz"))
    t0, n = int(g["t0"]), g["u"].shape[1]
    assert t0 + n == steps
    err = np.abs(u[t0:steps - 1, :, 0].T - g["u"][:, : n - 1]).max()
    print(f"README replay: max |u − fixture| {err:.3e}")
    assert err < 1e-8 and np.abs(u[:t0]).max() == 0
    # a plant that differs from the design model
    vx, vu = plan.download(d)
    case = cc.from_values(S[0], S[1], np.concatenate(vx + vu), B2=P.B2)
    A2 = (sp.identity(P.Nx) + sp.diags(0.25 * np.ones(P.Nx - 1), 1) - sp.diags(0.2 * np.ones(P.Nx - 1), -1)).tocsc()
    x0 = np.zeros((P.Nx, 1))
    w = np.zeros((120, P.Nx, 1)); w[10, 29, 0] = 1.0
    L = np.longdouble
    Ad, Bd = cc.dense_plant(case, L, A2)
    ref, xl = cc.Reference(case), np.zeros((P.Nx, 1), dtype=L)
    xr, ur = [], []
    for k in range(120):                                           # the linear mismatched plant in long double
        uu, _ = ref.step(xl)
        xr.append(xl); ur.append(uu)
        xl = Ad @ xl + np.asarray(w[k], dtype=L) + Bd @ uu
    xr, ur = np.array(xr), np.array(ur)
    assert 1.0 <= np.abs(xr).max() <= cc.GROWTH_BOUND and np.abs(xr[-1]).max() > 1e-6   # the mismatch leaves a tail the nominal loop kills
    ctl.reset()
    A64, B64 = cc.dense_plant(case, np.float64, A2)
    d_xk = _to_dev(x0)
    x = x0.copy()
    xs, us = [], []
    for k in range(120):
        d_uk = ctl.step(d_xk)
        torch.cuda.synchronize()
        uk = d_uk.cpu().numpy()
        xs.append(x); us.append(uk)
        x = A64 @ x + w[k] + B64 @ uk
        d_xk.copy_(torch.from_numpy(x))
    print(f"README mismatched plant: rel err x {cc.check(np.array(xs), xr, 'x'):.3e} u {cc.check(np.array(us), ur, 'u'):.3e}")
    ctl.close(); loop.close(); plan.close()


def test_error_paths_leave_the_controller_usable(slc, gpu_ctx):
    import torch
    case = cc.case("T2")
    SLS_EINVAL = slc._capi.SLS_EINVAL
    ctl = slc.Controller(gpu_ctx, (case.Nx, case.Nu), [case.Sx, case.Su], nscen=3)
    x = cc.random_x("T2", 6, 3)
    d_x = _to_dev(x)
    d_u = torch.empty((case.Nu, 3), dtype=torch.float64, device=_dev())
    with pytest.raises(slc.SLSError) as e:                          # a step before the first load
        ctl.step(d_x[0], u=d_u)
    assert e.value.code == SLS_EINVAL
    d_vals = _to_dev(case.values)
    ctl.load(d_vals)
    lib = slc.load_library()
    assert lib.sls_controller_step(ctl.handle, None, None, d_u.data_ptr(), None) == SLS_EINVAL        # null d_x
    assert lib.sls_controller_step(ctl.handle, None, d_x.data_ptr(), None, None) == SLS_EINVAL        # null d_u with Nu > 0
    assert ctl.k == 0                                               # a refused step does not count
    with pytest.raises(slc.SLSError) as e:
        slc.Controller(gpu_ctx, (case.Nx, case.Nu), [case.Sx, case.Su], nscen=0)
    assert e.value.code == SLS_EINVAL
    with pytest.raises(slc.SLSError) as e:
        slc.Controller(gpu_ctx, (case.Nx, case.Nu), [case.Sx, case.Su], nscen=1, dev_slot=5)
    assert e.value.code == SLS_EINVAL
    d_uall, d_w = _feed(ctl, d_x)
    torch.cuda.synchronize()
    ur, wr = cc.reference(case, x)
    cc.check(d_uall.cpu().numpy(), ur, "u after refusals"); cc.check(d_w.cpu().numpy(), wr, "ŵ after refusals")
    ctl.close()
