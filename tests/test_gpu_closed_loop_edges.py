"""GPU tests of the closed-loop simulator (csrc/sls_closed_loop.hip) at its structural edges: every lane layout
closed_loop_step_kernel<SCN> is instantiated for, full and with a ragged last chunk, on an operator whose rows sit on either
side of every boundary of the `fir` lambda's unrolled and tail loops (the ladder of tests/closed_loop_cases.py; the host twin
tests/test_closed_loop_host.py asserts that the rows are there); the state sls_closed_loop_run keeps between runs (ŵ buffer and
its capacity, the cached hipGraph and its key, the plain-launch path of steps < 3); T = 1, T = 2 and a plant without actuators.

Reference: the long-double dense restatement of the recursion, for EVERY scenario.  Tolerance: the one of
test_gpu_closed_loop.py, 1e-11 relative to max(1, max|reference|), for x and u separately.

Largest relative error of the layout test on an MI355X, per lane layout (x / u), against the tolerance of 1e-11:
    SCN  1: 1.7e-16 / 1.6e-16      SCN  2: 1.6e-16 / 1.7e-16      SCN  4: 1.6e-16 / 1.8e-16      SCN  8: 1.6e-16 / 2.9e-16
    SCN 16: 1.6e-16 / 2.2e-16      SCN 32: 1.9e-16 / 3.2e-16      SCN 64: 1.4e-16 / 5.2e-16
A few units in the last place of FP64: the tolerance is never approached.  The run sequence and the edge operators stay below
2.2e-16.  (The tests print each figure before they assert: run with -s.)
"""
import numpy as np
import pytest

import closed_loop_cases as clc

pytestmark = pytest.mark.gpu
RTOL = 1e-11
NSCEN_MAX = 130


def _scn(nscen):
    scn = 1
    while scn < 64 and scn < nscen:
        scn <<= 1
    return scn


@pytest.fixture(scope="module")
def ladder():
    return clc.ladder()


@pytest.fixture(scope="module")
def ladder_run(ladder):
    """One disturbance and one reference for all layouts: scenarios do not interact, so a run on the first n of the 130
    scenarios must equal the first n of the reference."""
    w = clc.ladder_w(NSCEN_MAX)
    x, u = clc.reference(ladder, w)
    w.setflags(write=False); x.setflags(write=False); u.setflags(write=False)
    return w, x, u


def _device_values(case):
    import torch
    return torch.from_numpy(case.values.copy()).to(torch.device("cuda:0"))


def _check(x, u, xr, ur, what):
    assert x.shape == xr.shape and u.shape == ur.shape, what
    assert np.isfinite(x).all() and np.isfinite(u).all(), what
    ex, eu = clc.rel_err(x, xr), clc.rel_err(u, ur)
    print(f"{what}: rel err x {ex:.3e} u {eu:.3e}")
    for s in range(x.shape[2]):                                   # every scenario, each against its own magnitude
        assert clc.rel_err(x[:, :, s], xr[:, :, s]) < RTOL, (what, s)
        assert clc.rel_err(u[:, :, s], ur[:, :, s]) < RTOL, (what, s)
    return ex, eu


@pytest.mark.parametrize("nscen", [1, 2, 3, 4, 7, 16, 17, 32, 33, 64, 65, 130])
def test_every_lane_layout_on_the_ladder(slc, gpu_ctx, ladder, ladder_run, nscen):
    """SCN = 1, 2, 4, 8, 16, 32, 64, each with all scenario slots live and with dead lanes in the last chunk; 130 scenarios
    are three chunks in grid.y.  Every row length of the ladder, every scenario."""
    w, xr, ur = ladder_run
    loop = slc.ClosedLoop(gpu_ctx, slc.Plant(ladder.A, ladder.B1, ladder.B2), [ladder.Sx, ladder.Su])
    assert loop.n_entries == ladder.n_entries
    d_vals = _device_values(ladder)
    x, u = loop.simulate(d_vals.data_ptr(), np.ascontiguousarray(w[:, :, :nscen]), steps=ladder.steps)
    _check(x, u, xr[:, :, :nscen], ur[:, :, :nscen], f"ladder nscen={nscen} SCN={_scn(nscen)}")
    assert np.abs(u[:, 0]).max() == 0                              # the actuator with an empty operator row
    assert np.abs(u[:, clc.LADDER_ORPHAN]).max() > 0               # the one that drives no state is still reported
    loop.close()


def test_run_sequence_on_one_loop(slc, gpu_ctx, ladder):
    """What sls_closed_loop_run keeps between runs, through the device-pointer entry on a non-default stream: capture,
    replay, new contents behind unchanged pointers, a larger problem (ŵ grows, new key), a smaller one (stale history behind
    the live part), the plain launches of steps < 3, the first key again, no disturbance, and a key that run_host dropped."""
    import torch
    dev = torch.device("cuda:0")
    Nx, Nu, Nw = ladder.Nx, ladder.Nu, ladder.Nw
    loop = slc.ClosedLoop(gpu_ctx, slc.Plant(ladder.A, ladder.B1, ladder.B2), [ladder.Sx, ladder.Su])
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(99)
    d_vals = _device_values(ladder)
    scale = 1.0

    class Buffers:
        def __init__(self, steps, nscen):
            self.steps, self.nscen = steps, nscen
            self.w = torch.empty((steps, Nw, nscen), dtype=torch.float64, device=dev)
            self.x = torch.empty((steps, Nx, nscen), dtype=torch.float64, device=dev)
            self.u = torch.empty((steps, Nu, nscen), dtype=torch.float64, device=dev)
            self.refill()

        def refill(self):
            self.hw = rng.standard_normal((self.steps, Nw, self.nscen))
            self.w.copy_(torch.from_numpy(self.hw))

    def run(b, what, with_w=True):
        b.x.fill_(float("nan")); b.u.fill_(float("nan"))
        torch.cuda.synchronize()
        loop.run(d_vals.data_ptr(), b.w.data_ptr() if with_w else None, b.steps, b.nscen, b.x.data_ptr(), b.u.data_ptr(),
                 stream=stream.cuda_stream)
        stream.synchronize()
        x, u = b.x.cpu().numpy(), b.u.cpu().numpy()
        xr, ur = clc.reference(ladder, b.hw if with_w else None, steps=b.steps, nscen=b.nscen, scale=scale)
        _check(x, u, xr, ur, what)
        return x, u

    a = Buffers(40, 3)
    xa, _ = run(a, "(a) capture")
    xb, _ = run(a, "(b) replay")
    assert np.array_equal(xa, xb)
    d_vals.mul_(0.5); scale = 0.5                                   # exact in FP64: the reference's Φ·0.5 is the device's
    a.refill()
    xc, _ = run(a, "(c) new Φ and w behind the same pointers")
    assert np.abs(xc - xb).max() > 1e-3                             # the result followed the contents
    d = Buffers(40, 17)
    run(d, "(d) larger: ŵ grows, new key")
    e = Buffers(10, 2)
    run(e, "(e) smaller: stale history behind the live part")
    for steps in (2, 1):                                            # (f) plain launches
        f = Buffers(steps, 3)
        x, u = run(f, f"(f) steps={steps}")
        assert not x[0].any() and not u[-1].any()
    run(a, "(g) the first key again")
    h = Buffers(8, 3)
    x, u = run(h, "(h) no disturbance", with_w=False)
    assert not x.any() and not u.any()
    xs, us = loop.simulate(d_vals.data_ptr(), a.hw, steps=a.steps)  # (i) run_host destroys the graph …
    xr, ur = clc.reference(ladder, a.hw, steps=a.steps, scale=scale)
    _check(xs, us, xr, ur, "(i) simulate")
    xi, _ = run(a, "(i) the first key after run_host dropped its graph")   # … and the earlier key captures afresh
    assert np.array_equal(xi, xs)
    assert loop.last_ms() > 0
    loop.close()


@pytest.mark.parametrize("nscen", [1, 5])
@pytest.mark.parametrize("name", clc.SMALL)
def test_edge_operators(slc, gpu_ctx, name, nscen):
    """T = 1 (no β entries, min(t, T−1) = 0), T = 2, and a plant without actuators (B₂ is Nx × 0)."""
    case = clc.small_case(name)
    w = clc.small_w(5)[:, :, :nscen]
    xr, ur = clc.reference(case, w)
    loop = slc.ClosedLoop(gpu_ctx, slc.Plant(case.A, case.B1, case.B2), [case.Sx, case.Su])
    assert loop.n_entries == case.n_entries
    d_vals = _device_values(case)
    x, u = loop.simulate(d_vals.data_ptr(), np.ascontiguousarray(w), steps=case.steps)
    assert u.shape == (case.steps, case.Nu, nscen)
    _check(x, u, xr, ur, f"{name} nscen={nscen}")
    assert np.abs(x).max() > 0
    loop.close()
