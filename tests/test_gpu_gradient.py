"""Multipliers and the gradient of the 𝓗₂ cost in A, B2 and the LQR diagonals on resident plans (SLS_PLAN_MULTIPLIERS,
sls_plan_gradient; csrc/sls_gradient.hip) against the reference of gradient_cases.py.

Bounds.  STATIONARITY and GRADIENT are, per case, 100× the larger of the figure measured once on an MI355X and the reference's own
(both are in DESIGN §3.18 and printed by `-s`); the gradient bound is relative to max|g| and never looser than 1e-6, the Φ contract.
The error follows residual / σ_min of the worst column, which differs per plant — hence per case.  The comparison of the device
with the host twin fed the device's own μ and z sums the same products in the same order: 4·N·2⁻⁵³·Σ|terms| per entry.  The finite
differences on the device use the host bound, 1e-7·max|fd| at step 1e-6.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import gradient_cases as gc
from son_cases import set_knobs

pytestmark = pytest.mark.gpu

HOMES = {"lds": {"SLS_VEC_LDS": "1"}, "global": {"SLS_VEC_GLOBAL": "1"}}          # where λ lives in the one-wave kernel
# ‖Eᵀμ − ∇J‖∞ / max|∇J|, measured on an MI355X (the same in both homes of λ) | the reference's own → bound = 100 × the larger
#   chain17 6.4e-15 | 1.2e-13    T1 3.7e-16 | 4.6e-15    T2 2.2e-16 | 1.2e-15    weighted 3.6e-15 | 6.4e-14
#   full32  1.1e-16 | 1.0e-15    groups 1.5e-14 | 1.0e-13    infeasible 1.3e-14 | 2.8e-13
STATIONARITY = {"chain17": 1.3e-11, "T1": 4.6e-13, "T2": 1.3e-13, "weighted": 6.4e-12, "full32": 1.0e-13, "groups": 1.1e-11,
                "infeasible": 2.8e-11}
# worst |g − g_reference| / max|g| over gA, gB2, gc1, gd12, measured the same way → bound = 100 × that (each far inside 1e-6):
#   chain17 9.0e-12    T1 2.7e-14    T2 2.2e-14    weighted 1.2e-12    full32 1.9e-14    groups 5.1e-12    infeasible 1.1e-11
GRADIENT = {"chain17": 9.0e-10, "T1": 2.7e-12, "T2": 2.2e-12, "weighted": 1.2e-10, "full32": 1.9e-12, "groups": 5.1e-10,
            "infeasible": 1.1e-9}
UPDATABLE = ("chain17", "T1", "T2", "full32", "groups", "infeasible")            # default weights: the plan can take the flag


def _torch():
    import torch
    return torch


class Run:
    """A flagged plan of a case with its value array (a torch tensor, mask order or packed), executed once."""

    def __init__(self, slc, ctx, name, packed=False, updatable=None, P=None):
        torch = _torch()
        cs = gc.case(slc, name)
        self.cs, self.name, self.packed = cs, name, packed
        upd = (name in UPDATABLE) if updatable is None else updatable
        self.plan = slc.Plan(ctx, P or cs["P"], cs["S"], groups=cs["I"], multipliers=True, updatable_weights=upd)
        self.upd = upd
        n = self.plan.info["n_packed"] if packed else self.plan.info["n_values"]
        self.vals = torch.zeros(max(n, 1), dtype=torch.float64, device=f"cuda:{self.plan.info['device']}")
        self.dv = self.vals.data_ptr()

    def execute(self):
        self.plan.execute(self.dv, packed=self.packed); self.plan.synchronize()
        return self

    def gradient(self, **kw):
        return self.plan.gradient_values(self.dv, packed=self.packed, weights=self.upd, **kw)

    def close(self):
        self.plan.close()


@pytest.fixture
def run(slc, gpu_ctx, monkeypatch):
    made = []

    def make(name, env=None, **kw):
        set_knobs(monkeypatch, env or {})
        r = Run(slc, gpu_ctx, name, **kw)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


@pytest.mark.parametrize("home", list(HOMES))
@pytest.mark.parametrize("name", gc.NAMES)
def test_multipliers_and_gradient_against_the_reference(slc, run, name, home):
    ref, cs = gc.reference(slc, name), gc.case(slc, name)
    r = run(name, HOMES[home]).execute()
    desc = r.plan.describe()
    assert "h2_column_wave_kernel" in desc and "twisted" not in desc and "tile" not in desc, desc
    status = r.plan.fetch_status()[0]
    live = np.isin(status, (0, 3))
    assert np.array_equal(live, ref["live"]), (status, ref["resid"])
    out = r.gradient()
    gA, gB, nskip = out[0], out[1], out[-1]
    assert nskip == int((~ref["live"]).sum())
    # stationarity of the device's own multipliers at the device's own Φ
    vx, vu = r.plan.download(r.dv)
    zs = gc.solutions_from_values(slc, name, vx, vu)
    mus = [r.plan.multipliers(q) for q in range(len(zs))]
    for q, cp in enumerate(ref["cps"]):
        assert mus[q].shape == (cs["T"] + 1, cp["n"])
    stat = max(gc.stationarity(cp, mus[q], zs[q]) for q, cp in enumerate(ref["cps"]) if ref["live"][q] and zs[q].size)
    errs = {k: float(np.abs(g - ref[k]).max() / np.abs(ref[k]).max()) for k, g in (("gA", gA), ("gB2", gB))}
    if r.upd:
        errs.update({k: float(np.abs(g - ref[k]).max() / np.abs(ref[k]).max()) for k, g in (("gc1", out[2]), ("gd12", out[3]))})
    print(f"{name}/{home}: stationarity {stat:.2e} (reference {ref['stationarity']:.2e}); gradient errors relative to max|g| "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert stat <= STATIONARITY[name]
    assert max(errs.values()) <= GRADIENT[name] <= 1e-6, errs
    # the device against the host twin fed the device's own μ and z: the same products in the same order
    hA, hB, bd = slc.gradient_host(cs["P"], cs["S"], mus, vx, vu, cs["I"], col_status=status, return_bound=True)
    for got, want, n, s in ((gA, hA, bd["terms_A"], bd["abs_A"]), (gB, hB, bd["terms_B2"], bd["abs_B2"])):
        assert np.all(np.abs(got - want) <= 4.0 * n * 2.0 ** -53 * s), float(np.abs(got - want).max())
    # a second call gives the same bits; so does the device path into fresh tensors
    again = r.gradient()
    assert all(np.array_equal(a, b) for a, b in zip(out[:-1], again[:-1]))
    dev = r.plan.gradient(r.dv, weights=r.upd)
    r.plan.synchronize()
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(out[:-1], dev))


@pytest.mark.parametrize("name", ["chain17", "groups", "infeasible"])
def test_packed_layout_gives_the_same_bits(slc, run, name):
    a = run(name).execute()
    b = run(name, packed=True).execute()
    ga, gb = a.gradient(), b.gradient()
    assert len(ga) == len(gb) and all(np.array_equal(x, y) for x, y in zip(ga[:-1], gb[:-1])) and ga[-1] == gb[-1]
    for q in (0, len(gc.reference(slc, name)["cps"]) - 1):
        assert np.array_equal(a.plan.multipliers(q), b.plan.multipliers(q))


def test_column_weights(slc, run):
    torch = _torch()
    ref, cs = gc.reference(slc, "chain17"), gc.case(slc, "chain17")
    r = run("chain17").execute()
    base = r.gradient()
    n = len(ref["cps"])
    ones = r.gradient(column_weights=np.ones(n))
    assert all(np.array_equal(x, y) for x, y in zip(base[:-1], ones[:-1]))
    total = [np.zeros_like(g) for g in base[:-1]]
    for j in range(n):
        e = np.zeros(n); e[j] = 1.0
        own = r.gradient(column_weights=e)
        live_j = np.zeros(n, dtype=bool); live_j[j] = True
        want = gc.gradient_from(cs["P"], ref["cps"], ref["mu"], ref["z"], live_j)
        for got, w, full in zip(own[:-1], want, (ref["gA"], ref["gB2"], ref["gc1"], ref["gd12"])):
            assert np.abs(got - w).max() <= GRADIENT["chain17"] * np.abs(full).max()
        # an entry outside the column's index sets gets exactly 0 from it
        assert np.all(own[0][want[0] == 0.0] == 0.0)
        total = [t + g for t, g in zip(total, own[:-1])]
    for t, g in zip(total, base[:-1]):
        assert np.abs(t - g).max() <= 64 * 2.0 ** -53 * np.abs(g).max() * n
    cw = torch.full((n,), 2.0, dtype=torch.float64, device=r.vals.device)
    dev = r.plan.gradient(r.dv, column_weights=cw)
    r.plan.synchronize()
    assert np.array_equal(dev[0].cpu().numpy(), 2.0 * base[0]) and np.array_equal(dev[1].cpu().numpy(), 2.0 * base[1])


def test_a_workgroup_that_solves_several_columns(slc, gpu_ctx, monkeypatch):
    """300 columns on 150 workgroups (SLS_MAX_PER_CU=1 on 256 CUs, as tests/test_gpu_column_reuse.py forces it): the second column
    of a workgroup must land in its own multiplier slot.  Against the same plan with grid == nsub, bit for bit."""
    torch = _torch()
    P = slc.workloads.chain_plant(300)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 9, 12, 1.5))
    got = {}
    for tag, env in (("reuse", {"SLS_MAX_PER_CU": "1"}), ("lifted", {})):
        set_knobs(monkeypatch, env)
        plan = slc.Plan(gpu_ctx, P, S, multipliers=True)
        try:
            vals = torch.zeros(plan.info["n_values"], dtype=torch.float64, device="cuda:0")
            plan.execute(vals.data_ptr()); plan.synchronize()
            gA, gB, nskip = plan.gradient_values(vals.data_ptr())
            got[tag] = dict(desc=plan.describe(), gA=gA, gB=gB, nskip=nskip, mu=[plan.multipliers(q) for q in (0, 149, 150, 151, 299)])
        finally:
            plan.close()
    assert "nsub=300 grid=150" in got["reuse"]["desc"] and "nsub=300 grid=300" in got["lifted"]["desc"], got["reuse"]["desc"]
    assert got["reuse"]["nskip"] == got["lifted"]["nskip"] == 0
    assert np.array_equal(got["reuse"]["gA"], got["lifted"]["gA"]) and np.array_equal(got["reuse"]["gB"], got["lifted"]["gB"])
    assert all(np.array_equal(a, b) for a, b in zip(got["reuse"]["mu"], got["lifted"]["mu"]))
    assert np.abs(got["reuse"]["gA"]).max() > 0 and all(np.abs(m).max() > 0 for m in got["reuse"]["mu"])


def _changed(cs, k_list, rel=1e-3):
    A = gc._csc(cs["P"].A).data.copy()
    for k in k_list:
        A[k] *= 1.0 + rel
    return A


def test_partial_execute_equals_full_execute(slc, run):
    """update_plant of three entries, then execute_dirty + gradient against a full execute + gradient: the same bits."""
    cs = gc.case(slc, "chain17")
    newA = _changed(cs, (3, 20, 41))
    a = run("chain17").execute()
    a.plan.track_changes(True)
    a.plan.update_plant(A=newA)
    nsolved = a.plan.execute_dirty(a.dv); a.plan.synchronize()
    assert 0 < nsolved <= 17
    b = run("chain17").execute()
    b.plan.update_plant(A=newA)
    b.execute()
    ga, gb = a.gradient(), b.gradient()
    assert all(np.array_equal(x, y) for x, y in zip(ga[:-1], gb[:-1]))
    assert all(np.array_equal(a.plan.multipliers(q), b.plan.multipliers(q)) for q in range(17))
    assert not np.array_equal(ga[0], gc.reference(slc, "chain17")["gA"])


def test_finite_differences_on_the_device(slc, run):
    """update_plant ± 1e-6 → execute → objective total, for five entries of A and two of B2 spread over the magnitudes of the
    reference's gradient (the largest included), under the host bound 1e-7·max|fd|."""
    cs, ref = gc.case(slc, "chain17"), gc.reference(slc, "chain17")
    r = run("chain17").execute()
    gA, gB = r.gradient()[:2]
    A0, B0 = gc._csc(cs["P"].A).data.copy(), gc._csc(cs["P"].B2).data.copy()
    oa, ob = np.argsort(-np.abs(ref["gA"])), np.argsort(-np.abs(ref["gB2"]))
    picks = [("A", int(oa[i])) for i in (0, len(oa) // 4, len(oa) // 2, 3 * len(oa) // 4, len(oa) - 1)] + [("B2", int(ob[0])), ("B2", int(ob[-1]))]
    h, fd, g = 1e-6, [], []
    for which, k in picks:
        tot = []
        for s in (1.0, -1.0):
            A, B = A0.copy(), B0.copy()
            (A if which == "A" else B)[k] += s * h
            r.plan.update_plant(A=A, B2=B)
            r.execute()
            tot.append(r.plan.objective_values(r.dv)[1])
        fd.append((tot[0] - tot[1]) / (2 * h)); g.append((gA if which == "A" else gB)[k])
    fd, g = np.array(fd), np.array(g)
    print("device finite differences:", np.abs(fd - g).max(), "against max|fd|", np.abs(fd).max(), "per entry", np.abs(fd - g))
    assert np.abs(fd - g).max() <= 1e-7 * np.abs(fd).max()


def test_h2_cost_layer(slc, run):
    torch = _torch()
    cs = gc.case(slc, "chain17")
    r = run("chain17")
    dev = r.vals.device
    A = torch.tensor(gc._csc(cs["P"].A).data, dtype=torch.float64, device=dev, requires_grad=True)
    B2 = torch.tensor(gc._csc(cs["P"].B2).data, dtype=torch.float64, device=dev, requires_grad=True)
    c1 = torch.ones(cs["P"].Nx, dtype=torch.float64, device=dev, requires_grad=True)
    J = slc.h2_cost(r.plan, r.vals, A=A, B2=B2, c1=c1)
    assert J.dim() == 0
    (3.0 * J).backward()
    torch.cuda.synchronize()
    want = r.gradient()
    assert abs(J.item() - r.plan.objective_values(r.dv)[1]) == 0.0
    assert np.array_equal(A.grad.cpu().numpy(), 3.0 * want[0]) and np.array_equal(B2.grad.cpu().numpy(), 3.0 * want[1])
    assert np.array_equal(c1.grad.cpu().numpy(), 3.0 * want[2])
    # ten steps of plain gradient descent on B2's values lower the total monotonically
    b = B2.detach().clone().requires_grad_(True)
    lr, costs = None, []
    for _ in range(10):
        J = slc.h2_cost(r.plan, r.vals, B2=b)
        J.backward()
        costs.append(J.item())
        if lr is None:
            lr = 0.02 / float(b.grad.abs().max())
        with torch.no_grad():
            b -= lr * b.grad
        b.grad = None
    costs.append(slc.h2_cost(r.plan, r.vals, B2=b).item())
    print("gradient descent on B2:", costs)
    assert all(c1_ < c0_ for c0_, c1_ in zip(costs, costs[1:]))


def test_error_paths(slc, gpu_ctx, monkeypatch):
    torch = _torch()
    set_knobs(monkeypatch, {})
    cs = gc.case(slc, "chain17")
    vals = torch.zeros(1 << 16, dtype=torch.float64, device="cuda:0")
    plain = slc.Plan(gpu_ctx, cs["P"], cs["S"])
    try:
        plain.execute(vals.data_ptr()); plain.synchronize()
        with pytest.raises(slc.SLSError) as e:
            plain.gradient_values(vals.data_ptr())
        assert e.value.code == slc._capi.SLS_EINVAL
        with pytest.raises(slc.SLSError) as e:
            plain.multipliers(0)
        assert e.value.code == slc._capi.SLS_EINVAL
    finally:
        plain.close()
    flagged = slc.Plan(gpu_ctx, cs["P"], cs["S"], multipliers=True)
    try:
        with pytest.raises(slc.SLSError) as e:                                   # before the first execute
            flagged.gradient_values(vals.data_ptr())
        assert e.value.code == slc._capi.SLS_EINVAL
        flagged.execute(vals.data_ptr()); flagged.synchronize()
        with pytest.raises(slc.SLSError) as e:                                   # gc1 without updatable weights
            flagged.gradient_values(vals.data_ptr(), weights=True)
        assert e.value.code == slc._capi.SLS_EINVAL
        with pytest.raises(slc.SLSError) as e:                                   # the tile pass would leave stale multipliers
            flagged.refine(vals.data_ptr())
        assert e.value.code == slc._capi.SLS_EUNSUPPORTED
        assert len(flagged.gradient_values(vals.data_ptr())) == 3
    finally:
        flagged.close()
    # a column beyond the 32-lane classes
    P = slc.workloads.chain_plant(120)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 20, 14, 1.5))
    with pytest.raises(slc.SLSError) as e:
        slc.Plan(gpu_ctx, P, S, multipliers=True)
    assert e.value.code == slc._capi.SLS_EUNSUPPORTED and "tile kernel" in str(e.value)
    with pytest.raises(slc.SLSError) as e:
        slc.Plan(gpu_ctx, cs["P"], cs["S"], multipliers=True, objective="sum_of_norms")
    assert e.value.code == slc._capi.SLS_EUNSUPPORTED
    # the one-shot call keeps no plan
    import ctypes as C
    m = slc._capi.Marshalled(cs["P"], cs["S"][0], cs["S"][1], None, flags=slc._capi.SLS_PLAN_MULTIPLIERS)
    T = cs["T"]
    dp = C.POINTER(C.c_double)
    bx = [np.zeros(max(n, 1)) for n in m.nnz_x]; bu = [np.zeros(max(n, 1)) for n in m.nnz_u]
    px = (dp * T)(*[a.ctypes.data_as(dp) for a in bx]); pu = (dp * T)(*[a.ctypes.data_as(dp) for a in bu])
    rc = gpu_ctx._lib.sls_h2_sf_solve(gpu_ctx.handle, *m.common_args(), px, pu, None, None)
    assert rc == slc._capi.SLS_EUNSUPPORTED
