"""sls_plan_update_weights on the device: a resident plan built with SLS_PLAN_WEIGHTS_UPDATABLE re-solves for new LQR weights
C1 = [diag(c); 0], D12 = [0; diag(d)] without a rebuild.

Cases (tests/weights_cases.py: those of tests/update_cases.py, each asserting its route through Plan.describe()): `t4`, `t4_long`,
`t4_zeros`, `t2`, `wave`, `tile`, the localized plan of chain_plant(70) (masks and references of `wave`), and `son` (fresh-plan
comparison and statuses only).  All plans carry the flag.  The reference is the NumPy oracle with the weights.

Per case: (a) the base solve on weighted(P, 11) is within oracle_c.TOL of the oracle, all statuses OK; (b) after update_weights to
seed 12 the next execute is within TOL of the oracle on weighted(P, 12), Φ moved by more than 1e-3, update_weights_result() == 0;
(c) a fresh flagged plan on weighted(P, 12) is executed twice and, if its two results are bitwise equal (judged on the fresh plan,
not on the code under test), the updated plan's Φ and statuses equal them bitwise; (d) objective_values after the update agrees with
objective_values_host on the new plant within objective_cases.summation_bound; (e) updating back gives bitwise the Φ of (a); (f) the
device path (torch tensors) gives bitwise the host path's Φ; (g) one half at a time: C1 on the device path, then D12 on the host
path.

Φ moves by 0.36 (`tile`) to 5.5 (`wave`) between the seeds against TOL = 1e-8: an update that did nothing fails (b)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import objective_cases as oc
import update_cases as uc
import weights_cases as wc
from oracle_c import TOL

pytestmark = pytest.mark.gpu

A, B = wc.SEED_A, wc.SEED_B


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _phi(plan, dv):
    plan.execute(dv); plan.synchronize()
    return np.concatenate(sum(plan.download(dv), []))


def _build(slc, ctx, cid, P, localized=False, flagged=True):
    _, S, groups, _, _, objective = uc.case(slc, cid)
    if localized:
        d, T, alpha = uc.CASES[cid][2]
        return slc.Plan.localized(ctx, P, d, T, alpha, updatable_weights=flagged)
    return slc.Plan(ctx, P, S, groups, objective=objective, updatable_weights=flagged)


def _run_case(slc, ctx, monkeypatch, cid, localized=False):
    P, S, groups, knobs, route, objective = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, {} if localized else knobs)
    PA, PB = wc.weighted(P, A), wc.weighted(P, B)
    (cA, dA), (cB, dB) = wc.diagonals(P, A), wc.diagonals(P, B)
    with_oracle = objective == "h2"
    plan = fresh = None
    try:
        plan = _build(slc, ctx, cid, PA, localized)
        desc = plan.describe()
        assert (desc.startswith("h2_column_") if localized else route in desc), desc
        dv = plan.alloc_values()
        # (a) base solve
        phi0 = _phi(plan, dv)
        st0 = plan.fetch_status()[0].copy()
        assert not with_oracle or np.all(st0 == 0), st0
        if with_oracle:
            e0 = np.abs(phi0 - wc.oracle_flat(slc, cid, A)).max()
            print(f"{cid}: {desc} base max |Φ − Φ_oracle| = {e0:.2e}")
            assert e0 < TOL
        assert all(np.array_equal(g, w) for g, w in zip(plan.weights(), (cA, dA)))
        # (b) updated solve, host path: a scipy matrix for C1, a 1-D array for D12
        plan.update_weights(C1=PB.C1, D12=dB)
        phi1 = _phi(plan, dv)
        st1 = plan.fetch_status()[0].copy()
        assert (not with_oracle or np.all(st1 == 0)) and plan.update_weights_result() == 0
        moved = np.abs(phi1 - phi0).max()
        print(f"{cid}: the update moved Φ by {moved:.3g}")
        assert moved > 1e-3
        if with_oracle:
            e1 = np.abs(phi1 - wc.oracle_flat(slc, cid, B)).max()
            print(f"{cid}: updated max |Φ − Φ_oracle| = {e1:.2e}")
            assert e1 < TOL
        assert all(np.array_equal(g, w) for g, w in zip(plan.weights(), (cB, dB)))
        # (d) objective after the update
        vx, vu = plan.download(dv)
        col, tot = plan.objective_values(dv)
        hcol, htot, n_terms, abs_sum = slc.objective_values_host(PB, S, vx, vu, None if localized else groups, objective=objective, return_bound=True)
        bound = oc.summation_bound(n_terms, abs_sum)
        print(f"{cid}: objective worst |Δ|/bound {(np.abs(col - hcol) / np.maximum(bound, 1e-300)).max():.3g}")
        assert np.all(np.abs(col - hcol) <= bound)
        assert abs(tot - htot) <= bound.sum() + 2 * len(col) * oc.U * np.abs(hcol).sum()
        # (c) bitwise against a fresh flagged plan on weighted(P, 12)
        fresh = _build(slc, ctx, cid, PB, localized)
        assert fresh.describe() == desc
        fv = fresh.alloc_values()
        f1 = _phi(fresh, fv); f2 = _phi(fresh, fv)
        assert np.array_equal(fresh.fetch_status()[0], st1)
        if np.array_equal(f1, f2):
            assert np.array_equal(phi1, f1), np.abs(phi1 - f1).max()
        else:
            print(f"{cid}: the fresh plan does not repeat bitwise ({np.abs(f1 - f2).max():.2e}): bitwise comparison not applicable")
        # (e) round trip
        plan.update_weights(C1=cA, D12=PA.D12)
        assert np.array_equal(_phi(plan, dv), phi0)
        # (f) the device path
        plan.update_weights(C1=_dev(cB), D12=_dev(dB))
        phi1d = _phi(plan, dv)
        assert plan.update_weights_result() == 0 and np.array_equal(plan.fetch_status()[0], st1)
        assert np.array_equal(phi1d, phi1), np.abs(phi1d - phi1).max()
        # (g) one half at a time: C1 back on the device path, then D12 on the host path, ends at seed 11
        plan.update_weights(C1=_dev(cA))
        plan.update_weights(D12=dA)
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_weights_result() == 0
    finally:
        for p in (plan, fresh):
            if p is not None:
                p.close()


@pytest.mark.parametrize("cid", list(wc.CASES))
def test_updated_plan_solves_the_reweighted_problem(slc, gpu_ctx, monkeypatch, cid):
    _run_case(slc, gpu_ctx, monkeypatch, cid)


def test_updated_localized_plan_solves_the_reweighted_problem(slc, gpu_ctx, monkeypatch):
    """Plan.localized(..., updatable_weights=True) on chain_plant(70), d 9, T 7, α 1.5: masks and references of the `wave` case."""
    _run_case(slc, gpu_ctx, monkeypatch, "wave", localized=True)


# ---- four-wave records ----

@pytest.mark.parametrize("cid", ["t4", "t4_zeros"])
def test_four_wave_plan_time_data_equals_a_fresh_plans(slc, gpu_ctx, monkeypatch, cid):
    """After an update the prepared records (twisted4_tables), the setup images with the weight table Wx (twisted4_images) and the
    static blocks S_k (twisted4_static) are, byte for byte, those of a fresh flagged plan on the re-weighted plant — on both paths; the weight table differs from the one
    before the update."""
    P, S, groups, knobs, route, _ = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, knobs)
    PA, PB = wc.weighted(P, A), wc.weighted(P, B)
    cB, dB = wc.diagonals(P, B)
    plan = slc.Plan(gpu_ctx, PA, S, groups, updatable_weights=True)
    fresh = slc.Plan(gpu_ctx, PB, S, groups, updatable_weights=True)
    try:
        assert route in plan.describe()

        def same(x, y):
            if isinstance(x, dict):
                return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
            if isinstance(x, (tuple, list)):
                return len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
            if isinstance(x, np.ndarray):
                return x.shape == y.shape and x.tobytes() == y.tobytes()
            return x == y
        before = (plan.twisted4_tables(), plan.twisted4_images(), plan.twisted4_static())
        want = (fresh.twisted4_tables(), fresh.twisted4_images(), fresh.twisted4_static())
        assert not same(before[1], want[1])
        for path in ("host", "device"):
            if path == "host":
                plan.update_weights(C1=cB, D12=dB)
            else:
                plan.update_weights(C1=PA.C1, D12=PA.D12)                      # back first, so that the device path has work to do
                plan.update_weights(C1=_dev(cB), D12=_dev(dB))
            assert plan.update_weights_result() == 0
            after = (plan.twisted4_tables(), plan.twisted4_images(), plan.twisted4_static())
            assert same(after[0], want[0]) and same(after[1], want[1]) and same(after[2], want[2]), path
    finally:
        plan.close(); fresh.close()


# ---- a flagged identity plan against an unflagged one ----

@pytest.mark.parametrize("cid", ["t4", "wave", "tile"])
def test_flagged_identity_plan_agrees_with_an_unflagged_one(slc, gpu_ctx, monkeypatch, cid):
    """Identity weights: the flagged plan solves with has_w = 1 records (hinv = 1), the unflagged one with none.  The two Φ agree
    within TOL; bitwise equality is not required (DESIGN §3.13 says where it was observed)."""
    P, S, groups, knobs, route, _ = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, knobs)
    plans = [slc.Plan(gpu_ctx, P, S, groups, updatable_weights=f) for f in (True, False)]
    try:
        assert plans[0].describe() == plans[1].describe() and route in plans[0].describe()
        phis = [_phi(p, p.alloc_values()) for p in plans]
        assert all(np.all(p.fetch_status()[0] == 0) for p in plans)
        print(f"{cid}: flagged vs unflagged max |ΔΦ| = {np.abs(phis[0] - phis[1]).max():.2e}, bitwise equal: {np.array_equal(*phis)}")
        assert np.abs(phis[0] - phis[1]).max() < TOL
        assert all(np.array_equal(g, np.ones(n)) for g, n in zip(plans[0].weights(), (P.Nx, P.Nu)))
    finally:
        for p in plans:
            p.close()


# ---- refused values, refused calls, malformed arguments ----

@pytest.mark.parametrize("bad", [0.0, np.nan, np.inf])
def test_refused_values_on_both_paths(slc, gpu_ctx, monkeypatch, bad):
    """One value of C1's new diagonal breaks the value rule.  Host path: SLSError (SLS_EINVAL) that names the position, the plan
    untouched — the next execute bitwise as before.  Device path: update_weights_result() == 1, that variable keeps its old records
    and every other value is applied — Φ equals a fresh plan's on the diagonal with that value put back."""
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    (cA, dA), (cB, dB) = wc.diagonals(P, A), wc.diagonals(P, B)
    k = 34                                                    # a state inside the index set of column 35
    plan = slc.Plan(gpu_ctx, wc.weighted(P, A), S, groups, updatable_weights=True)
    fresh = None
    try:
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        c = cB.copy(); c[k] = bad
        with pytest.raises(slc._capi.SLSError) as ei:
            plan.update_weights(C1=c, D12=dB)
        assert ei.value.code == slc._capi.SLS_EINVAL and f"C1 diagonal position {k} " in str(ei.value), str(ei.value)
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_weights_result() == 0
        assert all(np.array_equal(g, w) for g, w in zip(plan.weights(), (cA, dA)))
        plan.update_weights(C1=_dev(c), D12=_dev(dB))
        got = _phi(plan, dv)
        assert plan.update_weights_result() == 1 and np.all(plan.fetch_status()[0] == 0)
        kept = c.copy(); kept[k] = cA[k]
        hc, hd = plan.weights()
        assert np.array_equal(hc.view(np.uint64), kept.view(np.uint64)) and np.array_equal(hd, dB)
        fresh = slc.Plan(gpu_ctx, wc.with_weights(P, kept, dB), S, groups, updatable_weights=True)
        fv = fresh.alloc_values()
        f1 = _phi(fresh, fv); f2 = _phi(fresh, fv)
        assert np.abs(got - f1).max() < TOL and np.abs(got - phi0).max() > 1e-3
        if np.array_equal(f1, f2):
            assert np.array_equal(got, f1), np.abs(got - f1).max()
        # a valid update afterwards is applied in full and reported so
        plan.update_weights(C1=_dev(cA), D12=_dev(dA))
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_weights_result() == 0
    finally:
        plan.close()
        if fresh is not None:
            fresh.close()


def test_unflagged_plan_and_malformed_arguments_are_refused(slc, gpu_ctx, monkeypatch):
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    PA = wc.weighted(P, A)
    cB, dB = wc.diagonals(P, B)
    plain = slc.Plan(gpu_ctx, PA, S, groups)
    plan = slc.Plan(gpu_ctx, PA, S, groups, updatable_weights=True)
    try:
        pv, dv = plain.alloc_values(), plan.alloc_values()
        p0, phi0 = _phi(plain, pv), _phi(plan, dv)
        assert np.array_equal(p0, phi0)                       # non-uniform weights: the flag adds no record and changes no bit
        with pytest.raises(slc._capi.SLSError) as ei:
            plain.update_weights(C1=cB, D12=dB)
        assert ei.value.code == slc._capi.SLS_EINVAL and "not built with SLS_PLAN_WEIGHTS_UPDATABLE" in str(ei.value)
        with pytest.raises(slc._capi.SLSError):
            plain.weights()
        assert np.array_equal(_phi(plain, pv), p0) and plain.update_weights_result() == 0
        with pytest.raises(ValueError):
            plan.update_weights(C1=np.ones(P.Nx + 1))
        with pytest.raises(ValueError):
            plan.update_weights(D12=_dev(np.ones(P.Nu - 1)))
        with pytest.raises(ValueError):
            plan.update_weights(C1=PA.D12)                                    # the other block: not C1's shape
        with pytest.raises(ValueError):
            plan.update_weights(C1=_dev(cB), D12=dB)                          # one path per call
        with pytest.raises(ValueError):
            plan.update_weights()
        lib = slc._capi.load_library()                                        # both NULL at the C boundary
        assert lib.sls_plan_update_weights(plan.handle, None, None, None, 0) == slc._capi.SLS_EINVAL
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_weights_result() == 0
        # a shape outside the rule is refused when the plan is built, with the reason
        off = sp.csc_matrix(PA.C1).copy(); off.indices[3] += 1
        with pytest.raises(slc._capi.SLSError) as ei:
            slc.Plan(gpu_ctx, slc.Plant(P.A, P.B1, P.B2, off, 0, PA.D12), S, groups, updatable_weights=True)
        assert ei.value.code == slc._capi.SLS_EUNSUPPORTED and "own z-row" in str(ei.value)
    finally:
        plain.close(); plan.close()


# ---- stream order ----

@pytest.mark.parametrize("path", ["host", "device"])
def test_execute_update_execute_on_one_stream_without_host_waits(slc, gpu_ctx, monkeypatch, path):
    import torch
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    (cA, dA), (cB, dB) = wc.diagonals(P, A), wc.diagonals(P, B)
    plan = slc.Plan(gpu_ctx, wc.weighted(P, A), S, groups, updatable_weights=True)
    try:
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        plan.update_weights(C1=cB, D12=dB)
        phi1 = _phi(plan, dv)
        plan.update_weights(C1=cA, D12=dA); plan.synchronize()
        assert not np.array_equal(phi0, phi1)
        n = plan.info["n_values"]
        v1 = torch.zeros(n, dtype=torch.float64, device="cuda:0"); v2 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        new = (_dev(cB), _dev(dB)) if path == "device" else (cB, dB)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        plan.execute(v1.data_ptr(), stream=s)
        plan.update_weights(C1=new[0], D12=new[1], stream=s)
        plan.execute(v2.data_ptr(), stream=s)
        plan.synchronize(s)
        assert plan.update_weights_result() == 0
        assert np.array_equal(v1.cpu().numpy(), phi0)
        assert np.array_equal(v2.cpu().numpy(), phi1)
    finally:
        plan.close()


# ---- the staging of host values: through the context's pinned buffer, or (SLS_PAGEABLE_D2H) from the caller's arrays ----

@pytest.mark.parametrize("halves", ["both", "C1", "D12"])
def test_host_update_without_the_pinned_buffer(slc, gpu_ctx, monkeypatch, halves):
    """With SLS_PAGEABLE_D2H=1 no pinned buffer is handed out: a host-path update copies from the caller's arrays and waits.  Φ
    after it equals bitwise what the same plan gave for the same update through the pinned buffer, update_weights_result() == 0
    and weights() returns exactly the arrays passed (the half not passed keeps seed 11's values)."""
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    monkeypatch.delenv("SLS_PAGEABLE_D2H", raising=False)
    (cA, dA), (cB, dB) = wc.diagonals(P, A), wc.diagonals(P, B)
    new = {k: v for k, v in (("C1", cB), ("D12", dB)) if halves in ("both", k)}
    held = (new.get("C1", cA), new.get("D12", dA))
    plan = slc.Plan(gpu_ctx, wc.weighted(P, A), S, groups, updatable_weights=True)
    try:
        assert route in plan.describe()
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        plan.update_weights(**new)
        want = _phi(plan, dv)                                             # through the pinned buffer
        assert not np.array_equal(want, phi0)
        plan.update_weights(C1=cA, D12=dA)
        assert np.array_equal(_phi(plan, dv), phi0)
        monkeypatch.setenv("SLS_PAGEABLE_D2H", "1")
        plan.update_weights(**new)
        got = _phi(plan, dv)
        assert plan.update_weights_result() == 0
        assert all(np.array_equal(g, w) for g, w in zip(plan.weights(), held))
        assert np.array_equal(got, want), np.abs(got - want).max()
    finally:
        plan.close()


def test_pinned_buffer_is_not_reused_under_an_update_in_flight(slc, gpu_ctx, monkeypatch):
    """A host-path update leaves an asynchronous copy reading the context's pinned buffer.  The caller's arrays are overwritten as
    soon as the call returns, and fetch_status(), which stages through the same buffer, follows at once: the plan still holds the
    values passed, and its Φ is a fresh plan's on them."""
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    monkeypatch.delenv("SLS_PAGEABLE_D2H", raising=False)
    cB, dB = wc.diagonals(P, B)
    plan = fresh = None
    try:
        plan = slc.Plan(gpu_ctx, wc.weighted(P, A), S, groups, updatable_weights=True)
        dv = plan.alloc_values()
        _phi(plan, dv)
        c, d = np.array(cB, dtype=np.float64), np.array(dB, dtype=np.float64)
        plan.update_weights(C1=c, D12=d)
        c[:] = 7.0; d[:] = 9.0
        st = plan.fetch_status()[0]
        hc, hd = plan.weights()
        assert np.all(st == 0)
        assert np.array_equal(hc, cB) and np.array_equal(hd, dB)
        got = _phi(plan, dv)
        assert np.abs(got - wc.oracle_flat(slc, "t4", B)).max() < TOL
        fresh = slc.Plan(gpu_ctx, wc.weighted(P, B), S, groups, updatable_weights=True)
        fv = fresh.alloc_values()
        f1 = _phi(fresh, fv); f2 = _phi(fresh, fv)
        if np.array_equal(f1, f2):
            assert np.array_equal(got, f1), np.abs(got - f1).max()
    finally:
        for p in (plan, fresh):
            if p is not None:
                p.close()


# ---- an update detaches an attached refinement ----

def test_weights_update_detaches_the_refinement(slc, oracle, gpu_ctx, monkeypatch):
    """The near-singular column of test_update_detaches_the_refinement (tools/fuzz_h2.py problem 77, column 21, with the stagnation
    rule of rounds 1–2), taken with its LQR blocks [C1 D12] = I and the flag: after `refine` attached the tile pass, an update with
    the same weights drops it — the next execute shows the unrefined error again — and a second `refine`, which passes the plant
    with the weights the device holds, restores it."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    col = 21
    assert np.array_equal(sp.hstack([P.C1, P.D12]).toarray(), np.eye(P.Nx + P.Nu)) and P.D11.nnz == 0
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])

    def err_of(vx, vu):
        Px, Pu = slc.assemble_phi(S[0], S[1], vx, vu, dropzeros=False)
        got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
        return np.abs(got - z).max()
    plan = slc.Plan(gpu_ctx, P, S, [[col], [col + 1]], updatable_weights=True)
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        e0 = err_of(*plan.download(dv))
        assert e0 > 1e-6
        assert plan.refine(dv) >= 1
        plan.execute(dv); plan.synchronize()
        assert err_of(*plan.download(dv)) < 1e-8                              # the attached pass runs with every execute
        plan.update_weights(C1=np.ones(P.Nx), D12=np.ones(P.Nu))             # same values: only the detach shows
        plan.execute(dv); plan.synchronize()
        e1 = err_of(*plan.download(dv))
        print(f"unrefined {e0:.2e}, after the identity weights update {e1:.2e}")
        assert e1 > 1e-6 and plan.update_weights_result() == 0
        assert plan.refine(dv) >= 1
        assert np.array_equal(plan.m.nzval["C1"], np.ones(P.Nx)) and np.array_equal(plan.m.nzval["D12"], np.ones(P.Nu))
        assert err_of(*plan.download(dv)) < 1e-8
    finally:
        plan.close()


# ---- change tracking ----

def _tracking_setup(slc, ctx, monkeypatch, cid="wave"):
    P, S, groups, knobs, route, _ = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, knobs)
    plan = slc.Plan(ctx, wc.weighted(P, A), S, groups, updatable_weights=True)
    assert route in plan.describe()
    return P, S, groups, plan


@pytest.mark.parametrize("path", ["host", "device"])
def test_one_changed_weight_marks_the_subproblems_that_hold_it(slc, gpu_ctx, monkeypatch, path):
    """`wave`: all 70 columns of chain_plant(70).  The weight of state 30 changes: exactly the subproblems whose s_x contains state
    30 are marked (the set computed on the host from the index sets); then input 4's weight: those whose s_u contains it, added to
    the marks.  execute_dirty then equals a full execute bitwise and clears the marks.  The same values again mark nothing."""
    import torch
    P, S, groups, plan = _tracking_setup(slc, gpu_ctx, monkeypatch)
    try:
        sx, su = wc.index_sets(P, S)
        cols = [g[0] for g in groups]
        cA, dA = wc.diagonals(P, A)
        n = plan.info["n_values"]
        v = torch.zeros(n, dtype=torch.float64, device="cuda:0"); torch.cuda.synchronize()
        plan.track_changes(True)
        plan.execute(v.data_ptr()); plan.synchronize()
        give = (lambda a: _dev(a)) if path == "device" else (lambda a: a)
        c = cA.copy(); c[30] *= 1.5
        plan.update_weights(C1=give(c))
        want = np.array([30 in sx[q] for q in cols], dtype=np.uint8)
        assert 0 < want.sum() < len(cols) and np.array_equal(plan.dirty(), want)
        d = dA.copy(); d[4] *= 0.5
        plan.update_weights(D12=give(d))
        want |= np.array([4 in su[q] for q in cols], dtype=np.uint8)
        assert 0 < want.sum() < len(cols) and np.array_equal(plan.dirty(), want)
        plan.update_weights(C1=give(c), D12=give(d))                          # nothing new: no new mark
        assert np.array_equal(plan.dirty(), want)
        assert plan.execute_dirty(v.data_ptr()) == int(want.sum())
        plan.synchronize()
        full = torch.zeros(n, dtype=torch.float64, device="cuda:0"); torch.cuda.synchronize()
        plan.execute(full.data_ptr()); plan.synchronize()
        assert np.array_equal(v.cpu().numpy().view(np.uint64), full.cpu().numpy().view(np.uint64))
        assert not plan.dirty().any()
        plan.update_weights(C1=give(c), D12=give(d))                          # the same values again mark none
        assert not plan.dirty().any() and plan.update_weights_result() == 0
    finally:
        plan.close()


# ---- plant update and weights update on one plan ----

@pytest.mark.parametrize("cid", ["t4", "tile"])
def test_plant_update_and_weights_update_interleave(slc, gpu_ctx, monkeypatch, cid):
    """Update A and B2, then the weights, then execute: bitwise a fresh flagged plan on the plant that has both (when that plan
    repeats bitwise), and within TOL of it in any case; then the other order back to the start."""
    P, S, groups, knobs, route, _ = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, knobs)
    Q = uc.perturb(P)
    cB, dB = wc.diagonals(P, B)
    cA, dA = wc.diagonals(P, A)
    plan = slc.Plan(gpu_ctx, wc.weighted(P, A), S, groups, updatable_weights=True)
    fresh = slc.Plan(gpu_ctx, wc.with_weights(Q, cB, dB), S, groups, updatable_weights=True)
    try:
        assert route in plan.describe() and fresh.describe() == plan.describe()
        dv, fv = plan.alloc_values(), fresh.alloc_values()
        phi0 = _phi(plan, dv)
        plan.update_plant(A=Q.A, B2=Q.B2)
        plan.update_weights(C1=cB, D12=dB)
        got = _phi(plan, dv)
        assert plan.update_result() == 0 and plan.update_weights_result() == 0
        f1 = _phi(fresh, fv); f2 = _phi(fresh, fv)
        assert np.array_equal(plan.fetch_status()[0], fresh.fetch_status()[0])
        assert np.abs(got - f1).max() < TOL and np.abs(got - phi0).max() > 1e-3
        if np.array_equal(f1, f2):
            assert np.array_equal(got, f1), np.abs(got - f1).max()
        plan.update_weights(C1=_dev(cA), D12=_dev(dA))
        plan.update_plant(A=P.A, B2=P.B2)
        assert np.array_equal(_phi(plan, dv), phi0)
    finally:
        plan.close(); fresh.close()
