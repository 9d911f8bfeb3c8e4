"""sls_plan_update_plant on the device: a resident plan re-solves for new values of A and B2 without a rebuild.

Cases (tests/update_cases.py; each asserts its route through Plan.describe()):

  id          plant, columns (one group each)                        masks / knob                      route
  t4          chain_plant(70), (0,1,2,35,67,68,69)                   d 9, T 7, α 1.5                   h2_column_twisted4_kernel<32,12>
  t4_long     chain_plant(70), (0,1,2,3,35,66,67,68,69)              d 9, T 29, α 1.5                  four-wave
  t4_zeros    banded 64-state plant with stored 0.0 on the ±3        masks of the plain banded plant,  four-wave
              diagonals of A and the −3 diagonal of B2, range(20,44,3)  d 4, T 12, α 1
  t2          as t4                                                  SLS_TWISTED4=0                    two-wave twisted
  wave        as t4 but all 70 columns                               SLS_NO_TWISTED=1                  one-wave
  tile        grid_plant(10, 1), (0,9,45,55,90,99,4,50)              d 3, T 4, α 8 (ñx = 41)           tile (+ twisted)
  localized   Plan.localized on chain_plant(70)                      d 9, T 7, α 1.5                   as routed
  son         as wave, sum-of-norms objective, T 4                   —                                 fresh-plan comparison only
                                                                                                       (no oracle, statuses as the fresh plan's)

Per case: (a) the base solve agrees with the C restatement of the oracle on P within oracle_c.TOL; (b) after update_plant with
perturb(P) the next execute agrees with the oracle on perturb(P) within TOL, all statuses OK, update_result() == 0; (c) a fresh
plan built on perturb(P) is executed twice and, if its two results are bitwise equal (the precondition is judged on the fresh
plan, not on the code under test), the updated plan's Φ is bitwise equal to them; (d) objective_values after the update equals
objective_values_host on perturb(P) and the downloaded Φ within objective_cases.summation_bound; (e) updating back to P gives
bitwise the Φ of (a).  (b) runs through the host path and through the device path (torch tensors): bitwise the same Φ.

Φ moves by 0.13 to 17.9 between P and perturb(P) (update_cases.py), against TOL = 1e-8: an update that did nothing fails (b)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import objective_cases as oc
import update_cases as uc
from oracle_c import TOL, c_oracle_flat

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def _oracle(slc, cid, which):
    """Φ of the C restatement on P ("base") or perturb(P) ("pert") in mask order, feasibility asserted; computed once per plant,
    columns and masks (the localized case shares `wave`'s), read-only."""
    name, cols, dTa = uc.CASES[cid][:3]
    key = (name, cols, dTa, which)
    if key not in _oracle_cache:
        P, S, groups = uc.case(slc, cid)[:3]
        Q = P if which == "base" else uc.perturb(P)
        want, info = c_oracle_flat(slc, Q, S, [g[0] for g in groups])
        assert np.all(np.array(info["status"]) == 0), info["status"]
        want.setflags(write=False)
        _oracle_cache[key] = want
    return _oracle_cache[key]


def _nz(M):
    return sp.csc_matrix(M).data


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _phi(plan, dv):
    plan.execute(dv); plan.synchronize()
    return np.concatenate(sum(plan.download(dv), []))


def _build(slc, ctx, cid, P, localized=False):
    _, S, groups, _, _, objective = uc.case(slc, cid)
    if localized:
        d, T, alpha = uc.CASES[cid][2]
        return slc.Plan.localized(ctx, P, d, T, alpha)
    return slc.Plan(ctx, P, S, groups, objective=objective)


def _run_case(slc, ctx, monkeypatch, cid, localized=False):
    P, S, groups, knobs, route, objective = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, {} if localized else knobs)
    Q = uc.perturb(P)
    with_oracle = objective == "h2"
    plan = fresh = None
    try:
        plan = _build(slc, ctx, cid, P, localized)
        desc = plan.describe()
        assert (desc.startswith("h2_column_") if localized else route in desc), desc
        dv = plan.alloc_values()
        # (a) base solve
        phi0 = _phi(plan, dv)
        st0 = plan.fetch_status()[0].copy()
        assert not with_oracle or np.all(st0 == 0), st0       # son: no oracle, statuses are compared with the fresh plan's
        if with_oracle:
            e0 = np.abs(phi0 - _oracle(slc, cid, "base")).max()
            print(f"{cid}: {desc} base max |Φ − Φ_oracle| = {e0:.2e}")
            assert e0 < TOL
        # (b) updated solve, host path: a scipy matrix for A, an nzval array for B2
        plan.update_plant(A=Q.A, B2=_nz(Q.B2))
        phi1 = _phi(plan, dv)
        st1 = plan.fetch_status()[0].copy()
        assert (not with_oracle or np.all(st1 == 0)) and plan.update_result() == 0
        moved = np.abs(phi1 - phi0).max()
        print(f"{cid}: the update moved Φ by {moved:.3g}")
        assert moved > 1e-3
        if with_oracle:
            e1 = np.abs(phi1 - _oracle(slc, cid, "pert")).max()
            print(f"{cid}: updated max |Φ − Φ_oracle| = {e1:.2e}")
            assert e1 < TOL
        # (d) objective after the update
        vx, vu = plan.download(dv)
        col, tot = plan.objective_values(dv)
        hcol, htot, n_terms, abs_sum = slc.objective_values_host(Q, S, vx, vu, None if localized else groups, objective=objective, return_bound=True)
        bound = oc.summation_bound(n_terms, abs_sum)
        print(f"{cid}: objective worst |Δ|/bound {(np.abs(col - hcol) / np.maximum(bound, 1e-300)).max():.3g}")
        assert np.all(np.abs(col - hcol) <= bound)
        assert abs(tot - htot) <= bound.sum() + 2 * len(col) * oc.U * np.abs(hcol).sum()
        # (c) bitwise against a fresh plan on perturb(P)
        fresh = _build(slc, ctx, cid, Q, localized)
        assert fresh.describe() == desc
        fv = fresh.alloc_values()
        f1 = _phi(fresh, fv); f2 = _phi(fresh, fv)
        assert np.array_equal(fresh.fetch_status()[0], st1)
        if np.array_equal(f1, f2):
            assert np.array_equal(phi1, f1), np.abs(phi1 - f1).max()
        else:
            print(f"{cid}: the fresh plan does not repeat bitwise ({np.abs(f1 - f2).max():.2e}): bitwise comparison not applicable")
        # (e) round trip
        plan.update_plant(A=_nz(P.A), B2=P.B2)
        assert np.array_equal(_phi(plan, dv), phi0)
        # (b) through the device path
        tA, tB = _dev(_nz(Q.A)), _dev(_nz(Q.B2))
        plan.update_plant(A=tA, B2=tB)
        phi1d = _phi(plan, dv)
        assert plan.update_result() == 0 and np.array_equal(plan.fetch_status()[0], st1)
        assert np.array_equal(phi1d, phi1), np.abs(phi1d - phi1).max()
        # one matrix at a time: A back to P's on the device path, then B2 on the host path, ends at P
        plan.update_plant(A=_dev(_nz(P.A)))
        plan.update_plant(B2=_nz(P.B2))
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_result() == 0
    finally:
        for p in (plan, fresh):
            if p is not None:
                p.close()


@pytest.mark.parametrize("cid", list(uc.CASES))
def test_updated_plan_solves_the_new_plant(slc, gpu_ctx, monkeypatch, cid):
    _run_case(slc, gpu_ctx, monkeypatch, cid)


def test_updated_localized_plan_solves_the_new_plant(slc, gpu_ctx, monkeypatch):
    """Plan.localized (index sets and masks built on the device) on chain_plant(70), d 9, T 7, α 1.5: the masks, and so the oracle
    references, are those of the `wave` case."""
    _run_case(slc, gpu_ctx, monkeypatch, "wave", localized=True)


def test_update_in_the_packed_layout(slc, gpu_ctx, monkeypatch):
    import torch
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    Q = uc.perturb(P)
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        assert route in plan.describe()
        pk = torch.zeros(plan.info["n_packed"], dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        dest = plan.packed_dest()

        def solve():
            plan.execute(pk.data_ptr(), packed=True); plan.synchronize()
            full = np.zeros(plan.info["n_values"]); full[dest] = pk.cpu().numpy()
            return full
        assert np.abs(solve() - _oracle(slc, "t4", "base")).max() < TOL
        plan.update_plant(A=Q.A, B2=Q.B2)
        got = solve()
        assert np.abs(got - _oracle(slc, "t4", "pert")).max() < TOL and plan.update_result() == 0
        dv = plan.alloc_values()
        assert np.array_equal(_phi(plan, dv), got)                      # the two layouts name the same values
    finally:
        plan.close()


# ---- four-wave records ----

@pytest.mark.parametrize("cid", ["t4", "t4_zeros"])
def test_four_wave_records_hold_the_gathered_new_values(slc, gpu_ctx, monkeypatch, cid):
    """After an update the prepared records show the same indices, counts and bit words, and exactly the gathered new values: the
    NumPy restatement of test_gpu_twisted4_prepared.py (CSR order, entries outside the index set and stored zeros dropped) on
    perturb(P).  t4_zeros: the counts stay below the capacities (7, 7, 4, 4) — stored zeros are still skipped."""
    from test_gpu_twisted4_prepared import _assert_tables_equal, _restate
    P, S, groups, knobs, route, _ = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, knobs)
    Q = uc.perturb(P)
    cols = [g[0] for g in groups]
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        assert route in plan.describe()
        before = plan.twisted4_tables()
        _assert_tables_equal(before, _restate(P, S, cols, before["caps"]), len(cols))
        for path in ("host", "device"):
            src = Q if path == "host" else P
            if path == "host":
                plan.update_plant(A=src.A, B2=src.B2)
            else:
                plan.update_plant(A=_dev(_nz(src.A)), B2=_dev(_nz(src.B2)))
            assert plan.update_result() == 0
            after = plan.twisted4_tables()
            assert after["caps"] == before["caps"] and np.array_equal(after["counts"], before["counts"]) and np.array_equal(after["bits"], before["bits"])
            for name in ("arow", "acol", "brow", "bcol"):
                assert np.array_equal(after[name][0], before[name][0]), name
            _assert_tables_equal(after, _restate(src, S, cols, after["caps"]), len(cols))
            if path == "host":
                assert not np.array_equal(after["arow"][1], before["arow"][1])
        if cid == "t4_zeros":
            assert before["caps"] == (7, 7, 4, 4) and np.all(before["counts"] < np.array(before["caps"]))
    finally:
        plan.close()


# ---- the zero rule, non-finite values, malformed arguments (t4_zeros) ----

def _zeros_setup(slc, ctx, monkeypatch):
    P, S, groups, knobs, route, _ = uc.case(slc, "t4_zeros")
    uc.set_knobs(monkeypatch, knobs)
    plan = slc.Plan(ctx, P, S, groups)
    assert route in plan.describe()
    return P, S, groups, plan


def _fresh_phi(slc, ctx, P, S, groups):
    """(Φ, repeats bitwise) of a fresh plan"""
    fresh = slc.Plan(ctx, P, S, groups)
    try:
        fv = fresh.alloc_values()
        f1 = _phi(fresh, fv); f2 = _phi(fresh, fv)
        assert np.all(fresh.fetch_status()[0] == 0)
        return f1, np.array_equal(f1, f2)
    finally:
        fresh.close()


@pytest.mark.parametrize("bad", ["zero_rule", "nan"])
def test_refused_entries_on_both_paths(slc, gpu_ctx, monkeypatch, bad):
    """One entry of A's new values breaks a rule: a plan-time zero set to 0.3, or a NaN on a non-zero entry.  Host path: SLSError
    (SLS_EINVAL) and the plan is untouched — the following execute is bitwise unchanged.  Device path: update_result() == 1, that
    entry keeps its old value and every other entry is updated — Φ equals a fresh plan's on the array with that entry put back."""
    P, S, groups, plan = _zeros_setup(slc, gpu_ctx, monkeypatch)
    try:
        A0 = _nz(P.A)
        Q = uc.perturb(P)
        k = int(np.flatnonzero(A0 == 0.0)[40]) if bad == "zero_rule" else int(np.flatnonzero(A0 != 0.0)[100])
        a = _nz(Q.A).copy(); a[k] = 0.3 if bad == "zero_rule" else np.nan
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        with pytest.raises(slc._capi.SLSError) as ei:
            plan.update_plant(A=a, B2=Q.B2)
        assert ei.value.code == slc._capi.SLS_EINVAL and f"A nzval position {k} " in str(ei.value), str(ei.value)
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_result() == 0
        assert plan.m.nzval is None                                       # the marshalled plant did not move either
        assert all(np.array_equal(g, w) for g, w in zip(plan.plant_values(), (A0, _nz(P.B2))))
        plan.update_plant(A=_dev(a), B2=_dev(_nz(Q.B2)))
        got = _phi(plan, dv)
        assert plan.update_result() == 1
        assert np.all(plan.fetch_status()[0] == 0)
        kept = a.copy(); kept[k] = A0[k]
        hA, hB = plan.plant_values()                                      # the plan's own values: every entry but the refused one
        assert np.array_equal(hA.view(np.uint64), kept.view(np.uint64)) and np.array_equal(hB, _nz(Q.B2))
        R = uc.with_values(P, A_data=kept, B2_data=_nz(Q.B2))
        want, info = c_oracle_flat(slc, R, S, [g[0] for g in groups])
        assert np.all(np.array(info["status"]) == 0)
        assert np.abs(got - want).max() < TOL
        f, repeats = _fresh_phi(slc, gpu_ctx, R, S, groups)
        if repeats:
            assert np.array_equal(got, f), np.abs(got - f).max()
        # a valid update afterwards is applied in full and reported so
        plan.update_plant(A=_dev(_nz(P.A)), B2=_dev(_nz(P.B2)))
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_result() == 0
    finally:
        plan.close()


def test_malformed_arguments_raise_value_error(slc, gpu_ctx, monkeypatch):
    P, S, groups, plan = _zeros_setup(slc, gpu_ctx, monkeypatch)
    try:
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        with pytest.raises(ValueError):
            plan.update_plant(A=np.ones(_nz(P.A).size + 1))
        with pytest.raises(ValueError):
            plan.update_plant(B2=_dev(np.ones(_nz(P.B2).size - 1)))
        with pytest.raises(ValueError):
            plan.update_plant(A=uc.banded(slc).A)                         # the plain banded plant: no stored zeros, another pattern
        with pytest.raises(ValueError):
            plan.update_plant(A=_dev(_nz(P.A)), B2=_nz(P.B2))             # one path per call
        plan.update_plant()                                               # both absent: a no-op
        assert np.array_equal(_phi(plan, dv), phi0) and plan.update_result() == 0
    finally:
        plan.close()


def test_non_zero_entry_may_become_zero(slc, gpu_ctx, monkeypatch):
    """A[28, 29] = 0.0 (an interior entry of a solved column: the union that forms the column's index set does not shrink, so
    the plan's index sets are still the reference's).  The C restatement calls all eight columns of that plant feasible."""
    P, S, groups, plan = _zeros_setup(slc, gpu_ctx, monkeypatch)
    try:
        A = sp.csc_matrix(P.A)
        k = int(A.indptr[29] + np.flatnonzero(A.indices[A.indptr[29]:A.indptr[30]] == 28)[0])
        a = A.data.copy()
        assert a[k] == 0.2
        a[k] = 0.0
        R = uc.with_values(P, A_data=a)
        want, info = c_oracle_flat(slc, R, S, [g[0] for g in groups])
        assert np.all(np.array(info["status"]) == 0)
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        for path in ("host", "device"):
            plan.update_plant(A=a if path == "host" else _dev(a))
            got = _phi(plan, dv)
            err = np.abs(got - want).max()
            print(f"{path}: A[28,29] → 0.0: max |Φ − Φ_oracle| = {err:.2e}, moved {np.abs(got - phi0).max():.3g}")
            assert plan.update_result() == 0 and np.all(plan.fetch_status()[0] == 0)
            assert err < TOL
            plan.update_plant(A=A.data)
            assert np.array_equal(_phi(plan, dv), phi0)
    finally:
        plan.close()


# ---- stream order ----

@pytest.mark.parametrize("path", ["host", "device"])
def test_execute_update_execute_on_one_stream_without_host_waits(slc, gpu_ctx, monkeypatch, path):
    import torch
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    Q = uc.perturb(P)
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        plan.update_plant(A=Q.A, B2=Q.B2)
        phi1 = _phi(plan, dv)
        plan.update_plant(A=P.A, B2=P.B2); plan.synchronize()
        assert not np.array_equal(phi0, phi1)
        n = plan.info["n_values"]
        v1 = torch.zeros(n, dtype=torch.float64, device="cuda:0"); v2 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        new = (_dev(_nz(Q.A)), _dev(_nz(Q.B2))) if path == "device" else (_nz(Q.A), _nz(Q.B2))
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        plan.execute(v1.data_ptr(), stream=s)
        plan.update_plant(A=new[0], B2=new[1], stream=s)
        plan.execute(v2.data_ptr(), stream=s)
        plan.synchronize(s)
        assert plan.update_result() == 0
        assert np.array_equal(v1.cpu().numpy(), phi0)
        assert np.array_equal(v2.cpu().numpy(), phi1)
    finally:
        plan.close()


# ---- the staging of host values: through the context's pinned buffer, or (SLS_PAGEABLE_D2H) from the caller's arrays ----

@pytest.mark.parametrize("halves", ["both", "A", "B2"])
def test_host_update_without_the_pinned_buffer(slc, gpu_ctx, monkeypatch, halves):
    """With SLS_PAGEABLE_D2H=1 no pinned buffer is handed out: a host-path update copies from the caller's arrays and waits.  Φ
    after it equals bitwise what the same plan gave for the same update through the pinned buffer, update_result() == 0 and
    plant_values() returns exactly the arrays passed (the half not passed keeps P's values)."""
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    monkeypatch.delenv("SLS_PAGEABLE_D2H", raising=False)
    Q = uc.perturb(P)
    new = {k: v for k, v in (("A", _nz(Q.A)), ("B2", _nz(Q.B2))) if halves in ("both", k)}
    held = (new.get("A", _nz(P.A)), new.get("B2", _nz(P.B2)))
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        assert route in plan.describe()
        dv = plan.alloc_values()
        phi0 = _phi(plan, dv)
        plan.update_plant(**new)
        want = _phi(plan, dv)                                             # through the pinned buffer
        assert not np.array_equal(want, phi0)
        plan.update_plant(A=_nz(P.A), B2=_nz(P.B2))
        assert np.array_equal(_phi(plan, dv), phi0)
        monkeypatch.setenv("SLS_PAGEABLE_D2H", "1")
        plan.update_plant(**new)
        got = _phi(plan, dv)
        assert plan.update_result() == 0
        assert all(np.array_equal(g, w) for g, w in zip(plan.plant_values(), held))
        assert np.array_equal(got, want), np.abs(got - want).max()
    finally:
        plan.close()


def test_pinned_buffer_is_not_reused_under_an_update_in_flight(slc, gpu_ctx, monkeypatch):
    """A host-path update leaves an asynchronous copy reading the context's pinned buffer.  The caller's array is overwritten as
    soon as the call returns, and fetch_status(), which stages through the same buffer, follows at once: the plan still holds the
    values passed, and its Φ is a fresh plan's on them."""
    P, S, groups, knobs, route, _ = uc.case(slc, "t4")
    uc.set_knobs(monkeypatch, knobs)
    monkeypatch.delenv("SLS_PAGEABLE_D2H", raising=False)
    Q = uc.perturb(P)
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        dv = plan.alloc_values()
        _phi(plan, dv)
        a, b = _nz(Q.A).copy(), _nz(Q.B2).copy()
        plan.update_plant(A=a, B2=b)
        a[:] = 7.0; b[:] = -7.0
        st = plan.fetch_status()[0]
        hA, hB = plan.plant_values()
        assert np.all(st == 0)
        assert np.array_equal(hA, _nz(Q.A)) and np.array_equal(hB, _nz(Q.B2))
        got = _phi(plan, dv)
        assert np.abs(got - _oracle(slc, "t4", "pert")).max() < TOL
        f, repeats = _fresh_phi(slc, gpu_ctx, Q, S, groups)
        if repeats:
            assert np.array_equal(got, f), np.abs(got - f).max()
    finally:
        plan.close()


# ---- an update detaches an attached refinement ----

def test_update_detaches_the_refinement(slc, oracle, gpu_ctx, monkeypatch):
    """The near-singular column of test_resident_plan_refine_attaches_tile_pass (tools/fuzz_h2.py problem 77, column 21, with the
    stagnation rule of rounds 1–2): after `refine` attached the tile pass, an identity update (the same values) drops it — the
    next execute shows the unrefined error again — and a second `refine`, which passes the marshalled plant, restores it."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    col = 21
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])

    def err_of(vx, vu):
        Px, Pu = slc.assemble_phi(S[0], S[1], vx, vu, dropzeros=False)
        got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
        return np.abs(got - z).max()
    plan = slc.Plan(gpu_ctx, P, S, [[col], [col + 1]])
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        e0 = err_of(*plan.download(dv))
        assert e0 > 1e-6
        assert plan.refine(dv) >= 1
        plan.execute(dv); plan.synchronize()
        assert err_of(*plan.download(dv)) < 1e-8                          # the attached pass runs with every execute
        plan.update_plant(A=P.A, B2=P.B2)                                 # same values: only the detach shows
        plan.execute(dv); plan.synchronize()
        e1 = err_of(*plan.download(dv))
        print(f"unrefined {e0:.2e}, after the identity update {e1:.2e}")
        assert e1 > 1e-6 and plan.update_result() == 0
        assert plan.refine(dv) >= 1
        assert err_of(*plan.download(dv)) < 1e-8
        # device path, the way a loop over operating points uses it: one buffer per matrix, overwritten for the next point.
        # Two updates (a scaled plant, then P again) through the same tensors, which are then overwritten once more: the plan
        # keeps no tensor, and `refine` passes the plant the device holds — P — not what the buffers hold by then.
        import torch
        tA, tB = _dev(1.1 * _nz(P.A)), _dev(0.9 * _nz(P.B2))
        plan.update_plant(A=tA, B2=tB)
        plan.synchronize()
        tA.copy_(torch.from_numpy(_nz(P.A))); tB.copy_(torch.from_numpy(_nz(P.B2))); torch.cuda.synchronize()
        plan.update_plant(A=tA, B2=tB)
        plan.synchronize()
        tA.mul_(3.0); tB.zero_(); torch.cuda.synchronize()
        assert not any(isinstance(v, torch.Tensor) for v in vars(plan).values())
        plan.execute(dv); plan.synchronize()
        assert err_of(*plan.download(dv)) > 1e-6 and plan.update_result() == 0     # detached again
        assert plan.refine(dv) >= 1
        assert np.array_equal(plan.m.nzval["A"], _nz(P.A)) and np.array_equal(plan.m.nzval["B2"], _nz(P.B2))
        assert err_of(*plan.download(dv)) < 1e-8
    finally:
        plan.close()
