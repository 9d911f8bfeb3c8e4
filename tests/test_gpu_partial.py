"""The partial re-solve on the device: sls_plan_execute_columns, sls_plan_track_changes, sls_plan_execute_dirty.

Cases: tests/update_cases.py (`t4`, `t4_long`, `t4_zeros`, `t2`, `wave`, `tile`, `son`; each asserts its route through
Plan.describe()), the localized plan of chain_plant(70), and the coupled groups of tests/golden/coupled_group_phi.npz (the
construction of test_gpu_tile.py::test_coupled_column_groups_match_golden, restated: the smallest coupled plan the suite has).
Change sets and the NumPy reference of the dependency rule: tests/partial_cases.py; tests/test_partial_host.py asserts on the CPU
that each of them marks some but not all subproblems.

Everything compared is bits (uint64 views of the value arrays, against a NaN sentinel with a payload no solve produces) or integer
sets.  There is no tolerance.

execute_columns: the plan solves P, is updated to perturb(P), and only then runs the subset, so that a status / residual /
iteration word of an unselected subproblem that were rewritten would show the new plant's value: unselected words must equal the
words of the full execute on P, selected ones those of a full execute on perturb(P), selected entries that execute's bits, and every
other entry the sentinel.  Of the update cases only `tile` has two launches (tile + twisted; `wave` routes its 70 columns into one
h2_column_wave_kernel launch), so the one-subproblem-per-launch subset and the subset that leaves a launch empty run there.

Dirty path, per case, update path (host / device) and change set of the case's plant: track_changes, full execute into v,
update_plant with the local change, dirty() == reference, execute_dirty(v) returns the reference's count, v == a full execute of the
updated plan into a fresh array over the whole array, dirty() all zero; then the same back to P, which must end at the first
execute's bits."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import partial_cases as pc
import update_cases as uc

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0x7FF8DEAD0000BEEF)


def _sentinel_array(n):
    import torch
    t = torch.from_numpy(np.full(max(n, 1), SENTINEL, dtype=np.uint64).view(np.float64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _bits(t, n):
    return t.cpu().numpy().view(np.uint64)[:n].copy()


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda:0")          # a copy: the references are read-only
    torch.cuda.synchronize()
    return t


def _nz(M):
    return sp.csc_matrix(M).data


def _status(plan):
    st, rs, it = plan.fetch_status()
    return st.copy(), rs.view(np.uint64).copy(), it.copy()


def _owners(plan, S, cols):
    """owner[i] = subproblem (col_status position) that writes entry i of the mask-order value array: the entries of column c of
    every 𝓢x[t], 𝓢u[t] belong to the subproblem of column c; −1 for columns the plan does not solve"""
    q_of = -np.ones(S[0][0].shape[1], dtype=np.int64)
    q_of[np.asarray(cols)] = np.arange(len(cols))
    owner = -np.ones(plan.info["n_values"], dtype=np.int64)
    for masks, offs in ((S[0], plan.off_x), (S[1], plan.off_u)):
        for t, M in enumerate(masks):
            M = sp.csc_matrix(M); M.sort_indices()
            assert offs[t + 1] - offs[t] == M.nnz
            owner[offs[t]:offs[t + 1]] = q_of[np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))]
    return owner


def _full(plan, n, packed):
    v = _sentinel_array(n)
    plan.execute(v.data_ptr(), packed=packed); plan.synchronize()
    return _bits(v, n)


def _launch_members(desc, sets):
    """Which subproblems each launch of Plan.describe() holds, from ñx: a wave / twisted launch <NPL,RPL> holds up to
    (64/NPL)·RPL states, the smallest listed class that fits takes the column, tile / general launches the rest.  The counts must
    reproduce every launch's nsub (else the inference is wrong, and the test says so)."""
    launches = [s for s in desc.split(";") if s]
    caps = []
    for s in launches:
        m = re.match(r"h2_column_(wave|twisted4?)_kernel<(\d+),(\d+)", s)
        caps.append((64 // int(m.group(2))) * int(m.group(3)) if m else None)
    members = [[] for _ in launches]
    for q, (sx, _) in enumerate(sets):
        fit = [(c, i) for i, c in enumerate(caps) if c is not None and len(sx) <= c]
        li = min(fit)[1] if fit else [i for i, c in enumerate(caps) if c is None][0]
        members[li].append(q)
    for s, mem in zip(launches, members):
        assert int(re.search(r"nsub=(\d+)", s).group(1)) == len(mem), (desc, [len(m) for m in members])
    return members


def _check_subset(plan, subs, expect, owner, n, packed, st0, st2, v_full):
    """execute_columns(subs) into a sentinel array on the updated plan: `expect` (subs expanded to whole groups) is what runs"""
    v = _sentinel_array(n)
    k = plan.execute_columns(v.data_ptr(), subs, packed=packed); plan.synchronize()
    got = _bits(v, n)
    st1 = _status(plan)
    sel = np.isin(owner, expect)
    assert k == len(expect), (k, expect)
    assert np.array_equal(got[sel], v_full[sel])
    assert np.all(got[~sel] == SENTINEL)
    for q in expect:                                                       # not vacuous: every selected subproblem wrote values
        assert np.any(got[owner == q] != SENTINEL), q
    un = np.setdiff1d(np.arange(len(st0[0])), expect)
    for w0, w1, w2 in zip(st0, st1, st2):
        assert np.array_equal(w1[un], w0[un]) and np.array_equal(w1[expect], w2[expect])


def _run_execute_columns(plan, S, cols, P0, Q, packed=False, extra_subsets=(), groups=None):
    """The sequence of the module docstring on a plan built on P0; Q = the plant it is updated to (None: no update, for plans
    whose update is not under test here)."""
    n = plan.info["n_packed"] if packed else plan.info["n_values"]
    owner = _owners(plan, S, cols)
    if packed:
        owner = owner[plan.packed_dest()]
    nsub = plan.info["n_subproblems"]
    assert nsub == len(cols)
    _full(plan, n, packed)
    st0 = _status(plan)
    if Q is not None:
        plan.update_plant(A=Q.A, B2=Q.B2)
    v_full = _full(plan, n, packed)
    st2 = _status(plan)
    if Q is not None:
        assert not np.array_equal(st0[1], st2[1])                          # the residual words moved with the plant
    # restore the status words of P's execute: an unselected word must keep THAT value through the subset runs
    # (a full execute on P, then the update again, leaves P's words and perturb(P)'s operator)
    def reset():
        if Q is not None:
            plan.update_plant(A=P0.A, B2=P0.B2); _full(plan, n, packed); plan.update_plant(A=Q.A, B2=Q.B2)
    grp_of = np.arange(nsub) if groups is None else np.repeat(np.arange(len(groups)), [len(g) for g in groups])
    for subs in [[0, nsub // 2, nsub - 1], *extra_subsets]:
        reset()
        expect = np.flatnonzero(np.isin(grp_of, grp_of[np.asarray(subs)]))
        _check_subset(plan, subs, expect, owner, n, packed, st0, st2, v_full)
    assert np.all(plan.dirty() == 0)                                       # a listed run never touches the marks


def _plan(slc, ctx, monkeypatch, cid, localized=False):
    P, S, groups, knobs, route, objective = uc.case(slc, cid)
    uc.set_knobs(monkeypatch, {} if localized else knobs)
    if localized:
        d, T, alpha = uc.CASES[cid][2]
        plan = slc.Plan.localized(ctx, P, d, T, alpha)
        groups = [[c] for c in range(P.Nx)]
    else:
        plan = slc.Plan(ctx, P, S, groups, objective=objective)
    desc = plan.describe()
    assert (desc.startswith("h2_column_") if localized else route in desc), desc
    return plan, P, S, groups, desc


# ---- execute_columns ----

@pytest.mark.parametrize("cid", list(uc.CASES))
def test_execute_columns_writes_only_the_listed_subproblems(slc, gpu_ctx, monkeypatch, cid):
    plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, cid)
    try:
        extra = []
        if desc.count(";") > 1:                                            # `tile`: one subproblem per launch; one launch left empty
            mem = _launch_members(desc, pc.index_sets(slc, P, S, groups))
            extra = [sorted(m[0] for m in mem), sorted(q for m in mem[1:] for q in m)]
        else:
            assert cid != "tile"
        _run_execute_columns(plan, S, [g[0] for g in groups], P, uc.perturb(P), extra_subsets=extra)
    finally:
        plan.close()


@pytest.mark.parametrize("cid", ["t4", "wave"])
def test_execute_columns_in_the_packed_layout(slc, gpu_ctx, monkeypatch, cid):
    plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, cid)
    try:
        _run_execute_columns(plan, S, [g[0] for g in groups], P, uc.perturb(P), packed=True)
    finally:
        plan.close()


def test_execute_columns_on_a_localized_plan(slc, gpu_ctx, monkeypatch):
    plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, "wave", localized=True)
    try:
        _run_execute_columns(plan, S, list(range(P.Nx)), P, uc.perturb(P), extra_subsets=[[3], list(range(0, 70, 2))])
    finally:
        plan.close()


def _coupled(slc):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "coupled_group_phi.npz"))
    Nx = int(g["Nx"])
    Pc = slc.workloads.chain_plant(Nx)
    Nu = Pc.Nu
    W = sp.csc_matrix((g["diag_W_data"], g["diag_W_indices"], g["diag_W_indptr"]), shape=(Nx + Nu, Nx + Nu))
    B1 = sp.csc_matrix((g["B1_data"], g["B1_indices"], g["B1_indptr"]), shape=(Nx, Nx))
    D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nx + Nu, Nx))
    P = slc.Plant(Pc.A, B1, Pc.B2, W[:, :Nx], D11, W[:, Nx:])
    S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    gp = g["group_ptr"]; gc = g["group_cols"]
    return P, [list(S[0]), list(S[1])], [[int(c) for c in gc[gp[i]:gp[i + 1]]] for i in range(len(gp) - 1)]


def test_execute_columns_selects_a_coupled_group_as_a_whole(slc, gpu_ctx):
    """Groups of 1–4 columns coupled through B1[c_j, c_j]: one work item of the tile kernel each.  Listing one column of a group
    (not its first) runs the whole group; the other groups keep the sentinel."""
    P, S, groups = _coupled(slc)
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        assert "dense_hessian_cg" in plan.describe(), plan.describe()
        cols = [c for g in groups for c in g]
        first = np.cumsum([0] + [len(g) for g in groups])
        multi = [i for i, g in enumerate(groups) if len(g) > 1]
        assert len(multi) >= 2
        a, b = multi[0], multi[-1]
        subsets = [[int(first[a]) + 1], [int(first[a]) + len(groups[a]) - 1, int(first[b]) + 1]]
        _run_execute_columns(plan, S, cols, P, None, extra_subsets=subsets, groups=groups)
    finally:
        plan.close()


def test_execute_columns_refuses_bad_lists_and_a_refined_plan(slc, oracle, gpu_ctx, monkeypatch):
    """The library's own argument checks (past the Python wrapper's): unsorted, repeated, out of range → SLS_EINVAL; nsubs = 0
    returns 0; and with a refinement attached (the near-singular column of test_update_detaches_the_refinement) both selected
    runs return SLS_EUNSUPPORTED."""
    import ctypes as C
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    plan = slc.Plan(gpu_ctx, P, S, [[21], [22]])
    try:
        dv = plan.alloc_values()
        lib = plan._lib
        k = C.c_int64(5)
        for bad in ([1, 0], [1, 1], [0, 2], [-1]):
            arr = np.asarray(bad, dtype=np.int64)
            rc = lib.sls_plan_execute_columns(plan.handle, None, dv, 0, arr.ctypes.data_as(C.POINTER(C.c_int64)), arr.size, C.byref(k))
            assert rc == slc._capi.SLS_EINVAL and k.value == 0, (bad, rc)
        assert lib.sls_plan_execute_columns(plan.handle, None, dv, 0, None, 0, C.byref(k)) == 0 and k.value == 0
        plan.execute(dv); plan.synchronize()
        assert plan.execute_columns(dv, [1]) == 1
        plan.synchronize()
        assert plan.refine(dv) >= 1
        for call in (lambda: plan.execute_columns(dv, [0]), lambda: plan.execute_dirty(dv)):
            with pytest.raises(slc._capi.SLSError) as ei:
                call()
            assert ei.value.code == slc._capi.SLS_EUNSUPPORTED
    finally:
        plan.close()


# ---- the dirty path ----

def _update(plan, a, b, path):
    if path == "device":
        plan.update_plant(A=None if a is None else _dev(a), B2=None if b is None else _dev(b))
    else:
        plan.update_plant(A=a, B2=b)


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("cid", list(uc.CASES))
def test_execute_dirty_equals_a_full_execute(slc, gpu_ctx, monkeypatch, cid, path):
    plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, cid)
    plant = uc.CASES[cid][0]
    try:
        n = plan.info["n_values"]
        plan.track_changes()
        assert np.all(plan.dirty() == 0)
        v = _sentinel_array(n)
        plan.execute(v.data_ptr()); plan.synchronize()
        v0 = _bits(v, n)
        for name in pc.CHANGES[plant]:
            a, b, exp, marks = pc.reference(slc, plant, name, P, S, groups)
            assert (0 < marks.sum() < marks.size) if exp == "some" else marks.sum() == 0, (cid, name, marks)
            for back in (False, True):                                    # to the changed values, then back to P's
                _update(plan, (a if not back else _nz(P.A)) if a is not None else None,
                        (b if not back else _nz(P.B2)) if b is not None else None, path)
                assert np.array_equal(plan.dirty(), marks), (cid, name, back)
                assert plan.update_result() == 0
                k = plan.execute_dirty(v.data_ptr()); plan.synchronize()
                assert k == int(marks.sum()), (cid, name, back, k)
                got = _bits(v, n)
                assert np.array_equal(got, _full(plan, n, False)), (cid, name, back)
                assert np.all(plan.dirty() == 0)
                if back:
                    assert np.array_equal(got, v0)
                elif exp == "some" and name != "negzero":
                    assert not np.array_equal(got, v0)                     # the change moved Φ: the re-solve did something
    finally:
        plan.close()


def test_execute_dirty_on_a_localized_plan_and_in_the_packed_layout(slc, gpu_ctx, monkeypatch):
    for localized, packed in ((True, False), (False, True)):
        plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, "wave", localized=localized)
        try:
            n = plan.info["n_packed"] if packed else plan.info["n_values"]
            plan.track_changes()
            v = _sentinel_array(n)
            plan.execute(v.data_ptr(), packed=packed); plan.synchronize()
            a, b, _, marks = pc.reference(slc, "chain70", "A35_36", P, S, groups)
            plan.update_plant(A=a)
            assert np.array_equal(plan.dirty(), marks)
            assert plan.execute_dirty(v.data_ptr(), packed=packed) == int(marks.sum())
            plan.synchronize()
            assert np.array_equal(_bits(v, n), _full(plan, n, packed))
            assert np.all(plan.dirty() == 0)
        finally:
            plan.close()


def test_execute_dirty_on_coupled_groups(slc, gpu_ctx):
    """The coupled plan of test_execute_columns_selects_a_coupled_group_as_a_whole: every column of a group has the group's
    index sets, so the reference marks whole groups and n_solved is their column count."""
    P, S, groups = _coupled(slc)
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        n = plan.info["n_values"]
        sets = pc.index_sets(slc, P, S, groups)
        a = _nz(P.A).copy()
        a[pc._pos(P.A, 1, 1)] += 0.125
        marks = pc.affected(P, sets, *pc.changed_flags(P, a, None))
        grp_of = np.repeat(np.arange(len(groups)), [len(g) for g in groups])
        assert 0 < marks.sum() < marks.size
        assert all(len(set(marks[grp_of == g])) == 1 for g in range(len(groups)))          # whole groups
        assert any(marks[grp_of == g][0] and len(groups[g]) > 1 for g in range(len(groups)))
        plan.track_changes()
        v = _sentinel_array(n)
        plan.execute(v.data_ptr()); plan.synchronize()
        v0 = _bits(v, n)
        plan.update_plant(A=a)
        assert np.array_equal(plan.dirty(), marks)
        assert plan.execute_dirty(v.data_ptr()) == int(marks.sum())
        plan.synchronize()
        got = _bits(v, n)
        assert np.array_equal(got, _full(plan, n, False)) and not np.array_equal(got, v0)
        assert np.all(plan.dirty() == 0)
    finally:
        plan.close()


def test_marks_accumulate_and_tracking_can_be_off(slc, gpu_ctx, monkeypatch):
    plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, "wave")
    try:
        n = plan.info["n_values"]
        a1, _, _, m1 = pc.reference(slc, "chain70", "A35_35", P, S, groups)
        _, b2, _, m2 = pc.reference(slc, "chain70", "B0_0", P, S, groups)
        assert np.any(m1 & ~m2) and np.any(m2 & ~m1)
        # tracking was never on: updates mark nothing, execute_dirty solves nothing and leaves the array alone
        v = _sentinel_array(n)
        plan.update_plant(A=a1)
        assert np.all(plan.dirty() == 0)
        assert plan.execute_dirty(v.data_ptr()) == 0
        plan.synchronize()
        assert np.all(_bits(v, n) == SENTINEL)
        plan.update_plant(A=_nz(P.A))
        # two updates in a row OR their marks; a full execute neither reads nor clears them
        plan.track_changes()
        plan.execute(v.data_ptr()); plan.synchronize()
        plan.update_plant(A=a1)
        assert np.array_equal(plan.dirty(), m1)
        plan.update_plant(B2=_dev(b2))
        assert np.array_equal(plan.dirty(), m1 | m2)
        w = _full(plan, n, False)
        assert np.array_equal(plan.dirty(), m1 | m2)
        assert plan.execute_dirty(v.data_ptr()) == int((m1 | m2).sum())
        plan.synchronize()
        assert np.array_equal(_bits(v, n), w) and np.all(plan.dirty() == 0)
        # clear_dirty drops marks without solving; turning tracking on again clears them too; off: later updates mark nothing
        plan.update_plant(A=_nz(P.A))
        assert np.array_equal(plan.dirty(), m1)
        plan.clear_dirty(); plan.synchronize()
        assert np.all(plan.dirty() == 0)
        plan.update_plant(A=a1)
        plan.track_changes(True)
        assert np.all(plan.dirty() == 0)
        plan.track_changes(False)
        plan.update_plant(A=_nz(P.A), B2=_nz(P.B2))
        assert np.all(plan.dirty() == 0)
    finally:
        plan.close()


def test_a_refused_entry_marks_nothing(slc, gpu_ctx, monkeypatch):
    """Device path on banded_zeros: a plan-time zero set to 0.3 and a NaN on a non-zero entry are refused (update_result counts
    them) and mark nothing; together with an accepted change, only that change marks."""
    plan, P, S, groups, desc = _plan(slc, gpu_ctx, monkeypatch, "t4_zeros")
    try:
        A0 = _nz(P.A)
        kz = pc._pos(P.A, 30, 33); kn = pc._pos(P.A, 30, 30)
        assert A0[kz] == 0.0 and A0[kn] != 0.0
        plan.track_changes()
        for k, val in ((kz, 0.3), (kn, np.nan)):
            a = A0.copy(); a[k] = val
            plan.update_plant(A=_dev(a))
            assert plan.update_result() == 1 and np.all(plan.dirty() == 0)
        sets = pc.index_sets(slc, P, S, groups)
        a = A0.copy(); a[kz] = 0.3; a[pc._pos(P.A, 22, 22)] += 0.5
        good = a.copy(); good[kz] = 0.0
        want = pc.affected(P, sets, *pc.changed_flags(P, good, None))
        assert 0 < want.sum() < want.size
        all_if_counted = pc.affected(P, sets, (a != A0).astype(np.uint8), np.zeros(_nz(P.B2).size, dtype=np.uint8))
        assert not np.array_equal(want, all_if_counted)                    # the refused entry alone would mark other columns
        plan.update_plant(A=_dev(a))
        assert plan.update_result() == 1 and np.array_equal(plan.dirty(), want)
    finally:
        plan.close()


@pytest.mark.parametrize("plant", ["random", "dense_row"])
def test_marks_on_rows_of_one_entry_and_on_a_dense_row(slc, gpu_ctx, monkeypatch, plant):
    """Marks only (nothing is solved): every row of the random plant, A's entries and B2's, and the 72-entry row of B2 of the
    dense-row plant, whose subproblems reach ñu = 72."""
    uc.set_knobs(monkeypatch, {})
    P, S, groups = pc.setting(slc, plant)
    plan = slc.Plan(gpu_ctx, P, S, groups)
    try:
        plan.track_changes()
        for name in pc.CHANGES[plant]:
            a, b, exp, marks = pc.reference(slc, plant, name)
            plan.update_plant(A=a, B2=b)
            assert np.array_equal(plan.dirty(), marks), (plant, name)
            plan.update_plant(A=None if a is None else _nz(P.A), B2=None if b is None else _nz(P.B2))
            plan.clear_dirty()
    finally:
        plan.close()
