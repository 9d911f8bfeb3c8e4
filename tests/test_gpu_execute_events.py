"""sls_plan_execute with the timing events bound to the solve kernel's own dispatch (a plan that executes as one launch) against
the same build with SLS_EXEC_MARKERS=1, which records the events around the launch as every other plan does.

The knob is read when a plan is built, so both paths live in one process: a plan built inside `_markers(monkeypatch, True)` keeps
the stream markers, one built inside `_markers(monkeypatch, False)` takes the dispatch path where it applies.  Results are compared
as bits; there is no tolerance except in the interval test, whose bounds are stated there."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import update_cases as uc

pytestmark = pytest.mark.gpu

POOL = 64          # kEventPool: timed executes in flight per plan
SENTINEL = np.uint64(0x7FF8DEAD0000BEEF)


def _markers(monkeypatch, on):
    if on:
        monkeypatch.setenv("SLS_EXEC_MARKERS", "1")
    else:
        monkeypatch.delenv("SLS_EXEC_MARKERS", raising=False)


def _plan(slc, ctx, P, S, monkeypatch, markers, groups=None):
    _markers(monkeypatch, markers)
    plan = slc.Plan(ctx, P, S, groups)
    monkeypatch.delenv("SLS_EXEC_MARKERS", raising=False)
    return plan


def _launches(plan):
    return [s for s in plan.describe().split(";") if s.strip()]


def _results(plan, dv):
    st, rs, it = plan.fetch_status()
    phi = np.concatenate(sum(plan.download(dv), []))
    return (np.asarray(st).copy(), np.asarray(rs).view(np.uint64).copy(), np.asarray(it).copy(), phi.view(np.uint64).copy())


def test_both_paths_give_the_same_answers(slc, gpu_ctx, readme, monkeypatch):
    """1, 3 and 70 executes enqueued back to back (70 > pool: the last ones go untimed), then status and Φ: equal bits."""
    P, S, _ = readme
    fast = _plan(slc, gpu_ctx, P, S, monkeypatch, False)
    mark = _plan(slc, gpu_ctx, P, S, monkeypatch, True)
    try:
        assert len(_launches(fast)) == 1 and len(_launches(mark)) == 1, (fast.describe(), mark.describe())
        df, dm = fast.alloc_values(), mark.alloc_values()
        for k in (1, 3, 70):
            for plan, dv in ((fast, df), (mark, dm)):
                for _ in range(k):
                    plan.execute(dv)
            rf, rm = _results(fast, df), _results(mark, dm)
            assert np.all(rf[0] == 0), rf[0]
            for a, b in zip(rf, rm):
                assert np.array_equal(a, b), k
    finally:
        fast.close(); mark.close()


def test_every_timed_execute_is_counted(slc, gpu_ctx, readme, monkeypatch):
    P, S, _ = readme
    plan = _plan(slc, gpu_ctx, P, S, monkeypatch, False)
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        plan.kernel_time_ms()                  # drain
        for k in (1, 3, POOL):
            for _ in range(k):
                plan.execute(dv)
            ms, n = plan.kernel_time_ms()
            print(f"k={k}: n={n} avg {ms:.5f} ms")
            assert n == k and ms > 0
        for _ in range(200):
            plan.execute(dv)
        ms, n = plan.kernel_time_ms()
        print(f"k=200: n={n} avg {ms:.5f} ms")
        assert POOL <= n <= 200 and ms > 0
    finally:
        plan.close()


def test_the_interval_is_the_kernel(slc, gpu_ctx, readme, monkeypatch):
    """0.8 · ms_mark ≤ ms_fast ≤ wall.  Lower bound: profiles/r10_bench_readme.json against the kernel trace of the same round
    put the dispatch at 0.97 of the marker interval; a start event that took the end time, or a pair bound to different commands,
    lands far below 0.8.  Upper bound: a kernel cannot last longer than a synchronised call of it."""
    P, S, _ = readme
    out = {}
    for name, markers in (("fast", False), ("mark", True)):
        plan = _plan(slc, gpu_ctx, P, S, monkeypatch, markers)
        try:
            dv = plan.alloc_values()
            for _ in range(8):
                plan.execute(dv)
            plan.synchronize(); plan.kernel_time_ms()
            for _ in range(32):
                plan.execute(dv)
            ms, n = plan.kernel_time_ms()
            assert n == 32
            out[name] = ms
            if not markers:
                t0 = time.perf_counter()
                for _ in range(32):
                    plan.execute(dv); plan.synchronize()
                out["wall"] = 1e3 * (time.perf_counter() - t0) / 32
        finally:
            plan.close()
    print(f"ms_fast {out['fast']:.5f}  ms_mark {out['mark']:.5f}  wall {out['wall']:.5f}")
    assert 0.8 * out["mark"] <= out["fast"] <= out["wall"], out


def test_status_and_timing_follow_the_last_execute(slc, readme):
    """tests/test_gpu_twisted4_helper.py's test of the same name, on the dispatch path: executes below and above the 64-event
    timing pool, kernel_time_ms() reports every timed launch, fetch_status / download see the last execute's results either way,
    and a status read of one plan does not wait for another plan's work queued on a different stream."""
    import torch
    P, S, _ = readme
    ctx = slc.Context([0])
    try:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        a = slc.Plan(ctx, P, S)
        b = slc.Plan(ctx, P, S)
        da, db = a.alloc_values(), b.alloc_values()
        a.kernel_time_ms()                     # drain the accumulator
        b.kernel_time_ms()
        for _ in range(3):
            a.execute(da, stream=sa.cuda_stream)
        st_a, rs_a, _ = a.fetch_status()
        va = np.concatenate(sum(a.download(da), []))
        ms, n = a.kernel_time_ms()
        assert n == 3 and ms > 0
        assert np.all(np.asarray(st_a) == 0)

        k = 600
        for _ in range(k):
            b.execute(db, stream=sb.cuda_stream)
        a.execute(da, stream=sa.cuda_stream)
        st_a2, _, _ = a.fetch_status()         # waits for a's last execute only
        b_busy = not sb.query()
        assert b_busy, "stream of plan b finished before plan a's status read returned: cannot tell the waits apart"
        st_b, rs_b, _ = b.fetch_status()       # waits for b's last execute (untimed once the pool is full)
        assert sb.query()
        vb = np.concatenate(sum(b.download(db), []))
        ms_b, n_b = b.kernel_time_ms()
        assert 64 <= n_b <= k and ms_b > 0
        assert np.array_equal(np.asarray(st_a2), np.asarray(st_a)) and np.array_equal(np.asarray(st_b), np.asarray(st_a))
        assert np.array_equal(va, vb)
        a.close(); b.close()
    finally:
        ctx.close()


def _column_of_entry(plan, S):
    """col[i] = the column (= subproblem: the plan has no groups) that writes entry i of the mask-order value array"""
    col = -np.ones(plan.info["n_values"], dtype=np.int64)
    for masks, offs in ((S[0], plan.off_x), (S[1], plan.off_u)):
        for t, M in enumerate(masks):
            M = sp.csc_matrix(M); M.sort_indices()
            assert offs[t + 1] - offs[t] == M.nnz
            col[offs[t]:offs[t + 1]] = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    assert col.min() >= 0
    return col


def test_selected_run_ends_at_its_kernel(slc, gpu_ctx, readme, monkeypatch):
    """execute_columns on three columns into a sentinel array, then download with no synchronisation in between: the three
    columns hold the full execute's bits, every other entry the sentinel, and the marker build gives the same array."""
    import torch
    P, S, _ = readme
    subs = [0, 7, 58]
    got = {}
    for name, markers in (("fast", False), ("mark", True)):
        plan = _plan(slc, gpu_ctx, P, S, monkeypatch, markers)
        try:
            assert len(_launches(plan)) == 1
            n = plan.info["n_values"]
            full = torch.zeros(n, dtype=torch.float64, device="cuda:0")
            v = torch.from_numpy(np.full(n, SENTINEL, dtype=np.uint64).view(np.float64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            plan.execute(full.data_ptr())
            ref = np.concatenate(sum(plan.download(full.data_ptr()), [])).view(np.uint64).copy()
            assert plan.execute_columns(v.data_ptr(), subs) == len(subs)
            out = np.concatenate(sum(plan.download(v.data_ptr()), [])).view(np.uint64).copy()
            sel = np.isin(_column_of_entry(plan, S), subs)
            assert sel.any() and not sel.all()
            assert np.array_equal(out[sel], ref[sel])
            assert np.all(ref[sel] != SENTINEL)
            assert np.all(out[~sel] == SENTINEL)
            got[name] = out
        finally:
            plan.close()
    assert np.array_equal(got["fast"], got["mark"])


def test_two_launch_plan_keeps_the_markers(slc, gpu_ctx, monkeypatch):
    """update_cases' `tile` case executes as two launches (tile + twisted) behind a counter memset: the dispatch path does not
    apply whatever the knob says — three executes are three timed intervals, and Φ has the same bits under both settings."""
    P, S, groups, knobs, route, _ = uc.case(slc, "tile")
    uc.set_knobs(monkeypatch, knobs)
    phi = {}
    for markers in (False, True):
        plan = _plan(slc, gpu_ctx, P, S, monkeypatch, markers, groups)
        try:
            assert len(_launches(plan)) == 2 and route in plan.describe(), plan.describe()
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize(); plan.kernel_time_ms()
            for _ in range(3):
                plan.execute(dv)
            ms, n = plan.kernel_time_ms()
            assert n == 3 and ms > 0
            phi[markers] = np.concatenate(sum(plan.download(dv), [])).view(np.uint64).copy()
        finally:
            plan.close()
    assert np.array_equal(phi[False], phi[True])
