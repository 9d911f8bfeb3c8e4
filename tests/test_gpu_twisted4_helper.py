"""Four-wave twisted kernel after the helper-wave changes (row form of X through LDS, X/S updates held in place per pivot)
and the two-event execute path (a timed execute's stop event is the plan's "done" point)."""
import numpy as np
import pytest


@pytest.mark.gpu
@pytest.mark.parametrize("d,T,expect_cls", [(8, 17, "<32,10"), (8, 24, "<32,10"), (9, 29, "<32,12"), (10, 30, "<32,12")])
def test_four_wave_matches_two_wave_kernel(slc, gpu_ctx, d, T, expect_cls, monkeypatch):
    """ñx = 2d+3 = 19 (class <32,10>) and 21 / 23 (<32,12>), odd and even horizons: the four-wave kernel keeps the statuses of
    the two-wave kernel and agrees with it to 1e-9 on every column."""
    P = slc.workloads.chain_plant(70)
    S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5))
    cols = list(range(20, 50, 3))
    out = {}
    for four, name in (("1", "h2_column_twisted4_kernel"), ("0", "h2_column_twisted_kernel")):
        monkeypatch.setenv("SLS_TWISTED4", four)
        plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
        try:
            assert name + expect_cls in plan.describe(), plan.describe()
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize()
            st, rs, it = plan.fetch_status()
            out[four] = (np.asarray(st).copy(), np.concatenate(sum(plan.download(dv), [])))
        finally:
            plan.close()
    assert np.array_equal(out["1"][0], out["0"][0])
    assert np.all(out["1"][0] == 0)
    assert np.abs(out["1"][1] - out["0"][1]).max() < 1e-9


@pytest.mark.gpu
def test_status_and_timing_follow_the_last_execute(slc, readme):
    """Executes below and above the 64-event timing pool: kernel_time_ms() reports every timed launch (all of them below the
    pool, at least a pool's worth above it), and fetch_status / download see the last execute's results either way.  A status
    read of one plan does not wait for another plan's work queued on a different stream."""
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
