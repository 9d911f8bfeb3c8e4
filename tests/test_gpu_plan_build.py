"""Plan construction (csrc/sls_plan_build.cpp on csrc/sls_arena.h) on the device: the footprint of every plan against the one
recorded before construction moved to the shared arena type (tests/golden/plan_footprints.json), a reused and dirty arena, a
second live plan with its own arena, scratch and streams, and the two first-use allocations that are laid out by the same arena
(partial re-solve, achievability residual).  Small shapes; every test builds a handful of plans."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _load_gen():
    spec = importlib.util.spec_from_file_location("make_golden_plan_footprints", os.path.join(GOLDEN, "make_golden_plan_footprints.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_gen()
with open(os.path.join(GOLDEN, "plan_footprints.json")) as _f:
    RECORDED = json.load(_f)
CASES = {c["name"]: c for c in gen.cases()}


def _solve(plan):
    """(Φ in mask order, status, residual, iters) of one execute."""
    dv = plan.alloc_values()
    plan.execute(dv); plan.synchronize()
    st, rs, it = (np.asarray(a).copy() for a in plan.fetch_status())
    return np.concatenate(sum(plan.download(dv), [])), st, rs, it


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


_fresh = {}


def _fresh_result(slc, plant):
    """The plan of `plant` built on a context of its own and solved: computed once, shared, never changed."""
    if plant not in _fresh:
        P, S, _ = gen.problem(slc, plant)
        with slc.Context([0]) as ctx:
            plan = slc.Plan(ctx, P, S)
            try:
                _fresh[plant] = _solve(plan)
            finally:
                plan.close()
        for a in _fresh[plant]:
            a.setflags(write=False)
    return _fresh[plant]


def test_recorded_cases_are_the_generators():
    assert set(CASES) == set(RECORDED["cases"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_footprint_equals_the_recorded_one(slc, name):
    """workspace_bytes, n_packed, n_values and describe() of the plan, on a context that lends everything, equal what the build of
    RECORDED["commit"] gave on the same device type; a refusal is refused with the same text."""
    import torch
    assert int(torch.cuda.get_device_properties(0).multi_processor_count) == RECORDED["ncu"]
    with slc.Context([0]) as ctx:
        got = gen.footprint(slc, ctx, CASES[name])
    print(name, got)
    assert got == RECORDED["cases"][name]


def test_reused_dirty_arena_gives_the_fresh_context_results(slc):
    """One context: the README plan is built, run, fetched and destroyed; then a smaller plan (chain of 24 states, T = 4) and the
    README plan again borrow the arena, scratch and streams it left behind.  Each gives Φ, status, residual and iteration counts
    bitwise equal to the same plan on a fresh context, and before its first execute a host-path update with its own values is
    refused nowhere: the refusal counter and the status words were cleared, not inherited.  (The short horizon leaves the columns
    of the smaller plan infeasible, on the fresh context too: its status words are not the README plan's zeros.  No small plan is more than 4× + 64 MiB
    apart from another: the re-allocation for a wastefully large arena is not reached here.)"""
    with slc.Context([0]) as ctx:
        P, S, _ = gen.problem(slc, "readme_chain")
        first = slc.Plan(ctx, P, S)
        try:
            ws_first = first.info["workspace_bytes"]
            assert _same(_solve(first), _fresh_result(slc, "readme_chain"))
        finally:
            first.close()
        for plant in ("chain24_T4", "readme_chain"):
            P, S, _ = gen.problem(slc, plant)
            plan = slc.Plan(ctx, P, S)
            try:
                plan.update_plant(A=P.A, B2=P.B2)
                assert plan.update_result() == 0
                assert _same(_solve(plan), _fresh_result(slc, plant)), plant
                if plant == "readme_chain":
                    assert plan.info["workspace_bytes"] == ws_first
            finally:
                plan.close()


@pytest.mark.parametrize("first_closed", ["older", "newer"])
def test_second_live_plan_has_its_own_arena_scratch_and_streams(slc, first_closed):
    """Two plans alive on one context: the second cannot borrow.  Both execute (the first again after the second was built and
    run) and equal the fresh-context results bitwise; they are destroyed in either order; a third plan then borrows again and
    reports the recorded workspace_bytes."""
    with slc.Context([0]) as ctx:
        P, S, _ = gen.problem(slc, "readme_chain")
        Q, R, _ = gen.problem(slc, "chain24_T4")
        a = slc.Plan(ctx, P, S)
        b = None
        try:
            b = slc.Plan(ctx, Q, R)
            got_a = _solve(a)
            got_b = _solve(b)
            again_a = _solve(a)
            assert _same(got_a, _fresh_result(slc, "readme_chain")) and _same(again_a, got_a)
            assert _same(got_b, _fresh_result(slc, "chain24_T4"))
        finally:
            for p in ((a, b) if first_closed == "older" else (b, a)):
                if p is not None:
                    p.close()
        c = slc.Plan(ctx, P, S)
        try:
            assert c.info["workspace_bytes"] == RECORDED["cases"]["readme_chain"]["workspace_bytes"]
            assert _same(_solve(c), _fresh_result(slc, "readme_chain"))
        finally:
            c.close()


def test_partial_resolve_buffers_start_cleared_on_a_used_arena(slc):
    """The marks of the partial re-solve come from an allocation of their own, made by the first call: right after
    track_changes(on) they are all zero, on a plan whose arena and scratch an earlier plan has used."""
    with slc.Context([0]) as ctx:
        P, S, _ = gen.problem(slc, "readme_chain")
        first = slc.Plan(ctx, P, S)
        try:
            _solve(first)
        finally:
            first.close()
        plan = slc.Plan(ctx, P, S)
        try:
            ws = plan.info["workspace_bytes"]
            plan.track_changes(True)
            d = plan.dirty()
            assert d.shape == (plan.info["n_subproblems"],) and not d.any()
            assert _same(_solve(plan), _fresh_result(slc, "readme_chain"))          # the launch table behind the cleared buffers is intact
            dv = plan.alloc_values()
            plan.execute(dv); plan.synchronize()
            assert plan.execute_columns(dv, [0, 7, 58]) == 3
            plan.synchronize()
            assert np.array_equal(np.concatenate(sum(plan.download(dv), [])), _fresh_result(slc, "readme_chain")[0])
            info = slc._capi.sls_plan_info()
            slc._capi.check(plan._lib.sls_plan_get_info(plan.handle, ctypes.byref(info)))
            assert info.workspace_bytes == ws                                       # not counted in the plan's footprint
        finally:
            plan.close()


def test_residual_with_an_empty_halo_list_equals_the_recorded_values(slc):
    """sls_plan_fetch_residual on two uncoupled blocks of 3 states, T = 2: every index set is its block, so the halo list is empty
    and its table has nothing to upload.  Bitwise the values recorded with the footprints."""
    with slc.Context([0]) as ctx:
        got = gen.two_blocks_residual(slc, ctx)
    print(got)
    assert got["halo_inf"] == [0.0] * 6                       # no halo row at all
    assert got == RECORDED["residual"]
