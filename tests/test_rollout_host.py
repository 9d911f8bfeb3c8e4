"""The ensemble rollout on the host (no GPU): the plan-time tables (csrc/sls_rollout.cpp: build_rollout_tables, through
sls_debug_rollout_tables) and the serial twin of the device object (RolloutHost, through sls_debug_rollout_host: the same tables,
mirrored ring, double buffers, owner flags and stats reduction as the kernel) — held to SciPy's own CSR conversion and to the
long-double statement of the recursion in tests/rollout_cases.py, which shares no code with either.  Every reference the rollout
tests use is shown to keep max|x| below rollout_cases.GROWTH_BOUND = 1e6 (the tolerances are relative), and the reference itself
is tied to the simulator's (closed_loop_cases.reference) on the design plant."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import closed_loop_cases as clc
import controller_cases as cc
import rollout_cases as rc


@pytest.fixture(scope="module")
def cases():
    return {name: rc.case(name) for name in rc.ALL}


def _plant(slc, case):
    return slc.Plant(case.A, case.B1, case.B2)


HOST_STEPS = {"ladder": 100, "T1": 40, "T2": 40, "T4": 40, "T5": 40, "Nu0": 40}


@pytest.mark.parametrize("name", rc.ALL)
def test_host_twin_against_the_long_double_reference(slc, cases, name):
    """Per-scenario perturbed plants, a non-zero x_0, weights other than 1, dense w; nscen 3.  The ladder runs 100 steps (its ring
    of 32 slots wraps three times), the others 40."""
    case = cases[name]
    steps, nscen = HOST_STEPS[name], 3
    assert steps >= 3 * cc.ring_slots(case.T) + 2
    Av, Bv = rc.perturbed(case, nscen)
    q, r = rc.weights(case)
    x0, w = rc.initial_state(name, nscen), rc.disturbance(name, steps, nscen)
    ref = rc.reference(case, steps, nscen, w=w, A_vals=Av, B2_vals=Bv, x0=x0, q=q, r=r)
    assert float(np.abs(ref["x"]).max()) < rc.GROWTH_BOUND
    got = slc.rollout_host(_plant(slc, case), [case.Sx, case.Su], case.values, nscen, steps, w=w, A=Av, B2=Bv, per_scenario=True,
                           q=q, r=r, x0=x0)
    errs = rc.check_all(got, ref, name)
    print(name, {k: f"{v:.2e}" for k, v in errs.items()}, "max|x|", float(np.abs(ref["x"]).max()))
    assert np.array_equal(got["x"][0], x0)
    b1 = slc.rollout_host(_plant(slc, case), [case.Sx, case.Su], case.values, nscen, steps, w=w, A=Av, B2=Bv, per_scenario=True,
                          q=q, r=r, x0=x0, index_base=1)
    assert all(np.array_equal(b1[k], got[k]) for k in got)


@pytest.mark.parametrize("name", ("ladder", "T1", "T2", "Nu0"))
def test_reference_replays_the_simulators_reference(cases, name):
    """Design plant, x_0 = 0, one run: the rows of closed_loop_cases.reference (its last u row is the never-assigned zero)."""
    case = cases[name]
    w = clc.ladder_w(3) if name == "ladder" else clc.small_w(3)
    xs, us = clc.reference(case, w)
    ref = rc.reference(case, case.steps - 1, 3, w=w[:-1])
    assert float(np.abs(ref["x"] - xs[:-1]).max()) < 1e-15 and float(np.abs(ref["state"] - xs[-1]).max()) < 1e-15
    if case.Nu:
        assert float(np.abs(ref["u"] - us[:-1]).max()) < 1e-15


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", rc.ALL)
def test_tables_against_scipy_and_the_owner_rule(slc, cases, name, base):
    """CSR of A and B₂ as SciPy builds it, the gather's source positions, and the owner flags: every actuator is counted exactly
    once — by the first state row that stores its column, or by its orphan wave."""
    case = cases[name]
    t = slc.rollout_tables(_plant(slc, case), [case.Sx, case.Su], index_base=base)
    assert t["n_entries"] == case.n_entries
    for M, key in ((case.A, "A"), (case.B2, "B2")):
        csc = sp.csc_matrix(M).copy(); csc.sort_indices()
        pos = sp.csc_matrix((np.arange(1, csc.nnz + 1, dtype=np.float64), csc.indices, csc.indptr), shape=csc.shape).tocsr()
        pos.sort_indices()
        assert np.array_equal(t[key + "_ptr"], pos.indptr) and np.array_equal(t[key + "_idx"], pos.indices)
        assert np.array_equal(t[key + "_src"], pos.data.astype(np.int64) - 1)
        assert np.array_equal(csc.data[t[key + "_src"]], csc.tocsr().data)
    counted = np.zeros(case.Nu, dtype=int)
    np.add.at(counted, t["B2_idx"][t["B2_owner"] == 1], 1)
    np.add.at(counted, t["orphan"], 1)
    assert np.array_equal(counted, np.ones(case.Nu, dtype=int))
    rows = np.repeat(np.arange(case.Nx), np.diff(t["B2_ptr"]))
    for j in range(case.Nu):
        mine = rows[t["B2_idx"] == j]
        if mine.size:
            assert rows[(t["B2_idx"] == j) & (t["B2_owner"] == 1)].tolist() == [mine.min()]
        else:
            assert j in t["orphan"]
    if name == "ladder":
        assert t["orphan"].tolist() == [clc.LADDER_ORPHAN] and int((t["B2_idx"] == clc.LADDER_SHARED).sum()) == 2
    if name == "Nu0":
        assert t["B2_idx"].size == 0 and t["orphan"].size == 0


def test_every_actuator_is_counted_exactly_once(slc, cases):
    """q = 0 and r = e_j: the cost is Σ_k u_k[j]² of the twin's own u — for the actuator two states share, for the orphan, for the
    one with an empty operator row (exactly 0) and for the others; the peak of u is that of the recorded rows."""
    case = cases["ladder"]
    steps, nscen = 40, 2
    w = rc.disturbance("ladder", steps, nscen)
    P, S = _plant(slc, case), [case.Sx, case.Su]
    for j in range(case.Nu):
        r = np.zeros(case.Nu); r[j] = 1.0
        got = slc.rollout_host(P, S, case.values, nscen, steps, w=w, q=np.zeros(case.Nx), r=r)
        want = (got["u"][:, j, :].astype(np.longdouble) ** 2).sum(axis=0)
        if j == 0:
            assert not got["cost"].any()
        else:
            assert float((np.abs(got["cost"] - want) / want).max()) < 1e-14, j
    assert np.array_equal(got["peak_u"], np.abs(got["u"]).max(axis=(0, 1)))
    assert np.array_equal(got["peak_x"], np.abs(got["x"]).max(axis=(0, 1)))


@pytest.mark.parametrize("name", rc.ALL)
def test_a_chunked_run_equals_a_single_run(slc, cases, name):
    case = cases[name]
    steps = rc.ring_steps(case.T)
    Av, Bv = rc.perturbed(case, 2)
    x0, w = rc.initial_state(name, 2), rc.disturbance(name, steps, 2)
    kw = dict(w=w, A=Av, B2=Bv, per_scenario=True, x0=x0)
    P, S = _plant(slc, case), [case.Sx, case.Su]
    one = slc.rollout_host(P, S, case.values, 2, steps, **kw)
    many = slc.rollout_host(P, S, case.values, 2, steps, chunks=rc.ring_chunks(case.T), **kw)
    single = slc.rollout_host(P, S, case.values, 2, steps, chunks=[1] * steps, **kw)
    for k in one:
        assert np.array_equal(one[k], many[k]) and np.array_equal(one[k], single[k]), (name, k)
    with pytest.raises(slc.SLSError):
        slc.rollout_host(P, S, case.values, 2, steps, chunks=[steps - 1], **kw)


def test_shared_values_and_phi_switch(slc, cases):
    """set_plant with one shared array equals per-scenario copies of it; NULL keeps the plan's values; a Φ switched at step 15
    follows the reference that switches at the same step."""
    case = cases["T5"]
    steps, nscen = 30, 3
    Av, Bv = rc.perturbed(case, nscen)
    w = rc.disturbance("T5", steps, nscen)
    P, S = _plant(slc, case), [case.Sx, case.Su]
    a = slc.rollout_host(P, S, case.values, nscen, steps, w=w, A=Av[:, 0], B2=Bv[:, 0])
    b = slc.rollout_host(P, S, case.values, nscen, steps, w=w, A=np.repeat(Av[:, :1], nscen, axis=1), B2=np.repeat(Bv[:, :1], nscen, axis=1),
                         per_scenario=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c = slc.rollout_host(P, S, case.values, nscen, steps, w=w, A=rc.csc_values(case.A))
    d = slc.rollout_host(P, S, case.values, nscen, steps, w=w)
    assert all(np.array_equal(c[k], d[k]) for k in c)
    half = np.where(np.isnan(case.values), np.nan, 0.5 * case.values)
    got = slc.rollout_host(P, S, case.values, nscen, steps, w=w, A=Av, B2=Bv, per_scenario=True, switch=(15, half), chunks=[10, 20])
    ref = rc.reference(case, steps, nscen, w=w, A_vals=Av, B2_vals=Bv, switch=(15, 0.5))
    print({k: f"{v:.2e}" for k, v in rc.check_all(got, ref, "switch").items()})
    assert np.array_equal(got["x"][:16], slc.rollout_host(P, S, case.values, nscen, steps, w=w, A=Av, B2=Bv, per_scenario=True)["x"][:16])


def test_growth_bound_of_every_reference_the_gpu_tests_use(cases):
    """max|x| < 1e6 (in fact far below): the lane-layout run, the ring runs, the sequence run"""
    worst = {}
    case = cases["ladder"]
    Av, Bv = rc.perturbed(case, 130)
    ref = rc.reference(case, rc.LAYOUT_STEPS, 130, w=rc.disturbance("ladder", rc.LAYOUT_STEPS, 130), A_vals=Av, B2_vals=Bv,
                       x0=rc.initial_state("ladder", 130))
    worst["layout"] = float(np.abs(ref["x"]).max())
    for name in rc.RING:
        c = cases[name]
        Av, Bv = rc.perturbed(c, 3)
        n = rc.ring_steps(c.T)
        ref = rc.reference(c, n, 3, w=rc.disturbance(name, n, 3), A_vals=Av, B2_vals=Bv, x0=rc.initial_state(name, 3))
        worst[name] = float(np.abs(ref["x"]).max())
    print("max|x| per reference:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) < rc.GROWTH_BOUND


def test_host_code_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_rollout.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_rollout.cpp."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_rollout.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_rollout.cpp")]
    exe = str(tmp_path / "sanitize_rollout")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_rollout: clean" in r.stdout and "runtime error" not in r.stderr


def test_python_surface_and_null_context(slc, cases):
    new = {"sls_rollout_plan", "sls_rollout_load", "sls_rollout_set_plant", "sls_rollout_set_weights", "sls_rollout_reset",
           "sls_rollout_run", "sls_rollout_stats", "sls_rollout_fetch", "sls_rollout_info", "sls_rollout_destroy"}
    assert new <= set(slc._capi.EXPORTS)
    for name in ("load", "set_plant", "set_weights", "reset", "run", "stats", "state", "from_plant"):
        assert callable(getattr(slc.Rollout, name)), name
    lib = slc.load_library()
    assert lib.sls_abi_version() == 2
    case = cases["T2"]
    m = slc._capi.Marshalled(_plant(slc, case), case.Sx, case.Su)
    h = C.c_void_p()
    assert lib.sls_rollout_plan(None, 0, C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, 1, C.byref(h)) == slc._capi.SLS_EINVAL
    assert not h.value and "null context" in slc._capi.last_error(None)
    assert lib.sls_rollout_run(None, None, None, 1, None, None) == slc._capi.SLS_EINVAL
