"""The stand-alone controller on the host (no GPU): the table builder the plan uses (csrc/sls_symbolic.cpp:
build_controller_operator, through sls_debug_controller_tables) and the serial twin of the device step (csrc/sls_controller.cpp,
through sls_debug_controller_host: the same tables, the same mirrored ring and β double buffer as the kernel) — held to a NumPy
count from the masks and to the long-double statement of the recursion in tests/controller_cases.py, which shares no code with
either.  The reference itself is tied to the simulator's (closed_loop_cases.reference), and every input sequence the controller
tests use is shown to keep max|ŵ| below controller_cases.GROWTH_BOUND: the tolerance RTOL = 1e-11 is relative to max(1, max|ref|),
so a bound on growth is a condition of the comparison, not part of it."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import closed_loop_cases as clc
import controller_cases as cc


@pytest.fixture(scope="module")
def cases():
    return {name: cc.case(name) for name in cc.ALL}


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", cc.ALL)
def test_tables_against_a_numpy_count_from_the_masks(slc, cases, name, base):
    case = cases[name]
    Nx, Nu, T = case.Nx, case.Nu, case.T
    row_ptr, lag, col, perm = slc.controller_tables((Nx, Nu), [case.Sx, case.Su], index_base=base)
    nb, nu = clc.row_lengths(case.Sx, case.Su)
    assert row_ptr[0] == 0 and np.array_equal(np.diff(row_ptr), np.concatenate([nb, nu]))
    assert len(lag) == len(col) == len(perm) == case.n_entries == row_ptr[-1]
    # dense stored-TRUE masks: β row i gathers Sx[τ] (Φx[τ+1]), τ = 1 … T−1; u row j gathers Su[τ−1] (Φu[τ]), τ = 1 … T
    def dense(m):
        m = sp.csc_matrix(m)
        d = np.zeros(m.shape, dtype=bool)
        cols = np.repeat(np.arange(m.shape[1]), np.diff(m.indptr))
        keep = np.asarray(m.data, dtype=bool)
        d[m.indices[keep], cols[keep]] = True
        return d
    Mx = np.array([dense(m) for m in case.Sx[1:]]).reshape(T - 1, Nx, Nx)
    Mu = np.array([dense(m) for m in case.Su]).reshape(T, Nu, Nx)
    vals = case.values[perm]
    assert np.isfinite(vals).all()                                     # no poisoned position: Sx[0] and stored-false entries are absent
    for r in range(Nx + Nu):
        e0, e1 = row_ptr[r], row_ptr[r + 1]
        M = Mx[:, r, :] if r < Nx else Mu[:, r - Nx, :]
        want_lag, want_col = np.nonzero(M)                             # row-major: ascending in (τ, c)
        assert np.array_equal(lag[e0:e1], want_lag + 1) and np.array_equal(col[e0:e1], want_col), (name, r)
        Phi = case.Phix[lag[e0:e1], r, col[e0:e1]] if r < Nx else case.Phiu[lag[e0:e1] - 1, r - Nx, col[e0:e1]]
        assert np.array_equal(vals[e0:e1], Phi), (name, r)             # perm points at the entry's own value
    assert len(np.unique(perm)) == len(perm)
    stored_false = sum(int(np.count_nonzero(~np.asarray(m.data, dtype=bool))) for m in list(case.Sx[1:]) + list(case.Su))
    assert stored_false == (0 if name in clc.SMALL else 1)             # the ladder and the ring cases carry one each
    assert sum(m.nnz for m in case.Sx[1:]) + sum(m.nnz for m in case.Su) == case.n_entries + stored_false


@pytest.mark.parametrize("name", cc.ALL)
def test_host_twin_against_the_long_double_reference(slc, cases, name):
    """x ~ N(0,1) comes from no plant.  nscen 3; the ladder runs 100 steps (its ring of 32 slots wraps three times), the small
    and ring cases 40 (rings of 1, 2, 4, 4 and 8 slots)."""
    case = cases[name]
    steps = cc.HOST_STEPS[name]
    assert steps >= 3 * cc.ring_slots(case.T) + 2
    x = cc.random_x(name, steps, 3)
    ur, wr = cc.reference(case, x)
    u, w = slc.controller_host((case.Nx, case.Nu), [case.Sx, case.Su], case.values, x)
    eu, ew = cc.check(u, ur, f"{name} u"), cc.check(w, wr, f"{name} ŵ")
    print(f"{name}: rel err u {eu:.3e} ŵ {ew:.3e}, max|ŵ| {float(np.abs(wr).max()):.3f}")
    if case.Nu:
        assert np.abs(ur).max() > 0.1
    b1 = slc.controller_host((case.Nx, case.Nu), [case.Sx, case.Su], case.values, x, index_base=1)
    assert np.array_equal(b1[0], u) and np.array_equal(b1[1], w)


@pytest.mark.parametrize("name", ("ladder",) + clc.SMALL)
def test_reference_replays_the_simulators_reference(cases, name):
    """Fed the x of closed_loop_cases.reference, the recursion returns that reference's u in rows 0 … steps−2 with difference
    exactly 0.0; the simulator's last u row is the README's never-assigned zero, the controller computes a value there."""
    case = cases[name]
    w = (clc.ladder_w(3) if name == "ladder" else clc.small_w(3))
    xs, us = clc.reference(case, w)
    u, what = cc.reference(case, xs)
    assert u.dtype == np.longdouble and np.array_equal(u[:-1], us[:-1])
    assert not us[-1].any()
    if case.Nu:
        assert np.abs(u[-1]).max() > 0
    assert not what[0].any()                                           # x_0 = 0 in the simulator


def test_growth_bound_of_every_input_sequence(cases):
    """max|ŵ| ≤ 10 on every sequence the controller tests use: the random-x runs of both test files as they are used, the same
    for 200 steps, and the non-linear interleaved loops (there max|x| as well)."""
    worst = {}
    for name in cc.ALL:
        case = cases[name]
        for steps, nscen in ((cc.HOST_STEPS[name], 3), (200, 3)):
            _, w = cc.reference(case, cc.random_x(name, steps, nscen))
            worst[name] = max(worst.get(name, 0.0), float(np.abs(w).max()))
    _, w = cc.reference(cases["ladder"], cc.random_x("ladder", 70, 130))    # the lane-layout run of the GPU test
    worst["ladder130"] = float(np.abs(w).max())
    for switch in (None, (20, 0.5)):                                        # the run sequence of the GPU test, with and without the new Φ
        _, w = cc.reference(cases["ladder"], cc.random_x("ladder", 40, 3, seed=1), switch=switch)
        worst["sequence"] = max(worst.get("sequence", 0.0), float(np.abs(w).max()))
    for name, steps in cc.LOOP_STEPS.items():
        x0, wd = cc.loop_inputs(name, steps)
        x, _, w = cc.reference_loop(cases[name], x0, wd)
        worst["loop " + name] = max(float(np.abs(w).max()), float(np.abs(x).max()))
    print("max|ŵ| per sequence:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= cc.GROWTH_BOUND, worst


def test_host_code_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_controller.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_controller.cpp: the table
    builder and the host twin on a ladder-like operator (T = 24) and on T = 4 / T = 5, both index bases."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_controller.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_controller.cpp")]
    exe = str(tmp_path / "sanitize_controller")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_controller: clean" in r.stdout and "runtime error" not in r.stderr


def test_abi_version_and_null_context(slc, cases):
    import ctypes as C
    lib = slc.load_library()
    assert lib.sls_abi_version() == 2
    case = cases["T2"]
    m = slc._capi.Marshalled.masks_only(case.Nx, case.Nu, case.Sx, case.Su)
    h = C.c_void_p()
    assert lib.sls_controller_plan(None, 0, C.byref(m.dims), m.Sx, m.Su, 1, C.byref(h)) == slc._capi.SLS_EINVAL
    assert not h.value
    assert "null context" in slc._capi.last_error(None)
