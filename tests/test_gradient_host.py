"""Host side of the gradient of the 𝓗₂ cost in A, B2 and the LQR diagonals (include/sls_mi355x.h: sls_plan_gradient):
no device anywhere in this file.

  1. The reference (gradient_cases.py: dense per-column KKT, minimum-norm multiplier, envelope formulas) against central
     differences of the reference's own total cost, for EVERY stored entry of A and B2 and every diagonal weight, on chain17,
     weighted and groups.  Step h = 1e-6; bound 1e-7·max|fd| per array: the O(h²) truncation (h²/6 times a third derivative)
     plus the differences' cancellation (a few 2⁻⁵³·J/h = 1e-10·J, absolute, with J of the size of max|fd|), with margin.
     Measured worst, relative to max|fd|: 1.7e-9 for A, 7.6e-9 for B2, 1.6e-9 for the weights (`-s` prints every figure).
  2. The library's host twin (`gradient_host`, long double, device order) given the reference's μ and z, per entry within
     4·N·2⁻⁵³·Σ|terms| of the reference's double evaluation (N products; both sides round differently).
  3. The entry tables against a brute-force enumeration; every stored entry has a (subproblem, slot) pair or lies outside every
     index set.
  4. csrc/sls_gradient.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_sanitize/sanitize_gradient.cpp).
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gradient_cases as gc

H = 1e-6
FD_CASES = ("chain17", "weighted", "groups")


def _central(f, x0):
    """central differences of f in every component of x0, step H (the SVDs release the GIL: eight threads)."""
    def one(i):
        xp, xm = x0.copy(), x0.copy()
        xp[i] += H; xm[i] -= H
        return (f(xp) - f(xm)) / (2 * H)
    with ThreadPoolExecutor(8) as ex:
        return np.array(list(ex.map(one, range(x0.size))))


@pytest.mark.parametrize("name", FD_CASES)
def test_reference_matches_central_differences(slc, name):
    cs, ref = gc.case(slc, name), gc.reference(slc, name)
    assert ref["live"].all(), "every column of this case is feasible"
    P = cs["P"]
    A, B2, C1, D12 = gc._csc(P.A), gc._csc(P.B2), gc._csc(P.C1), gc._csc(P.D12)
    assert C1.nnz == P.Nx and D12.nnz == P.Nu, "diagonal weights: one stored entry per column"
    for label, x0, g, kw in (("A", A.data, ref["gA"], "A_data"), ("B2", B2.data, ref["gB2"], "B2_data"),
                             ("c1", C1.data, ref["gc1"], "c1"), ("d12", D12.data, ref["gd12"], "d12")):
        fd = _central(lambda x, kw=kw: gc.total_cost(slc, name, **{kw: x}), np.array(x0, dtype=np.float64))
        err, big = np.abs(fd - g).max(), np.abs(fd).max()
        print(f"{name} {label}: max|fd − g| = {err:.2e}, max|fd| = {big:.3e}, relative {err / big:.1e}")
        assert err <= 1e-7 * big, (name, label, err, big)


@pytest.mark.parametrize("name", gc.NAMES)
def test_reference_is_stationary(slc, name):
    ref = gc.reference(slc, name)
    print(f"{name}: ‖Eᵀμ − ∇J‖∞ / max|∇J| = {ref['stationarity']:.1e} over {int(ref['live'].sum())} feasible columns")
    assert ref["stationarity"] <= 1e-10 and ref["live"].any()


@pytest.mark.parametrize("name", gc.NAMES)
def test_twin_against_reference(slc, name):
    cs, ref = gc.case(slc, name), gc.reference(slc, name)
    vx, vu = gc.mask_order_values(slc, name)
    status = np.where(ref["live"], 0, 1).astype(np.int32)
    gA, gB, bd = slc.gradient_host(cs["P"], cs["S"], ref["mu"], vx, vu, cs["I"], col_status=status, return_bound=True)
    for label, got, want, n, s in (("A", gA, ref["gA"], bd["terms_A"], bd["abs_A"]), ("B2", gB, ref["gB2"], bd["terms_B2"], bd["abs_B2"])):
        bound = 4.0 * n * 2.0 ** -53 * s
        print(f"{name} {label}: max|twin − ref| = {np.abs(got - want).max():.2e}, largest bound {bound.max():.2e}")
        assert np.all(np.abs(got - want) <= bound), (name, label)
        assert np.all(got[n == 0] == 0.0)
    # column weights: a unit vector gives that column's own gradient, all-ones the default
    ones = slc.gradient_host(cs["P"], cs["S"], ref["mu"], vx, vu, cs["I"], col_status=status, column_weights=np.ones(len(ref["mu"])))
    assert np.array_equal(ones[0], gA) and np.array_equal(ones[1], gB)
    j = int(np.flatnonzero(ref["live"])[0])
    e = np.zeros(len(ref["mu"])); e[j] = 1.0
    own = slc.gradient_host(cs["P"], cs["S"], ref["mu"], vx, vu, cs["I"], col_status=status, column_weights=e)
    live_j = np.zeros(len(ref["mu"]), dtype=bool); live_j[j] = True
    wantA, wantB, _, _ = gc.gradient_from(cs["P"], ref["cps"], ref["mu"], ref["z"], live_j)
    assert np.abs(own[0] - wantA).max() <= 1e-12 * max(np.abs(wantA).max(), 1.0)
    assert np.abs(own[1] - wantB).max() <= 1e-12 * max(np.abs(wantB).max(), 1.0)


@pytest.mark.parametrize("name", gc.NAMES)
def test_tables_against_enumeration(slc, name):
    cs, ref = gc.case(slc, name), gc.reference(slc, name)
    tb = slc.gradient_tables(cs["P"], cs["S"], cs["I"])
    got = sorted((int(q), int(p), int(a), int(b)) for q in range(len(ref["cps"]))
                 for p, a, b in tb["ent"][tb["ent_ptr"][q]:tb["ent_ptr"][q + 1]])
    want = sorted(gc.brute_tables(cs["P"], ref["cps"]))
    assert got == want and len(got) > 0
    # the inverse map: per stored entry its slots, subproblems ascending, every slot once
    nent = cs["P"].A.nnz + cs["P"].B2.nnz
    assert tb["inv_ptr"].size == nent + 1 and tb["inv_ptr"][-1] == len(got)
    assert sorted(tb["inv_slot"].tolist()) == list(range(len(got)))
    sub_of_slot = np.repeat(np.arange(len(ref["cps"])), np.diff(tb["ent_ptr"]))
    for p in range(nent):
        sl = tb["inv_slot"][tb["inv_ptr"][p]:tb["inv_ptr"][p + 1]]
        assert np.all(tb["ent"][sl, 0] == p)
        assert np.array_equal(tb["inv_sub"][tb["inv_ptr"][p]:tb["inv_ptr"][p + 1]], sub_of_slot[sl])
        assert np.all(np.diff(sub_of_slot[sl]) > 0)
        # an entry without a pair is outside every index set (by the enumeration, which looked at every subproblem)
        if sl.size == 0:
            assert not any(w[1] == p for w in want)


def test_host_code_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_gradient.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_gradient.cpp."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_gradient.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_gradient.cpp")]
    exe = str(tmp_path / "sanitize_gradient")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_gradient: clean" in r.stdout and "runtime error" not in r.stderr


def test_python_surface(slc):
    assert slc._capi.SLS_PLAN_MULTIPLIERS == 4 and slc._capi.SLS_ABI_VERSION == 2
    lib = slc.load_library()
    for sym in ("sls_plan_gradient", "sls_plan_fetch_gradient", "sls_plan_fetch_multipliers", "sls_debug_gradient_host"):
        assert hasattr(lib, sym)
    for name in ("gradient", "gradient_values", "multipliers"):
        assert callable(getattr(slc.Plan, name))
    assert callable(slc.h2_cost) and callable(slc.gradient_host) and callable(slc.gradient_tables)
