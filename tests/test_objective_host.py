"""Objective values on the host (no GPU): sls_debug_objective_host — the host symbolic pass's objective records
(Symbolic::obj_pool) and the serial evaluator of csrc/sls_objective.cpp, the reference the GPU tests compare against.

Bounds.  Against golden costs: the tolerances the suite already uses for the same quantity (tests/test_gpu_parity.py:38-39 for
the README chain; 1e-7·max(1, J), the objective tolerance of tests/test_sum_of_norms.py, for the weighted goldens).  Against the
direct NumPy statement of the reference's formula on the same Φ: the summation bound 2·N·2⁻⁵³·S (objective_cases.summation_bound).
Measured worst cases (this file's prints): README per column 3.9e-14, total 4.3e-11; weighted / general / coupled (dense, diagonal W)
goldens relative 1.3e-15 / 6.6e-16 / 4.9e-15, 1.1e-15; formula cases at most 0.07 of the bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import objective_cases as oc


def test_readme_golden_identity_cost(slc):
    P, S, I, vx, vu, cost = oc.readme_golden(slc)
    col, tot = slc.objective_values_host(P, S, oc.split(vx, S[0]), oc.split(vu, S[1]), I)
    print("README: per column", np.abs(col - cost).max(), "total", abs(tot - 893.3262819770))
    assert np.abs(col - cost).max() < 1e-8
    assert abs(tot - 893.3262819770) < 1e-7
    for c, want in ((1, 1.739859), (11, 23.545630), (30, 18.830872), (59, 22.362423)):     # the project's anchors (1-based columns)
        assert abs(col[c - 1] - want) < 1e-6


@pytest.mark.parametrize("case", ["weighted", "general", "coupled_dense", "coupled_diag"])
def test_weighted_general_and_coupled_goldens(slc, case):
    """`cost` of the oracle's SLS_H2(..., return_diag=True), stored with the golden Φ it belongs to."""
    if case == "weighted":
        P, S, I, vx, vu, cost = oc.weighted_golden(slc)
    elif case == "general":
        P, S, I, vx, vu, cost = oc.general_golden(slc)
    else:
        P, S, I, vx, vu, cost = oc.coupled_golden(slc, case.split("_")[1])
    col, tot = slc.objective_values_host(P, S, oc.split(vx, S[0]), oc.split(vu, S[1]), I)
    if I is not None:
        first = oc.group_firsts(I)
        rest = np.setdiff1d(np.arange(len(col)), first)
        assert np.all(col[rest] == 0.0)            # the joint value sits on the group's first column
        col = col[first]
    rel = np.abs(col - cost) / np.maximum(1.0, np.abs(cost))
    print(case, "worst relative", rel.max())
    assert rel.max() < 1e-7
    assert abs(tot - cost.sum()) < 1e-7 * max(1.0, cost.sum())


@pytest.fixture(scope="module")
def chain23_phi(slc, oracle):
    """One Φ for every cost variant (they share A, B2 and the masks): the oracle's solution of the default cost."""
    P, S, _ = oc.chain23_variant(slc, "default")
    Phix, Phiu = oracle.SLS_H2(oracle.OraclePlant(P.A, P.B1, P.B2), S)
    return Phix, Phiu


@pytest.mark.parametrize("name", ["scale36", "b_zero", "d11", "ridge"])
def test_direct_statement_of_the_reference_formula(slc, oracle, chain23_phi, name):
    P, S, ridge = oc.chain23_variant(slc, name)
    Phix, Phiu = chain23_phi
    vx, vu = oracle.values_in_mask_order(Phix, S[0]), oracle.values_in_mask_order(Phiu, S[1])
    col, tot, n_terms, abs_sum = slc.objective_values_host(P, S, vx, vu, ridge=ridge, return_bound=True)
    want = oc.reference_formula(oracle, P, S, Phix, Phiu, ridge)
    if name == "b_zero":
        # B1[7,7] = 0: the column's true cost is the constant (0 here) whatever Φ is; it minimised, and reports, the norm of its
        # minimum-norm point (include/sls_mi355x.h)
        assert want[7] == 0.0
        want[7] = sum(float(F[:, 7].multiply(F[:, 7]).sum()) for F in Phix + Phiu)
    bound = oc.summation_bound(n_terms, abs_sum)
    print(name, "worst |Δ|/bound", (np.abs(col - want) / bound).max())
    assert np.all(np.abs(col - want) <= bound)
    assert abs(tot - want.sum()) <= bound.sum() + 2 * len(col) * oc.U * np.abs(want).sum()
    if name == "scale36":
        base, _ = slc.objective_values_host(*oc.chain23_variant(slc, "default")[:2], vx, vu)
        assert np.all(np.abs(col - 36.0 * base) <= bound)


def test_index_base_one_gives_the_same_bits(slc):
    P, S, I, vx, vu, _ = oc.coupled_golden(slc, "dense")
    a = slc.objective_values_host(P, S, oc.split(vx, S[0]), oc.split(vu, S[1]), I)
    b = slc.objective_values_host(P, S, oc.split(vx, S[0]), oc.split(vu, S[1]), I, index_base=1)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_host_evaluator_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_objective.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_objective.cpp: identity,
    diagonal, dense and coupled costs, D11, a ridge term, a b = 0 column, both objectives, both index bases."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_objective.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_objective.cpp")]
    exe = str(tmp_path / "sanitize_objective")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_objective: clean" in r.stdout and "runtime error" not in r.stderr
