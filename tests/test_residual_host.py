"""Achievability residual on the host (no GPU): sls_debug_residual_host — the host symbolic pass, the halo lists of
csrc/sls_symbolic.cpp (build_halo_rows) and the serial evaluator of csrc/sls_residual.cpp, the reference the GPU tests compare
against — held to a NumPy statement of the definition (residual_cases.numpy_residual: dense columns, np.longdouble) that shares
no code with it.

Bound.  Both sides accumulate in long double and round once, so they differ by far less than what the twin reports for a
double-precision evaluation of the same sums in another order: 2·N·2⁻⁵³·S (objective_cases.summation_bound) with, per column, N the
largest term count of one entry of Δ and S the largest sum of absolute terms (res_inf, halo_inf), or the term count and absolute
sum of the whole column (res_l1).  That is the bound the GPU tests use; no tolerance here is hand-picked."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import objective_cases as oc
import residual_cases as rc


def _check_against_numpy(slc, oracle, P, S, I, vx, vu, tag):
    r, b, halo = slc.residual_host(P, S, vx, vu, I, return_bound=True, return_halo=True)
    want_inf, want_halo, want_l1, want_H = rc.numpy_residual(oracle, P, S, I, vx, vu)
    assert len(halo) == len(want_H) == len(r.res_inf)
    for q, (h, w) in enumerate(zip(halo, want_H)):                     # H(q) as an exact set, ascending
        assert np.array_equal(h, w), (tag, q, h, w)
    eb = oc.summation_bound(b["ent_terms"], b["ent_abs"])
    lb = oc.summation_bound(b["l1_terms"], b["l1_abs"])
    print(tag, "worst |Δ|/bound: res_inf", float((np.abs(r.res_inf - want_inf) / np.maximum(eb, 1e-300)).max()),
          "halo_inf", float((np.abs(r.halo_inf - want_halo) / np.maximum(eb, 1e-300)).max()),
          "res_l1", float((np.abs(r.res_l1 - want_l1) / np.maximum(lb, 1e-300)).max()), "| max_inf", r.max_inf, "E1", r.e1_norm)
    assert np.all(np.abs(r.res_inf - want_inf) <= eb)
    assert np.all(np.abs(r.halo_inf - want_halo) <= eb)
    assert np.all(np.abs(r.res_l1 - want_l1) <= lb)
    empty = np.array([h.size == 0 for h in want_H])
    assert np.all(r.halo_inf[empty] == 0.0) and not np.any(np.signbit(r.halo_inf[empty]))
    assert r.max_inf == r.res_inf.max() and r.e1_norm == r.res_l1.max()
    return r, want_H


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_twin_against_the_numpy_statement_on_the_goldens(slc, oracle, name):
    P, S, I, vx, vu = rc.golden_case(slc, name)
    r, H = _check_against_numpy(slc, oracle, P, S, I, vx, vu, name)
    if name == "readme":
        # By pattern every column has halo rows (s_x is the band of d + 1 states around c, A reaches one state further), but the
        # masks keep Φ off the outermost rows of s_x, so nothing arrives there: exactly 0.0, not merely small
        assert all(h.size > 0 for h in H) and np.all(r.halo_inf == 0.0)
        assert r.max_inf <= 1e-9                                        # the suite's certificate level for a solve
    if name == "infeasible":
        g = np.load(os.path.join(rc.GOLDEN, "infeasible_chain.npz"))
        bad = g["col_resid"] > 1e-9
        assert bad.sum() == 12 and np.all(r.res_inf[bad] > 1e-9) and np.all(r.res_inf[~bad] <= 1e-9)
    if name in ("coupled_dense", "coupled_diag", "grouped"):
        assert len(r.res_inf) == P.Nx == sum(len(g) for g in I)        # one value per column of every group


@pytest.fixture(scope="module")
def oracle_phi(slc, oracle):
    """Φ of the cases without a golden, once per module: the Python oracle for the small chains (it also reports the reduced
    residual the status rests on), the C restatement for the grids."""
    import sls_oracle_cport as cp
    out = {}
    for name in rc.ORACLE_CASES:
        P, S, I = rc.oracle_case(slc, name)
        Po = oracle.OraclePlant(P.A, P.B1, P.B2)
        if name.startswith("grid"):
            Phix, Phiu, info = cp.SLS_H2(Po, S, nthreads=8)
            reduced = np.asarray(info["resid"])
        else:
            Phix, Phiu, dg = oracle.SLS_H2(Po, S, return_diag=True)
            reduced = np.array([d["resid"] for d in dg])
        out[name] = (P, S, I, oracle.values_in_mask_order(Phix, S[0]), oracle.values_in_mask_order(Phiu, S[1]), reduced)
    return out


@pytest.mark.parametrize("name", rc.ORACLE_CASES)
def test_twin_against_the_numpy_statement_on_oracle_solutions(slc, oracle, oracle_phi, name):
    P, S, I, vx, vu, reduced = oracle_phi[name]
    r, H = _check_against_numpy(slc, oracle, P, S, I, vx, vu, name)
    b = slc.residual_host(P, S, vx, vu, I, return_bound=True)[1]
    if name == "halo":
        # the case must not degenerate: columns the reduced problem calls solved (SLS_COL_OK level, 1e-9) whose Φ breaks the
        # full-plant identities on rows outside s_x
        ok_but_invalid = (reduced <= 1e-9) & (r.halo_inf > 1e-3)
        print("halo: reduced residual", reduced, "halo_inf", r.halo_inf)
        assert ok_but_invalid.any()
        assert np.all(r.res_inf >= r.halo_inf)
    if name in ("grid9", "grid12"):
        rows = np.array([h.size for h in H]) + np.array([len(oracle.sparsity_dim_reduction(
            oracle.OraclePlant(P.A, P.B1, P.B2), [c], S)[3]) for c in range(P.Nx)])
        edge = 64 if name == "grid9" else 128
        assert rows.min() < edge < rows.max() and edge in rows           # one stride more on some columns than on others
    if name == "dense_rows":
        na, nb = np.diff(P.A.tocsr().indptr), np.diff(P.B2.tocsr().indptr)
        assert na[5] > 8 and na[2] <= 8 < na[2] + nb[2] and na[9] == 8 and nb[9] == 1   # the three ways past eight entries a row
        assert b["ent_terms"].max() > 9
    if name == "whole":
        assert all(h.size == 0 for h in H) and np.all(r.halo_inf == 0.0)  # s_x is the whole plant: no row is left for a halo
    if name in ("T1", "T2"):
        assert len(S[0]) == int(name[1]) and np.all(r.res_inf > 1e-9)     # too short a horizon to be feasible: least-squares points


def test_stale_phi_against_a_changed_plant(slc, oracle):
    """The README Φ against a plant whose A moved on three entries: the twin sees the defect, the NumPy statement agrees."""
    P, S, I, vx, vu = rc.golden_case(slc, "readme")
    P2 = slc.Plant(rc.perturbed_A(P), P.B1, P.B2)
    r, _ = _check_against_numpy(slc, oracle, P2, S, I, vx, vu, "stale")
    assert r.max_inf > 1e-6


def test_trivial_column_reports_one(slc, oracle):
    """A column outside its own s_x (row 5 taken out of the mask columns s_x(5) is the union of): Φ = 0 and row c sits in the halo —
    1.0 in all three numbers."""
    P, S, _ = rc.oracle_case(slc, "T2")
    Sx = [m.tolil(copy=True) for m in S[0]]
    for m in Sx:
        m[5, 4:7] = False
    Sx = [m.tocsc() for m in Sx]
    for m in Sx:
        m.eliminate_zeros(); m.sort_indices()
    S2 = [Sx, S[1]]
    vx = [np.zeros(m.nnz) for m in S2[0]]; vu = [np.zeros(m.nnz) for m in S2[1]]
    r, halo = slc.residual_host(P, S2, vx, vu, return_halo=True)
    assert 5 in halo[5] and 5 not in oracle.sparsity_dim_reduction(oracle.OraclePlant(P.A, P.B1, P.B2), [5], S2)[3]
    assert r.res_inf[5] == 1.0 and r.halo_inf[5] == 1.0 and r.res_l1[5] == 1.0
    _check_against_numpy(slc, oracle, P, S2, None, vx, vu, "trivial")


def test_index_base_one_gives_the_same_bits(slc):
    P, S, I, vx, vu = rc.golden_case(slc, "coupled_dense")
    a = slc.residual_host(P, S, vx, vu, I)
    b = slc.residual_host(P, S, vx, vu, I, index_base=1)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def test_host_twin_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_residual.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_residual.cpp: a chain with
    halo rows from A and from B2 and a grid in pair groups, both index bases, whole and as a shard."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_residual.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_residual.cpp")]
    exe = str(tmp_path / "sanitize_residual")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_residual: clean" in r.stdout and "runtime error" not in r.stderr
