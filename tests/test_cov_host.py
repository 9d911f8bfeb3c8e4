"""The 𝓗₂ shares and the covariance entries on the host (no GPU): the serial twins of the device passes (csrc/sls_norms.cpp:
norms_h2_host, norms_cov_host, through sls_debug_norms_h2_host / sls_debug_norms_cov_host — the same tables and per-entry
operations as the kernels) held to the long-double Σ = Σ_t G[t]·G[t]ᵀ of tests/cov_cases.py, which shares no code with them, at
the tolerances derived there; the table invariant the covariance kernel relies on; the refusals; the pattern helper."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import cov_cases as cc
import norms_cases as nc


@pytest.fixture(scope="module")
def cases():
    return {name: nc.case(name) for name in cc.ALL}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", cc.ALL)
def test_host_twin_against_the_long_double_covariance(slc, cases, name, weighted):
    c = cases[name]
    cz, b = nc.weights(c) if weighted else (None, None)
    ref = cc.reference(c, cz, b)
    dims, S = (c.Nx, c.Nu), [c.Sx, c.Su]
    row, col, tot = slc.norms_h2_host(dims, S, c.values, cz=cz, b=b)
    er, ec, et = nc.rel(row, ref.row), nc.rel(col, ref.col), nc.rel(tot[:1], [ref.row.sum()])
    print(f"{name} weighted={weighted}: rel err row_h2 {er:.2e} col_h2 {ec:.2e} (tol {cc.h2_rtol(c):.2e}) total {et:.2e} (tol {cc.total_rtol(c):.2e})")
    assert er <= cc.h2_rtol(c) and ec <= cc.h2_rtol(c) and et <= cc.total_rtol(c)
    assert tot[1] == row.max()
    row1, col1, tot1 = slc.norms_h2_host(dims, S, c.values, cz=cz, b=b, index_base=1)
    assert np.array_equal(row1, row) and np.array_equal(col1, col) and np.array_equal(tot1, tot)
    lists = cc.pair_lists(c)
    assert {"all", "reversed", "one", "duplicates"} <= set(lists)
    got = {}
    for key, (pi, pj) in lists.items():
        got[key] = slc.norms_cov_host(dims, S, c.values, pi, pj, cz=cz, b=b)
        e = cc.cov_error(got[key], ref, pi, pj)
        print(f"  {key}: {len(pi)} pairs, worst error / tolerance {e:.3f}")
        assert e <= 1.0
        assert np.array_equal(slc.norms_cov_host(dims, S, c.values, pi + 1, pj + 1, cz=cz, b=b, index_base=1), got[key])
    assert np.array_equal(got["reversed"], got["all"][::-1])           # (j, i) and (i, j): the same bits
    i, j = lists["all"]
    d = got["all"][i == j]                                              # the diagonal against row_h2, the two tolerances added
    tol = cc.h2_rtol(c) * np.asarray(ref.row, dtype=float) + np.asarray(cc.cov_atol(ref, i[i == j], j[i == j]), dtype=float)
    assert np.all(np.abs(d - row) <= tol)


def test_the_cases_hold_what_the_tests_need(cases):
    lad = cases["ladder"]
    i, j = cc.all_pairs(lad)
    assert len(i) == lad.N * (lad.N + 1) // 2
    la = np.minimum(lad.row_len[i], lad.row_len[j])
    assert {0, 1, 49, 64, 65, 66, 97, 128, 129, 130, 192, 194, 256, 258, 516, 576} <= set(la)      # the shorter list: every chunk edge
    assert np.any(lad.row_len[i] < lad.row_len[j]) and np.any(lad.row_len[i] > lad.row_len[j])     # either list is the shorter
    ties = 0                                                            # equal lengths, settled by the row index: the small cases
    for c in cases.values():
        ci, cj = cc.all_pairs(c)
        ties += int(np.count_nonzero((c.row_len[ci] == c.row_len[cj]) & (ci != cj) & (c.row_len[ci] > 0)))
    assert ties > 0
    ref = cc.reference(lad)
    sh = ref.shared[i, j]
    assert np.any((sh == 0) & (la > 0)) and np.any((sh > 0) & (sh < la)) and sh.max() == 576
    h = cases["HOLES"]
    assert list(cc.empty_rows(h)) == [nc.HOLES_EMPTY_ROW_X, h.Nx + nc.HOLES_EMPTY_ROW_U] and list(cc.empty_rows(lad)) != []
    assert "empty" in cc.pair_lists(h) and "state_input" not in cc.pair_lists(cases["Nu0"])


@pytest.mark.parametrize("name", cc.ALL)
def test_row_keys_ascend_strictly_within_a_row(slc, cases, name):
    """what the intersection relies on: a row's keys are strictly ascending, so a key has at most one partner"""
    c = cases[name]
    row_ptr, rk = slc.norms_tables((c.Nx, c.Nu), [c.Sx, c.Su])[:2]
    for i in range(c.N):
        k = rk[row_ptr[i]:row_ptr[i + 1]]
        assert np.all(np.diff(k.astype(np.int64)) > 0)
        assert len(k) == c.row_len[i]


@pytest.mark.parametrize("name", ["ladder", "Nu0", "HOLES"])
def test_weights_against_prescaled_values(slc, cases, name):
    """cz, b against NULL weights on values scaled on the host by cz[row]·b[col], the product formed first as the load does:
    the same roundings on both sides, and the same loop order — the same bits"""
    c = cases[name]
    cz, b = nc.weights(c, seed=5)
    dims, S = (c.Nx, c.Nu), [c.Sx, c.Su]
    pre = nc.prescale(c, cz, b)
    for w, p in zip(slc.norms_h2_host(dims, S, c.values, cz=cz, b=b), slc.norms_h2_host(dims, S, pre)):
        assert np.array_equal(w, p)
    pi, pj = cc.all_pairs(c)
    assert np.array_equal(slc.norms_cov_host(dims, S, c.values, pi, pj, cz=cz, b=b), slc.norms_cov_host(dims, S, pre, pi, pj))


def test_closed_forms_nan_and_refusals(slc, cases):
    c = cases["T1"]                                                     # T = 1: a state row of [diag(d)·w; Φu[0]·w] holds one entry
    cz, b = nc.weights(c)
    row, col, tot = slc.norms_h2_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, cz=cz, b=b)
    v = c.values[:c.Nx] * (cz[:c.Nx] * b)
    assert np.array_equal(row[:c.Nx], v * v)
    s = np.arange(c.Nx)
    assert np.array_equal(slc.norms_cov_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, s, s, cz=cz, b=b), v * v)
    assert not np.any(slc.norms_cov_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, s[:-1], s[1:], cz=cz, b=b))   # disjoint: exactly 0
    h = cases["HOLES"]
    dims, S = (h.Nx, h.Nu), [h.Sx, h.Su]
    row, col, tot = slc.norms_h2_host(dims, S, h.values)
    assert row[nc.HOLES_EMPTY_ROW_X] == 0 and row[h.Nx + nc.HOLES_EMPTY_ROW_U] == 0 and col[nc.HOLES_EMPTY_COL] == 0
    pi, pj = cc.pair_lists(h)["empty"]
    assert not np.any(slc.norms_cov_host(dims, S, h.values, pi, pj))
    assert slc.norms_cov_host(dims, S, h.values, [], []).shape == (0,)
    # a NaN in one read entry: +inf in its row and its column, NaN in exactly the pairs that share its key
    tables = slc.norms_tables(dims, S)
    e = len(tables[1]) // 2
    i = int(np.searchsorted(tables[0], e, side="right")) - 1
    key = int(tables[1][e])
    bad = np.array(h.values); bad[tables[2][e]] = np.nan
    rowb, colb, totb = slc.norms_h2_host(dims, S, bad)
    assert np.array_equal(np.flatnonzero(np.isinf(rowb)), [i]) and np.array_equal(np.flatnonzero(np.isinf(colb)), [key % h.Nx])
    assert np.isposinf(totb).all() and not np.isnan(rowb).any() and not np.isnan(colb).any()
    pi, pj = cc.all_pairs(h)
    good, covb = slc.norms_cov_host(dims, S, h.values, pi, pj), slc.norms_cov_host(dims, S, bad, pi, pj)
    has = np.array([key in tables[1][tables[0][r]:tables[0][r + 1]] for r in range(h.N)])
    hit = ((pi == i) & has[pj]) | ((pj == i) & has[pi])
    assert hit.sum() > 1 and np.array_equal(np.isnan(covb), hit) and np.array_equal(covb[~hit], good[~hit])
    # refusals: the message names the position
    for pi, pj, base, at in (([0, h.N], [0, 0], 0, 1), ([0, 0, 0], [0, 1, -1], 0, 2), ([0], [1], 1, 0), ([h.N + 1], [1], 1, 0)):
        with pytest.raises(slc.SLSError, match=f"pair {at} ") as ei:
            slc.norms_cov_host(dims, S, h.values, pi, pj, index_base=base)
        assert ei.value.code == slc._capi.SLS_EINVAL
    with pytest.raises(ValueError):
        slc.norms_cov_host(dims, S, h.values, [0, 1], [0])


def test_covariance_pattern_of_a_plant():
    import slc_amd as slc
    rows, cols, data = [0, 0, 1, 2, 2, 3, 3, 1], [0, 1, 1, 1, 2, 0, 3, 3], [0.5, 0.2, 0.5, 0.3, 0.5, 0.1, 0.0, 0.0]
    A = sp.csc_matrix((data, (rows, cols)), shape=(4, 4))               # (3,3) and (1,3): stored zeros are not neighbours
    P = slc.Plant(A, sp.identity(4), sp.csc_matrix(np.eye(4)[:, :2]))
    pi, pj = slc.covariance_pattern_of(P)
    want = [(0, 0), (0, 1), (0, 3), (1, 1), (1, 2), (2, 2), (3, 3), (4, 4), (5, 5)]
    assert pi.dtype == np.int64 and list(zip(pi.tolist(), pj.tolist())) == want
    p1 = slc.ClosedLoopNorms.covariance_pattern_of(P, index_base=1)
    assert np.array_equal(p1[0], pi + 1) and np.array_equal(p1[1], pj + 1)


def test_host_code_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_norms.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_cov.cpp: the two twins over a
    ladder-like operator and one with empty rows, every pair, and the refusals of out-of-range pairs."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_cov.cpp"), os.path.join(csrc, "sls_symbolic.cpp"), os.path.join(csrc, "sls_norms.cpp")]
    exe = str(tmp_path / "sanitize_cov")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    bld = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert bld.returncode == 0, bld.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_cov: clean" in r.stdout and "runtime error" not in r.stderr
