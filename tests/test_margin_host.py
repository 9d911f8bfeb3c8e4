"""The robust-stability margins on the host (no GPU): the plan-time tables (csrc/sls_margin.cpp: build_margin_tables, through
sls_debug_margin_tables) and the twin of the device passes (margin_host, through sls_debug_margin_host: the same tables and the
same fma chain per entry, the sums in long double) — held to SciPy's CSR conversion, to the Boolean defect pattern and to the dense
long-double statement of the definition in tests/margin_cases.py, which shares no code with either.  The twin is held within its
own derived bound 2·N·2⁻⁵³·S; nothing here picks a tolerance.  The definition itself is tied to the closed loop: the ŵ that the
rollout's reference produces on perturbed plants obeys ŵ_{k+1} = B₁w_k − Σ_τ D[τ]·ŵ_{k−τ}."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import controller_cases as cc
import margin_cases as mc
import rollout_cases as rc

L = np.longdouble


@pytest.fixture(scope="module")
def cases():
    return {name: mc.case(name) for name in mc.ALL}


def _plant(slc, case):
    return slc.Plant(case.A, case.B1, case.B2)


@pytest.mark.parametrize("nscen", [1, 5])
@pytest.mark.parametrize("name", mc.ALL)
def test_twin_against_the_long_double_reference(slc, cases, name, nscen):
    """Per-scenario perturbed plants (every stored value times a factor in [0.8, 1.2]); every output of the twin within its own
    2·N·2⁻⁵³·S of the dense reference, both index bases give the same bits, Σ_i row_l1 = Σ_j col_l1 within the two bounds."""
    case = cases[name]
    Av, Bv = mc.perturbed(case, nscen)
    ref = mc.reference(case, nscen, Av, Bv)
    got = slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, nscen, A=Av, B2=Bv, per_scenario=True)
    worst = mc.check_against_twin(ref, got, name)
    print(name, nscen, "largest error / bound", f"{worst:.3f}", "l1", got["l1"], "e1", got["e1"])
    assert float(ref["l1"].max()) > 0.05
    b1 = slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, nscen, A=Av, B2=Bv, per_scenario=True, index_base=1)
    assert all(np.array_equal(b1[k], got[k]) for k in got)
    gap = np.abs(got["row_l1"].astype(L).sum(axis=0) - got["col_l1"].astype(L).sum(axis=0))
    room = mc.bound(got["row_n"][:, None], got["row_s"]).sum(axis=0) + mc.bound(got["col_n"][:, None], got["col_s"]).sum(axis=0)
    assert (gap <= room).all(), (name, gap, room)
    assert np.array_equal(got["row_n"].sum(), got["col_n"].sum())


def test_design_values_shared_values_and_null(slc, cases):
    """NULL keeps the plan's values; one shared array equals per-scenario copies of it; scenario s does not depend on nscen or on
    its position."""
    case = cases["T5"]
    P, S = _plant(slc, case), [case.Sx, case.Su]
    Av, Bv = mc.perturbed(case, 5)
    a = slc.margin_host(P, S, case.values, 3)
    b = slc.margin_host(P, S, case.values, 3, A=rc.csc_values(case.A), B2=rc.csc_values(case.B2))
    c = slc.margin_host(P, S, case.values, 3, A=Av[:, 2], B2=Bv[:, 2])
    d = slc.margin_host(P, S, case.values, 3, A=np.repeat(Av[:, 2:3], 3, axis=1), B2=np.repeat(Bv[:, 2:3], 3, axis=1), per_scenario=True)
    e = slc.margin_host(P, S, case.values, 5, A=Av, B2=Bv, per_scenario=True)
    one = slc.margin_host(P, S, case.values, 1, A=Av[:, 2], B2=Bv[:, 2])
    for k in ("row_l1", "col_l1", "l1", "e1"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(c[k], d[k]), k
        assert np.array_equal(e[k][..., 2], one[k][..., 0]) and np.array_equal(c[k][..., 1], one[k][..., 0]), k
    mc.check_against_twin(mc.reference(case, 3), a, "design plant")


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", mc.ALL)
def test_tables_against_scipy_and_the_boolean_pattern(slc, cases, name, base):
    case = cases[name]
    t = slc.margin_tables(_plant(slc, case), [case.Sx, case.Su], index_base=base)
    Nx, Nu, T = case.Nx, case.Nu, case.T
    assert t["n_entries"] == case.n_entries
    for M, key in ((case.A, "A"), (case.B2, "B2")):             # the plant by rows, as SciPy converts it
        csc = sp.csc_matrix(M).copy(); csc.sort_indices()
        pos = sp.csc_matrix((np.arange(1, csc.nnz + 1, dtype=np.float64), csc.indices, csc.indptr), shape=csc.shape).tocsr()
        pos.sort_indices()
        assert np.array_equal(t[key + "_ptr"], pos.indptr) and np.array_equal(t[key + "_idx"], pos.indices)
        assert np.array_equal(t[key + "_src"], pos.data.astype(np.int64) - 1)
    # Φ by columns: segment (j, τ) lists the stored-true rows of [Sx[τ]; Su[τ]][:, j] ascending — none of Sx[0] — and phi_perm
    # finds each in the mask-order array
    Px, Pu = mc.boolean_phi(case)
    seg = t["phi_seg"]
    assert seg[0] == 0 and seg[-1] == t["n_entries"] and (np.diff(seg) >= 0).all()
    for j in range(Nx):
        for tau in range(T):
            rows = t["phi_row"][seg[j * T + tau]:seg[j * T + tau + 1]]
            want = np.concatenate([np.flatnonzero(Px[tau][:, j]) if tau else np.zeros(0, dtype=int), Nx + np.flatnonzero(Pu[tau][:, j])])
            assert np.array_equal(rows, want), (j, tau)
            for r, p in zip(rows, t["phi_perm"][seg[j * T + tau]:seg[j * T + tau + 1]]):
                assert p == (mc.value_index(case, "x", tau, r, j) if r < Nx else mc.value_index(case, "u", tau, r - Nx, j))
    assert not np.isnan(case.values[t["phi_perm"]]).any() and np.isnan(case.values).sum() == len(case.values) - t["n_entries"]
    # the defect pattern by columns and by rows
    pat, own, _, _ = mc.pattern(case)
    assert t["n_defect"] == int(pat.sum())
    dp, key = t["def_ptr"], t["def_key"]
    for j in range(Nx):
        tau, i = np.nonzero(pat[:, :, j])
        assert np.array_equal(key[dp[j]:dp[j + 1]], tau * Nx + i), j
        for k, st in zip(key[dp[j]:dp[j + 1]], t["def_start"][dp[j]:dp[j + 1]]):
            ta, i = divmod(int(k), Nx)
            if ta + 1 < T and own[ta, i, j]:
                assert t["phi_row"][st] == i and seg[j * T + ta + 1] <= st < seg[j * T + ta + 2]
            else:
                assert st == -1
    col_of = np.repeat(np.arange(Nx), np.diff(dp))
    rp, perm = t["row_ptr"], t["row_perm"]
    assert sorted(perm.tolist()) == list(range(t["n_defect"]))
    for i in range(Nx):
        mine = perm[rp[i]:rp[i + 1]]
        assert (key[mine] % Nx == i).all() and (np.diff(mine) > 0).all()
        assert rp[i + 1] - rp[i] == int(pat[:, i, :].sum())
    assert (np.diff(col_of[perm[rp[0]:rp[1]]]) >= 0).all()


def test_the_new_operator_meets_every_boundary_it_names(slc, cases):
    """What the docstring of margin_cases.edges promises, counted from the tables the library builds"""
    case = cases["edges"]
    t = slc.margin_tables(_plant(slc, case), [case.Sx, case.Su])
    Nx, T, nb = case.Nx, case.T, mc.EDGES_BLOCK
    col_len, row_len = np.diff(t["def_ptr"]), np.diff(t["row_ptr"])
    assert tuple(col_len[nb:]) == mc.EDGES_COLUMN_LENGTHS and col_len[mc.EDGES_EMPTY_COLUMN] == 0 and row_len[mc.EDGES_EMPTY_ROW] == 0
    assert set(range(8)) <= set((col_len[col_len >= 8] % 8).tolist()) and set(range(8)) <= set((row_len[row_len >= 8] % 8).tolist())
    assert set(range(8)) <= set(col_len.tolist()) and t["n_defect"] % 2 == 1
    assert tuple(np.diff(t["A_ptr"])[:nb]) == mc.EDGES_A_ROWS and not np.diff(t["A_ptr"])[nb:].any()
    assert tuple(np.diff(t["B2_ptr"])[:nb]) == mc.EDGES_B2_ROWS and not np.diff(t["B2_ptr"])[nb:].any()
    seg_len = np.diff(t["phi_seg"]).reshape(Nx, T)
    assert set(mc.EDGES_SEGMENT_LENGTHS) <= set(seg_len[:nb, 1:].ravel().tolist())
    assert set(seg_len[:nb, 0].tolist()) == {0, 1, 2, 3, 4}
    pat, own, viaA, viaB = mc.pattern(case)
    assert (own & ~viaA & ~viaB).any() and ((viaA | viaB) & ~own).any() and (viaA[0] & ~own[0]).any()
    assert (own[:, nb:, :] == pat[:, nb:, :]).all()             # rows ≥ 6: Φ alone
    # the searches: hits at the first and the last position of a segment, misses below, between and above
    A, B2 = sp.csr_matrix(case.A), sp.csr_matrix(case.B2)
    kinds = set()
    for j in range(nb):
        for tau in range(1, T):
            rows = t["phi_row"][t["phi_seg"][j * T + tau]:t["phi_seg"][j * T + tau + 1]]
            for i in np.flatnonzero(pat[tau, :nb, j]):
                for r in np.concatenate([A.indices[A.indptr[i]:A.indptr[i + 1]], Nx + B2.indices[B2.indptr[i]:B2.indptr[i + 1]]]):
                    if rows.size == 0:
                        kinds.add("empty")
                    elif r in rows:
                        kinds.add("first" if r == rows[0] else "last" if r == rows[-1] else "inside")
                    else:
                        kinds.add("below" if r < rows[0] else "above" if r > rows[-1] else "between")
    assert kinds >= {"first", "last", "inside", "below", "above", "between"}, kinds
    false_at = [(tt, M) for tt, M in enumerate(case.Sx) if not np.asarray(sp.csc_matrix(M).data, dtype=bool).all()]
    assert len(false_at) == 1 and false_at[0][0] == 2


@pytest.mark.parametrize("name", ["T2", "T5", "ladder"])
def test_the_definition_is_the_loops_own_recursion(cases, name):
    """rollout_cases.reference on perturbed plants with a random w; ŵ rebuilt from its x by controller_cases.Reference; then
    ŵ_{k+1} = B₁·w_k − Σ_τ D[τ]·ŵ_{k−τ} in long double, at controller_cases.RTOL under the growth condition of the rollout tests."""
    case = cases[name]
    steps, nscen = 40, 3
    Av, Bv = mc.perturbed(case, nscen)
    w = rc.disturbance(name, steps, nscen)
    ref = rc.reference(case, steps, nscen, w=w, A_vals=Av, B2_vals=Bv)
    assert float(np.abs(ref["x"]).max()) < rc.GROWTH_BOUND
    x = np.concatenate([ref["x"], ref["state"][None]])
    _, what = cc.reference(case, x)
    D = mc.defect(case, nscen, Av, Bv)
    B1 = np.asarray(sp.csc_matrix(case.B1).toarray(), dtype=L)
    want = np.zeros((steps, case.Nx, nscen), dtype=L)
    for k in range(steps):
        acc = B1 @ np.asarray(w[k], dtype=L)
        for tau in range(min(case.T, k + 1)):
            acc = acc - np.einsum("sij,js->is", D[:, tau], what[k - tau])
        want[k] = acc
    assert float(np.abs(want).max()) > 0.1
    print(name, "largest relative error", cc.check(np.asarray(what[1:], dtype=np.float64), want, name))
    err = np.abs(what[1:] - want).max(axis=(0, 1)) / np.maximum(1, np.abs(want).max(axis=(0, 1)))
    assert (err < cc.RTOL).all(), err


def test_nan_reach_on_the_host(slc, cases):
    """A NaN in one plant value of one scenario, and in one read Φ value: +inf exactly where margin_cases.reach_of_* says, the
    rest bitwise unchanged; unread positions (Sx[0], stored-false) may hold anything."""
    case = cases["edges"]
    P, S = _plant(slc, case), [case.Sx, case.Su]
    nscen = 4
    Av, Bv = mc.perturbed(case, nscen)
    clean = slc.margin_host(P, S, case.values, nscen, A=Av, B2=Bv, per_scenario=True)
    Acsc = sp.csc_matrix(case.A); Acsc.sort_indices()
    nz = Acsc.nnz // 2
    k = int(np.searchsorted(Acsc.indptr, nz, side="right") - 1); i = int(Acsc.indices[nz])
    bad = Av.copy(); bad[nz, 3] = np.nan
    got = slc.margin_host(P, S, case.values, nscen, A=bad, B2=Bv, per_scenario=True)
    rows, cols = mc.reach_of_plant(case, "A", i, k)
    assert rows.any() and cols.any() and not cols.all()
    for key, hit in (("row_l1", rows), ("col_l1", cols)):
        assert np.isposinf(got[key][hit, 3]).all() and np.array_equal(got[key][~hit, 3], clean[key][~hit, 3])
        assert np.array_equal(got[key][:, :3], clean[key][:, :3])
    assert np.isposinf(got["l1"][3]) and np.isposinf(got["e1"][3]) and np.array_equal(got["l1"][:3], clean["l1"][:3])
    t, r, c = mc.phi_probe(case)
    vals = case.values.copy(); vals[mc.value_index(case, "x", t, r, c)] = np.nan
    got = slc.margin_host(P, S, vals, nscen, A=Av, B2=Bv, per_scenario=True)
    rows, cols = mc.reach_of_phi(case, "x", t, r, c)
    for key, hit in (("row_l1", rows), ("col_l1", cols)):
        assert np.isposinf(got[key][hit]).all() and np.array_equal(got[key][~hit], clean[key][~hit]), key
    junk = np.where(np.isnan(case.values), 1e300, case.values)
    other = slc.margin_host(P, S, junk, nscen, A=Av, B2=Bv, per_scenario=True)
    assert all(np.array_equal(other[k], clean[k]) for k in clean)


def test_host_code_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_rollout.cpp + csrc/sls_margin.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer
    and UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_margin.cpp."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_margin.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_rollout.cpp"), os.path.join(csrc, "sls_margin.cpp")]
    exe = str(tmp_path / "sanitize_margin")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_margin: clean" in r.stdout and "runtime error" not in r.stderr


def test_python_surface_and_null_context(slc, cases):
    new = {"sls_margin_plan", "sls_margin_load", "sls_margin_set_plant", "sls_margin_run", "sls_margin_fetch", "sls_margin_info",
           "sls_margin_destroy"}
    assert new <= set(slc._capi.EXPORTS)
    for name in ("load", "set_plant", "run_async", "margins", "certified", "gain_bound", "close"):
        assert callable(getattr(slc.RobustMargin, name)), name
    assert callable(slc.margin_host) and callable(slc.margin_tables)
    lib = slc.load_library()
    assert lib.sls_abi_version() == 2
    case = cases["T2"]
    m = slc._capi.Marshalled(_plant(slc, case), case.Sx, case.Su)
    h = C.c_void_p()
    assert lib.sls_margin_plan(None, 0, C.byref(m.dims), C.byref(m.plant), m.Sx, m.Su, 1, C.byref(h)) == slc._capi.SLS_EINVAL
    assert not h.value and "null context" in slc._capi.last_error(None)
    assert lib.sls_margin_run(None, None, None, None, None) == slc._capi.SLS_EINVAL
    assert lib.sls_margin_load(None, None, None) == slc._capi.SLS_EINVAL
    assert lib.sls_margin_fetch(None, None, None, None, None) == slc._capi.SLS_EINVAL
    assert lib.sls_margin_info(None, None, None, None, None) == slc._capi.SLS_EINVAL
    lib.sls_margin_destroy(None)
    with pytest.raises(slc.SLSError):
        slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, 0)
    with pytest.raises(ValueError):
        slc.margin_host(_plant(slc, case), [case.Sx, case.Su], case.values, 2, A=np.zeros(3))
