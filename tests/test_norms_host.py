"""The closed-loop norms on the host (no GPU): the table builder the plan uses (csrc/sls_symbolic.cpp: build_norms_operator,
through sls_debug_norms_tables) and the serial twin of the device passes (csrc/sls_norms.cpp, through sls_debug_norms_host: the
same tables, twiddles and per-entry operations as the kernels) — held to a brute-force enumeration of the masks and to the
long-double references of tests/norms_cases.py, which share no code with either.

Two conditions of the GPU tests are established here, on the CPU: the tolerance of the σ parity (norms_cases.HINF_RTOL: 8 × the
deviation of a plain complex128 run of the same iteration, floor 64·2⁻⁵³), and the convergence condition of every (case, ω) that
is compared with an SVD — (σ₂/σ₁)^(2·iters) ≤ 1e-12 from the reference's own singular values, asserted for EVERY pair."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import norms_cases as nc


@pytest.fixture(scope="module")
def cases():
    return {name: nc.case(name) for name in nc.ALL}


def _brute_force(c):
    """every stored-true entry as (row, t, col, index in the mask-order array), by a plain walk over the CSC storage"""
    out, o = [], 0
    for masks, r0 in ((c.Sx, 0), (c.Su, c.Nx)):
        for t, M in enumerate(masks):
            M = sp.csc_matrix(M)
            for col in range(M.shape[1]):
                for k in range(M.indptr[col], M.indptr[col + 1]):
                    if M.data[k]:
                        out.append((r0 + int(M.indices[k]), t, col, o + k))
            o += M.nnz
    return out


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", nc.ALL)
def test_tables_against_a_brute_force_enumeration_of_the_masks(slc, cases, name, base):
    c = cases[name]
    row_ptr, rk, rp, col_ptr, ck, cp = slc.norms_tables((c.Nx, c.Nu), [c.Sx, c.Su], index_base=base)
    ent = _brute_force(c)
    assert len(ent) == c.n_entries == len(rk) == len(ck) == row_ptr[-1] == col_ptr[-1]
    by_row = sorted(ent, key=lambda e: (e[0], e[1], e[2]))             # rows ascending in (t, col)
    by_col = sorted(ent, key=lambda e: (e[2], e[1], e[0]))             # columns ascending in (t, row)
    assert np.array_equal(rk, [t * c.Nx + col for _, t, col, _ in by_row])
    assert np.array_equal(rp, [p for *_, p in by_row])
    assert np.array_equal(ck, [t * c.N + r for r, t, _, _ in by_col])
    assert np.array_equal(cp, [p for *_, p in by_col])
    assert row_ptr[0] == 0 and np.array_equal(np.diff(row_ptr), np.bincount([e[0] for e in ent], minlength=c.N))
    assert col_ptr[0] == 0 and np.array_equal(np.diff(col_ptr), np.bincount([e[2] for e in ent], minlength=c.Nx))
    assert np.array_equal(np.diff(row_ptr), c.row_len) and np.array_equal(np.diff(col_ptr), c.col_len)
    assert np.isfinite(c.values[rp]).all() and np.isfinite(c.values[cp]).all()     # no poisoned position
    assert np.array_equal(np.sort(rp), np.sort(cp)) and len(np.unique(rp)) == len(rp)
    for i in range(c.N):                                                # the value behind every entry is the entry's own
        e = slice(row_ptr[i], row_ptr[i + 1])
        assert np.array_equal(c.values[rp[e]], c.G[rk[e] // c.Nx, i, rk[e] % c.Nx])
    for j in range(c.Nx):
        e = slice(col_ptr[j], col_ptr[j + 1])
        assert np.array_equal(c.values[cp[e]], c.G[ck[e] // c.N, ck[e] % c.N, j])


def test_the_cases_hold_what_the_tests_need(cases):
    lad = cases["ladder"]
    assert sorted(set(lad.row_len[lad.Nx:])) == [0, 49, 97, 192, 256, 576]                 # input rows: the ladder's own lengths
    assert {1, 2, 3, 4, 5, 6, 8, 9, 10, 16, 17, 18, 32, 33, 34, 64, 65, 66, 128, 129, 130, 194, 258, 516} == set(lad.row_len[:lad.Nx])
    assert lad.row_len.max() > 256 + 192 and lad.col_len.max() > 64
    h = cases["HOLES"]
    assert h.row_len[nc.HOLES_EMPTY_ROW_X] == 0 and h.row_len[h.Nx + nc.HOLES_EMPTY_ROW_U] == 0 and h.col_len[nc.HOLES_EMPTY_COL] == 0
    assert np.count_nonzero(h.row_len == 0) == 2 and np.count_nonzero(h.col_len == 0) == 1
    assert cases["T1"].T == 1 and cases["Nu0"].Nu == 0
    for c in cases.values():
        assert np.isnan(c.values).sum() == (0 if c.name in ("T1", "T2", "Nu0") else 1)
    assert len(nc.LAYOUT_OMEGAS) == nc.LAYOUT_MAX_FREQ == 65 and len(set(nc.LAYOUT_OMEGAS)) == 65


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", nc.ALL)
def test_host_twin_against_the_references(slc, cases, name, weighted):
    c = cases[name]
    cz, b = nc.weights(c) if weighted else (None, None)
    h = slc.norms_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, cz=cz, b=b, omega=nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS)
    G = nc.dense(c, cz, b)
    row, col = nc.l1_reference(G)
    er, ec = nc.rel(h["row_l1"], row), nc.rel(h["col_l1"], col)
    ref = nc.sigma_reference(c, nc.PARITY_OMEGAS, nc.PARITY_ITERS, cz, b)
    es = nc.rel(h["sigma"], ref)
    print(f"{name} weighted={weighted}: rel err row_l1 {er:.2e} col_l1 {ec:.2e} (tol {nc.l1_rtol(c):.2e}), sigma {es:.2e} (tol {nc.HINF_RTOL:.2e})")
    assert er <= nc.l1_rtol(c) and ec <= nc.l1_rtol(c)
    assert h["totals"][0] == h["row_l1"].max() and h["totals"][1] == h["col_l1"].max()
    assert es <= nc.HINF_RTOL
    assert h["peak"] == h["sigma"].max() and h["argpeak"] == int(np.argmax(h["sigma"]))
    assert h["sigma"][2] == h["sigma"][3] and h["sigma"][5] == h["sigma"][6]               # σ(−ω) = σ(ω), bit for bit
    b1 = slc.norms_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, cz=cz, b=b, omega=nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS, index_base=1)
    assert all(np.array_equal(b1[k], h[k]) for k in ("row_l1", "col_l1", "totals", "sigma"))


def test_parity_tolerance_comes_from_a_plain_complex128_run(cases):
    """HINF_RTOL = max(8 × the deviation of a plain complex128 NumPy run of the same iteration from the long-double one, 64·2⁻⁵³):
    measured again here over every (case, ω), weighted and not, against the figure recorded in norms_cases.py"""
    worst = 0.0
    for c in cases.values():
        for cz, b in ((None, None), nc.weights(c)):
            G = nc.dense(c, cz, b)
            ref = nc.sigma_reference(c, nc.PARITY_OMEGAS, nc.PARITY_ITERS, cz, b)
            plain = [nc.power_iteration(nc.at_omega(G, w, np.complex128), nc.PARITY_ITERS) for w in nc.PARITY_OMEGAS]
            worst = max(worst, nc.rel(plain, ref))
    print(f"plain complex128 run: worst relative deviation {worst:.3e} (recorded {nc.HINF_PLAIN_DEVIATION:.1e}; tolerance {nc.HINF_RTOL:.3e})")
    assert nc.HINF_RTOL == max(8.0 * nc.HINF_PLAIN_DEVIATION, 64.0 * 2.0 ** -53)
    assert worst <= 2.0 * nc.HINF_PLAIN_DEVIATION                      # another BLAS may order the sums differently


def test_convergence_condition_of_every_svd_comparison(slc, cases):
    """(σ₂/σ₁)^(2·iters) ≤ 1e-12 for every (case, ω) compared with an SVD — a condition, not a tolerance: no pair is excluded.
    Then the host twin at those iters against σ₁, relative 1e-9."""
    assert set(nc.SVD_OMEGAS) == set(nc.ALL) == set(nc.SVD_ITERS)
    for name, c in cases.items():
        om, iters = nc.SVD_OMEGAS[name], nc.SVD_ITERS[name]
        top = [nc.svd_top2(c, w) for w in om]
        for w, (s1, s2) in zip(om, top):
            assert s1 > 0 and (s2 / s1) ** (2 * iters) <= nc.SVD_GAP, (name, w, s2 / s1, iters)
        h = slc.norms_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, omega=om, iters=iters)
        e = nc.rel(h["sigma"], [s1 for s1, _ in top])
        print(f"{name}: iters {iters}, worst gap {max(s2 / s1 for s1, s2 in top):.4f}, rel err against σ_max {e:.2e}")
        assert e <= nc.SVD_RTOL
        assert np.all(h["sigma"] <= np.array([s1 for s1, _ in top]) * (1 + 64 * nc.U))     # a lower bound


def test_sigma_does_not_decrease_with_iters(slc, cases):
    """1, 2, 4, 8 iterations: non-decreasing up to one rounding of the final norm"""
    for c in cases.values():
        s = [slc.norms_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, omega=nc.MONOTONE_OMEGAS, iters=k)["sigma"] for k in nc.MONOTONE_ITERS]
        for a, b in zip(s, s[1:]):
            assert np.all(b >= a * (1 - 2.0 ** -52)), (c.name, a, b)


def test_closed_forms_and_refusals(slc, cases):
    c = cases["T1"]                                                     # T = 1: G(ω) = G[0] for every ω
    cz, b = nc.weights(c)
    h = slc.norms_host((c.Nx, c.Nu), [c.Sx, c.Su], c.values, cz=cz, b=b, omega=[0.0, 0.4, -2.2, np.pi], iters=3)
    assert len(set(h["sigma"])) == 1
    d = c.values[:c.Nx]
    for i in range(c.Nx):                                               # a state row of [I·w; Φu[0]] holds one entry
        assert h["row_l1"][i] == abs(d[i] * (cz[i] * b[i]))
    hz = cases["HOLES"]
    h = slc.norms_host((hz.Nx, hz.Nu), [hz.Sx, hz.Su], hz.values)
    assert h["row_l1"][nc.HOLES_EMPTY_ROW_X] == 0 and h["row_l1"][hz.Nx + nc.HOLES_EMPTY_ROW_U] == 0 and h["col_l1"][nc.HOLES_EMPTY_COL] == 0
    assert "sigma" not in h
    bad = np.array(hz.values)
    k = int(np.flatnonzero(np.isfinite(bad))[5])
    bad[k] = np.nan                                                     # a NaN in a read entry: +inf in its row and column
    h = slc.norms_host((hz.Nx, hz.Nu), [hz.Sx, hz.Su], bad)
    assert np.count_nonzero(np.isinf(h["row_l1"])) == 1 and np.count_nonzero(np.isinf(h["col_l1"])) == 1
    assert np.isinf(h["totals"]).all() and not np.isnan(h["row_l1"]).any()
    for kw in (dict(omega=[0.1], iters=0), dict(omega=[np.inf], iters=2), dict(omega=[np.nan], iters=2), dict(cz=np.full(hz.N, np.inf)),
               dict(b=np.full(hz.Nx, np.nan))):
        with pytest.raises(slc.SLSError) as ei:
            slc.norms_host((hz.Nx, hz.Nu), [hz.Sx, hz.Su], hz.values, **kw)
        assert ei.value.code == slc._capi.SLS_EINVAL


def test_from_plant_takes_diagonal_weights_and_refuses_the_rest():
    import slc_amd as slc
    from slc_amd.norms import plant_weights
    A = sp.diags([np.full(4, 0.5), np.full(5, 0.9)], [1, 0]).tocsc()
    B2 = sp.csc_matrix(np.eye(5)[:, :2])
    cz, b = plant_weights(slc.Plant(A, sp.identity(5), B2))
    assert np.array_equal(cz, np.ones(7)) and np.array_equal(b, np.ones(5))
    q, r, w = np.arange(1.0, 6.0), np.array([0.5, 2.0]), np.linspace(0.1, 0.5, 5)
    C1 = sp.vstack([sp.diags(q), sp.csc_matrix((2, 5))])
    D12 = sp.vstack([sp.csc_matrix((5, 2)), sp.diags(r)])
    cz, b = plant_weights(slc.Plant(A, sp.diags(w), B2, C1, 0, D12))
    assert np.array_equal(cz, np.concatenate([q, r])) and np.array_equal(b, w)
    C1x = C1.tolil(); C1x[0, 1] = 0.3
    with pytest.raises(ValueError, match="not diagonal.*sparse triple product"):
        plant_weights(slc.Plant(A, sp.identity(5), B2, C1x.tocsc(), 0, D12))
    B1x = sp.identity(5, format="lil"); B1x[3, 0] = 1.0
    with pytest.raises(ValueError, match="B1 is not diagonal"):
        plant_weights(slc.Plant(A, B1x.tocsc(), B2))
    D11 = sp.lil_matrix((7, 5)); D11[0, 0] = 1.0
    with pytest.raises(ValueError, match="D11"):
        plant_weights(slc.Plant(A, sp.identity(5), B2, C1, D11.tocsc(), D12))


def test_host_code_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp + csrc/sls_norms.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_norms.cpp: the table builder and
    the host twin on a ladder-like operator (Nx 24, Nu 6, T 24) and on Nu = 0, both index bases."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_norms.cpp"), os.path.join(csrc, "sls_symbolic.cpp"), os.path.join(csrc, "sls_norms.cpp")]
    exe = str(tmp_path / "sanitize_norms")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    bld = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert bld.returncode == 0, bld.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_norms: clean" in r.stdout and "runtime error" not in r.stderr


def test_null_context_is_refused(slc, cases):
    import ctypes as C
    lib = slc.load_library()
    c = cases["T2"]
    m = slc._capi.Marshalled.masks_only(c.Nx, c.Nu, c.Sx, c.Su)
    h = C.c_void_p()
    assert lib.sls_norms_plan(None, 0, C.byref(m.dims), m.Sx, m.Su, None, None, 4, C.byref(h)) == slc._capi.SLS_EINVAL
    assert not h.value and "null context" in slc._capi.last_error(None)
