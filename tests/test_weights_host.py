"""sls_plan_update_weights on the host (no GPU): the updatable symbolic pass (SLS_PLAN_WEIGHTS_UPDATABLE), its shape and value
rules, and the host twin weight_records_host (csrc/sls_weights.cpp) through sls_debug_weights_host.

What must hold is exact: the twin rewrites the weight pool of a flagged pass to the bits a fresh flagged pass on the re-weighted
plant holds (hinv = 1 / (b²·v² + ridge), each operation rounded once), a pass without the flag is what it was before the flag
existed, and a refused value is written nowhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import update_cases as uc
import weights_cases as wc

FLAG = 2


def _plants(slc):
    """name: (plant, masks) — chain-23, the banded 64-state plant, grid-10"""
    wl = slc.workloads
    out = {}
    for name, P, (d, T, alpha) in (("chain23", wl.chain_plant(23), (4, 5, 1.5)), ("banded64", uc.banded(slc), (4, 6, 1.0)),
                                   ("grid10", wl.grid_plant(10, 1), (3, 4, 8.0))):
        S = wl.localization_masks(P.A, P.B2, d, T, alpha)
        out[name] = (P, [list(S[0]), list(S[1])])
    return out


_cache = {}


def _plant(slc, name):
    if not _cache:
        _cache.update(_plants(slc))
    return _cache[name]


def _pass(slc, P, S, *, flagged, base=0, groups=None, ridge=None, c1=None, d12=None, strict=0):
    """dict of sls_debug_weights_host's outputs (rc, msg included); the pool is sized by a first call"""
    lib = slc._capi.load_library()
    m = slc._capi.Marshalled(P, S[0], S[1], groups, index_base=base, flags=FLAG if flagged else 0)
    dp, i32p, i64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    ns = m.n_sub
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    rx, ru = (None, None) if ridge is None else (f(ridge[0]), f(ridge[1]))
    c1, d12 = f(c1), f(d12)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    n_w = C.c_int64(-1)
    head = (*m.common_args(), ptr(rx), ptr(ru))
    rc0 = lib.sls_debug_weights_host(*head, None, None, 0, C.byref(n_w), *([None] * 10))
    if rc0:
        return {"rc": rc0, "msg": lib.sls_last_error(None).decode()}
    has_w, n_x, n_u = (np.zeros(max(ns, 1), dtype=np.int32) for _ in range(3))
    off_w = np.zeros(max(ns, 1), dtype=np.int64)
    w = np.full(max(n_w.value, 1), np.nan); obj = np.full(2 * max(ns, 1), np.nan); b2 = np.full(max(ns, 1), np.nan)
    diag = np.full(P.Nx + P.Nu, np.nan); dirty = np.zeros(max(ns, 1), dtype=np.uint8); rej = C.c_int64(-1)
    rc = lib.sls_debug_weights_host(*head, ptr(c1), ptr(d12), int(strict), C.byref(n_w), has_w.ctypes.data_as(i32p),
                                    off_w.ctypes.data_as(i64p), n_x.ctypes.data_as(i32p), n_u.ctypes.data_as(i32p), ptr(w), ptr(obj), ptr(b2),
                                    ptr(diag), dirty.ctypes.data_as(u8p), C.byref(rej))
    return {"rc": rc, "msg": lib.sls_last_error(None).decode() if rc else "", "has_w": has_w[:ns], "off_w": off_w[:ns], "n_x": n_x[:ns],
            "n_u": n_u[:ns], "w": w[:n_w.value], "obj": obj[:2 * ns], "b2": b2[:ns], "diag": diag, "dirty": dirty[:ns], "rejected": rej.value}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_tables(x, y, what=("has_w", "off_w", "n_x", "n_u", "obj")):
    return np.array_equal(_bits(x["w"]), _bits(y["w"])) and all(np.array_equal(x[k], y[k]) for k in what)


def _ridge(P, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.01, 0.3, P.Nx), rng.uniform(0.01, 0.3, P.Nu)


# ---- the twin against a fresh pass ----

@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("with_ridge", [False, True], ids=["plain", "ridge"])
@pytest.mark.parametrize("name", ["chain23", "banded64", "grid10"])
def test_twin_reproduces_a_fresh_flagged_pass(slc, name, with_ridge, base):
    P, S = _plant(slc, name)
    ridge = _ridge(P) if with_ridge else None
    cA, dA = wc.diagonals(P, wc.SEED_A)
    cB, dB = wc.diagonals(P, wc.SEED_B)
    fresh = _pass(slc, wc.weighted(P, wc.SEED_B), S, flagged=True, base=base, ridge=ridge)
    assert fresh["rc"] == 0 and fresh["w"].size > 0 and np.all(fresh["has_w"] == 1)
    for start, c0, d0 in ((P, np.ones(P.Nx), np.ones(P.Nu)), (wc.weighted(P, wc.SEED_A), cA, dA)):          # from identity, from seed 11
        got = _pass(slc, start, S, flagged=True, base=base, ridge=ridge, c1=cB, d12=dB)
        assert got["rc"] == 0 and got["rejected"] == 0
        assert _same_tables(got, fresh) and np.array_equal(_bits(got["diag"]), _bits(np.r_[cB, dB]))
        assert np.all(got["dirty"] == 1)                                                                 # every record moved
        # one half at a time leaves the other half's records and diagonals alone
        half = _pass(slc, start, S, flagged=True, base=base, ridge=ridge, c1=cB)
        want = _pass(slc, wc.with_weights(P, cB, d0), S, flagged=True, base=base, ridge=ridge)
        assert half["rc"] == 0 and _same_tables(half, want) and np.array_equal(_bits(half["diag"]), _bits(np.r_[cB, d0]))
        # the same values again change no bit and mark nothing
        again = _pass(slc, start, S, flagged=True, base=base, ridge=ridge, c1=c0, d12=d0)
        assert again["rc"] == 0 and np.all(again["dirty"] == 0) and _same_tables(again, _pass(slc, start, S, flagged=True, base=base, ridge=ridge))


def test_record_is_the_documented_formula(slc):
    """hinv = 1 / (b²·v² + ridge) with each operation rounded once — NumPy's float64 arithmetic — on a plant whose B1 diagonal
    varies and has a zero; the g halves stay zero; a b = 0 column keeps no record without a ridge."""
    P0, S = _plant(slc, "chain23")
    b = 0.5 + 0.1 * np.arange(P0.Nx); b[7] = 0.0
    P = slc.Plant(P0.A, sp.diags(b).tocsc(), P0.B2)
    c, d = wc.diagonals(P, wc.SEED_A)
    # the index sets, from the masks' last time step as the reference takes them (src/reduction.jl:14)
    An = (sp.csc_matrix(P.A) != 0).astype(np.int64)
    sx_all = sp.csc_matrix(sp.csc_matrix(S[0][-1]).astype(np.int64) @ An)
    su_all = sp.csc_matrix(sp.csc_matrix(S[1][-1]).astype(np.int64) @ An)
    for ridge in (None, _ridge(P)):
        got = _pass(slc, wc.with_weights(P, c, d), S, flagged=True, ridge=ridge)
        assert got["rc"] == 0
        assert np.array_equal(got["b2"], b * b)
        for q in range(P.Nx):
            sx = np.sort(sx_all.indices[sx_all.indptr[q]:sx_all.indptr[q + 1]]); su = np.sort(su_all.indices[su_all.indptr[q]:su_all.indptr[q + 1]])
            assert (got["n_x"][q], got["n_u"][q]) == (sx.size, su.size)
            if b[q] == 0.0 and ridge is None:
                assert got["has_w"][q] == 0
                continue
            assert got["has_w"][q] == 1
            nm, o = sx.size + su.size, got["off_w"][q]
            v = np.r_[c[sx], d[su]]
            r = np.zeros(nm) if ridge is None else np.r_[ridge[0][sx], ridge[1][su]]
            want = 1.0 / ((b[q] * b[q]) * (v * v) + r)
            assert np.array_equal(_bits(got["w"][o:o + nm]), _bits(want)), q
            assert np.all(got["w"][o + nm:o + 2 * nm] == 0.0)
            assert got["obj"][2 * q] == 1.0 and got["obj"][2 * q + 1] == 0.0


# ---- the flag changes nothing for plans that do not set it ----

@pytest.mark.parametrize("name", ["chain23", "banded64", "grid10"])
def test_unflagged_pass_is_unchanged(slc, name):
    """Identity weights: no record at all, scale b² = 1.  Uniform weights 2·I: still no record, scale b²·4.  Non-uniform
    weights: the records a flagged pass holds, bit for bit — there the flag has nothing to add.  And the flagged identity pass
    holds hinv = 1 / b² = 1 in every record."""
    P, S = _plant(slc, name)
    ident = _pass(slc, P, S, flagged=False)
    assert ident["rc"] == 0 and ident["w"].size == 0 and np.all(ident["has_w"] == 0) and np.all(ident["off_w"] == 0)
    assert np.array_equal(ident["obj"], np.tile([1.0, 0.0], P.Nx)) and np.all(ident["b2"] == 0.0)
    unif = _pass(slc, wc.with_weights(P, 2.0 * np.ones(P.Nx), 2.0 * np.ones(P.Nu)), S, flagged=False)
    assert unif["rc"] == 0 and unif["w"].size == 0 and np.all(unif["has_w"] == 0) and np.array_equal(unif["obj"], np.tile([4.0, 0.0], P.Nx))
    Q = wc.weighted(P, wc.SEED_A)
    plain, flagged = _pass(slc, Q, S, flagged=False), _pass(slc, Q, S, flagged=True)
    assert plain["rc"] == 0 and flagged["rc"] == 0 and np.all(plain["has_w"] == 1) and _same_tables(plain, flagged)
    fi = _pass(slc, P, S, flagged=True)
    nm = (fi["n_x"] + fi["n_u"]).astype(np.int64)
    assert fi["rc"] == 0 and np.all(fi["has_w"] == 1) and fi["w"].size == 2 * nm.sum()
    assert np.array_equal(fi["off_w"], 2 * (np.cumsum(nm) - nm)) and np.array_equal(fi["obj"], np.tile([1.0, 0.0], P.Nx))
    for q in range(P.Nx):
        o = fi["off_w"][q]
        assert np.all(fi["w"][o:o + nm[q]] == 1.0) and np.all(fi["w"][o + nm[q]:o + 2 * nm[q]] == 0.0)
    # an update needs the flag
    r = _pass(slc, Q, S, flagged=False, c1=np.ones(P.Nx))
    assert r["rc"] == slc._capi.SLS_EINVAL and "SLS_PLAN_WEIGHTS_UPDATABLE" in r["msg"]


# ---- the shape rule ----

def test_shapes_outside_the_rule_are_refused_with_the_reason(slc):
    P, S = _plant(slc, "chain23")
    Nx, Nu = P.Nx, P.Nu
    C1, D12 = wc.lqr_blocks(Nx, Nu, np.ones(Nx), np.ones(Nu))
    EU = slc._capi.SLS_EUNSUPPORTED
    off = C1.copy(); off.indices[3] += 1                                     # column 3's entry on z-row 4
    r = _pass(slc, slc.Plant(P.A, P.B1, P.B2, off, 0, D12), S, flagged=True)
    assert r["rc"] == EU and "column 3 of C1" in r["msg"] and "own z-row 3" in r["msg"], r["msg"]
    two = sp.lil_matrix(C1); two[Nx + 1, 2] = 0.5                             # a second entry in column 2
    r = _pass(slc, slc.Plant(P.A, P.B1, P.B2, two.tocsc(), 0, D12), S, flagged=True)
    assert r["rc"] == EU and "column 2 of C1 stores 2 entries" in r["msg"], r["msg"]
    offd = D12.copy(); offd.indices[0] -= 1                                  # D12's first entry on a state row
    r = _pass(slc, slc.Plant(P.A, P.B1, P.B2, C1, 0, offd), S, flagged=True)
    assert r["rc"] == EU and "column 0 of D12" in r["msg"], r["msg"]
    D11 = sp.lil_matrix((Nx + Nu, P.Nw)); D11[4, 4] = 0.3                     # z-row 4 is selected by column 4 (4 ∈ s_x(4))
    r = _pass(slc, slc.Plant(P.A, P.B1, P.B2, C1, D11.tocsc(), D12), S, flagged=True)
    assert r["rc"] == EU and "D11 has a non-zero on z-row 4 of column 4" in r["msg"], r["msg"]
    B1 = sp.lil_matrix(sp.identity(Nx)); B1[8, 9] = 0.5                       # couples the group {8, 9}
    r = _pass(slc, slc.Plant(P.A, B1.tocsc(), P.B2, C1, 0, D12), S, flagged=True, groups=[[8, 9]])
    assert r["rc"] == EU and "coupled column group" in r["msg"], r["msg"]
    # every one of them is a plan the library builds without the flag
    for Q, g in ((slc.Plant(P.A, P.B1, P.B2, off, 0, D12), None), (slc.Plant(P.A, P.B1, P.B2, C1, D11.tocsc(), D12), None),
                 (slc.Plant(P.A, B1.tocsc(), P.B2, C1, 0, D12), [[8, 9]])):
        assert _pass(slc, Q, S, flagged=False, groups=g)["rc"] == 0
    # the index-set-free half on its own
    lib = slc._capi.load_library()
    m = slc._capi.Marshalled(wc.weighted(P, wc.SEED_A), [], [], None)
    dg = np.zeros(Nx + Nu)
    assert lib.sls_debug_weights_shape_check(C.byref(m.dims), C.byref(m.plant), dg.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(dg, np.r_[wc.diagonals(P, wc.SEED_A)])
    m = slc._capi.Marshalled(slc.Plant(P.A, P.B1, P.B2, off, 0, D12), [], [], None)
    assert lib.sls_debug_weights_shape_check(C.byref(m.dims), C.byref(m.plant), None) == EU


# ---- the value rule ----

@pytest.mark.parametrize("base", [0, 1])
def test_value_rule_on_both_paths(slc, base):
    """0.0 without a ridge, NaN and inf are refused: the host path (strict) names the matrix and the position and writes nothing,
    the device path's twin skips the value, keeps its records and counts it.  0.0 with a positive ridge is accepted."""
    P, S = _plant(slc, "chain23")
    start = wc.weighted(P, wc.SEED_A)
    cA, dA = wc.diagonals(P, wc.SEED_A)
    cB, dB = wc.diagonals(P, wc.SEED_B)
    base_tables = _pass(slc, start, S, flagged=True, base=base)
    for which, k, v, word in (("C1", 6, 0.0, "zero cost weight"), ("D12", 3, 0.0, "zero cost weight"), ("C1", 11, np.nan, "not finite"),
                              ("D12", 0, np.inf, "not finite"), ("C1", 22, -np.inf, "not finite")):
        c, d = cB.copy(), dB.copy()
        (c if which == "C1" else d)[k] = v
        r = _pass(slc, start, S, flagged=True, base=base, c1=c, d12=d, strict=1)
        assert r["rc"] == slc._capi.SLS_EINVAL and f"{which} diagonal position {k} " in r["msg"] and word in r["msg"], r["msg"]
        assert _same_tables(r, base_tables) and np.array_equal(r["diag"], np.r_[cA, dA])          # untouched
        r = _pass(slc, start, S, flagged=True, base=base, c1=c, d12=d, strict=0)
        kept_c, kept_d = c.copy(), d.copy()
        (kept_c if which == "C1" else kept_d)[k] = (cA if which == "C1" else dA)[k]
        want = _pass(slc, wc.with_weights(P, kept_c, kept_d), S, flagged=True, base=base)
        assert r["rc"] == 0 and r["rejected"] == 1 and _same_tables(r, want) and np.array_equal(r["diag"], np.r_[kept_c, kept_d])
    # with a positive ridge a zero weight is a regular value, at plan time and in an update
    ridge = _ridge(P)
    c = cB.copy(); c[6] = 0.0
    r = _pass(slc, start, S, flagged=True, base=base, ridge=ridge, c1=c, d12=dB, strict=1)
    want = _pass(slc, wc.with_weights(P, c, dB), S, flagged=True, base=base, ridge=ridge)
    assert r["rc"] == 0 and want["rc"] == 0 and r["rejected"] == 0 and _same_tables(r, want)
    # … and without one it is refused at plan time too
    r = _pass(slc, wc.with_weights(P, c, dB), S, flagged=True, base=base)
    assert r["rc"] == slc._capi.SLS_EUNSUPPORTED and "zero cost weight" in r["msg"]


# ---- sanitizers ----

def test_weights_under_sanitizers(tmp_path):
    """csrc/sls_weights.cpp + csrc/sls_symbolic.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by the stand-alone program tests/host_sanitize/sanitize_weights.cpp."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_weights.cpp"), os.path.join(csrc, "sls_weights.cpp"), os.path.join(csrc, "sls_symbolic.cpp")]
    exe = str(tmp_path / "sanitize_weights")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_weights: clean" in r.stdout and "runtime error" not in r.stderr


# ---- Python surface ----

def test_python_surface_is_declared(slc):
    for name in ("update_weights", "update_weights_result", "weights"):
        assert callable(getattr(slc.Plan, name))
    assert {"sls_plan_update_weights", "sls_plan_update_weights_result", "sls_plan_fetch_weights"} <= set(slc._capi.EXPORTS)
    assert slc._capi.SLS_PLAN_WEIGHTS_UPDATABLE == FLAG
    lib = slc._capi.load_library()
    assert lib.sls_plan_update_weights.restype is C.c_int and len(lib.sls_plan_update_weights.argtypes) == 5
    n = C.c_int64(7)
    assert lib.sls_plan_update_weights(None, None, None, None, 0) == slc._capi.SLS_EINVAL          # null plans are refused
    assert lib.sls_plan_update_weights_result(None, C.byref(n)) == slc._capi.SLS_EINVAL
    assert lib.sls_plan_fetch_weights(None, None, None) == slc._capi.SLS_EINVAL


def test_update_weights_checks_its_arguments_without_a_device(slc):
    P, _ = _plant(slc, "chain23")
    plan = slc.Plan.__new__(slc.Plan)
    plan.m = slc._capi.Marshalled(P, [], [], None, flags=FLAG)
    plan.handle = None
    calls = []

    class _Lib:
        def sls_plan_update_weights(self, *a):
            calls.append(a)
            return 0
    plan._lib = _Lib()
    plan.ctx = type("Ctx", (), {"handle": None})()
    C1, D12 = wc.lqr_blocks(P.Nx, P.Nu, *wc.diagonals(P, wc.SEED_A))
    with pytest.raises(ValueError, match="diagonal values"):
        plan.update_weights(C1=np.ones(P.Nx + 1))
    with pytest.raises(ValueError, match="diagonal values"):
        plan.update_weights(D12=np.ones((P.Nu, 1)))
    with pytest.raises(ValueError, match="one stored entry per column"):
        plan.update_weights(C1=D12)                                           # the other block: wrong shape
    off = C1.copy(); off.indices[3] += 1
    with pytest.raises(ValueError, match="one stored entry per column"):
        plan.update_weights(C1=off)
    with pytest.raises(ValueError, match="C1, D12 or both"):
        plan.update_weights()
    assert calls == []
    plan.update_weights(C1=C1, D12=wc.diagonals(P, wc.SEED_A)[1])             # a matrix and a 1-D array
    assert len(calls) == 1 and calls[0][4] == 0 and plan._weights_updated
