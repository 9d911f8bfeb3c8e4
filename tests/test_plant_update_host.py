"""sls_plan_update_plant on the host (no GPU): the value map from CSC nzval positions to the plan's four operator arrays, the
zero and finite rules, and the host twin apply_operator_update (csrc/sls_symbolic.cpp) through sls_debug_operator_update_host.

What must hold is exact: after an update the four arrays are `csc_to_csr` / the transposed storage of the NEW matrix, bit for bit
(values are copied, never computed), and a refused update leaves them as they were."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import update_cases as uc


def _random_plant(slc, seed):
    rng = np.random.default_rng(seed)
    Nx, Nu = 37, 11
    A = sp.random(Nx, Nx, density=0.15, random_state=rng, format="csc") + sp.identity(Nx)
    B2 = sp.random(Nx, Nu, density=0.2, random_state=rng, format="csc")
    A, B2 = sp.csc_matrix(A), sp.csc_matrix(B2)
    A.data[::7] = 0.0                                   # stored zeros, kept by Plant
    return slc.Plant(A, sp.identity(Nx, format="csc"), B2)


def _plants(slc):
    return {"chain": slc.workloads.chain_plant(70), "banded_zeros": uc.banded(slc, stored_zeros=True), "random": _random_plant(slc, 3)}


def _host_update(slc, P, A_new, B2_new, base):
    """(rc, A_val, At_val, B_val, Bt_val, row_pos, zero) of sls_debug_operator_update_host"""
    lib = slc._capi.load_library()
    m = slc._capi.Marshalled(P, [], [], None, index_base=base)
    nA, nB = sp.csc_matrix(P.A).nnz, sp.csc_matrix(P.B2).nnz
    dp = C.POINTER(C.c_double)
    out = [np.full(max(n, 1), np.nan) for n in (nA, nA, nB, nB)]
    pos = np.zeros(max(nA + nB, 1), dtype=np.int32); zero = np.zeros(max(nA + nB, 1), dtype=np.uint8)
    a = None if A_new is None else np.ascontiguousarray(A_new, dtype=np.float64)
    b = None if B2_new is None else np.ascontiguousarray(B2_new, dtype=np.float64)
    rc = lib.sls_debug_operator_update_host(C.byref(m.dims), m.plant.A, m.plant.B2, None if a is None else a.ctypes.data_as(dp),
                                            None if b is None else b.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in out],
                                            pos.ctypes.data_as(C.POINTER(C.c_int32)), zero.ctypes.data_as(C.POINTER(C.c_uint8)))
    return (rc, out[0][:nA], out[1][:nA], out[2][:nB], out[3][:nB], pos[:nA + nB], zero[:nA + nB])


def _expected(M):
    """(row-ordered values, CSC-ordered values) of a CSC matrix, stored zeros kept"""
    M = sp.csc_matrix(M)
    R = M.tocsr(); R.sort_indices()                     # a format conversion keeps explicitly stored zeros
    assert R.nnz == M.nnz
    return R.data, M.data


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", ["chain", "banded_zeros", "random"])
def test_update_gives_the_arrays_of_the_new_matrix(slc, name, base):
    P = _plants(slc)[name]
    Q = uc.perturb(P)
    A0, B0, A1, B1 = (sp.csc_matrix(M) for M in (P.A, P.B2, Q.A, Q.B2))
    assert np.array_equal(A0.indices, A1.indices) and np.array_equal((A0.data == 0), (A1.data == 0)) and not np.array_equal(A0.data, A1.data)
    for a_new, b_new, wantA, wantB in ((A1.data, B1.data, A1, B1), (A1.data, None, A1, B0), (None, B1.data, A0, B1), (None, None, A0, B0)):
        rc, Av, Atv, Bv, Btv, pos, zero = _host_update(slc, P, a_new, b_new, base)
        assert rc == 0
        for got, want in zip((Av, Atv), _expected(wantA)):
            assert _same_bits(got, want)
        for got, want in zip((Bv, Btv), _expected(wantB)):
            assert _same_bits(got, want)
        # the map is a permutation of each matrix's positions, and the marks are the plan-time zeros
        assert sorted(pos[:A0.nnz]) == list(range(A0.nnz)) and sorted(pos[A0.nnz:]) == list(range(B0.nnz))
        assert np.array_equal(zero.astype(bool), np.r_[A0.data == 0.0, B0.data == 0.0])


@pytest.mark.parametrize("base", [0, 1])
def test_zero_rule_and_nan_refusals_leave_the_arrays_untouched(slc, base):
    P = uc.banded(slc, stored_zeros=True)
    A0, B0 = sp.csc_matrix(P.A), sp.csc_matrix(P.B2)
    Q = uc.perturb(P)
    kzA, kzB, knz = int(np.flatnonzero(A0.data == 0.0)[5]), int(np.flatnonzero(B0.data == 0.0)[2]), int(np.flatnonzero(A0.data != 0.0)[9])
    lib = slc._capi.load_library()
    for which, k, v, word in (("A", kzA, 0.3, "must stay 0.0"), ("B2", kzB, -1e-300, "must stay 0.0"), ("A", knz, np.nan, "not finite"),
                              ("B2", 0, np.inf, "not finite"), ("A", kzA, np.nan, "not finite")):
        a, b = sp.csc_matrix(Q.A).data.copy(), sp.csc_matrix(Q.B2).data.copy()
        (a if which == "A" else b)[k] = v
        rc, Av, Atv, Bv, Btv, _, _ = _host_update(slc, P, a, b, base)
        msg = lib.sls_last_error(None).decode()
        assert rc == slc._capi.SLS_EINVAL, (which, k, v)
        assert f"{which} nzval position {k} " in msg and word in msg, msg
        for got, want in zip((Av, Atv), _expected(A0)):
            assert _same_bits(got, want)
        for got, want in zip((Bv, Btv), _expected(B0)):
            assert _same_bits(got, want)
    # a non-zero entry may become 0.0 (either sign), and a plan-time zero may be rewritten with 0.0
    a = sp.csc_matrix(Q.A).data.copy(); a[knz] = 0.0; a[kzA] = -0.0
    rc, Av, Atv, _, _, _, _ = _host_update(slc, P, a, None, base)
    assert rc == 0 and _same_bits(Atv, a)


def test_update_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and UndefinedBehaviorSanitizer and driven by
    the stand-alone program tests/host_sanitize/sanitize_update.cpp: value map, zero marks and apply_operator_update on chain,
    banded stored-zero and random plants in both index bases, refusals, and maps / arrays of the wrong length."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_update.cpp"), os.path.join(csrc, "sls_symbolic.cpp")]
    exe = str(tmp_path / "sanitize_update")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_update: clean" in r.stdout and "runtime error" not in r.stderr


# ---- Python surface ----

def test_python_surface_is_declared(slc):
    assert callable(getattr(slc.Plan, "update_plant")) and callable(getattr(slc.Plan, "update_result"))
    assert callable(getattr(slc.Plan, "plant_values"))
    assert {"sls_plan_update_plant", "sls_plan_update_result", "sls_plan_fetch_plant"} <= set(slc._capi.EXPORTS)
    lib = slc._capi.load_library()
    assert lib.sls_plan_update_plant.restype is C.c_int and len(lib.sls_plan_update_plant.argtypes) == 5
    assert lib.sls_plan_update_plant.argtypes[-1] is C.c_int
    assert lib.sls_plan_update_result.restype is C.c_int and lib.sls_plan_update_result.argtypes[1] == C.POINTER(C.c_int64)
    assert lib.sls_abi_version() == 2
    # null plans are refused, not dereferenced
    n = C.c_int64(7)
    assert lib.sls_plan_update_plant(None, None, None, None, 0) == slc._capi.SLS_EINVAL
    assert lib.sls_plan_update_result(None, C.byref(n)) == slc._capi.SLS_EINVAL
    assert lib.sls_plan_fetch_plant(None, None, None) == slc._capi.SLS_EINVAL and len(lib.sls_plan_fetch_plant.argtypes) == 3


class _NoDevicePlan:
    """A Plan's Python side without a device: `update_plant` marshals and checks its arguments before it reaches the library."""

    def __init__(self, slc, P):
        self.plan = slc.Plan.__new__(slc.Plan)
        self.plan.m = slc._capi.Marshalled(P, [], [], None)
        self.plan.handle = None                        # close() / __del__ have nothing to free

        class _Lib:
            calls = []

            def sls_plan_update_plant(self, *a):
                self.calls.append(a)
                return 0
        self.lib = self.plan._lib = _Lib()
        self.plan.ctx = type("Ctx", (), {"handle": None})()


def _struct_nzval(m, name, n):
    return np.ctypeslib.as_array(getattr(m.plant, name).contents.nzval, shape=(n,))


def test_update_plant_checks_pattern_and_length_without_a_device(slc):
    P = uc.banded(slc, stored_zeros=True)
    Q = uc.perturb(P)
    nA = sp.csc_matrix(P.A).nnz
    h = _NoDevicePlan(slc, P)
    plan = h.plan
    with pytest.raises(ValueError, match="pattern of A"):
        plan.update_plant(A=uc.banded(slc).A)                             # same matrix by value, fewer stored entries
    moved = sp.csc_matrix(Q.B2).copy(); moved.indices[-1] -= 1
    with pytest.raises(ValueError, match="pattern of B2"):
        plan.update_plant(B2=moved)
    with pytest.raises(ValueError, match="nzval entries"):
        plan.update_plant(A=np.ones(nA - 1))
    with pytest.raises(ValueError, match="nzval entries"):
        plan.update_plant(B2=np.ones((sp.csc_matrix(P.B2).nnz, 1)))
    plan.update_plant()                                                   # nothing given: nothing to do
    assert h.lib.calls == []                                              # nothing reached the library ...
    assert plan.m.nzval is None                                           # ... and nothing was copied: a plan that is never updated pays nothing
    assert np.array_equal(_struct_nzval(plan.m, "A", nA), sp.csc_matrix(P.A).data)
    plan.update_plant(A=Q.A, B2=sp.csc_matrix(Q.B2).data)                 # a matrix and an nzval array
    assert len(h.lib.calls) == 1 and h.lib.calls[0][4] == 0
    # the marshalled plant (what a later refine passes) holds the new values, in the arrays the ctypes structs point at
    assert np.array_equal(plan.m.nzval["A"], sp.csc_matrix(Q.A).data) and np.array_equal(plan.m.nzval["B2"], sp.csc_matrix(Q.B2).data)
    assert np.array_equal(_struct_nzval(plan.m, "A", nA), sp.csc_matrix(Q.A).data)
    assert plan._plant_updated
    assert np.array_equal(sp.csc_matrix(P.A).data, uc.banded(slc, stored_zeros=True).A.data)      # the caller's plant is not written
