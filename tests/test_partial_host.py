"""The partial re-solve on the host (no GPU): which subproblems a plant update touches.

The rule (tests/partial_cases.py): subproblem q is affected when a changed A[i,j] has i, j ∈ s_x(q) or a changed B2[i,k] has
i ∈ s_x(q) and k ∈ s_u(q).  sls_debug_affected_host — mark_affected_host of csrc/sls_symbolic.cpp, the host twin of
changed_entries_kernel's flag layout and mark_affected_kernel — must give exactly the NumPy reference's marks for every change
set, in both index bases.  Everything compared is a set of integers; there is no tolerance."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import partial_cases as pc
import update_cases as uc

ALL_SETS = [(plant, name) for plant in pc.CHANGES for name in pc.CHANGES[plant]]


def _host_marks(slc, P, S, groups, fa, fb, base):
    lib = slc._capi.load_library()
    m = slc._capi.Marshalled(P, S[0], S[1], groups, index_base=base)
    u8p = C.POINTER(C.c_uint8)
    d = np.full(max(m.n_sub, 1), 7, dtype=np.uint8)                       # every byte must be written
    rc = lib.sls_debug_affected_host(*m.common_args(), fa.ctypes.data_as(u8p), fb.ctypes.data_as(u8p), d.ctypes.data_as(u8p))
    assert rc == 0, slc._capi.last_error()
    return d[: m.n_sub]


@pytest.mark.parametrize("plant", list(pc.CHANGES))
def test_reference_marks_some_but_not_all(slc, plant):
    """The reference alone: every change set that changes something marks 0 < affected < all subproblems of its setting, and one
    that changes nothing marks none — so the comparisons below, and on the GPU, cannot pass vacuously."""
    n_some = 0
    for name in pc.CHANGES[plant]:
        a, b, exp, marks = pc.reference(slc, plant, name)
        k = int(marks.sum())
        if exp == "some":
            assert 0 < k < marks.size, (plant, name, k, marks.size)
            n_some += 1
        else:
            assert k == 0, (plant, name, k)
            fa, fb = pc.changed_flags(pc.setting(slc, plant)[0], a, b)
            assert fa.sum() == 0 and fb.sum() == 0
    assert n_some > 0


def test_reference_edges(slc):
    """What the change sets are there for: the off-diagonal entry marks fewer columns than the diagonal one (a column with 35
    but not 36 in s_x stays clean); 0.0 → −0.0 is one changed entry; the random plant has rows of exactly one stored entry;
    the dense row changes more entries than a wavefront has lanes."""
    P, S, groups = pc.setting(slc, "chain70")
    sets = pc.index_sets(slc, P, S, groups)
    d = pc.reference(slc, "chain70", "A35_35")[3]; o = pc.reference(slc, "chain70", "A35_36")[3]
    only35 = [q for q, (sx, _) in enumerate(sets) if 35 in sx and 36 not in sx]
    assert only35 and all(d[q] == 1 and o[q] == 0 for q in only35)
    assert np.all(o <= d) and o.sum() < d.sum()
    Pz = pc.setting(slc, "banded_zeros")[0]
    a, b, _, _ = pc.reference(slc, "banded_zeros", "negzero")
    fa, fb = pc.changed_flags(Pz, a, b)
    assert fa.sum() == 1 and fb.sum() == 0 and np.array_equal(a, uc.banded(slc, stored_zeros=True).A.data)   # equal by value
    Pr = pc.setting(slc, "random")[0]
    one_entry_rows = 0
    for r in range(Pr.Nx):
        _, bnew, exp, _ = pc.reference(slc, "random", f"B_row{r}")
        one_entry_rows += exp == "some" and int(pc.changed_flags(Pr, None, bnew)[1].sum()) == 1
    assert one_entry_rows > 0
    Pd = pc.setting(slc, "dense_row")[0]
    _, bnew, _, _ = pc.reference(slc, "dense_row", "B_row36")
    assert pc.changed_flags(Pd, None, bnew)[1].sum() > 64


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("plant", list(pc.CHANGES))
def test_host_twin_equals_the_reference(slc, plant, base):
    P, S, groups = pc.setting(slc, plant)
    for name in pc.CHANGES[plant]:
        a, b, _, marks = pc.reference(slc, plant, name)
        fa, fb = pc.changed_flags(P, a, b)
        got = _host_marks(slc, P, S, groups, fa, fb, base)
        assert np.array_equal(got, marks), (plant, name, np.flatnonzero(got != marks))


def test_host_twin_on_coupled_groups(slc):
    """Groups of several columns share the group's index sets: every column of a group is marked with it."""
    P, S, _ = pc.setting(slc, "chain70")
    groups = [[0, 1], [34, 35, 36], [50], [68, 69]]
    sets = pc.index_sets(slc, P, S, groups)
    a, b, _ = pc.CHANGES["chain70"]["A35_35"](P)
    fa, fb = pc.changed_flags(P, a, b)
    want = pc.affected(P, sets, fa, fb)
    assert 0 < want.sum() < want.size and want[2] == want[3] == want[4] == 1
    for base in (0, 1):
        assert np.array_equal(_host_marks(slc, P, S, groups, fa, fb, base), want)


def test_affected_under_sanitizers(tmp_path):
    """csrc/sls_symbolic.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and UndefinedBehaviorSanitizer and driven by
    the stand-alone program tests/host_sanitize/sanitize_affected.cpp: mark_affected_host against a brute-force statement of the
    rule on a banded plant with a dense B2 row and a random plant, both index bases, ñx = 1 and ñu = 0 subproblems, accumulation,
    maps of the wrong plant."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_affected.cpp"), os.path.join(csrc, "sls_symbolic.cpp")]
    exe = str(tmp_path / "sanitize_affected")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_affected: clean" in r.stdout and "runtime error" not in r.stderr


# ---- Python surface ----

def test_python_surface_is_declared(slc):
    for name in ("track_changes", "execute_columns", "execute_dirty", "dirty", "clear_dirty"):
        assert callable(getattr(slc.Plan, name)), name
    new = {"sls_plan_execute_columns", "sls_plan_track_changes", "sls_plan_execute_dirty", "sls_plan_fetch_dirty", "sls_plan_clear_dirty"}
    assert new <= set(slc._capi.EXPORTS)
    lib = slc._capi.load_library()
    assert lib.sls_plan_execute_columns.restype is C.c_int and len(lib.sls_plan_execute_columns.argtypes) == 7
    assert lib.sls_plan_execute_columns.argtypes[4] == C.POINTER(C.c_int64) and lib.sls_plan_execute_columns.argtypes[5] is C.c_int64
    assert len(lib.sls_plan_execute_dirty.argtypes) == 5 and lib.sls_plan_execute_dirty.argtypes[-1] == C.POINTER(C.c_int64)
    assert len(lib.sls_plan_track_changes.argtypes) == 2 and lib.sls_plan_fetch_dirty.argtypes[1] == C.POINTER(C.c_uint8)
    assert lib.sls_abi_version() == 2                                     # no struct that crosses the ABI changed
    # null plans are refused, not dereferenced
    n = C.c_int64(7)
    assert lib.sls_plan_execute_columns(None, None, None, 0, None, 0, C.byref(n)) == slc._capi.SLS_EINVAL and n.value == 0
    assert lib.sls_plan_execute_dirty(None, None, None, 0, None) == slc._capi.SLS_EINVAL
    assert lib.sls_plan_track_changes(None, 1) == slc._capi.SLS_EINVAL
    assert lib.sls_plan_fetch_dirty(None, None) == slc._capi.SLS_EINVAL
    assert lib.sls_plan_clear_dirty(None, None) == slc._capi.SLS_EINVAL


class _NoDevicePlan:
    """A Plan's Python side without a device: `execute_columns` checks its list before it reaches the library."""

    def __init__(self, slc, n):
        self.plan = slc.Plan.__new__(slc.Plan)
        self.plan.handle = None                        # close() / __del__ have nothing to free
        self.plan.info = {"n_subproblems": n}

        class _Lib:
            calls = []

            def sls_plan_execute_columns(self, *a):
                self.calls.append(a)
                a[-1]._obj.value = int(a[5])
                return 0
        self.lib = self.plan._lib = _Lib()
        self.plan.ctx = type("Ctx", (), {"handle": None})()


def test_execute_columns_checks_its_list_without_a_device(slc):
    h = _NoDevicePlan(slc, 10)
    plan = h.plan
    for bad in ([3, 2], [1, 1], [-1, 2], [0, 10], [[1, 2]], [0.5, 2.0]):
        with pytest.raises(ValueError):
            plan.execute_columns(0, bad)
    assert h.lib.calls == []                                              # nothing reached the library
    assert plan.execute_columns(0, []) == 0 and h.lib.calls == []         # an empty list enqueues nothing
    assert plan.execute_columns(0, [0, 4, 9], packed=True) == 3
    assert len(h.lib.calls) == 1 and h.lib.calls[0][3] == 1 and h.lib.calls[0][5] == 3
    assert plan.execute_columns(0, np.array([2, 7], dtype=np.int32)) == 2
