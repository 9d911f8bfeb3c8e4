"""CPU tests of the host side: C-ABI loads and exports what include/sls_mi355x.h declares, the
symbolic pass (reduction / layout / sharding) and the Plant mirror.  No compute calls."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, ROOT


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(sls_[a-z0-9_]+)\s*\(", hdr))


def test_library_exports_every_declared_symbol(slc):
    """Both directions: everything include/*.h declares is exported, and the library exports no `sls_*` C symbol that no
    header names (the diagnostic hooks live in include/sls_mi355x_debug.h, outside the drop-in boundary)."""
    import subprocess
    declared = _declared("sls_mi355x.h")
    debug = _declared("sls_mi355x_debug.h")
    assert declared and debug, "no prototypes parsed"
    assert not (declared & debug)
    lib = slc.load_library()
    for name in sorted(declared | debug):
        assert hasattr(lib, name), f"{name} declared in a header but not exported"
    assert declared == set(slc._capi.EXPORTS)
    so = os.path.join(ROOT, "systemlevelcontrol.jl_amd", "libsls_mi355x.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-2] in "TW"}
    c_syms = {n for n in exported if re.fullmatch(r"sls_[a-z0-9_]+", n)}
    assert c_syms == declared | debug, sorted(c_syms ^ (declared | debug))
    assert lib.sls_abi_version() == 2


def test_no_cpu_fallback_without_device(slc, readme):
    lib = slc.load_library()
    if lib.sls_device_count() > 0:
        pytest.skip("a GPU is present")
    P, S, _ = readme
    with pytest.raises(slc.SLSError) as ei:
        slc.SLS_H2(P, S)
    assert ei.value.code == slc._capi.SLS_ENODEVICE


def _single_step_masks(P):
    Ab = (P.A != 0).astype(np.int32).tocsc()
    R = sp.identity(P.Nx, dtype=np.int32, format="csc")
    for _ in range(9):
        R = ((R @ Ab) != 0).astype(np.int32).tocsc()
    Sx = (R != 0).tocsc(); Sx.sort_indices()
    Su = ((((P.B2.T != 0).astype(np.int32)) @ R) != 0).tocsc(); Su.sort_indices()
    return Sx, Su


@pytest.mark.parametrize("base", [0, 1])
def test_capi_reduction_known_answer(slc, readme, base):
    """reference test/reduction_test.jl:11-24 through the C ABI, with Julia (1-based) and C (0-based) indices."""
    ka = json.load(open(os.path.join(GOLDEN, "reduction_known_answer.json")))
    P, _, _ = readme
    Sx, Su = _single_step_masks(P)
    lib = slc.load_library()
    cap = slc._capi

    def csc(M, cls, dt):
        M = sp.csc_matrix(M); M.sort_indices()
        cp = (M.indptr.astype(np.int64) + base); rv = (M.indices.astype(np.int64) + base)
        nz = np.ascontiguousarray(M.data, dtype=dt)
        keep = (cp, rv, nz)
        s = cls(M.shape[0], M.shape[1], cp.ctypes.data_as(C.POINTER(C.c_int64)), rv.ctypes.data_as(C.POINTER(C.c_int64)),
                nz.ctypes.data_as(C.POINTER(C.c_double if dt == np.float64 else C.c_uint8)))
        return s, keep
    A, k1 = csc(P.A, cap.sls_csc_f64, np.float64)
    sx_, k2 = csc(Sx, cap.sls_csc_bool, np.uint8)
    su_, k3 = csc(Su, cap.sls_csc_bool, np.uint8)
    dims = cap.sls_dims(P.Nx, P.Nu, P.Nz, P.Nw, 1, base, 0)
    cj = np.asarray(ka["cj"], dtype=np.int64) + base
    sx = np.zeros(P.Nx, dtype=np.int64); su = np.zeros(P.Nu, dtype=np.int64)
    nsx, nsu = C.c_int64(), C.c_int64()
    i64p = C.POINTER(C.c_int64)
    rc = lib.sls_sparsity_dim_reduction(C.byref(dims), C.byref(A), C.byref(sx_), C.byref(su_), cj.ctypes.data_as(i64p),
                                        len(cj), sx.ctypes.data_as(i64p), C.byref(nsx), su.ctypes.data_as(i64p), C.byref(nsu))
    assert rc == 0
    assert (sx[:nsx.value] - base).tolist() == ka["expected_sx"]
    assert (su[:nsu.value] - base).tolist() == ka["expected_su"]


def test_symbolic_pass_is_index_base_invariant(slc, readme):
    """Julia hands over 1-based colptr/rowval/group columns (index_base = 1): the symbolic pass must produce the same
    layout as for the 0-based copies of the same matrices (destinations are offsets into the value array, base-free)."""
    P, S, _ = readme
    groups = [list(range(0, 20)), [25], list(range(40, 59))]
    for g, rng in ((None, (0, P.Nx)), (None, (10, 30)), (groups, (0, 3)), (groups, (1, 3))):
        d0, n0, i0 = slc.dist.packed_layout(P, S, g, rng, index_base=0)
        d1, n1, i1 = slc.dist.packed_layout(P, S, g, rng, index_base=1)
        assert n0 == n1 and np.array_equal(d0, d1)
        assert {k: v for k, v in i0.items() if not k.startswith("t_")} == {k: v for k, v in i1.items() if not k.startswith("t_")}


def test_packed_layout_matches_oracle_counts(slc, readme, golden_readme):
    P, S, _ = readme
    dest, nval, info = slc.dist.packed_layout(P, S, None, (0, P.Nx))
    assert nval == 26413 + 9616
    assert len(dest) == int(golden_readme["col_nfree"].sum()) == 36029          # Σfree = nnz(𝓢x)+nnz(𝓢u)
    assert len(np.unique(dest)) == len(dest) and dest.min() == 0 and dest.max() == nval - 1
    assert info["max_nx"] == 21 and info["max_nu"] == 8 and info["n_subproblems"] == 59
    assert abs(info["flops_alg"] - 5.05e7) / 5.05e7 < 0.01                      # SURVEY §8d ΣF_alg
    # shards tile the packed set
    cuts = slc.dist.shard_groups(P, S, None, 4)
    assert cuts[0] == 0 and cuts[-1] == P.Nx and np.all(np.diff(cuts) > 0)
    parts = [slc.dist.packed_layout(P, S, None, (int(cuts[i]), int(cuts[i + 1])))[0] for i in range(4)]
    assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(nval))


def test_shard_groups_balances_cost(slc, readme):
    P, S, _ = readme
    cuts = slc.dist.shard_groups(P, S, None, 8)
    # cost ∝ ñx³: edge columns (ñx = 11) are ≈7× cheaper than interior ones (ñx = 21) ⇒ edge shards are wider
    widths = np.diff(cuts)
    assert widths[0] > widths[3] and widths[-1] > widths[4]
    assert widths.sum() == P.Nx


def test_validation_errors(slc, readme):
    P, S, _ = readme
    bad = [S[0][:-1], S[1]]
    with pytest.raises(ValueError):
        slc._capi.Marshalled(P, bad[0], bad[1])
    # wrong mask shape → SLS_EINVAL from the library (host-only entry point)
    Sx_bad = [sp.csc_matrix((P.Nx + 1, P.Nx), dtype=bool)] * len(S[0])
    with pytest.raises(slc.SLSError) as ei:
        slc.dist.packed_layout(P, [Sx_bad, S[1]], None, (0, 1))
    assert ei.value.code == slc._capi.SLS_EINVAL
    # unsorted group → EINVAL
    with pytest.raises(slc.SLSError):
        slc.dist.packed_layout(P, S, [[3, 1]], (0, 1))
    # a column in two groups → EINVAL (two subproblems would race for the same column of Φ; the reference would add them)
    with pytest.raises(slc.SLSError) as ei:
        slc.dist.packed_layout(P, S, [[1, 2], [2, 5]], (0, 2))
    assert ei.value.code == slc._capi.SLS_EINVAL and "more than one group" in str(ei.value)


def test_unsupported_cost_is_reported_not_guessed(slc, readme):
    """What this build cannot solve is reported, never approximated: a cost that leaves a free variable without weight.  A dense
    cost Hessian [C1 D12]ᵀ[C1 D12] and column groups coupled through a non-diagonal B1[c_j,c_j] block (src/synthesis.jl:42) are
    accepted since round 2 (symbolic pass only here; the solves are in tests/test_gpu_tile.py)."""
    P, S, _ = readme
    rng = np.random.default_rng(0)
    W = sp.csc_matrix(rng.normal(size=(P.Nx + P.Nu, P.Nx + P.Nu)))
    Pw = slc.Plant(P.A, P.B1, P.B2, W[:, :P.Nx], 0, W[:, P.Nx:])
    dest, nval, info = slc.dist.packed_layout(Pw, S, None, (0, 1))
    assert info["n_subproblems"] == 1
    # a multi-column group coupled through B1[c_j,c_j] is accepted since round 2 (one work item for the group; the solve is in
    # tests/test_gpu_tile.py) — unless one of its columns lies outside the group's own s_x, where the reference's Φ̃·B̃1 is a
    # DimensionMismatch
    B1c = sp.lil_matrix(sp.identity(P.Nx)); B1c[3, 4] = 0.5
    Pc = slc.Plant(P.A, B1c.tocsc(), P.B2)
    dest, nval, info = slc.dist.packed_layout(Pc, S, [[3, 4]], (0, 1))
    assert info["n_subproblems"] == 2
    slc.dist.packed_layout(Pc, S, None, (0, 4))                        # the same B1 with single-column groups
    Wz = sp.lil_matrix(sp.identity(P.Nx + P.Nu)); Wz[0, 0] = 0.0
    Pz = slc.Plant(P.A, P.B1, P.B2, sp.csc_matrix(Wz)[:, :P.Nx], 0, sp.csc_matrix(Wz)[:, P.Nx:])
    with pytest.raises(slc.SLSError) as ei:
        slc.dist.packed_layout(Pz, S, None, (0, 1))
    assert ei.value.code == slc._capi.SLS_EUNSUPPORTED


def test_plant_mirror_defaults_and_errors(slc):
    """reference test/types_GeneralizedPlant_test.jl:106-120 (SF defaults, LQR default weights) and :123-130 (errors)."""
    A = sp.random(12, 12, 0.3, random_state=1); B1 = sp.identity(12); B2 = sp.random(12, 5, 0.4, random_state=2)
    P = slc.Plant(A, B1, B2)
    assert P.Ts is slc.StateFeedback and (P.Nx, P.Nz, P.Ny, P.Nw, P.Nu) == (12, 17, 12, 12, 5)
    assert (abs(sp.hstack([P.C1, P.D12]) - sp.identity(17))).nnz == 0 and P.D11.nnz == 0
    assert (abs(P.C2 - sp.identity(12))).nnz == 0 and P.D21.shape == (0, 12) and P.D22.shape == (0, 5)
    assert len(list(P)) == 9
    with pytest.raises(ValueError):
        slc.Plant(sp.random(12, 11, 0.3), B1, B2)
    with pytest.raises(ValueError):
        slc.Plant(A, sp.identity(11), B2)
    with pytest.raises(ValueError):
        slc.Plant(A, B1, B2, sp.identity(17, format="csc")[:, :11], 0, sp.identity(17, format="csc")[:, 12:])
    # output-feedback plants are not on this path: SLS_𝓗₂ returns nothing (src/synthesis.jl:13,30)
    Pof = slc.Plant(A, B1, B2, sp.identity(17, format="csc")[:, :12], 0, sp.identity(17, format="csc")[:, 12:], sp.random(3, 12, 0.5), np.zeros((3, 12)), np.zeros((3, 5)))
    assert Pof.Ts is slc.OutputFeedback
    assert slc.SLS_H2(Pof, [[], []]) is None


@pytest.mark.parametrize("case", ["readme", "grid", "random", "nilpotent", "chain_alpha2"])
def test_localization_masks_match_boolean_matrix_powers(slc, case):
    """sls_localization_masks (level sets of exact k-step walks, host threads) against the SciPy restatement of the
    README recipe (README.md:53-54: Boolean matrix powers), pattern for pattern, for every t."""
    wl = slc.workloads
    if case == "readme":
        P = wl.chain_plant(59); d, T, al = 9, 29, 1.5
    elif case == "grid":
        P = wl.grid_plant(12, 3); d, T, al = 4, 10, 1.5
    elif case == "random":
        P = wl.random_plant(300, 2, 2, seed=3); d, T, al = 3, 9, 1.0
    elif case == "nilpotent":        # no diagonal: (A≠0)^k is "exactly k steps", not "within k steps"
        A = sp.diags(np.ones(19), -1).tocsc() + sp.csc_matrix(([1.0], ([0], [19])), shape=(20, 20))
        P = slc.Plant(A, sp.identity(20, format="csc"), sp.identity(20, format="csc")[:, [0, 5, 11]]); d, T, al = 5, 12, 1.0
    else:
        P = wl.chain_plant(700); d, T, al = 6, 7, 2.0
    Sx0, Su0 = wl.localization_masks(P.A, P.B2, d, T, al)
    Sx1, Su1 = wl.localization_masks_native(P.A, P.B2, d, T, al)
    for a, b in zip(Sx0 + Su0, Sx1 + Su1):
        a = sp.csc_matrix(a); a.eliminate_zeros(); a.sort_indices()
        assert a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


def _build_c_example(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "solve_readme")
    libdir = os.path.join(root, "systemlevelcontrol.jl_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
           os.path.join(root, "examples", "solve_readme.c"), "-o", exe, "-L" + libdir, "-lsls_mi355x",
           "-Wl,-rpath," + libdir, "-lm"]
    subprocess.check_call(cmd)
    return exe


def test_header_is_plain_c_and_library_links_from_c(slc, tmp_path):
    """include/sls_mi355x.h compiles as strict C99 and a C host links against the shared library (the position of the
    Julia `ccall` binding): examples/solve_readme.c builds without warnings.  Running it needs the GPU (test_gpu_parity)."""
    exe = _build_c_example(tmp_path)
    assert os.path.exists(exe)


def _layout_worker(args):
    import slc_amd
    P, S = args
    return int(slc_amd.dist.packed_layout(P, S, None, (0, P.Nx))[2]["n_subproblems"])


def test_symbolic_pass_survives_fork(slc):
    """The symbolic pass parks its host worker threads between calls; a fork()ed child (Python multiprocessing's "fork" start
    method) inherits the pool object without its threads and must get a fresh pool instead of waiting for them forever."""
    import multiprocessing as mp
    P = slc.workloads.chain_plant(1024)
    S = list(slc.workloads.localization_masks_native(P.A, P.B2, 6, 12, 1.5))
    assert _layout_worker((P, S)) == 1024                      # parent: creates the pool (1024 groups → several threads)
    with mp.get_context("fork").Pool(2) as pool:
        assert pool.map(_layout_worker, [(P, S), (P, S)]) == [1024, 1024]


def test_symbolic_pass_under_sanitizers(tmp_path):
    """The host symbolic pass and kernel selection (csrc/sls_symbolic.cpp, csrc/sls_routing.cpp: plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by tests/host_sanitize/sanitize_symbolic.cpp over chain / grid / random plants, both
    index bases, all four table layouts, shard ranges with an empty shard, caller groups, the device passes' input builders, the
    closed-loop operator and malformed inputs; and over the host arithmetic of plan construction (csrc/sls_arena.h, the solver
    knobs, the scratch layout and the sum-of-norms weights check of csrc/sls_routing.cpp).  A second run, outside lab mode, checks
    the solver parameters' defaults.  (GPU sanitizers are not available on this pool; this is the CPU build.)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_symbolic.cpp"), os.path.join(csrc, "sls_symbolic.cpp"),
           os.path.join(csrc, "sls_routing.cpp")]
    exe = str(tmp_path / "sanitize_symbolic")
    # sls_device.h marks a few size helpers __host__ __device__ for hipcc; g++ sees plain functions
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_symbolic: clean" in r.stdout and "runtime error" not in r.stderr
    for done in ("solver knobs: done", "arena layout: done", "scratch layout: done", "sum-of-norms weights: done"):
        assert done in r.stdout
    env.pop("SLS_LAB", None)                                  # latched on first use: the defaults need a process of their own
    r = subprocess.run([exe, "defaults"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_symbolic: defaults clean" in r.stdout and "runtime error" not in r.stderr


def _launch_list_cases():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_launch_lists", os.path.join(GOLDEN, "make_golden_launch_lists.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_launch_lists_match_the_recorded_plans(slc):
    """Kernel selection (csrc/sls_routing.cpp) without a device: for every case of tests/golden/make_golden_launch_lists.py,
    sls_debug_describe_launches with the CU count of the recording device gives, character for character, the string that
    `Plan.describe()` gave for the live plan on the MI355X (tests/golden/launch_lists.json).  A routing change shows up here;
    an intended one regenerates the golden file on the GPU box."""
    gen = _launch_list_cases()
    with open(os.path.join(GOLDEN, "launch_lists.json")) as f:
        golden = json.load(f)
    cases = gen.cases(slc)
    assert {c["name"] for c in cases} == set(golden["cases"])
    wrong = {}
    for case in cases:
        P, S, groups = gen.problem(slc, case["plant"])
        with gen.knobs(case["env"]):
            got = slc.dist.describe_launches(P, S, groups, gen.group_range(slc, case, P, S, groups), golden["ncu"],
                                             objective=case["objective"])
        if got != golden["cases"][case["name"]]:
            wrong[case["name"]] = (got, golden["cases"][case["name"]])
    assert not wrong, wrong


def test_graft_entry_build_runs():
    """__graft_entry__.build() — the driver's "does it build" check — end to end: make (a no-op when up to date), import, ABI check."""
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    ge = importlib.import_module("__graft_entry__")
    assert ge.build() is None
