"""Reference and change sets shared by tests/test_partial_host.py and tests/test_gpu_partial.py (a plain module like
update_cases.py; not a conftest).

The feature under test re-solves only the subproblems a plant update touched.  Subproblem q reads the plant only through
A[s_x(q), s_x(q)] and B2[s_x(q), s_u(q)], so the rule is:

    q is affected  ⇔  some changed A[i, j] has i ∈ s_x(q) and j ∈ s_x(q),  or  some changed B2[i, k] has i ∈ s_x(q) and k ∈ s_u(q)

`affected` states it in NumPy over index sets from sls_sparsity_dim_reduction (the library's host reduction, pinned against the
reference's own by tests/test_oracle.py and tests/test_symbolic_cases_host.py).  An entry counts as changed when the update
accepts it (finite, and a plan-time zero stays zero) and the BITS of the new value differ from the current one: `changed_flags`.

Change sets (`CHANGES[plant]`: name → function P ↦ (A nzval or None, B2 nzval or None, expectation)); expectation "some" means
0 < affected < all must hold for the setting's columns — asserted on the reference alone by the host test, so that the GPU tests
cannot pass vacuously — and "none" that nothing may be marked:

  chain70       A[35,35];  A[35,36] (off-diagonal: a column with 35 but not 36 in s_x stays clean);  B2[0,0];
                an entry rewritten with its own value (none)
  banded_zeros  a stored zero of A rewritten as −0.0: the bits differ, it counts
  grid10        one corner entry, one centre entry of A
  random        the `_random_plant` of test_plant_update_host.py, restated: for every plant row, all of A's entries in it, and
                all of B2's (rows of one entry included); a row whose entries are all stored zeros changes nothing and is skipped
  dense_row     a 72-state banded plant whose B2 has one dense row of 72 entries — more changed entries in one row than a
                wavefront has lanes (the random plant, 37 × 11, has no such row)"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import update_cases as uc

_cache = {}


def random_plant(slc, seed=3):
    """`_random_plant` of test_plant_update_host.py, restated."""
    rng = np.random.default_rng(seed)
    Nx, Nu = 37, 11
    A = sp.random(Nx, Nx, density=0.15, random_state=rng, format="csc") + sp.identity(Nx)
    B2 = sp.random(Nx, Nu, density=0.2, random_state=rng, format="csc")
    A, B2 = sp.csc_matrix(A), sp.csc_matrix(B2)
    A.data[::7] = 0.0                                   # stored zeros, kept by Plant
    return slc.Plant(A, sp.identity(Nx, format="csc"), B2)


def dense_row_plant(slc):
    """72 states: A tridiagonal, B2 = I plus row 36 dense (72 stored entries in one row)."""
    n = 72
    A = sp.csc_matrix(sp.identity(n) + sp.diags(0.2 * np.ones(n - 1), 1) - sp.diags(0.2 * np.ones(n - 1), -1))
    B2 = sp.lil_matrix(sp.identity(n))
    B2[36, :] = 0.05 + 0.01 * np.arange(n)
    B2[36, 36] = 1.0
    B2 = sp.csc_matrix(B2)
    A.sort_indices(); B2.sort_indices()
    return slc.Plant(A, sp.identity(n, format="csc"), B2)


def setting(slc, plant):
    """(P, S, groups) the host test (and the GPU mark tests of the plants no update case uses) runs a plant's change sets on."""
    if plant not in _cache:
        if plant == "chain70":
            _cache[plant] = uc.case(slc, "wave")[:3]
        elif plant == "banded_zeros":
            _cache[plant] = uc.case(slc, "t4_zeros")[:3]
        elif plant == "grid10":
            _cache[plant] = uc.case(slc, "tile")[:3]
        else:
            P = random_plant(slc) if plant == "random" else dense_row_plant(slc)
            d, T = (1, 3) if plant == "random" else (3, 4)
            S = slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5)
            _cache[plant] = (P, [list(S[0]), list(S[1])], [[c] for c in range(P.Nx)])
    return _cache[plant]


def _nz(M):
    return sp.csc_matrix(M).data


def _pos(M, i, j):
    """nzval position of the stored entry (i, j) of a CSC matrix"""
    M = sp.csc_matrix(M)
    hit = np.flatnonzero(M.indices[M.indptr[j]:M.indptr[j + 1]] == i)
    assert hit.size == 1, (i, j)
    return int(M.indptr[j] + hit[0])


def _one(name, i, j, f):
    def build(P):
        a, b = _nz(P.A).copy(), _nz(P.B2).copy()
        v = a if name == "A" else b
        k = _pos(P.A if name == "A" else P.B2, i, j)
        v[k] = f(v[k])
        return (a, None, "some") if name == "A" else (None, b, "some")
    return build


def _same(P):
    return _nz(P.A).copy(), _nz(P.B2).copy(), "none"


def _negzero(P):
    a = _nz(P.A).copy()
    k = _pos(P.A, 30, 33)                                # the +3 diagonal of banded_zeros: stored 0.0
    assert a[k] == 0.0 and not np.signbit(a[k])
    a[k] = -0.0
    return a, None, "some"


def _row(name, r):
    def build(P):
        M = sp.csc_matrix(P.A if name == "A" else P.B2)
        v = M.data.copy()
        sel = (M.indices == r) & (v != 0.0)              # stored zeros stay (the zero rule)
        v[sel] += 1.0
        exp = "some" if sel.any() else "none"
        return (v, None, exp) if name == "A" else (None, v, exp)
    return build


CHANGES = {
    "chain70": {"A35_35": _one("A", 35, 35, lambda v: v + 0.25), "A35_36": _one("A", 35, 36, lambda v: 1.5 * v),
                "B0_0": _one("B2", 0, 0, lambda v: 0.5 * v), "same": _same},
    "banded_zeros": {"negzero": _negzero},
    "grid10": {"corner": _one("A", 0, 0, lambda v: v + 0.125), "centre": _one("A", 45, 45, lambda v: v - 0.125)},
    "random": {**{f"A_row{r}": _row("A", r) for r in range(37)}, **{f"B_row{r}": _row("B2", r) for r in range(37)}},
    "dense_row": {"B_row36": _row("B2", 36)},
}


def changed_flags(P, a_new, b_new):
    """(flags over A's nzval positions, flags over B2's): accepted by the update rules and different in their bits"""
    out = []
    for M, new in ((P.A, a_new), (P.B2, b_new)):
        old = _nz(M)
        if new is None:
            out.append(np.zeros(old.size, dtype=np.uint8)); continue
        new = np.ascontiguousarray(new, dtype=np.float64)
        accepted = np.isfinite(new) & ~((old == 0.0) & (new != 0.0))
        out.append((accepted & (new.view(np.uint64) != old.view(np.uint64))).astype(np.uint8))
    return out


def index_sets(slc, P, S, groups, base=0):
    """[(s_x, s_u)] per subproblem in col_status order (every column of a group has the group's sets): 0-based, ascending"""
    lib = slc.load_library(); cap = slc._capi
    i64p = C.POINTER(C.c_int64)
    keep = []

    def csc(M, cls, dt):
        M = sp.csc_matrix(M); M.sort_indices()
        cp = M.indptr.astype(np.int64) + base; rv = M.indices.astype(np.int64) + base
        nz = np.ascontiguousarray(M.data, dtype=dt)
        keep.extend([cp, rv, nz])
        return cls(M.shape[0], M.shape[1], cp.ctypes.data_as(i64p), rv.ctypes.data_as(i64p),
                   nz.ctypes.data_as(C.POINTER(C.c_double if dt == np.float64 else C.c_uint8)))
    Nx, Nu = P.Nx, P.Nu
    a = csc(P.A, cap.sls_csc_f64, np.float64); sx_ = csc(S[0][-1], cap.sls_csc_bool, np.uint8); su_ = csc(S[1][-1], cap.sls_csc_bool, np.uint8)
    dims = cap.sls_dims(Nx, Nu, Nx + Nu, Nx, 1, base, 0)
    sx = np.zeros(Nx, dtype=np.int64); su = np.zeros(max(Nu, 1), dtype=np.int64)
    nsx, nsu = C.c_int64(), C.c_int64()
    out = []
    for g in groups:
        cj = np.asarray(g, dtype=np.int64) + base
        rc = lib.sls_sparsity_dim_reduction(C.byref(dims), C.byref(a), C.byref(sx_), C.byref(su_), cj.ctypes.data_as(i64p), len(g),
                                            sx.ctypes.data_as(i64p), C.byref(nsx), su.ctypes.data_as(i64p), C.byref(nsu))
        assert rc == 0, rc
        out += [(np.sort(sx[:nsx.value] - base), np.sort(su[:nsu.value] - base))] * len(g)
    return out


def affected(P, sets, flags_a, flags_b):
    """The rule, in NumPy: uint8 per subproblem."""
    A, B = sp.csc_matrix(P.A), sp.csc_matrix(P.B2)
    A.sort_indices(); B.sort_indices()
    colA = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr)); colB = np.repeat(np.arange(B.shape[1]), np.diff(B.indptr))
    ka, kb = np.flatnonzero(flags_a), np.flatnonzero(flags_b)
    ai, aj = A.indices[ka], colA[ka]
    bi, bk = B.indices[kb], colB[kb]
    out = np.zeros(len(sets), dtype=np.uint8)
    for q, (sx, su) in enumerate(sets):
        hit = np.any(np.isin(ai, sx) & np.isin(aj, sx)) or np.any(np.isin(bi, sx) & np.isin(bk, su))
        out[q] = 1 if hit else 0
    return out


def reference(slc, plant, name, P=None, S=None, groups=None):
    """(A nzval or None, B2 nzval or None, expectation, affected marks) of a change set on (P, S, groups), by default the
    plant's `setting`; computed once per (plant, change set, columns), read-only."""
    if P is None:
        P, S, groups = setting(slc, plant)
    key = ("ref", plant, name, tuple(tuple(g) for g in groups), (len(S[0]), S[0][-1].nnz, S[1][-1].nnz))
    if key not in _cache:
        a, b, exp = CHANGES[plant][name](P)
        fa, fb = changed_flags(P, a, b)
        skey = ("sets", plant, key[3], key[4])
        if skey not in _cache:
            _cache[skey] = index_sets(slc, P, S, groups)
        marks = affected(P, _cache[skey], fa, fb)
        for v in (a, b, marks):
            if v is not None:
                v.setflags(write=False)
        _cache[key] = (a, b, exp, marks)
    return _cache[key]
