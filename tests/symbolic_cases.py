"""Plants for the device symbolic pass (csrc/sls_masks.hip, expand_tables_kernel, the retry loop of csrc/sls_symbolic_device.cpp) at its
bitmap, level-list and mask-word edges, and an independent reference for everything that pass produces.

The reference is NumPy/SciPy only and takes nothing from the library:
  levels      L_k(c) = column c of (A≠0)^k,  U_k(c) = column c of (B2ᵀ≠0)(A≠0)^k      (README.md:52-54, Boolean matrix powers)
  schedule    kx[t] = min(d, ⌊αt⌋),  ku[t] = min(d+1, ⌊αt⌋),  t = 0…T−1
  masks       𝓢x[t] = L_kx[t],  𝓢u[t] = U_ku[t]
  index sets  s_x(c), s_u(c) = ascending rows of (𝓢[T]·(A≠0))[:, c]                     (reference src/reduction.jl:14)
  tables      layout [column][t][s_x, s_u]: mask byte = membership of the row in the mask column; destination = value-array
              offset of time step t + the column's CSC position + rank inside the column, −1 where masked
(A≠0) and (B2≠0) are by value: stored zeros are not edges.  A plain module like tile_cases.py, not a conftest."""
import functools
import os
import re

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "systemlevelcontrol.jl_amd", "csrc")


# ------------------------------------------------------------------ the limits, read from the sources
@functools.lru_cache(maxsize=None)
def limits():
    """The constants the edges are measured against, read from the sources so that the case table cannot drift from them
    silently: LDS limit, the starting capacities of the three retry loops, bytes per list entry, the fixed LDS words of the
    tables kernel (named constants of csrc/sls_symbolic_device.h, which host and kernel share), the level limit, and the
    column round of level_prefix_kernel."""
    plan = open(os.path.join(CSRC, "sls_symbolic_device.h"), encoding="utf-8").read()
    rout = open(os.path.join(CSRC, "sls_routing.h"), encoding="utf-8").read()
    sym = open(os.path.join(CSRC, "sls_symbolic.cpp"), encoding="utf-8").read()
    msk = open(os.path.join(CSRC, "sls_masks.hip"), encoding="utf-8").read()
    m = re.search(r"constexpr int kMaxLds = (\d+) \* 1024;", rout)
    lim = {"max_lds": int(m.group(1)) * 1024}
    const = {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", plan)}
    lim["cap0_masks"], lim["cap0_index"], lim["cap0_tables"] = const["kMaskCap0"], const["kIndexCap0"], const["kTablesCap0"]
    lim["entry_masks"], lim["entry_index"], lim["entry_tables"] = const["kMaskEntryBytes"], const["kIndexEntryBytes"], const["kTablesEntryBytes"]
    lim["level_starts"] = const["kLevelStarts"]
    assert "int32_t* pu = px + kLevelStarts;" in msk
    m = re.search(r"if \(L\.kmax \+ 2 > (\d+)\)", sym)
    lim["max_levels"] = int(m.group(1))
    m = re.search(r"for \(int b = 0; b < Nx; b \+= (\d+)\)", msk)
    lim["prefix_round"] = int(m.group(1))
    assert f"__launch_bounds__({lim['prefix_round']}) void level_prefix_kernel" in msk
    lim["grid_per_cu"] = 8                                       # min(Nx, 8·CUs) workgroups; an MI355X has 256 CUs
    lim["max_grid"] = 8 * 256
    return lim


def bitmap_bytes(Nx, Nu):
    return ((Nx + 31) // 32 + (max(Nu, 1) + 31) // 32) * 4


def cap_limit_masks(Nx, Nu):
    L = limits()
    return min(max(Nx, Nu), (L["max_lds"] - bitmap_bytes(Nx, Nu)) // L["entry_masks"])


def cap_limit_index(Nx, Nu):
    L = limits()
    return min(max(Nx, Nu), (L["max_lds"] - bitmap_bytes(Nx, Nu)) // L["entry_index"])


def cap_limit_tables(Nx, Nu, T):
    L = limits()
    fixed = bitmap_bytes(Nx, Nu) + 2 * L["level_starts"] * 4 + 4 * T * 4
    return (L["max_lds"] - fixed) // L["entry_tables"]


# ------------------------------------------------------------------ the reference
def schedule(d, T, alpha):
    kx = [min(d, int(np.floor(alpha * t))) for t in range(T)]
    ku = [min(d + 1, int(np.floor(alpha * t))) for t in range(T)]
    return kx, ku


def _pattern(M):
    """(M ≠ 0) by value as an int32 CSC matrix with sorted indices"""
    M = sp.csc_matrix(M, dtype=np.float64).copy()
    M.eliminate_zeros()
    M.sort_indices()
    return sp.csc_matrix((np.ones(M.nnz, dtype=np.int32), M.indices, M.indptr), shape=M.shape)


def _binary(M):
    M = sp.csc_matrix(M)
    M.eliminate_zeros()
    M.sort_indices()
    return sp.csc_matrix((np.ones(M.nnz, dtype=np.int32), M.indices, M.indptr), shape=M.shape)


class Reference:
    """Everything the device pass produces for (A, B2, d, T, α), by Boolean matrix powers."""

    def __init__(self, A, B2, d, T, alpha):
        self.Nx, self.Nu, self.d, self.T, self.alpha = A.shape[0], B2.shape[1], d, T, alpha
        self.kx, self.ku = schedule(d, T, alpha)
        self.kmax = max(self.kx + self.ku)
        self.K1 = self.kmax + 1
        self.KL = max(self.kmax, self.kx[-1] + 1, self.ku[-1] + 1)
        self.Ab = _pattern(A)
        Bt = _pattern(sp.csc_matrix(B2).T)
        self.L = [sp.identity(self.Nx, dtype=np.int32, format="csc")]
        for _ in range(self.KL):
            self.L.append(_binary(self.L[-1] @ self.Ab))
        self.U = [_binary(Bt @ Lk) for Lk in self.L]
        self.Sx = [self.L[k] for k in self.kx]
        self.Su = [self.U[k] for k in self.ku]

    def masks(self):
        """2T CSC patterns (indptr, indices), 0-based"""
        return [(M.indptr, M.indices) for M in self.Sx], [(M.indptr, M.indices) for M in self.Su]

    def index_sets(self, Sx_last=None, Su_last=None):
        """s_x(c), s_u(c) of every column as two CSC patterns: rows of (𝓢[T]·(A≠0)).  Given masks count structurally (a stored
        false is still a stored entry of the product: findnz)."""
        out = []
        for M in (self.Sx[-1] if Sx_last is None else Sx_last, self.Su[-1] if Su_last is None else Su_last):
            M = sp.csc_matrix(M)
            M.sort_indices()
            patt = sp.csc_matrix((np.ones(M.nnz, dtype=np.int32), M.indices, M.indptr), shape=M.shape)
            Pm = (patt @ self.Ab).tocsc()
            Pm.sort_indices()                                   # products of non-negative integers: no cancellation
            assert Pm.nnz == 0 or Pm.data.min() > 0
            out.append(Pm)
        return out

    def tables(self):
        """mask bytes, destinations, index pool and n_values of the plan tables, layout [column][t][s_x, s_u]"""
        PX, PU = self.index_sets()
        T, Nx = self.T, self.Nx
        off_x = np.concatenate([[0], np.cumsum([M.nnz for M in self.Sx])])
        off_u = off_x[-1] + np.concatenate([[0], np.cumsum([M.nnz for M in self.Su])])
        masks, dests, idx = [], [], []
        for c in range(Nx):
            sx = PX.indices[PX.indptr[c]:PX.indptr[c + 1]]
            su = PU.indices[PU.indptr[c]:PU.indptr[c + 1]]
            idx += [sx, su]
            for t in range(T):
                for s, M, off in ((sx, self.Sx[t], off_x[t]), (su, self.Su[t], off_u[t])):
                    col = M.indices[M.indptr[c]:M.indptr[c + 1]]
                    pos = np.searchsorted(col, s)
                    on = (pos < col.size) & (col[np.minimum(pos, max(col.size - 1, 0))] == s) if col.size else np.zeros(s.size, bool)
                    masks.append(on.astype(np.uint8))
                    dests.append(np.where(on, off + M.indptr[c] + pos, -1).astype(np.int32))
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        return dict(mask=cat(masks, np.uint8), dest=cat(dests, np.int32), idx=cat(idx, np.int32), n_values=int(off_u[-1]),
                    nx=np.diff(PX.indptr), nu=np.diff(PU.indptr))

    def regular(self):
        """every row of every mask column lies inside the column's index set (else the compact tables cannot express it)"""
        PX, PU = self.index_sets()
        for Ms, Pm in ((self.Sx, PX), (self.Su, PU)):
            for M in Ms:
                if (M - M.multiply(_binary(Pm))).nnz:
                    return False
        return True

    # ---- the properties the cases exist for ----
    def largest_mask_level(self):
        """largest list the mask kernel builds: levels and actuator sets 0…kmax"""
        return max(int(np.diff(M.indptr).max()) for M in self.L[:self.K1] + self.U[:self.K1])

    def largest_index_set(self):
        return max(int(np.diff(M.indptr).max()) for M in self.index_sets())

    def largest_pool(self):
        """largest per-column sum of the level sizes 0…KL, states and actuators apart (two pools of one capacity)"""
        px = sum(np.diff(M.indptr) for M in self.L[:self.KL + 1])
        pu = sum(np.diff(M.indptr) for M in self.U[:self.KL + 1])
        return int(max(px.max(), pu.max()))

    def widest_word_span(self):
        """most 32-bit bitmap words between the lowest and the highest member of one expanded level (k ≥ 1) or actuator set"""
        best = 0
        for M in self.L[1:self.KL + 1] + self.U[:self.KL + 1]:
            for c in np.flatnonzero(np.diff(M.indptr)):
                col = M.indices[M.indptr[c]:M.indptr[c + 1]]
                best = max(best, int(col[-1] >> 5) - int(col[0] >> 5) + 1)
        return best


# ------------------------------------------------------------------ plants
def _csc(rows, cols, vals, shape):
    return sp.csc_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=shape)


def chain(Nx):
    i = np.arange(Nx)
    r = np.concatenate([i, i[:-1], i[1:]]); c = np.concatenate([i, i[1:], i[:-1]])
    v = np.concatenate([np.ones(Nx), 0.2 * np.ones(Nx - 1), -0.2 * np.ones(Nx - 1)])
    return _csc(r, c, v, (Nx, Nx))


def actuators(Nx, states):
    """B2 = I[:, states]"""
    states = list(states)
    return _csc(states, range(len(states)), np.ones(len(states)), (Nx, len(states)))


def hub(Nx, m, e=0):
    """unit diagonal; state 0 feeds states 1…m, leaf 1 feeds e further states; nothing feeds back"""
    r = list(range(Nx)) + list(range(1, m + 1)) + list(range(m + 1, m + 1 + e))
    c = list(range(Nx)) + [0] * m + [1] * e
    v = [1.0] * Nx + [0.3] * m + [-0.25] * e
    return _csc(r, c, v, (Nx, Nx))


def far_chain(Nx=4200):
    A = chain(Nx).tolil()
    for src, dst in ((5, 2100), (5, 4190), (2060, 3), (4199, 0)):
        A[dst, src] = 0.15
    return A.tocsc()


def banded(Nx, hw):
    r, c, v = [], [], []
    for j in range(Nx):
        for i in range(max(0, j - hw), min(Nx, j + hw + 1)):
            r.append(i); c.append(j)
            v.append(1.0 if i == j else 0.04 * (1 + ((3 * i + 5 * j) % 7)) * (1 if i < j else -1))
    return _csc(r, c, v, (Nx, Nx))


def holes_plant():
    """stored value-zeros in A and B2; column 7 of A holds only stored zeros (its diagonal among them): its level 1 is empty;
    states 3, 4, 10 drive no actuator (row 4 of B2 holds a stored zero only)"""
    Nx = 14
    A = chain(Nx).tolil()
    A[0, 2] = 0.5; A[9, 12] = 0.5
    A = A.tocsc(); A.sort_indices()
    for c, kill in ((7, None), (2, 1), (11, 12)):
        lo, hi = A.indptr[c], A.indptr[c + 1]
        for e in range(lo, hi):
            if kill is None or A.indices[e] == kill:
                A.data[e] = 0.0
    B2 = sp.lil_matrix((Nx, 5))
    for j, rows in enumerate(((0, 1), (2,), (5, 6, 7), (8, 9), (11, 12, 13))):
        for r in rows:
            B2[r, j] = 1.0
    B2[4, 1] = 1.0
    B2 = B2.tocsc(); B2.sort_indices()
    B2.data[(B2.indices == 4).nonzero()[0]] = 0.0
    return A, B2


def _case(name, A, B2, d, T, alpha, edge, routes=("masks", "index", "tables", "host_tables"), **kw):
    return dict(name=name, make=(lambda: (A() if callable(A) else A, B2() if callable(B2) else B2)), d=d, T=T, alpha=alpha,
                edge=edge, routes=tuple(routes), **kw)


def _eye(n):
    return lambda: sp.identity(n, format="csc")


# the tables-pool pair: a hub under a deep schedule (KL = 61: 62 levels in the pool) on 335 states;
# pool = 1 + (1 + m) + 60·(1 + m + e) — 20395 entries is exactly what 160 KiB hold next to the fixed words, 20396 one too many
_POOL_SCHED = dict(d=59, T=3, alpha=30.0)

CASES = [
    _case("hub1024", lambda: hub(1100, 1023), _eye(1100), 1, 3, 1.5,
          "largest level = 1024 = the first capacity of the mask and index-set lists (no retry); hub pool 3073 > 2048: one retry of the tables kernel"),
    _case("hub1025", lambda: hub(1100, 1024), _eye(1100), 1, 3, 1.5,
          "largest level = 1025: total > cap, one retry in mask_levels and index_sets; pool 3076"),
    _case("pool2048", lambda: hub(700, 680, 2), _eye(700), 1, 3, 1.5, "hub pool = 2048 exactly: the tables kernel's first capacity holds it"),
    _case("pool2049", lambda: hub(700, 681, 1), _eye(700), 1, 3, 1.5, "hub pool = 2049: one entry over, one retry"),
    _case("hub_wideB", lambda: hub(40, 39), lambda: sp.csc_matrix(np.ones((40, 1300))), 1, 3, 1.5,
          "Nu = 1300 > Nx = 40: the actuator list sets cap_limit = max(Nx, Nu); the actuator level is 1300 > 1024"),
    _case("far4200", far_chain, lambda: actuators(4200, range(0, 4200, 3)), 2, 4, 1.5,
          "a level spans > 128 bitmap words: three rounds of bitmap_to_list; Nx > 2048 workgroups: second and third column per "
          "wave; level_prefix_kernel: five rounds with a ragged tail"),
    _case("deep", lambda: chain(70), _eye(70), 59, 24, 3.0, "kmax + 2 = 62 accepted: K1 = 61 levels, 61 bits of lv in use; pool 3115 > 2048"),
    _case("deep60", lambda: chain(70), _eye(70), 60, 24, 3.0, "kmax + 2 = 63: refused by the localized route, still computed by the mask route",
          routes=("masks", "index"), refuse=("tables",)),
    _case("dense40", lambda: sp.csc_matrix(np.ones((40, 40))), lambda: actuators(40, range(0, 40, 2)), 2, 3, 1.5,
          "every level has exactly cap = cap_limit = Nx entries"),
    _case("holes", lambda: holes_plant()[0], lambda: holes_plant()[1], 2, 4, 1.5,
          "stored value-zeros; an empty level 1 (ncur = 0, xmax = −1); state rows without an actuator (umax = −1)",
          routes=("masks", "index"), refuse=("tables",)),
    _case("fits_mask", lambda: hub(13000, 12999), _eye(13000), 1, 3, 1.5,
          "mask lists of cap_limit = Nx = 13000 entries: an LDS request of ≈159 KiB", routes=("masks", "index")),
    _case("too_big_mask", lambda: hub(14000, 13999), _eye(14000), 1, 3, 1.5,
          "a level of 14000 > cap_limit ≈ 13.36 k: SLS_EUNSUPPORTED, not a truncated mask", routes=("index",), refuse=("masks",)),
    _case("fits_pool", lambda: hub(335, 293, 41), _eye(335), routes=("masks", "index", "tables"), **_POOL_SCHED,
          edge="tables pool = cap_limit exactly: the whole 160 KiB of LDS requested"),
    _case("too_big_pool", lambda: hub(335, 294, 40), _eye(335), routes=("masks", "index"), refuse=("tables",), **_POOL_SCHED,
          edge="tables pool = cap_limit + 1: SLS_EUNSUPPORTED"),
]
for _n in (1023, 1025, 2049):
    CASES.append(_case(f"prefix{_n}", functools.partial(chain, _n), functools.partial(lambda n: actuators(n, range(0, n, 2)), _n), 1, 3, 1.5,
                       f"level_prefix_kernel: Nx = {_n} against its 1024-column rounds"))
for _n, _act in ((1, ()), (1, (0,)), (31, (30,)), (32, range(32)), (33, range(33)), (33, ()), (63, (0, 62)), (64, range(31, 64)),
                 (64, ()), (65, list(range(0, 62, 2)) + [64])):
    _act = list(_act)
    CASES.append(_case(f"words{_n}_u{len(_act)}", functools.partial(chain, _n), functools.partial(actuators, _n, _act), 2, 4, 1.5,
                       f"bitmap word boundary Nx = {_n}, Nu = {len(_act)}" + (", an actuator on the last state" if _act and _act[-1] == _n - 1 else "")))
for _a, _d, _T in ((0.0, 3, 5), (0.5, 2, 9), (1.0, 0, 4), (1.5, 3, 1), (0.05, 4, 130)):
    CASES.append(_case(f"sched_a{_a}_d{_d}_T{_T}", lambda: chain(23), lambda: actuators(23, (0, 1, 6, 7, 12, 13, 18, 19, 22)), _d, _T, _a,
                       "level schedule: " + ("levels repeat; " if _a < 1 else "") + ("T = 1; " if _T == 1 else "") + ("T > 64; " if _T > 64 else "") + ("d = 0" if _d == 0 else "")))

BAND_NX, BAND_HW, BAND_D, BAND_T = 200, 8, 3, 4
BAND_SPARSE_ACT = tuple(range(1, 100, 2)) + tuple(range(100, 200))       # every odd state of the left half, every state of the right
CASES.append(_case("band65", lambda: banded(BAND_NX, BAND_HW), _eye(BAND_NX), BAND_D, BAND_T, 1.5,
                   "interior ñx = 65, edge columns through 63 and 64 (ñx = 64 with ñu > 0: xbits = ~0); ñx + ñu = 128 among the sums"))
CASES.append(_case("band65_sparse", lambda: banded(BAND_NX, BAND_HW), lambda: actuators(BAND_NX, BAND_SPARSE_ACT), BAND_D, BAND_T, 1.5,
                   "a sparser B2: ñx + ñu on 64, 65, 128 and 129"))

BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
assert len(BY_NAME) == len(CASES)


def names(route):
    return [c["name"] for c in CASES if route in c["routes"]]


def refused(route):
    return [c["name"] for c in CASES if route in c.get("refuse", ())]


@functools.lru_cache(maxsize=None)
def plant(name):
    A, B2 = BY_NAME[name]["make"]()
    A = sp.csc_matrix(A, dtype=np.float64); B2 = sp.csc_matrix(B2, dtype=np.float64)
    A.sort_indices(); B2.sort_indices()
    return A, B2


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per case and shared; callers must not modify it"""
    c = BY_NAME[name]
    A, B2 = plant(name)
    return Reference(A, B2, c["d"], c["T"], c["alpha"])


@functools.lru_cache(maxsize=None)
def reference_tables(name):
    return reference(name).tables()


def holes_last_masks():
    """the `holes` case's last masks with stored-false entries (every third entry of 𝓢x[T], every fourth of 𝓢u[T]): they count
    structurally in the index sets"""
    ref = reference("holes")
    Sx = sp.csc_matrix(ref.Sx[-1], dtype=np.uint8).copy(); Su = sp.csc_matrix(ref.Su[-1], dtype=np.uint8).copy()
    Sx.data[::3] = 0; Su.data[::4] = 0
    return Sx, Su


# ------------------------------------------------------------------ the library's host pass, for comparison
def sample_columns(name):
    """every column of a small case; of a large one the first and last columns, the hubs and a fixed spread"""
    Nx = plant(name)[0].shape[0]
    if Nx <= 256:
        return list(range(Nx))
    return sorted(set([0, 1, 2, 3, 5, Nx // 2, Nx - 2, Nx - 1] + list(range(7, Nx, max(1, Nx // 40)))) & set(range(Nx)))


def host_reduction(slc, A, Sx_last, Su_last, cols, base):
    """sls_sparsity_dim_reduction (host) for single columns: ascending 0-based (s_x, s_u) per column"""
    import ctypes as C
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
    Nx, Nu = A.shape[0], Su_last.shape[0]
    a = csc(A, cap.sls_csc_f64, np.float64); sx_ = csc(Sx_last, cap.sls_csc_bool, np.uint8); su_ = csc(Su_last, cap.sls_csc_bool, np.uint8)
    dims = cap.sls_dims(Nx, Nu, Nx + Nu, Nx, 1, base, 0)
    sx = np.zeros(Nx, dtype=np.int64); su = np.zeros(max(Nu, 1), dtype=np.int64)
    nsx, nsu = C.c_int64(), C.c_int64()
    out = []
    for c in cols:
        cj = np.array([c + base], dtype=np.int64)
        rc = lib.sls_sparsity_dim_reduction(C.byref(dims), C.byref(a), C.byref(sx_), C.byref(su_), cj.ctypes.data_as(i64p), 1,
                                            sx.ctypes.data_as(i64p), C.byref(nsx), su.ctypes.data_as(i64p), C.byref(nsu))
        assert rc == 0, rc
        out.append((np.sort(sx[:nsx.value] - base), np.sort(su[:nsu.value] - base)))
    return out
