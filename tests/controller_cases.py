"""Operators, input sequences and the reference shared by tests/test_controller_host.py and tests/test_gpu_controller.py (a plain
module like closed_loop_cases.py; not a conftest, and free of HIP: nothing here loads the library).

The operation under test is the stand-alone controller step of csrc/sls_controller.h,

    ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
    u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
    β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}

The operators are those of closed_loop_cases.py — the row-length ladder (Nx 24, Nu 6, T 24: ring of 32 slots) and the small cases
T1, T2, Nu0 — plus two ring cases on Nx = 9, Nu = 3: T = 4, where the ring of 4 slots is exactly full and the slot a step
overwrites is the one just beyond the oldest it reads, and T = 5, where the ring (8 slots) is larger than T.  `values` arrays
stay NaN-poisoned where the operator must not read (all of Sx[0], every stored-false entry).

Tolerance of every comparison with the reference: the project's RTOL = 1e-11 relative to max(1, max|ref|), per scenario, as in
test_gpu_closed_loop_edges.py; a float64 evaluation of these sums in another order differs from long double by a few 1e-16.
Growth is a condition, not a tolerance: test_controller_host.py asserts max|ŵ| ≤ GROWTH_BOUND for every input sequence used."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import closed_loop_cases as clc

RTOL = 1e-11
GROWTH_BOUND = 10.0
RING = ("T4", "T5")
RING_NX, RING_NU = 9, 3
L = np.longdouble


def ring_case(name):
    """random masks and values on Nx = 9, Nu = 3 with T = 4 (ring exactly full) or T = 5 (ring of 8 > T); one stored-false entry"""
    Nx, Nu = RING_NX, RING_NU
    T = {"T4": 4, "T5": 5}[name]
    rng = np.random.default_rng(RING.index(name) + 400)
    Sx = [sp.identity(Nx, dtype=bool, format="csc")] + [clc._csc_mask(rng.random((Nx, Nx)) < 0.5) for _ in range(T - 1)]
    Su = [clc._csc_mask(rng.random((Nu, Nx)) < 0.6) for _ in range(T)]
    free = np.argwhere(~Sx[T - 1].toarray())[0]
    Sx[T - 1] = clc._store_false(Sx[T - 1], int(free[0]), int(free[1]))       # in the OLDEST lag: the far end of the window
    A = sp.random(Nx, Nx, 0.3, random_state=np.random.default_rng(6), format="csc") * 0.3
    B2 = sp.lil_matrix((Nx, Nu))
    for j in range(Nu):
        B2[3 * j + 1, j] = 1.0 - 0.3 * j
    vals_x, vals_u = clc._values(rng, Sx, Su)
    return clc._finish(A, sp.identity(Nx, format="csc"), B2.tocsc(), Sx, Su, vals_x, vals_u, 40)


def case(name):
    if name == "ladder":
        return clc.ladder()
    return clc.small_case(name) if name in clc.SMALL else ring_case(name)


ALL = ("ladder",) + clc.SMALL + RING
HOST_STEPS = {"ladder": 100, "T1": 40, "T2": 40, "Nu0": 40, "T4": 40, "T5": 40}     # ladder: the ring of 32 wraps three times
LOOP_STEPS = {"ladder": 60, "T1": 40, "T2": 40}


def ring_slots(T):
    R = 1
    while R < T:
        R <<= 1
    return R


def random_x(name, steps, nscen, seed=0):
    """x ~ N(0,1), [steps, Nx, nscen]: comes from no plant"""
    Nx = clc.LADDER_NX if name == "ladder" else clc.SMALL_NX
    return np.random.default_rng(5000 + 31 * ALL.index(name) + seed).standard_normal((steps, Nx, nscen))


def from_values(Sx, Su, values, **extra):
    """A case record (Nx, Nu, T, dense Phix / Phiu) from masks and a mask-order value array — a solved Φ downloaded from the device"""
    Sx, Su = [sp.csc_matrix(m) for m in Sx], [sp.csc_matrix(m) for m in Su]
    T, Nx, Nu = len(Sx), Sx[0].shape[0], Su[0].shape[0]
    Phix, Phiu = np.zeros((T, Nx, Nx)), np.zeros((T, Nu, Nx))
    o = 0
    for D, masks in ((Phix, Sx), (Phiu, Su)):
        for t, M in enumerate(masks):
            M.sort_indices()
            keep = np.asarray(M.data, dtype=bool)
            cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
            v = np.asarray(values[o:o + M.nnz]); o += M.nnz
            D[t, M.indices[keep], cols[keep]] = v[keep]
    assert o == len(values)
    return SimpleNamespace(Sx=Sx, Su=Su, Nx=Nx, Nu=Nu, T=T, Phix=Phix, Phiu=Phiu, values=np.asarray(values), **extra)


class Reference:
    """The three lines above with dense Φ in np.longdouble, all scenarios at once, one step at a time: `step(x)` returns
    (u_k, ŵ_k).  `scale` multiplies Φ and may be changed between steps (the history stays): a load of scaled Φ without reset."""

    def __init__(self, case, scale=1.0):
        self.T, self.Nx, self.Nu = case.T, case.Nx, case.Nu
        self.Phix, self.Phiu = np.asarray(case.Phix, dtype=L), np.asarray(case.Phiu, dtype=L)
        self.scale = scale
        self.reset()

    def reset(self):
        self.hist, self.beta, self.k = [], None, 0

    def step(self, x):
        x = np.asarray(x, dtype=L)
        if self.beta is None:
            self.beta = np.zeros_like(x)
        w = x - self.beta
        self.hist.append(w)
        s = L(self.scale)
        b = np.zeros_like(x)
        for tau in range(1, min(len(self.hist), self.T - 1) + 1):          # Φx[τ+1] 1-based = slice τ
            b += (self.Phix[tau] * s) @ self.hist[-tau]
        u = np.zeros((self.Nu, x.shape[1]), dtype=L)
        for tau in range(1, min(len(self.hist), self.T) + 1):
            u += (self.Phiu[tau - 1] * s) @ self.hist[-tau]
        self.beta = b
        self.hist = self.hist[-self.T:]
        self.k += 1
        return u, w


def reference(case, x, scale=1.0, switch=None):
    """u [steps, Nu, nscen], ŵ [steps, Nx, nscen] (longdouble) for the sequence x [steps, Nx, nscen].  switch = (k, scale'):
    Φ is multiplied by scale' from step k on, history kept."""
    ref = Reference(case, scale)
    us, ws = [], []
    for k in range(x.shape[0]):
        if switch is not None and k == switch[0]:
            ref.scale = switch[1]
        u, w = ref.step(x[k])
        us.append(u); ws.append(w)
    return np.array(us, dtype=L).reshape(x.shape[0], case.Nu, x.shape[2]), np.array(ws, dtype=L)


# ------------------------------------------------------------------ a plant the simulator cannot hold

def plant_step(A, B2, x, u, w):
    """x⁺ = A·x + 0.25·tanh(x) + w + B₂·u in the dtype of the dense arrays given (float64 on the host side of the GPU test,
    longdouble in the reference loop)"""
    return A @ x + x.dtype.type(0.25) * np.tanh(x) + w + B2 @ u


def loop_inputs(name, steps, nscen=3, Nx=None):
    """(x_0 [Nx, nscen], w [steps, Nx, nscen]) of the interleaved loop: x_0 random — an initial condition is a disturbance at
    time 0 — and a small random disturbance on every step"""
    if Nx is None:
        Nx = clc.LADDER_NX if name == "ladder" else clc.SMALL_NX
    rng = np.random.default_rng(900 + sum(map(ord, name)))
    return rng.standard_normal((Nx, nscen)), 0.3 * rng.standard_normal((steps, Nx, nscen))


def dense_plant(case, dtype, A=None):
    A = case.A if A is None else A
    return np.asarray(sp.csc_matrix(A).toarray(), dtype=dtype), np.asarray(sp.csc_matrix(case.B2).toarray(), dtype=dtype)


def reference_loop(case, x0, w, A=None, scale=1.0):
    """The closed loop of `Reference` with plant_step in longdouble: x [steps, Nx, nscen], u [steps, Nu, nscen], ŵ likewise"""
    Ad, Bd = dense_plant(case, L, A)
    ref = Reference(case, scale)
    x = np.asarray(x0, dtype=L)
    xs, us, ws = [], [], []
    for k in range(w.shape[0]):
        u, what = ref.step(x)
        xs.append(x); us.append(u); ws.append(what)
        x = plant_step(Ad, Bd, x, u, np.asarray(w[k], dtype=L))
    return np.array(xs, dtype=L), np.array(us, dtype=L).reshape(w.shape[0], case.Nu, w.shape[2]), np.array(ws, dtype=L)


def check(got, ref, what):
    """every scenario against its own magnitude; returns the largest relative error"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    worst = 0.0
    for s in range(ref.shape[-1]):
        e = clc.rel_err(got[..., s], ref[..., s])
        worst = max(worst, e)
        assert e < RTOL, (what, s, e)
    return worst
