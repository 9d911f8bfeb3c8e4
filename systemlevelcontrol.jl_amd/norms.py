"""Closed-loop 𝓛₁ and 𝓗∞ norms of the Φ that lives on the device.

Rows are the Nx state rows followed by the Nu input rows, N = Nx + Nu; for t = 0 … T−1

    G[t] = diag(cz) · [Φx[t]; Φu[t]] · diag(b)        N × Nx, real          G(ω) = Σ_t G[t] · e^{−iωt}

`l1()` gives the row and column absolute sums of G and their maxima — the 𝓛₁ norm (induced ℓ∞ → ℓ∞) and the 𝓔₁ norm; `hinf()`
gives, per frequency of the caller's grid, a power-iteration lower bound of σ_max(G(ω)) and the peak over the grid.  The peak is
a lower bound of the 𝓗∞ norm ON THAT GRID: refining the grid is the caller's business.  `h2()` splits the squared 𝓗₂ norm by
output row — the variance of every state and actuator under unit white w — and by disturbance column; `covariance()` gives
chosen entries of Σ = Σ_t G[t]·G[t]ᵀ, the steady-state covariance of z (exact for the FIR loop).  The passes run in libsls_mi355x.so
(sls_norms_*: HIP kernels); this module only marshals.  No CPU fallback: `norms_host` / `norms_tables` are the diagnostic host
twin the tests compare against, not a second backend.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _capi
from ._capi import _dev_ptr, _is_tensor
from .controller import _dims_of

_DP = C.POINTER(C.c_double)


def _vec(a, n, what):
    """a host weight vector as (float64 array or None, ctypes pointer or None)"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n,):
        raise ValueError(f"{what} must have {n} entries, got shape {a.shape}")
    return a, a.ctypes.data_as(_DP)


def _diagonal(M, what):
    """the diagonal of a square matrix that stores nothing else; ValueError otherwise"""
    M = sp.coo_matrix(M)
    off = (M.row != M.col) & (M.data != 0)
    if M.shape[0] != M.shape[1] or off.any():
        raise ValueError(f"{what} is not diagonal: the closed-loop norms fold diagonal weights into the entries of Φ; a general "
                         "weight needs a sparse triple product, which is out of scope")
    d = np.zeros(M.shape[0])
    np.add.at(d, M.row, M.data)
    return d


def plant_weights(P):
    """(cz [Nx+Nu], b [Nx]) of a Plant whose [C1 D12] and B1 are diagonal and whose D11 is zero: the class the fast kernels
    serve (`Plant(A, B1, B2)` and every diagonally weighted LQR).  ValueError otherwise."""
    if P.D11.nnz and np.any(P.D11.data):
        raise ValueError("D11 ≠ 0: the closed-loop norms cover G = [C1 D12]·Φ·B1 only; a feedthrough term is out of scope")
    cz = _diagonal(sp.hstack([sp.csc_matrix(P.C1), sp.csc_matrix(P.D12)]), "[C1 D12]")
    if cz.shape[0] != P.Nx + P.Nu:
        raise ValueError(f"[C1 D12] is not diagonal: it must be {P.Nx + P.Nu} × {P.Nx + P.Nu}")
    return cz, _diagonal(P.B1, "B1")


def covariance_pattern_of(P, index_base=0):
    """(pairs_i, pairs_j), int64: the "neighbour" pattern of a plant — the upper triangle (i ≤ j) of (A ≠ 0) ∪ I on the state
    rows, an entry of A below the diagonal counted at its mirror place, plus the diagonal of the input rows Nx … Nx+Nu−1.
    Sorted by (i, j), no duplicates."""
    A = sp.coo_matrix(P.A)
    nz = A.data != 0
    i, j = np.minimum(A.row[nz], A.col[nz]).astype(np.int64), np.maximum(A.row[nz], A.col[nz]).astype(np.int64)
    d = np.arange(P.Nx + P.Nu, dtype=np.int64)
    flat = np.unique(np.concatenate([i * (P.Nx + P.Nu) + j, d * (P.Nx + P.Nu) + d]))
    return flat // (P.Nx + P.Nu) + index_base, flat % (P.Nx + P.Nu) + index_base


class ClosedLoopNorms:
    """Row- and column-ordered tables of G built from the masks alone (sls_norms_plan) on one device of `ctx`, with the work
    vectors of `max_freq` frequencies.  P_or_dims: a Plant (only Nx, Nu are read) or (Nx, Nu); cz [Nx+Nu], b [Nx]: host weight
    vectors, None = ones.  `from_plant` takes them from a plant's diagonals.  ctx: a Context, None = the default context."""

    def __init__(self, P_or_dims, S, cz=None, b=None, max_freq=64, ctx=None, dev_slot=0, index_base=0):
        Sx, Su = S
        if ctx is None:
            from .synthesis import default_context
            ctx = default_context()
        self.ctx, self._lib = ctx, ctx._lib
        self.Nx, self.Nu = _dims_of(P_or_dims)
        self.N, self.T = self.Nx + self.Nu, len(Sx)
        self.device = ctx.devices[dev_slot] if 0 <= dev_slot < len(ctx.devices) else None
        self.m = _capi.Marshalled.masks_only(self.Nx, self.Nu, Sx, Su, index_base)
        _, pcz = _vec(cz, self.N, "cz")
        _, pb = _vec(b, self.Nx, "b")
        h = C.c_void_p()
        _capi.check(self._lib.sls_norms_plan(ctx.handle, dev_slot, C.byref(self.m.dims), self.m.Sx, self.m.Su, pcz, pb, int(max_freq),
                                             C.byref(h)), ctx.handle)
        self.handle = h
        self.index_base, self.npairs = int(index_base), 0

    covariance_pattern_of = staticmethod(covariance_pattern_of)

    @classmethod
    def from_plant(cls, P, Sx, Su, **kw):
        """G = [C1 D12]·Φ·B1, the closed-loop map w → z of P.  Raises ValueError for non-diagonal weights or D11 ≠ 0."""
        cz, b = plant_weights(P)
        return cls(P, [Sx, Su], cz=cz, b=b, **kw)

    @property
    def info(self):
        """{"n_entries": stored-true entries (a pass reads 12 B each), "device_bytes", "max_freq"}"""
        n, by, mf = C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(self._lib.sls_norms_info(self.handle, C.byref(n), C.byref(by), C.byref(mf)))
        return {"n_entries": n.value, "device_bytes": by.value, "max_freq": mf.value}

    def load(self, d_values, stream=None):
        """Φ from the mask-order device array `Plan.execute(packed=False)` fills (tensor or pointer).  Returns self."""
        if _is_tensor(d_values):
            d_values = d_values.data_ptr()
        _capi.check(self._lib.sls_norms_load(self.handle, stream, d_values), self.ctx.handle)
        return self

    def l1(self, stream=None):
        """(row_l1 [N], col_l1 [Nx], totals [2]) on the host: totals[0] is the 𝓛₁ norm, totals[1] the 𝓔₁ norm.  Waits."""
        row, col, tot = np.zeros(self.N), np.zeros(self.Nx), np.zeros(2)
        _capi.check(self._lib.sls_norms_fetch_l1(self.handle, stream, row.ctypes.data_as(_DP), col.ctypes.data_as(_DP),
                                                 tot.ctypes.data_as(_DP)), self.ctx.handle)
        return row, col, tot

    def l1_async(self, row_l1=None, col_l1=None, totals=None, stream=None):
        """the same pass into device tensors / pointers (each may be None); nothing waits"""
        _capi.check(self._lib.sls_norms_l1(self.handle, stream, _dev_ptr(row_l1, self.N, "row_l1"), _dev_ptr(col_l1, self.Nx, "col_l1"),
                                           _dev_ptr(totals, 2, "totals")), self.ctx.handle)

    def hinf(self, omega, iters=32, stream=None):
        """(sigma [nfreq], peak, argpeak) on the host for the angles `omega` (radians per sample): sigma[f] is a lower bound of
        σ_max(G(ω_f)) after `iters` power iterations, peak = max sigma — a lower bound of the 𝓗∞ norm on this grid only — and
        argpeak the index of the first frequency that attains it.  Waits."""
        om = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        sigma, peak = np.zeros(max(om.size, 1)), np.zeros(2)
        _capi.check(self._lib.sls_norms_fetch_hinf(self.handle, stream, om.ctypes.data_as(_DP), om.size, int(iters),
                                                   sigma.ctypes.data_as(_DP), peak.ctypes.data_as(_DP)), self.ctx.handle)
        return sigma[: om.size], float(peak[0]), int(peak[1])

    def hinf_async(self, omega, iters=32, sigma=None, peak=None, stream=None):
        """the same pass into device tensors / pointers sigma [nfreq], peak [2] (each may be None); only the twiddle upload is
        waited for, by the next call that needs the pinned buffer"""
        om = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        _capi.check(self._lib.sls_norms_hinf(self.handle, stream, om.ctypes.data_as(_DP), om.size, int(iters),
                                             _dev_ptr(sigma, om.size, "sigma"), _dev_ptr(peak, 2, "peak")), self.ctx.handle)

    def h2(self, stream=None):
        """(row_h2 [N], col_h2 [Nx], totals [2]) on the host: row_h2[i] = Σ_t Σ_j G[t][i,j]², the variance of z_i under unit white
        w (its square root is the RMS of that state or actuator); col_h2[j] the share of disturbance j; totals[0] = Σ row_h2,
        the squared 𝓗₂ norm, totals[1] = max row_h2.  Waits."""
        row, col, tot = np.zeros(self.N), np.zeros(self.Nx), np.zeros(2)
        _capi.check(self._lib.sls_norms_fetch_h2(self.handle, stream, row.ctypes.data_as(_DP), col.ctypes.data_as(_DP),
                                                 tot.ctypes.data_as(_DP)), self.ctx.handle)
        return row, col, tot

    def h2_async(self, row_h2=None, col_h2=None, totals=None, stream=None):
        """the same pass into device tensors / pointers (each may be None); nothing waits"""
        _capi.check(self._lib.sls_norms_h2(self.handle, stream, _dev_ptr(row_h2, self.N, "row_h2"), _dev_ptr(col_h2, self.Nx, "col_h2"),
                                           _dev_ptr(totals, 2, "totals")), self.ctx.handle)

    def set_covariance_pattern(self, pairs_i, pairs_j):
        """The entries (pairs_i[p], pairs_j[p]) of Σ = Σ_t G[t]·G[t]ᵀ that `covariance` evaluates, in the index base of the
        object: any order, duplicates and i == j allowed.  Uploads the list and allocates it and a result buffer; a second call
        replaces the first, empty lists clear the pattern.  Waits.  Returns self."""
        pi, pj = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int64) for a in (pairs_i, pairs_j))
        if pi.ndim != 1 or pi.shape != pj.shape:
            raise ValueError(f"pairs_i and pairs_j must be two lists of one length, got shapes {pi.shape} and {pj.shape}")
        ip = C.POINTER(C.c_int64)
        _capi.check(self._lib.sls_norms_cov_pattern(self.handle, pi.size, pi.ctypes.data_as(ip), pj.ctypes.data_as(ip)), self.ctx.handle)
        self.npairs = int(pi.size)
        return self

    def covariance(self, stream=None):
        """cov [npairs] on the host: cov[p] = Σ_t Σ_k G[t][i_p,k]·G[t][j_p,k] for the pairs of `set_covariance_pattern`.  Waits."""
        cov = np.zeros(max(self.npairs, 1))
        _capi.check(self._lib.sls_norms_fetch_cov(self.handle, stream, cov.ctypes.data_as(_DP)), self.ctx.handle)
        return cov[: self.npairs]

    def covariance_async(self, out, stream=None):
        """the same pass into a device tensor / pointer of npairs doubles; nothing waits"""
        _capi.check(self._lib.sls_norms_cov(self.handle, stream, _dev_ptr(out, self.npairs, "out")), self.ctx.handle)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.sls_norms_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def norms_tables(P_or_dims, S, index_base=0):
    """sls_debug_norms_tables (needs no device): (row_ptr [N+1], row_key, row_perm, col_ptr [Nx+1], col_key, col_perm) — rows
    ascending in key = t·Nx + col, columns ascending in key = t·N + row, perm into the mask-order array."""
    Nx, Nu = _dims_of(P_or_dims)
    m = _capi.Marshalled.masks_only(Nx, Nu, S[0], S[1], index_base)
    lib = _capi.load_library()
    n = C.c_int64()
    _capi.check(lib.sls_debug_norms_tables(C.byref(m.dims), m.Sx, m.Su, C.byref(n), None, None, None, None, None, None))
    row_ptr, col_ptr = np.zeros(Nx + Nu + 1, dtype=np.int32), np.zeros(Nx + 1, dtype=np.int32)
    rk, rp, ck, cp = (np.zeros(max(n.value, 1), dtype=np.int32) for _ in range(4))
    ip = C.POINTER(C.c_int32)
    _capi.check(lib.sls_debug_norms_tables(C.byref(m.dims), m.Sx, m.Su, C.byref(n), row_ptr.ctypes.data_as(ip), rk.ctypes.data_as(ip),
                                           rp.ctypes.data_as(ip), col_ptr.ctypes.data_as(ip), ck.ctypes.data_as(ip), cp.ctypes.data_as(ip)))
    k = n.value
    return row_ptr, rk[:k], rp[:k], col_ptr, ck[:k], cp[:k]


def norms_host(P_or_dims, S, values, cz=None, b=None, omega=None, iters=32, index_base=0):
    """sls_debug_norms_host (needs no device): the host twin.  values: Φ in mask order (host).  Returns a dict with row_l1,
    col_l1, totals and — when `omega` is given — sigma, peak, argpeak."""
    Nx, Nu = _dims_of(P_or_dims)
    m = _capi.Marshalled.masks_only(Nx, Nu, S[0], S[1], index_base)
    values = np.ascontiguousarray(values, dtype=np.float64)
    _, pcz = _vec(cz, Nx + Nu, "cz")
    _, pb = _vec(b, Nx, "b")
    row, col, tot = np.zeros(Nx + Nu), np.zeros(Nx), np.zeros(2)
    om = None if omega is None else np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
    nf = 0 if om is None else om.size
    sigma, peak = np.zeros(max(nf, 1)), np.zeros(2)
    _capi.check(_capi.load_library().sls_debug_norms_host(
        C.byref(m.dims), m.Sx, m.Su, values.ctypes.data_as(_DP), pcz, pb, om.ctypes.data_as(_DP) if nf else None, nf, int(iters),
        row.ctypes.data_as(_DP), col.ctypes.data_as(_DP), tot.ctypes.data_as(_DP), sigma.ctypes.data_as(_DP) if nf else None,
        peak.ctypes.data_as(_DP) if nf else None))
    out = {"row_l1": row, "col_l1": col, "totals": tot}
    if nf:
        out.update(sigma=sigma[:nf], peak=float(peak[0]), argpeak=int(peak[1]))
    return out


def norms_h2_host(P_or_dims, S, values, cz=None, b=None, index_base=0):
    """sls_debug_norms_h2_host (needs no device): the host twin of `h2`.  Returns (row_h2 [N], col_h2 [Nx], totals [2])."""
    Nx, Nu = _dims_of(P_or_dims)
    m = _capi.Marshalled.masks_only(Nx, Nu, S[0], S[1], index_base)
    values = np.ascontiguousarray(values, dtype=np.float64)
    _, pcz = _vec(cz, Nx + Nu, "cz")
    _, pb = _vec(b, Nx, "b")
    row, col, tot = np.zeros(Nx + Nu), np.zeros(Nx), np.zeros(2)
    _capi.check(_capi.load_library().sls_debug_norms_h2_host(C.byref(m.dims), m.Sx, m.Su, values.ctypes.data_as(_DP), pcz, pb,
                                                             row.ctypes.data_as(_DP), col.ctypes.data_as(_DP), tot.ctypes.data_as(_DP)))
    return row, col, tot


def norms_cov_host(P_or_dims, S, values, pairs_i, pairs_j, cz=None, b=None, index_base=0):
    """sls_debug_norms_cov_host (needs no device): the host twin of `set_covariance_pattern` + `covariance`.  Returns cov [npairs]."""
    Nx, Nu = _dims_of(P_or_dims)
    m = _capi.Marshalled.masks_only(Nx, Nu, S[0], S[1], index_base)
    values = np.ascontiguousarray(values, dtype=np.float64)
    _, pcz = _vec(cz, Nx + Nu, "cz")
    _, pb = _vec(b, Nx, "b")
    pi, pj = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int64) for a in (pairs_i, pairs_j))
    if pi.ndim != 1 or pi.shape != pj.shape:
        raise ValueError(f"pairs_i and pairs_j must be two lists of one length, got shapes {pi.shape} and {pj.shape}")
    cov = np.zeros(max(pi.size, 1))
    ip = C.POINTER(C.c_int64)
    _capi.check(_capi.load_library().sls_debug_norms_cov_host(C.byref(m.dims), m.Sx, m.Su, values.ctypes.data_as(_DP), pcz, pb, pi.size,
                                                              pi.ctypes.data_as(ip), pj.ctypes.data_as(ip), cov.ctypes.data_as(_DP)))
    return cov[: pi.size]
