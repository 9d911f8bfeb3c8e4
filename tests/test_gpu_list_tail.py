"""Row lists of Ã longer than the four register-cached entries, on every column-kernel family.

The one-wave, two-wave and four-wave kernels keep the first four entries of a lane's row list and column list of Ã in registers
and continue from LDS (`dotA_row` / `dotA_col`, the same text in each of the three kernels).  The chain plants of
the other tests have at most three entries per row, so the tail loop never runs there.  A 4-neighbour grid has five: the state
itself and its four neighbours.

Plant and masks: `grid_plant(n=7, act_every=1)` (49 states, every state actuated), `localization_masks` with d = 2, T = 8,
α = 1.5.  The index set of a column is the diamond of radius 3 around it, cut by the border:

  column  where                  ñx   longest row / column of Ã   size class
  24      centre                 25   5 / 5                       <32,14>
  8       second row and column  17   5 / 5                       <32,10>   (16 | 17: the first size of the 32-lane classes)
  3       middle of the border   16   5 / 5                       <16,4>
  0       corner                 10   5 / 5                       <16,3>

One column per plan, on three routes: the default one with SLS_T4_NMIN=0 SLS_T4_TMIN=0 (no size or horizon fence in front of the
four-wave kernel), SLS_TWISTED4=0 (two-wave kernel), SLS_NO_TWISTED=1 (one-wave kernel).  The four-wave kernel exists for the
32-lane classes only, so on the first route columns 3 and 0 (ñx ≤ 16) still run on the two-wave kernel; the table KERNEL below
is what `describe()` must say, and the host test asserts the same of `describe_launches`.

Reference: the C restatement of the oracle at its TOL = 1e-8 (oracle_c.py; derivation: header of test_gpu_parity.py), status 0
everywhere.  Where a column runs on the four-wave and on the two-wave kernel, statuses and pass counts are equal (as in
test_gpu_twisted4_tilesweep.py: the two share every step but the factorisation's schedule).
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_c import TOL, c_oracle_flat
from test_gpu_twisted4_prepared import _index_sets

NCU = 256
COLUMNS = (24, 8, 3, 0)
NX = {24: 25, 8: 17, 3: 16, 0: 10}
KNOBS = ("SLS_T4_NMIN", "SLS_T4_TMIN", "SLS_TWISTED4", "SLS_NO_TWISTED")
ROUTES = {
    "default": {"SLS_T4_NMIN": "0", "SLS_T4_TMIN": "0"},
    "two_wave": {"SLS_TWISTED4": "0"},
    "one_wave": {"SLS_NO_TWISTED": "1"},
}
KERNEL = {
    "default": {24: "h2_column_twisted4_kernel<32,14>", 8: "h2_column_twisted4_kernel<32,10>",
                3: "h2_column_twisted_kernel<16,4,", 0: "h2_column_twisted_kernel<16,3,"},
    "two_wave": {24: "h2_column_twisted_kernel<32,14,", 8: "h2_column_twisted_kernel<32,10,",
                 3: "h2_column_twisted_kernel<16,4,", 0: "h2_column_twisted_kernel<16,3,"},
    "one_wave": {24: "h2_column_wave_kernel<32,14>", 8: "h2_column_wave_kernel<32,10>",
                 3: "h2_column_wave_kernel<16,4>", 0: "h2_column_wave_kernel<16,3>"},
}

_cache = {}


def _problem(slc):
    """(P, S, Φ_oracle of the chosen columns, oracle statuses): computed once, never modified."""
    if not _cache:
        P = slc.workloads.grid_plant(n=7, act_every=1)
        S = list(slc.workloads.localization_masks(P.A, P.B2, 2, 8, 1.5))
        want, info = c_oracle_flat(slc, P, S, list(COLUMNS))
        ostatus = np.array(info["status"])
        want.setflags(write=False); ostatus.setflags(write=False)
        _cache["p"] = (P, S, want, ostatus)
    return _cache["p"]


def _set_route(monkeypatch, route):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def test_columns_have_list_tails_and_are_feasible(slc, monkeypatch):
    P, S, want, ostatus = _problem(slc)
    A = sp.csr_matrix(P.A)
    for c in COLUMNS:
        sx, _ = _index_sets(P, S, c)
        assert len(sx) == NX[c], (c, len(sx))
        At = A[sx][:, sx]
        assert np.diff(At.indptr).max() == 5 and np.diff(At.tocsc().indptr).max() == 5, c     # > 4: the tail loop runs
    assert np.all(ostatus == 0), ostatus
    for route in ROUTES:
        _set_route(monkeypatch, route)
        for c in COLUMNS:
            desc = slc.dist.describe_launches(P, S, [[c]], None, NCU)
            assert desc.startswith(KERNEL[route][c]) and " nsub=1 grid=1 " in desc and desc.count(";") == 1, (route, c, desc)


def _run(slc, gpu_ctx, P, S, c, name):
    plan = slc.Plan(gpu_ctx, P, S, [[c]])
    try:
        desc = plan.describe()
        assert desc.startswith(name) and desc.count(";") == 1, desc
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        st, rs, it = (np.asarray(a).copy() for a in plan.fetch_status())
        return np.concatenate(sum(plan.download(dv), [])), st, rs, it
    finally:
        plan.close()


def _column_entries(P, S, c):
    """Positions of column c's entries in the mask-order value array."""
    col = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(sp.csc_matrix(M).indptr)) for M in S[0] + S[1]])
    return col == c


@pytest.mark.gpu
@pytest.mark.parametrize("c", COLUMNS)
def test_list_tail_on_every_family(slc, gpu_ctx, c, monkeypatch):
    P, S, want, ostatus = _problem(slc)
    mine = _column_entries(P, S, c)
    out = {}
    for route in ROUTES:
        _set_route(monkeypatch, route)
        got, st, rs, it = _run(slc, gpu_ctx, P, S, c, KERNEL[route][c])
        err = np.abs(got[mine] - want[mine]).max()
        print(f"column {c} {route}: {KERNEL[route][c]} status {st.tolist()} passes {it.tolist()} residual {rs.max():.1e} "
              f"max |Φ − Φ_oracle| = {err:.2e}")
        assert np.all(st == 0), (route, st, rs)
        assert err < TOL, (route, err)
        assert not np.any(got[~mine]), route                 # a one-column plan writes its column only
        out[route] = (st, it)
    if "twisted4" in KERNEL["default"][c]:
        assert np.array_equal(out["default"][0], out["two_wave"][0])
        assert np.array_equal(out["default"][1], out["two_wave"][1]), (out["default"][1], out["two_wave"][1])
