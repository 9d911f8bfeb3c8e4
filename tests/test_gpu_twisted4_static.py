"""Four-wave twisted kernel: the helper wave's static build S_k and border X with the Ã / B̃ gathers held in registers.

For the three-tile classes (<32,10>, <32,12>) the helper gathers, once per column, the values its static build reads through
the first four Ã entries and the first two B̃ entries of every row, and the nine Ã values of its border; a rebuilt block then
reads weights only.  Rows with more entries than that finish in loops that still gather from LDS.  What can go wrong is
therefore (a) a cached value that belongs to another tile position, entry or direction, (b) the seam between the cached entries
and the tail loops, (c) the weights `hx`, `hu` inside `v = hav·w` when they are not 1, and (d) a rebuilt block that follows a
reused one.  The cases:

  plant, columns                          masks (d, T, α)        class     what it covers
  chain_plant(70), range(20, 50, 3)       (9, 29, 3.0)           <32,12>   a three-block ramp, then 25 reuses of the cached S
  banded plant, range(20, 44, 3)          (4, 12, 1.0)           <32,12>   five-block ramp
  banded plant                            (4,  9, 1.5)           <32,12>   ramp as on the README chain
  banded plant                            (4,  8, 1.0), T = 7    <32,12>   the ramp reaches the meeting block c = 4, so the downward
                                                                           helper rebuilds too; T = 7 is the smallest horizon behind
                                                                           the routing fence
  banded plant                            (3,  8, 1.0)           <32,10>   the other class with cached gathers
  banded plant, C1 / D12 non-constant     (4, 12, 1.0)           <32,12>   hx, hu ≠ 1

The banded plant has 64 states, A = I + 0.2·E₁ − 0.2·E₋₁ + 0.1·E₂ − 0.1·E₋₂, B1 = I, B2 = I + 0.5·E₋₁ − 0.25·E₋₂: five Ã
entries and three B̃ entries per row, so the cached entries and the tail loops run together on every interior row (the chain
has three and one).  The four-tile classes keep the LDS gathers; test_twisted_kernel_other_npl32_classes covers them.

Every case asserts the class string of the live plan, status 0 on every column on both sides, and max |ΔΦ| < TOL = 1e-8
against the oracle (the bound and its derivation: header of test_gpu_parity.py).  The reference of the default-weight cases is
the C restatement; it takes no weights, so the weighted case is held to the NumPy oracle (dense SVD per column), whose
"status 0" is an equality residual below 1e-9.  The host twin proves without a GPU that every case is routed to the four-wave
kernel on 256 compute units and that the oracle solves every column listed.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_c import TOL, c_oracle_flat
from conftest import flat_phi

NCU = 256
NB = 64                                     # states of the banded plant
BANDED_COLS = tuple(range(20, 44, 3))

# id → (plant, columns, d, T, α, class string in describe())
CASES = {
    "chain_ramp3_reuse25": ("chain", tuple(range(20, 50, 3)), 9, 29, 3.0, "h2_column_twisted4_kernel<32,12>"),
    "banded_ramp5": ("banded", BANDED_COLS, 4, 12, 1.0, "h2_column_twisted4_kernel<32,12>"),
    "banded_readme_ramp": ("banded", BANDED_COLS, 4, 9, 1.5, "h2_column_twisted4_kernel<32,12>"),
    "banded_ramp_to_middle_T8": ("banded", BANDED_COLS, 4, 8, 1.0, "h2_column_twisted4_kernel<32,12>"),
    "banded_ramp_to_middle_T7": ("banded", BANDED_COLS, 4, 7, 1.0, "h2_column_twisted4_kernel<32,12>"),
    "banded_class10": ("banded", BANDED_COLS, 3, 8, 1.0, "h2_column_twisted4_kernel<32,10>"),
    "banded_weighted": ("banded_weighted", BANDED_COLS, 4, 12, 1.0, "h2_column_twisted4_kernel<32,12>"),
}
_IDS = list(CASES)
# Columns of the weighted case left out because the device flags them or their residual stalls (the cancelling-diagonal defect
# of DESIGN §5.1 is data-dependent); at most one column in four.  None is left out.
WEIGHTED_LEFT_OUT = ()


def _banded(slc, weighted):
    def E(k, v):
        return sp.diags(v * np.ones(NB - abs(k)), k)
    A = (sp.identity(NB) + E(1, 0.2) - E(-1, 0.2) + E(2, 0.1) - E(-2, 0.1)).tocsc()
    B2 = (sp.identity(NB) + E(-1, 0.5) - E(-2, 0.25)).tocsc()
    B1 = sp.identity(NB, format="csc")
    if not weighted:
        return slc.Plant(A, B1, B2)
    q, r = np.linspace(0.5, 2.0, NB), np.linspace(1.0, 3.0, NB)
    C1 = sp.vstack([sp.diags(q), sp.csc_matrix((NB, NB))]).tocsc()
    D12 = sp.vstack([sp.csc_matrix((NB, NB)), sp.diags(r)]).tocsc()
    D11 = sp.csc_matrix((2 * NB, NB))
    return slc.Plant(A, B1, B2, C1, D11, D12)


_cache = {}


def _case(slc, cid):
    """(P, S, columns, class string, Φ_oracle in mask order, oracle status per column): computed once, never modified."""
    if cid not in _cache:
        kind, cols, d, T, alpha, cls = CASES[cid]
        P = slc.workloads.chain_plant(70) if kind == "chain" else _banded(slc, kind == "banded_weighted")
        S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, alpha))
        cols = [c for c in cols if not (kind == "banded_weighted" and c in WEIGHTED_LEFT_OUT)]
        if kind == "banded_weighted":
            import sls_oracle as o
            ox, ou, diags = o.SLS_H2(o.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12), S, [[c] for c in cols], return_diag=True)
            want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
            ostatus = np.array([0 if g["resid"] < 1e-9 else 1 for g in diags])
        else:
            want, oinfo = c_oracle_flat(slc, P, S, cols)
            ostatus = np.array(oinfo["status"])
        want.setflags(write=False); ostatus.setflags(write=False)
        _cache[cid] = (P, S, cols, cls, want, ostatus)
    return _cache[cid]


def test_weighted_columns_left_out_are_few():
    assert 4 * len(WEIGHTED_LEFT_OUT) <= len(BANDED_COLS) and set(WEIGHTED_LEFT_OUT) <= set(BANDED_COLS)


@pytest.mark.parametrize("cid", _IDS)
def test_cases_route_to_four_wave_kernel_and_oracle_solves_them(slc, cid):
    """Host twin: kernel selection for 256 compute units names the four-wave class of the table as the plan's only launch,
    with one workgroup per column, and the oracle reports every listed column solved.  The banded rows really have more
    entries than the helper caches (5 > 4 in Ã, 3 > 2 in B̃)."""
    P, S, cols, cls, want, ostatus = _case(slc, cid)
    desc = slc.dist.describe_launches(P, S, [[c] for c in cols], None, NCU)
    assert desc.startswith(cls + f" nsub={len(cols)} grid={len(cols)} ") and desc.count(";") == 1, desc
    assert np.all(ostatus == 0), ostatus
    assert np.abs(want).max() > 0.1
    if CASES[cid][0] != "chain":
        assert np.diff(sp.csr_matrix(P.A).indptr).max() == 5 and np.diff(sp.csr_matrix(P.B2).indptr).max() == 3
    if cid == "banded_weighted":
        hx, hu = P.C1.data, P.D12.data
        assert hx.min() < hx.max() and hu.min() < hu.max()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _IDS)
def test_static_build_from_registers_matches_oracle(slc, gpu_ctx, cid):
    P, S, cols, cls, want, ostatus = _case(slc, cid)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        desc = plan.describe()
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        st, rs, it = (np.asarray(a).copy() for a in plan.fetch_status())
        got = np.concatenate(sum(plan.download(dv), []))
    finally:
        plan.close()
    err = np.abs(got - want).max()
    print(f"{cid}: {desc} status {st.tolist()} residual {rs.max():.1e} passes {it.tolist()} max |Φ − Φ_oracle| = {err:.2e}")
    assert cls in desc, desc
    assert np.all(ostatus == 0), ostatus
    assert np.all(st == 0), (st, rs)
    assert got.shape == want.shape
    assert err < TOL, err
