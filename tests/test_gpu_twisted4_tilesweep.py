"""Four-wave twisted kernel, three-tile classes: P_k kept in the Gauss–Jordan's tile layout — in registers, in the workspace and in
all four substitution sweeps — and the fused sweep step's input vector formed one block ahead of the elimination.

What can go wrong is therefore (a) a tile entry that meets the wrong vector entry or a reduction over the wrong lanes (shows at
every size), (b) the padding rows and columns of the third tile, ñx … 23 (the sizes at the 8-lane tile edges and at the top of
either class), (c) the sweep input prepared ahead for a block that has no fused step (the middle block) or no predecessor
(blocks 0 and T), at short and long halves, (d) a later pass that reads P_k back from the workspace in another layout than the
first pass stored, or from a slot the launch did not write, (e) the residual pass of a weighted column feeding the first sweep,
(f) the four-tile classes, which keep the column layout behind `if constexpr`.

The reference is the two-wave kernel (SLS_TWISTED4=0 in lab mode), which the change does not touch: equal statuses, equal pass
counts, |ΔΦ| < 1e-9 (the bound of test_gpu_twisted4_helper.py).  The default-weight cases are also held to the C restatement of
the oracle at TOL = 1e-8, the suite's bound (derivation: header of test_gpu_parity.py).

Cases, all on chain plants with the README recipe (`chain_plant`, `localization_masks`); ñx as the host reports them
(interior columns 2d + 3 once the horizon lets the masks reach d; columns near the chain's ends one less per step):

  id             plant  (d, T, α)       columns          ñx              class     what it covers
  c10_T7         48     (8, 7, 3.0)     3, 9, 24         13, 19, 19      <32,10>   T = 7: halves of 4 and 3 blocks, the ramp still grows
                                                                                   at the meeting block; ñx = 13 is the smallest the
                                                                                   routing fence lets through; 19 with padding 19 … 23
  c10_T17_mix    48     (8, 17, 1.5)    3, 6, 7, 24      13, 16, 17, 19  <32,10>   16 | 17: the 8-lane tile edge; ramp long finished
                                                                                   (the cached static part is reused from block 8 on);
                                                                                   edge columns and an interior one in one launch
  c10_top20      48     (9, 12, 1.5)    2, 8, 9          13, 19, 20      <32,10>   ñx = 20, the top of <32,10>, an even size
  c12_T8         48     (9, 8, 3.0)     10, 24           21, 21          <32,12>   an even horizon, ñx = 21: the bottom of <32,12>
  c12_T7         48     (10, 7, 3.0)    5, 24            17, 23          <32,12>   T = 7 in the other class, 17 beside 23
  c12_top24      48     (11, 9, 1.5)    9, 10, 11        22, 23, 24      <32,12>   ñx = 24: no padding at all
  c12_mix        48     (10, 12, 1.5)   4, 11, 24        16, 23, 23      <32,12>   an edge column among interior ones, ramp growing
  load_path      70     (9, 29, 1.5)    20, 23, … 47     21              <32,12>   columns that take a second pass on both kernels: the
                                                                                   second pass loads every P_k from the workspace
  weighted       48     (9, 12, 1.5)    22, 24, 27       21              <32,12>   diagonal C1 / D12 ≠ I and D11 ≠ 0: has_w, g ≠ 0
  four_tile      48     (11, 12, 1.5)   24, 25           25              <32,14>   the untouched four-tile path

tests/golden/infeasible_chain.npz (23 states, d = 4: ñx ≤ 11) is routed to the two-wave kernel <16,3>, not to this one; the
host test below states that, so the fixture is not run here.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_c import TOL, c_oracle_flat
from test_gpu_twisted4_prepared import _index_sets, _masks_of, _bits

NCU = 256
FOUR = "h2_column_twisted4_kernel"
TWO = "h2_column_twisted_kernel"

# id → (plant, d, T, α, columns, ñx of the columns, four-wave class)
CASES = {
    "c10_T7": ("chain48", 8, 7, 3.0, (3, 9, 24), (13, 19, 19), "<32,10>"),
    "c10_T17_mix": ("chain48", 8, 17, 1.5, (3, 6, 7, 24), (13, 16, 17, 19), "<32,10>"),
    "c10_top20": ("chain48", 9, 12, 1.5, (2, 8, 9), (13, 19, 20), "<32,10>"),
    "c12_T8": ("chain48", 9, 8, 3.0, (10, 24), (21, 21), "<32,12>"),
    "c12_T7": ("chain48", 10, 7, 3.0, (5, 24), (17, 23), "<32,12>"),
    "c12_top24": ("chain48", 11, 9, 1.5, (9, 10, 11), (22, 23, 24), "<32,12>"),
    "c12_mix": ("chain48", 10, 12, 1.5, (4, 11, 24), (16, 23, 23), "<32,12>"),
    "load_path": ("chain70", 9, 29, 1.5, tuple(range(20, 50, 3)), (21,) * 10, "<32,12>"),
    "weighted": ("weighted48", 9, 12, 1.5, (22, 24, 27), (21, 21, 21), "<32,12>"),
    "four_tile": ("chain48", 11, 12, 1.5, (24, 25), (25, 25), "<32,14>"),
}
_IDS = list(CASES)
REPEAT_CASE = "c12_mix"

_cache = {}


def _plant(slc, kind):
    if kind == "chain48":
        return slc.workloads.chain_plant(48)
    if kind == "chain70":
        return slc.workloads.chain_plant(70)
    P = slc.workloads.chain_plant(48)
    Nx, Nu = P.A.shape[0], P.B2.shape[1]
    C1 = sp.vstack([sp.diags(np.linspace(0.5, 2.0, Nx)), sp.csc_matrix((Nu, Nx))]).tocsc()
    D12 = sp.vstack([sp.csc_matrix((Nx, Nu)), sp.diags(np.linspace(1.0, 3.0, Nu))]).tocsc()
    D11 = sp.lil_matrix((Nx + Nu, Nx))
    for c in range(Nx):
        D11[c, c] = 0.1 * (1 + c % 3)
        D11[(c + 2) % Nx, c] = -0.05
    return slc.Plant(P.A, P.B1, P.B2, C1, D11.tocsc(), D12)


def _case(slc, cid):
    """(P, S, columns, class, Φ_oracle or None, oracle status or None): computed once, never modified."""
    if cid not in _cache:
        kind, d, T, alpha, cols, _, cls = CASES[cid]
        P = _plant(slc, kind)
        S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, alpha))
        want = ostatus = None
        if kind != "weighted48":                         # the C restatement takes no weights
            want, oinfo = c_oracle_flat(slc, P, S, list(cols))
            ostatus = np.array(oinfo["status"])
            want.setflags(write=False); ostatus.setflags(write=False)
        _cache[cid] = (P, S, list(cols), cls, want, ostatus)
    return _cache[cid]


def _middle(T):
    return (T + 1) // 2 if T >= 7 else (T - 1) // 2


# ---- host twins (no GPU) ----

@pytest.mark.parametrize("cid", _IDS)
def test_cases_have_the_sizes_and_the_class_of_the_table(slc, cid):
    P, S, cols, cls, want, ostatus = _case(slc, cid)
    assert tuple(len(_index_sets(P, S, c)[0]) for c in cols) == CASES[cid][5]
    desc = slc.dist.describe_launches(P, S, [[c] for c in cols], None, NCU)
    assert desc.startswith(FOUR + cls + f" nsub={len(cols)} grid={len(cols)} ") and desc.count(";") == 1, desc
    if ostatus is not None:
        assert np.all(ostatus == 0), ostatus


def test_horizons_cover_both_ramp_shapes(slc):
    """Bit k of the upward mask-repeat word: block k has the masks of block k − 1.  Growing at the meeting block c: bit c clear."""
    grows = {}
    for cid in ("c10_T7", "c12_T8", "c12_mix", "c10_T17_mix", "load_path"):
        P, S, cols, _, _, _ = _case(slc, cid)
        T = len(S[0])
        sx, su = _index_sets(P, S, cols[-1])
        up, _ = _bits(_masks_of(S, cols[-1], sx, su))
        grows[cid] = not ((up >> _middle(T)) & 1)
    assert grows["c10_T7"] and grows["c12_T8"] and grows["c12_mix"]
    assert not grows["c10_T17_mix"] and not grows["load_path"]
    assert _middle(7) == 4 and 7 - _middle(7) == 3 and _middle(8) == 4


def test_infeasible_fixture_is_not_routed_to_the_four_wave_kernel(slc):
    import os
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "infeasible_chain.npz"))
    P = slc.workloads.chain_plant(int(g["Nx"]))
    S = list(slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"])))
    desc = slc.dist.describe_launches(P, S, None, None, NCU)
    assert FOUR not in desc and TWO in desc, desc


# ---- GPU ----

def _run(plan):
    dv = plan.alloc_values()
    plan.execute(dv); plan.synchronize()
    st, rs, it = (np.asarray(a).copy() for a in plan.fetch_status())
    return np.concatenate(sum(plan.download(dv), [])), st, rs, it


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _IDS)
def test_tile_sweeps_match_two_wave_kernel(slc, gpu_ctx, cid, monkeypatch):
    P, S, cols, cls, want, ostatus = _case(slc, cid)
    out = {}
    for four, name in (("1", FOUR + cls), ("0", TWO + "<")):
        monkeypatch.setenv("SLS_TWISTED4", four)
        plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
        try:
            desc = plan.describe()
            assert name in desc and desc.count(";") == 1, desc
            out[four] = _run(plan)
        finally:
            plan.close()
    (got, st, rs, it), (ref, st2, rs2, it2) = out["1"], out["0"]
    dev = np.abs(got - ref).max()
    err = np.abs(got - want).max() if want is not None else float("nan")
    print(f"{cid}: status {st.tolist()} / {st2.tolist()} passes {it.tolist()} / {it2.tolist()} residual {rs.max():.1e} / {rs2.max():.1e} "
          f"max |Φ4 − Φ2| = {dev:.2e}, max |Φ4 − Φ_oracle| = {err:.2e}")
    assert np.array_equal(st, st2), (st, st2)
    assert np.array_equal(it, it2), (it, it2)
    assert dev < 1e-9, dev
    if cid == "load_path":
        assert it.max() >= 2 and it2.max() >= 2, (it, it2)
    if want is not None:
        assert np.all(st == 0), (st, rs)
        assert err < TOL, err


def _execute_into_nan(plan):
    import torch
    n = plan.info["n_values"]
    v = torch.full((max(n, 1),), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    plan.execute(v.data_ptr()); plan.synchronize()
    st, rs, it = (np.asarray(a).copy() for a in plan.fetch_status())
    return v.cpu().numpy()[:n].copy(), st, rs, it


@pytest.mark.gpu
def test_repeat_and_plant_update_read_nothing_stale(slc, gpu_ctx):
    """A second execute into a NaN-filled value array equals the first bit for bit (nothing is read from the previous launch's
    workspace before this launch wrote it); the same after update_plant with scaled A and B2, against a freshly built plan."""
    P, S, cols, cls, _, _ = _case(slc, REPEAT_CASE)
    A, B2 = sp.csc_matrix(P.A).copy(), sp.csc_matrix(P.B2).copy()
    A.data = A.data * 1.0625; B2.data = B2.data * 0.875
    Q = slc.Plant(A, P.B1, B2)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    fresh = None
    try:
        assert FOUR + cls in plan.describe()
        first = _execute_into_nan(plan)
        second = _execute_into_nan(plan)
        plan.update_plant(A=Q.A, B2=Q.B2)
        upd = _execute_into_nan(plan)
        upd2 = _execute_into_nan(plan)
        fresh = slc.Plan(gpu_ctx, Q, S, [[c] for c in cols])
        ref = _execute_into_nan(fresh)
    finally:
        plan.close()
        if fresh is not None:
            fresh.close()
    # entries of columns outside the plan keep the NaN on every side: compare bit patterns
    bits = lambda r: r[0].view(np.uint64)
    assert np.all(first[1] == 0) and np.all(ref[1] == 0)
    assert not np.all(np.isnan(first[0])) and np.array_equal(np.isnan(first[0]), np.isnan(ref[0]))
    assert np.array_equal(bits(first), bits(second))
    assert all(np.array_equal(a, b) for a, b in zip(first[1:], second[1:]))
    assert not np.array_equal(bits(first), bits(upd))               # the update changed something
    assert np.array_equal(bits(upd), bits(ref)) and np.array_equal(bits(upd2), bits(ref))
    assert all(np.array_equal(a, b) for a, b in zip(upd[1:], ref[1:]))
