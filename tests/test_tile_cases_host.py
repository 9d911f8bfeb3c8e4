"""Host twin of tests/test_gpu_tile_ladder.py: everything about the tile kernel's size ladder (tests/tile_cases.py) that can be
proven without a GPU — the index-set sizes, the references' feasibility on every ladder column, and the launch list of every
case for 256 CUs — so that the shapes are known good before a GPU is used, and a later change to the masks, the reduction or the
routing cannot quietly take a size off the ladder or move a case to another home."""
import numpy as np
import pytest

import tile_cases as tc

_SIZES = [16 * k + o for k in range(1, 10) for o in (-1, 0, 1)]


@pytest.mark.parametrize("name", tc.PROBLEMS)
def test_ladder_hits_every_target_size(slc, oracle, name):
    """ñx of the 27 ladder columns is 15, 16, 17, 31, …, 145 exactly, by the oracle's reduction and by the library's own, and the
    two agree on the index sets themselves; the pivot tile counts are 1…10."""
    assert list(tc.TARGETS) == _SIZES and len(set(tc.problem(slc, name)["cols"])) == 27
    ours = tc.index_sets(slc, name)
    lib = tc.library_index_sets(slc, name)
    assert [len(sx) for sx, _ in ours] == _SIZES
    assert [len(sx) for sx, _ in lib] == _SIZES
    for (sx, su), (lx, lu) in zip(ours, lib):
        assert np.array_equal(np.sort(sx), np.sort(lx)) and np.array_equal(np.sort(su), np.sort(lu))
    for (sx, _), c in zip(ours, tc.problem(slc, name)["cols"]):
        assert c in sx
    assert sorted({tc.nt_of(len(sx)) for sx, _ in ours}) == list(range(1, 11))


def test_input_counts_straddle_the_row_padding(slc, oracle):
    """ñu of act_all and readme_act between them: on a multiple of 8 and of 16, just above one (by 1 or 2) and just below one (by
    at most 4) — the kernel rounds ñu up to a multiple of 8 for its carve (mmax) and to tiles for the build of Ã·Q."""
    nu = sorted({len(su) for name in ("act_all", "readme_act") for _, su in tc.index_sets(slc, name)})
    assert [len(su) for _, su in tc.index_sets(slc, "act_all")] != [len(su) for _, su in tc.index_sets(slc, "readme_act")]
    for M in (8, 16):
        assert any(m % M == 0 for m in nu), (M, nu)
        assert any(0 < m % M <= 2 for m in nu), (M, nu)
        assert any(m % M >= M - 4 for m in nu), (M, nu)
    assert nu[0] < 8 and nu[-1] > 144


@pytest.mark.parametrize("name", tc.PROBLEMS)
def test_reference_is_feasible_on_every_ladder_column(slc, oracle, name):
    """No column may be left out of a comparison: the reference solves all 27 (status 0; residual < 1e-12 in the C restatement,
    < 1e-9 in the NumPy oracle), and max |Φ| of every column is above 0.1, so that the absolute tolerance means something."""
    ref = tc.reference(slc, name)
    assert len(ref["status"]) == len(ref["resid"]) == 27
    assert np.all(ref["status"] == 0), ref["status"]
    assert ref["resid"].max() < tc.residual_bound(name), ref["resid"]
    _, big = tc.column_errors(slc, name, np.zeros_like(ref["flat"]))
    assert len(big) == 27 and big.min() > 0.1, big
    print(f"{name}: reference in {tc.oracle_seconds[name]:.2f} s, worst residual {ref['resid'].max():.1e}, smallest max|Φ| {big.min():.3f}")


@pytest.mark.parametrize("cid", tc.IDS)
def test_tile_launch_lists_on_256_cus(slc, cid, monkeypatch):
    """Kernel selection alone, for 256 CUs: every case gets its pinned launch list (kernel with template arguments, nsub, nmax,
    per_cu), every launch is the tile kernel, and the launches' nsub are the counts of ladder sizes the homes are meant to hold."""
    case = tc.get(cid)
    pr = tc.problem(slc, case["problem"])
    tc.set_knobs(monkeypatch, case["env"])
    desc = slc.dist.describe_launches(pr["P"], pr["S"], pr["groups"], None, tc.NCU)
    assert tc.short(desc) == case["pinned"], desc
    sizes = tc.launch_sizes(desc)
    assert all(k.startswith("h2_column_tile_kernel<") for k, _, _ in sizes) and sum(n for _, n, _ in sizes) == 27, desc
    assert all(("dense_hessian_cg" in k) == (case["problem"] == "dense") for k, _, _ in sizes), desc
    lds = [(n, nmax) for k, n, nmax in sizes if "block_in_LDS" in k]
    ws = [(n, nmax) for k, n, nmax in sizes if "block_in_workspace" in k]
    home = cid.split("-")[1]
    if home in ("lds", "default"):
        # the LDS launch holds exactly the targets ≤ 96
        assert lds == [(sum(n <= 96 for n in _SIZES), 96)] and ws == [(sum(n > 96 for n in _SIZES), 145)], desc
    elif home == "lds9":
        # no workspace launch remains for ñx ≤ 144
        assert ws == [(sum(n > 144 for n in _SIZES), 145)], desc
        assert sorted(lds) == [(sum(96 < n <= 144 for n in _SIZES), 144), (sum(n <= 96 for n in _SIZES), 96)], desc
    else:
        assert lds == [] and ws == [(27, 145)], desc
        assert all(("carve_in_workspace" in k) == (home == "carve") for k, _, _ in sizes), desc


def test_tile_table_names_every_home():
    """Each home of the block, with and without the CG build, appears by name in at least one pinned list."""
    pinned = ";".join(c["pinned"] for c in tc.CASES)
    for name in (tc._LDS, tc._WS, tc._BIG, tc._LDS_CG, tc._WS_CG, tc._BIG_CG):
        assert name + " " in pinned, name
    assert {c["problem"] for c in tc.CASES} == set(tc.PROBLEMS)


@pytest.mark.parametrize("Th", tc.SHORT_T)
def test_short_horizon_columns_are_feasible_and_in_the_workspace(slc, oracle, Th, monkeypatch):
    """The short-horizon cases compare something: at every horizon the C restatement finds both columns (ñx = 97, 113) feasible,
    and under SLS_FORCE_GENERAL=1 both run with the block in the workspace."""
    import sls_oracle_cport as cp
    pr = tc.short_problem(slc, Th)
    assert len(pr["S"][0]) == Th
    Po = oracle.OraclePlant(pr["P"].A, pr["P"].B1, pr["P"].B2)
    assert [len(oracle.sparsity_dim_reduction(Po, [c], pr["S"])[3]) for c in pr["cols"]] == [97, 113]
    _, _, info = cp.SLS_H2(Po, pr["S"], cols=pr["cols"], nthreads=2)
    assert np.all(info["status"] == 0) and info["resid"].max() < 1e-12, info
    tc.set_knobs(monkeypatch, tc.ENV_LDS)
    desc = slc.dist.describe_launches(pr["P"], pr["S"], pr["groups"], None, tc.NCU)
    assert tc.short(desc) == tc.SHORT_PINNED, desc
