"""Host twin of tests/test_gpu_symbolic_edges.py: what can be proven about the cases of tests/symbolic_cases.py without a GPU.
Every case hits the edge it is there for — computed from the NumPy/SciPy reference alone and measured against limits parsed out
of the sources (kMaxLds, the first capacities 1024 / 1024 / 2048 of the three retry loops, bytes per list entry, the 62-level
limit, the 1024-column round of level_prefix_kernel, 8·256 workgroups) — and the library's host pass (sls_localization_masks,
sls_sparsity_dim_reduction) equals that reference in both index bases, so that the reference itself is pinned before a GPU
test relies on it."""
import numpy as np
import pytest
import scipy.sparse as sp

import symbolic_cases as sc


def _sizes(name):
    tb = sc.reference_tables(name)
    return set(tb["nx"].tolist()), set((tb["nx"] + tb["nu"]).tolist()), tb


def test_limits_are_the_ones_the_cases_were_built_for():
    L = sc.limits()
    assert L["max_lds"] == 160 * 1024 and (L["cap0_masks"], L["cap0_index"], L["cap0_tables"]) == (1024, 1024, 2048)
    assert (L["entry_masks"], L["entry_index"], L["entry_tables"]) == (12, 4, 8)
    assert L["max_levels"] == 62 and L["prefix_round"] == 1024 and L["max_grid"] == 2048
    assert L["max_levels"] + 2 <= L["level_starts"] and L["max_levels"] - 1 <= 64          # level starts px[KL + 2]; bits of lv


def test_hub_cases_sit_on_both_sides_of_the_first_capacities():
    """hub1024 / hub1025: the largest level (mask kernel) and the largest index set (index-set kernel) are exactly the first
    capacity and one more; both hubs' pools exceed the tables kernel's first capacity, pool2048 / pool2049 sit on it."""
    L = sc.limits()
    a, b = sc.reference("hub1024"), sc.reference("hub1025")
    assert a.largest_mask_level() == L["cap0_masks"] == a.largest_index_set() == L["cap0_index"]
    assert b.largest_mask_level() == L["cap0_masks"] + 1 == b.largest_index_set()
    assert sc.cap_limit_masks(a.Nx, a.Nu) == 1100 > L["cap0_masks"] + 1
    assert (a.largest_pool(), b.largest_pool()) == (3073, 3076) and a.largest_pool() > L["cap0_tables"]
    p, q = sc.reference("pool2048"), sc.reference("pool2049")
    assert (p.KL, q.KL) == (3, 3)
    assert p.largest_pool() == L["cap0_tables"] and q.largest_pool() == L["cap0_tables"] + 1
    assert max(p.largest_mask_level(), q.largest_mask_level()) < L["cap0_masks"]           # only the pool retries there


def test_wide_input_case_lets_the_actuator_list_set_the_capacity():
    r = sc.reference("hub_wideB")
    assert (r.Nx, r.Nu) == (40, 1300) and sc.cap_limit_masks(r.Nx, r.Nu) == 1300 == sc.cap_limit_index(r.Nx, r.Nu)
    assert max(int(np.diff(M.indptr).max()) for M in r.L[:r.K1]) == 40
    assert r.largest_mask_level() == 1300 > sc.limits()["cap0_masks"]
    assert int(np.diff(r.index_sets()[1].indptr).max()) == 1300


def test_long_range_case_needs_three_scan_rounds_three_columns_per_wave_and_a_ragged_prefix_tail():
    L = sc.limits()
    r = sc.reference("far4200")
    assert 128 < r.widest_word_span() <= 192                     # 64 words per round of bitmap_to_list
    assert 2 * L["max_grid"] < r.Nx < 3 * L["max_grid"]          # waves 0…103 get a third column
    assert r.Nx // L["prefix_round"] == 4 and r.Nx % L["prefix_round"] not in (0, 1, L["prefix_round"] - 1)
    # the long edges are seen from both ends: a far state in a level of column 5, a low state in a level of column 2060
    assert {2100, 4190} <= set(r.L[1][:, 5].indices.tolist()) and 3 in r.L[1][:, 2060].indices
    # the columns after a wide one on the same wave (c + 2048, c + 4096) have ordinary narrow levels: leftovers would show
    assert r.L[2][:, 5 + 2048].nnz == 5 and r.L[2][:, 5 + 4096].nnz == 5


@pytest.mark.parametrize("n", [1023, 1025, 2049])
def test_prefix_cases_straddle_the_column_rounds(n):
    r = sc.reference(f"prefix{n}")
    assert r.Nx == n and n % sc.limits()["prefix_round"] in (1, sc.limits()["prefix_round"] - 1)
    assert "tables" in sc.BY_NAME[f"prefix{n}"]["routes"]       # only the localized route runs level_prefix_kernel


def test_word_cases_cover_every_bitmap_boundary():
    got = {(sc.reference(n).Nx, sc.reference(n).Nu) for n in sc.NAMES if n.startswith("words")}
    assert {nx for nx, _ in got} == {1, 31, 32, 33, 63, 64, 65}
    assert {nu for _, nu in got} >= {0, 1, 32, 33}
    for n in sc.NAMES:
        if n.startswith("words") and "last state" in sc.BY_NAME[n]["edge"]:
            B2 = sc.plant(n)[1]
            assert B2[B2.shape[0] - 1].nnz == 1
    assert any("last state" in sc.BY_NAME[n]["edge"] and sc.reference(n).Nx % 32 == 0 for n in sc.NAMES)      # bit 31 of a word
    assert any("last state" in sc.BY_NAME[n]["edge"] and sc.reference(n).Nx % 32 == 1 for n in sc.NAMES)      # bit 0 of a word


def test_dense_case_fills_every_list_to_the_brim():
    r = sc.reference("dense40")
    assert sc.cap_limit_masks(40, r.Nu) == 40 == sc.cap_limit_index(40, r.Nu)
    assert all(int(np.diff(M.indptr).min()) == 40 for M in r.L[1:])
    assert r.largest_mask_level() == 40 and r.largest_index_set() == 40


def test_deep_cases_sit_on_the_level_limit():
    L = sc.limits()
    r, r60 = sc.reference("deep"), sc.reference("deep60")
    assert r.kmax + 2 == L["max_levels"] and r.K1 == 61 and r.KL == 61 and r.largest_pool() == 3115 > L["cap0_tables"]
    assert r60.kmax + 2 == L["max_levels"] + 1
    assert sorted(set(r.kx)) != list(range(r.kmax + 1))         # not every level is a mask: lv carries unused bits too
    assert r.kmax in r.ku and 0 in r.kx


def test_schedule_cases():
    by = {(c["alpha"], c["d"], c["T"]): sc.reference(c["name"]) for c in sc.CASES if c["name"].startswith("sched")}
    assert set(by) == {(0.0, 3, 5), (0.5, 2, 9), (1.0, 0, 4), (1.5, 3, 1), (0.05, 4, 130)}
    assert by[(0.0, 3, 5)].kx == [0] * 5 and by[(0.0, 3, 5)].K1 == 1
    assert by[(0.5, 2, 9)].kx == [0, 0, 1, 1, 2, 2, 2, 2, 2] and by[(0.5, 2, 9)].ku == [0, 0, 1, 1, 2, 2, 3, 3, 3]
    assert by[(1.0, 0, 4)].kx == [0] * 4 and by[(1.0, 0, 4)].ku == [0, 1, 1, 1]
    assert by[(1.5, 3, 1)].T == 1 and by[(1.5, 3, 1)].KL == 1
    r = by[(0.05, 4, 130)]
    assert r.T > 2 * 64 and r.kx[63] != r.kx[64 + 63] and r.kx[-1] == 4 and r.ku[-1] == 5   # the second and third staging rounds differ from the first


def test_band_cases_hit_the_mask_word_boundaries():
    nx, nm, tb = _sizes("band65")
    assert max(nx) == 65 and {63, 64, 65} <= nx and 128 in nm
    assert int(np.bincount(tb["nx"])[65]) > 100                                            # the interior
    assert np.all(tb["nu"][tb["nx"] == 64] > 0)                                            # xbits = ~0 with actuators behind
    nx2, nm2, _ = _sizes("band65_sparse")
    assert {63, 64, 65} <= nx2 and {64, 65, 128, 129} <= nm2
    assert {64, 65, 128, 129} <= nm | nm2


def test_holes_case():
    r = sc.reference("holes")
    A, B2 = sc.plant("holes")
    assert (A.data == 0).sum() >= 5 and (B2.data == 0).sum() == 1 and A.nnz > r.Ab.nnz
    assert A[:, 7].nnz == 3 and r.Ab[:, 7].nnz == 0 and r.L[1][:, 7].nnz == 0 and r.L[0][:, 7].nnz == 1
    Bt = sp.csr_matrix(sc._pattern(B2))
    assert {3, 4, 10} <= set(np.flatnonzero(np.diff(Bt.indptr) == 0).tolist())
    assert not r.regular()                                      # column 7's own row lies outside its (empty) index set
    Sx, Su = sc.holes_last_masks()
    assert (Sx.data == 0).sum() > 0 and (Su.data == 0).sum() > 0 and Sx.nnz == r.Sx[-1].nnz


def test_lds_limit_pairs():
    """fits_mask / too_big_mask and fits_pool / too_big_pool lie on either side of what 160 KiB of LDS hold."""
    L = sc.limits()
    f, b = sc.reference("fits_mask"), sc.reference("too_big_mask")
    assert sc.cap_limit_masks(f.Nx, f.Nu) == f.Nx == f.largest_mask_level()
    lds = sc.bitmap_bytes(f.Nx, f.Nu) + L["entry_masks"] * f.Nx
    assert L["max_lds"] - 5 * 1024 < lds <= L["max_lds"]
    assert b.largest_mask_level() == 14000 > sc.cap_limit_masks(b.Nx, b.Nu) and 13300 < sc.cap_limit_masks(b.Nx, b.Nu) < 13400
    assert b.largest_index_set() <= sc.cap_limit_index(b.Nx, b.Nu)                          # the index-set list still holds it
    p, q = sc.reference("fits_pool"), sc.reference("too_big_pool")
    lim = sc.cap_limit_tables(p.Nx, p.Nu, p.T)
    assert lim == sc.cap_limit_tables(q.Nx, q.Nu, q.T)
    assert p.largest_pool() == lim and q.largest_pool() == lim + 1
    assert p.kmax + 2 == L["max_levels"] == q.kmax + 2
    fixed = sc.bitmap_bytes(p.Nx, p.Nu) + 2 * L["level_starts"] * 4 + 16 * p.T
    assert L["max_lds"] - L["entry_tables"] < fixed + L["entry_tables"] * lim <= L["max_lds"]


def test_every_listed_edge_has_a_named_case():
    for n in ("hub1024", "hub1025", "pool2048", "pool2049", "hub_wideB", "far4200", "prefix1023", "prefix1025", "prefix2049", "dense40",
              "deep", "deep60", "band65", "band65_sparse", "holes", "too_big_mask", "fits_mask", "too_big_pool", "fits_pool"):
        assert n in sc.BY_NAME, n
    assert sc.refused("tables") == ["deep60", "holes", "too_big_pool"] and sc.refused("masks") == ["too_big_mask"]
    for n in sc.names("tables"):
        assert sc.reference(n).regular(), n                     # the compact tables can express every case sent down that route


@pytest.mark.parametrize("name", sc.names("tables"))
def test_reference_tables_are_a_bijection(name):
    tb = sc.reference_tables(name)
    r = sc.reference(name)
    tgt = tb["dest"][tb["mask"] == 1]
    assert np.array_equal(np.sort(tgt), np.arange(tb["n_values"])) and np.all(tb["dest"][tb["mask"] == 0] == -1)
    assert tb["n_values"] == sum(M.nnz for M in r.Sx + r.Su) and tb["mask"].size == r.T * int((tb["nx"] + tb["nu"]).sum())


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", sc.NAMES)
def test_host_pass_equals_the_reference(slc, name, base):
    """sls_localization_masks: column pointers and row indices of every 𝓢x[t], 𝓢u[t]; sls_sparsity_dim_reduction: s_x, s_u of
    every (sampled, on the large cases) column — against the Boolean-matrix-power reference, in both index bases."""
    c = sc.BY_NAME[name]
    A, B2 = sc.plant(name)
    ref = sc.reference(name)
    hx, hu = slc.workloads.localization_masks_native(A, B2, c["d"], c["T"], c["alpha"], index_base=base)
    for H, R in zip(hx + hu, ref.Sx + ref.Su):
        assert H.shape == R.shape and np.array_equal(H.indptr, R.indptr) and np.array_equal(H.indices, R.indices)
    variants = [(ref.Sx[-1], ref.Su[-1])] + ([sc.holes_last_masks()] if name == "holes" else [])
    cols = sc.sample_columns(name)
    for Sx_last, Su_last in variants:
        PX, PU = ref.index_sets(Sx_last, Su_last)
        got = sc.host_reduction(slc, A, Sx_last, Su_last, cols, base)
        for col, (sx, su) in zip(cols, got):
            assert np.array_equal(sx, PX.indices[PX.indptr[col]:PX.indptr[col + 1]]), col
            assert np.array_equal(su, PU.indices[PU.indptr[col]:PU.indptr[col + 1]]), col
