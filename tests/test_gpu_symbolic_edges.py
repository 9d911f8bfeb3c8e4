"""The device symbolic pass at its bitmap, level-list and word edges (cases: tests/symbolic_cases.py; what each case reaches is
proven on the host by tests/test_symbolic_cases_host.py).  Everything here is compared BIT FOR BIT with the NumPy/SciPy
reference of that module — Boolean matrix powers, not the library's host pass — in both index bases:

  sls_localization_masks_device    mask_levels_kernel + its retry loop               (csrc/sls_masks.hip, csrc/sls_symbolic_device.cpp)
  sls_index_sets_device            index_sets_kernel + its retry loop
  sls_debug_plan_tables_localized  column_tables_kernel + its retry loop, level_prefix_kernel, expand_tables_kernel

Which case reaches what:
  retry of mask_levels / index_sets (cap 1024 doubled)    hub1025 (hub1024: exactly 1024, no retry), hub_wideB (the actuator list),
                                                          fits_mask (four doublings up to cap_limit = Nx, ≈159 KiB of LDS)
  retry of column_tables (pool cap 2048 doubled)          hub1024, hub1025, pool2049 (pool2048: exactly 2048, no retry), deep,
                                                          fits_pool (up to cap_limit: all 160 KiB)
  refusals (SLS_EUNSUPPORTED, the context stays usable)   too_big_mask, too_big_pool, deep60 (63 levels), holes (irregular)
  second and third round of bitmap_to_list                far4200 (a level over 132 bitmap words)
  second and third column per wave (grid-stride loop)     far4200 (4200 columns on 2048 workgroups), prefix2049 (one wave)
  level_prefix_kernel beside its 1024-column rounds       prefix1023, prefix1025, prefix2049, far4200 (five rounds, ragged tail)
  T > 64, T = 1, α < 1, α = 0, d = 0                      the sched_* cases
  K1 = 61 levels (61 bits of lv)                          deep, fits_pool
  empty level, rows without actuator, Nu = 0, Nu > Nx     holes, words*_u0, hub_wideB
  Nx on the bitmap word boundaries                        the words* cases;  every list exactly full: dense40
  ñx = 63, 64, 65; ñx + ñu = 64, 65, 128, 129; xbits = ~0 band65, band65_sparse (position 63 of a full word is only ever set
                                                          where a mask level reaches it: the hub columns, deep)"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import symbolic_cases as sc
from oracle_c import TOL

pytestmark = pytest.mark.gpu


def _plant(slc, name):
    A, B2 = sc.plant(name)
    return slc.Plant(A, sp.identity(A.shape[0], format="csc"), B2)


def _localized_tables(slc, ctx, P, d, T, alpha, base):
    """mask bytes, destinations, index pool of a plan built by the device-resident route; SLSError when it is refused"""
    m = slc._capi.Marshalled(P, [], [], None, index_base=base)
    m.dims.T = T
    n = C.c_int64(0); ni = C.c_int64(0)
    lib = ctx._lib
    slc._capi.check(lib.sls_debug_plan_tables_localized(ctx.handle, 0, C.byref(m.dims), C.byref(m.plant), d, alpha, C.byref(n), None, None,
                                                        C.byref(ni), None), ctx.handle)
    mask = np.zeros(n.value, dtype=np.uint8); dest = np.zeros(n.value, dtype=np.int32); idx = np.zeros(ni.value, dtype=np.int32)
    slc._capi.check(lib.sls_debug_plan_tables_localized(ctx.handle, 0, C.byref(m.dims), C.byref(m.plant), d, alpha, C.byref(n),
                                                        mask.ctypes.data_as(C.POINTER(C.c_uint8)), dest.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        C.byref(ni), idx.ctypes.data_as(C.POINTER(C.c_int32))), ctx.handle)
    return mask, dest, idx


def _host_tables(slc, ctx, P, S):
    m = slc._capi.Marshalled(P, S[0], S[1], None)
    n = C.c_int64(0); wc = C.c_int32(-1)
    lib = ctx._lib
    slc._capi.check(lib.sls_debug_plan_tables(ctx.handle, 0, *m.common_args(), 1, C.byref(n), None, None, C.byref(wc)), ctx.handle)
    mask = np.zeros(n.value, dtype=np.uint8); dest = np.zeros(n.value, dtype=np.int32)
    slc._capi.check(lib.sls_debug_plan_tables(ctx.handle, 0, *m.common_args(), 1, C.byref(n), mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              dest.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(wc)), ctx.handle)
    return mask, dest


def _good_call(slc, ctx):
    """a small call that must succeed on the same context after a refusal"""
    A, B2 = sc.plant("words33_u33")
    c = sc.BY_NAME["words33_u33"]
    ref = sc.reference("words33_u33")
    dx, du = slc.workloads.localization_masks_native(A, B2, c["d"], c["T"], c["alpha"], ctx=ctx)
    for D, R in zip(dx + du, ref.Sx + ref.Su):
        assert np.array_equal(D.indptr, R.indptr) and np.array_equal(D.indices, R.indices)
    tb = sc.reference_tables("words33_u33")
    mask, dest, idx = _localized_tables(slc, ctx, _plant(slc, "words33_u33"), c["d"], c["T"], c["alpha"], 0)
    assert np.array_equal(mask, tb["mask"]) and np.array_equal(dest, tb["dest"]) and np.array_equal(idx, tb["idx"])


@pytest.mark.parametrize("name", sc.names("masks"))
def test_device_masks_equal_the_matrix_power_recipe(slc, gpu_ctx, name):
    """sls_localization_masks_device: column pointers and row indices of every 𝓢x[t], 𝓢u[t] equal (A≠0)^kx[t] and
    (B2ᵀ≠0)(A≠0)^ku[t] by SciPy Boolean matrix powers, in both index bases.  hub1025, hub_wideB and fits_mask go through the
    retry loop of mask_levels_kernel (fits_mask up to cap_limit with ≈159 KiB of LDS), hub1024 and dense40 fill the list
    exactly, far4200 takes three rounds of bitmap_to_list and three columns per wave, deep60 runs 62 levels, holes has an empty
    level and rows without actuators, the words* cases put Nx and Nu on the bitmap word boundaries (Nu = 0 among them)."""
    c = sc.BY_NAME[name]
    A, B2 = sc.plant(name)
    ref = sc.reference(name)
    for base in (0, 1):
        dx, du = slc.workloads.localization_masks_native(A, B2, c["d"], c["T"], c["alpha"], ctx=gpu_ctx, index_base=base)
        assert len(dx) == len(du) == c["T"]
        for D, R in zip(dx + du, ref.Sx + ref.Su):
            assert D.shape == R.shape
            assert np.array_equal(D.indptr, R.indptr) and np.array_equal(D.indices, R.indices)


@pytest.mark.parametrize("name", sc.names("index"))
def test_device_index_sets_equal_the_product_rows(slc, gpu_ctx, name):
    """sls_index_sets_device on the case's last masks: every column's s_x, s_u are the ascending rows of (𝓢[T]·(A≠0))[:, c]
    (reference src/reduction.jl:14), in both index bases.  The hub cases put 1024 / 1025 / 1300 / 13000 / 14000 rows through the
    list (retry loop); `holes` also runs with stored-false mask entries, which count structurally."""
    A, _ = sc.plant(name)
    ref = sc.reference(name)
    variants = [(ref.Sx[-1].astype(bool), ref.Su[-1].astype(bool))] + ([sc.holes_last_masks()] if name == "holes" else [])
    for Sx_last, Su_last in variants:
        PX, PU = ref.index_sets(Sx_last, Su_last)
        for base in (0, 1):
            gx, gu = slc.workloads.index_sets_device(gpu_ctx, A, Sx_last, Su_last, index_base=base)
            for got, want in ((gx, PX), (gu, PU)):
                assert np.array_equal([len(v) for v in got], np.diff(want.indptr))
                assert np.array_equal(np.concatenate(got) if want.nnz else np.zeros(0, np.int64), want.indices)


@pytest.mark.parametrize("name", sc.names("tables"))
def test_device_resident_tables_equal_the_reference_tables(slc, gpu_ctx, name):
    """sls_debug_plan_tables_localized (column_tables_kernel count + fill, level_prefix_kernel, expand_tables_kernel): mask
    bytes, destinations and index pool equal the tables derived from the matrix-power reference, in both index bases; the
    destinations are a bijection onto 0 … n_values − 1; and where the host route applies, its tables are the same.
    hub1024, hub1025, pool2049, deep and fits_pool go through the pool retry (pool2048 sits exactly on the first capacity,
    fits_pool on the last), far4200 / prefix* run level_prefix_kernel beside its 1024-column rounds and give a wave several
    columns, sched_*_T130 stages T > 64, deep / fits_pool use K1 = 61 levels, band65* hit ñx = 63, 64, 65 and
    ñx + ñu = 64, 65, 128, 129."""
    c = sc.BY_NAME[name]
    P = _plant(slc, name)
    tb = sc.reference_tables(name)
    for base in (0, 1):
        mask, dest, idx = _localized_tables(slc, gpu_ctx, P, c["d"], c["T"], c["alpha"], base)
        assert mask.size == tb["mask"].size > 0 and np.array_equal(mask, tb["mask"])
        assert np.array_equal(dest, tb["dest"])
        assert np.array_equal(idx, tb["idx"])
        tgt = np.sort(dest[mask == 1])
        assert np.array_equal(tgt, np.arange(tb["n_values"])) and np.all(dest[mask == 0] == -1)
    if "host_tables" in c["routes"]:
        ref = sc.reference(name)
        mh, dh = _host_tables(slc, gpu_ctx, P, [[M.astype(bool) for M in ref.Sx], [M.astype(bool) for M in ref.Su]])
        assert np.array_equal(mh, tb["mask"]) and np.array_equal(dh, tb["dest"])


@pytest.mark.parametrize("name", sc.refused("masks") + sc.refused("tables"))
def test_refusals_leave_the_context_usable(slc, gpu_ctx, name):
    """What does not fit is refused with SLS_EUNSUPPORTED by a host-side check between launches — too_big_mask (a level of 14000
    beyond the LDS list), too_big_pool (one entry beyond the LDS pool), deep60 (63 levels), holes (a mask row outside its
    column's index set) — never answered with a truncated table, and a good call on the same context succeeds afterwards (the
    bail path left the slot's scratch usable)."""
    c = sc.BY_NAME[name]
    A, B2 = sc.plant(name)
    with pytest.raises(slc.SLSError) as ei:
        if name in sc.refused("masks"):
            slc.workloads.localization_masks_native(A, B2, c["d"], c["T"], c["alpha"], ctx=gpu_ctx)
        else:
            _localized_tables(slc, gpu_ctx, _plant(slc, name), c["d"], c["T"], c["alpha"], 0)
    assert ei.value.code == slc._capi.SLS_EUNSUPPORTED, ei.value
    _good_call(slc, gpu_ctx)


def test_band_solve_through_the_device_route_equals_the_mask_route_and_the_oracle(slc, gpu_ctx, oracle):
    """One solve, band65 (an actuator on every state): SLS_H2_localized equals SLS_H2 on the reference masks bit for bit, every
    column's status is OK, and a sample of columns — both edges, the interior, and one each at ñx = 63, 64, 65 — matches the
    SVD oracle at TOL = 1e-8."""
    c = sc.BY_NAME["band65"]
    P = _plant(slc, "band65")
    ref = sc.reference("band65")
    tb = sc.reference_tables("band65")
    S = [[M.astype(bool) for M in ref.Sx], [M.astype(bool) for M in ref.Su]]
    Lx, Lu, li = slc.SLS_H2_localized(P, c["d"], c["T"], c["alpha"], ctx=gpu_ctx, return_info=True, dropzeros=False)
    Mx, Mu, mi = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
    assert np.all(li["col_status"] == 0) and np.all(mi["col_status"] == 0)
    for a, b, R in zip(Lx + Lu, Mx + Mu, ref.Sx + ref.Su):
        assert np.array_equal(a.indptr, R.indptr) and np.array_equal(a.indices, R.indices)
        assert np.array_equal(b.indptr, R.indptr) and np.array_equal(b.indices, R.indices)
        assert np.array_equal(a.data, b.data)
    nx = tb["nx"]
    cols = [0, P.Nx - 1, P.Nx // 2] + [int(np.flatnonzero(nx == n)[0]) for n in (63, 64, 65)]
    assert [int(nx[q]) for q in cols[3:]] == [63, 64, 65]
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ox, ou = oracle.SLS_H2(Po, S, I=[[q] for q in cols])
    worst = 0.0
    for got, want in zip(Lx + Lu, ox + ou):
        g = sp.csc_matrix(got)[:, cols].toarray(); w = sp.csc_matrix(want)[:, cols].toarray()
        worst = max(worst, float(np.abs(g - w).max()))
    print(f"band65: worst |Φ − oracle| over columns {cols}: {worst:.2e}")
    assert worst < TOL
