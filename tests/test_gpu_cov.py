"""GPU tests of the 𝓗₂ shares and the covariance entries of a resident Φ (csrc/sls_norms.hip: sls_norms_h2, sls_norms_cov_pattern,
sls_norms_cov and their fetch forms).

Reference (tests/cov_cases.py): the dense long-double Σ = Σ_t G[t]·G[t]ᵀ of the case, sharing no code with the library.
Tolerances, derived there: row_h2 / col_h2 relative 4·(n + 2)·2⁻⁵³ with n the longest row or column; cov[p] absolute
4·(n_p + 3)·2⁻⁵³·Σ_k |G_i,k·G_j,k| with n_p the number of shared keys (0 shared keys: exactly 0.0); totals[0] relative
4·(n_entries + N + 2)·2⁻⁵³.  The host twin is held to the same bounds.

Shapes: the row-length ladder (Nx 24, Nu 6, T 24: rows of 0 … 576 entries, so pairs straddle every boundary of the 64-entry
chunks and either list can be the shorter one), T1, T2, Nu0, HOLES (empty rows and an empty column); the README chain end to
end; one list longer than the largest grid, so that a wave takes more than one pair.

Largest errors on an MI355X: row_h2 / col_h2 5.8e-16 relative (weighted ladder; tolerance 2.6e-13), totals[0] 2.2e-16 (tolerance
1.3e-12), cov 0.122 of its tolerance (weighted Nu0) and 0.090 of it against the twin; README chain col_h2 against the objective
values 3.8e-16 (tolerance 3.0e-13), covariance on the neighbour pattern 0.002 of its tolerance.  (The tests print each figure
before they assert: run with -s.)"""
import ctypes as C

import numpy as np
import pytest

import cov_cases as cc
import norms_cases as nc

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(_dev())        # a copy: fixtures are read-only


def _norms(slc, ctx, c, values=None, cz=None, b=None, load=True):
    nrm = slc.ClosedLoopNorms((c.Nx, c.Nu), [c.Sx, c.Su], cz=cz, b=b, max_freq=2, ctx=ctx)
    if load:
        nrm._keep = _to_dev(c.values if values is None else values)
        nrm.load(nrm._keep)
    return nrm


def _cov(nrm, pi, pj):
    return nrm.set_covariance_pattern(pi, pj).covariance()


@pytest.fixture(scope="module")
def cases():
    return {name: nc.case(name) for name in cc.ALL}


@pytest.fixture(scope="module")
def references(cases):
    """the long-double Σ of every case, unweighted and with the weights of norms_cases.weights, computed once"""
    return {(name, w): cc.reference(c, *(nc.weights(c) if w else (None, None))) for name, c in cases.items() for w in (False, True)}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", cc.ALL)
def test_h2_and_covariance_on_every_case(slc, gpu_ctx, cases, references, name, weighted):
    import torch
    c, ref = cases[name], references[name, weighted]
    cz, b = nc.weights(c) if weighted else (None, None)
    dims, S = (c.Nx, c.Nu), [c.Sx, c.Su]
    nrm = _norms(slc, gpu_ctx, c, cz=cz, b=b)
    row, col, tot = nrm.h2()
    hrow, hcol, htot = slc.norms_h2_host(dims, S, c.values, cz=cz, b=b)
    er, ec, et = nc.rel(row, ref.row), nc.rel(col, ref.col), nc.rel(tot[:1], [ref.row.sum()])
    tr, tc, tt = nc.rel(row, hrow), nc.rel(col, hcol), nc.rel(tot[:1], htot[:1])
    print(f"{name} weighted={weighted}: rel err row_h2 {er:.2e} col_h2 {ec:.2e} (twin {tr:.2e} {tc:.2e}; tol {cc.h2_rtol(c):.2e}) "
          f"total {et:.2e} (twin {tt:.2e}; tol {cc.total_rtol(c):.2e})")
    assert max(er, ec, tr, tc) <= cc.h2_rtol(c) and max(et, tt) <= cc.total_rtol(c)
    assert tot[1] == row.max()                                          # bit for bit
    row2, col2, tot2 = nrm.h2()
    assert np.array_equal(row, row2) and np.array_equal(col, col2) and np.array_equal(tot, tot2)
    d_row = torch.full((c.N,), float("nan"), dtype=torch.float64, device=_dev())
    d_col = torch.full((c.Nx,), float("nan"), dtype=torch.float64, device=_dev())
    d_tot = torch.full((2,), float("nan"), dtype=torch.float64, device=_dev())
    nrm.h2_async(d_row, d_col, d_tot)
    nrm.h2_async(None, None, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_row.cpu().numpy(), row) and np.array_equal(d_col.cpu().numpy(), col) and np.array_equal(d_tot.cpu().numpy(), tot)
    l1 = nrm.l1()                                                       # the two passes share result slots, not results
    assert not np.array_equal(l1[0], row) and np.array_equal(nrm.h2()[0], row) and np.array_equal(nrm.l1()[0], l1[0])
    got = {}
    for key, (pi, pj) in cc.pair_lists(c).items():
        got[key] = _cov(nrm, pi, pj)
        twin = slc.norms_cov_host(dims, S, c.values, pi, pj, cz=cz, b=b)
        e = cc.cov_error(got[key], ref, pi, pj)
        te = float((np.abs(got[key] - twin) / np.maximum(np.asarray(cc.cov_atol(ref, pi, pj), dtype=float), 1e-300)).max())
        print(f"  {key}: {len(pi)} pairs, worst error / tolerance {e:.3f} (against the twin {te:.3f})")
        assert e <= 1.0 and te <= 1.0
        assert np.array_equal(nrm.covariance(), got[key])              # call to call
        d_cov = torch.full((len(pi),), float("nan"), dtype=torch.float64, device=_dev())
        nrm.covariance_async(d_cov)
        torch.cuda.synchronize()
        assert np.array_equal(d_cov.cpu().numpy(), got[key])
    assert np.array_equal(got["reversed"], got["all"][::-1])           # (j, i) and (i, j): the same bits
    i, j = cc.pair_lists(c)["all"]
    diag = i == j                                                       # cov(i, i) against row_h2[i], the two tolerances added
    tol = cc.h2_rtol(c) * np.asarray(ref.row, dtype=float) + np.asarray(cc.cov_atol(ref, i[diag], j[diag]), dtype=float)
    assert np.all(np.abs(got["all"][diag] - row) <= tol)
    nrm.close()


def test_a_pair_does_not_depend_on_its_list(slc, gpu_ctx, cases):
    """alone, first, last, between duplicates of itself, in either order: the same bits as in the list of all pairs"""
    c = cases["ladder"]
    nrm = _norms(slc, gpu_ctx, c)
    i, j = cc.all_pairs(c)
    full = _cov(nrm, i, j)
    order = np.argsort(c.row_len)
    e = int(cc.empty_rows(c)[0])
    probes = [(int(order[-1]), int(order[-2])), (int(order[-1]), int(order[3])), (int(order[-3]), int(order[-3])),
              (int(order[len(order) // 2]), int(order[len(order) // 2 + 1])), (e, int(order[-1]))]
    k = len(i) // 2
    for a, b in probes:
        want = full[(i == min(a, b)) & (j == max(a, b))]
        assert want.shape == (1,)
        for x, y in ((a, b), (b, a)):
            assert np.array_equal(_cov(nrm, [x], [y]), want)
            assert _cov(nrm, np.concatenate([[x], i]), np.concatenate([[y], j]))[0] == want[0]
            assert _cov(nrm, np.concatenate([i, [x]]), np.concatenate([j, [y]]))[-1] == want[0]
            mid = _cov(nrm, np.concatenate([i[:k], [x, y, x], i[k:]]), np.concatenate([j[:k], [y, x, y], j[k:]]))
            assert np.all(mid[k:k + 3] == want[0]) and np.array_equal(np.delete(mid, [k, k + 1, k + 2]), full)
    nrm.close()


def test_disjoint_and_empty_rows_give_exactly_zero(slc, gpu_ctx, cases, references):
    c = cases["T1"]                                                     # T = 1: a state row holds its diagonal entry alone
    nrm = _norms(slc, gpu_ctx, c)
    s = np.arange(c.Nx)
    z = _cov(nrm, s[:-1], s[1:])
    assert z.shape == (c.Nx - 1,) and not np.any(z) and not np.any(np.signbit(z))
    v = c.values[:c.Nx]
    assert np.array_equal(_cov(nrm, s, s), v * v)
    nrm.close()
    for name in ("HOLES", "ladder"):
        c = cases[name]
        nrm = _norms(slc, gpu_ctx, c)
        i, j = cc.all_pairs(c)
        got = _cov(nrm, i, j)
        none = references[name, False].shared[i, j] == 0
        assert none.sum() > len(cc.empty_rows(c)) * c.N / 2 and not np.any(got[none]) and np.all(got[~none] != 0)
        row, col, _ = nrm.h2()
        assert np.array_equal(np.flatnonzero(row == 0), cc.empty_rows(c)) and np.array_equal(col == 0, c.col_len == 0)
        nrm.close()


@pytest.mark.parametrize("name", ["ladder", "HOLES"])
def test_a_nan_reaches_its_row_its_column_and_the_pairs_that_share_its_key(slc, gpu_ctx, cases, name):
    c = cases[name]
    nrm = _norms(slc, gpu_ctx, c)
    i, j = cc.all_pairs(c)
    row, col, tot = nrm.h2()
    good = _cov(nrm, i, j)
    tables = slc.norms_tables((c.Nx, c.Nu), [c.Sx, c.Su])
    e = len(tables[1]) // 2
    r = int(np.searchsorted(tables[0], e, side="right")) - 1
    key = int(tables[1][e])
    bad = np.array(c.values); bad[tables[2][e]] = np.nan
    nrm._keep = _to_dev(bad)
    nrm.load(nrm._keep)
    rowb, colb, totb = nrm.h2()
    assert np.array_equal(np.flatnonzero(np.isinf(rowb)), [r]) and np.array_equal(np.flatnonzero(np.isinf(colb)), [key % c.Nx])
    assert np.isposinf(rowb[r]) and np.isposinf(colb[key % c.Nx]) and np.isposinf(totb).all()
    keep = np.arange(c.N) != r
    keepc = np.arange(c.Nx) != key % c.Nx
    assert np.array_equal(rowb[keep], row[keep]) and np.array_equal(colb[keepc], col[keepc])
    covb = nrm.covariance()
    has = np.array([key in tables[1][tables[0][q]:tables[0][q + 1]] for q in range(c.N)])
    hit = ((i == r) & has[j]) | ((j == r) & has[i])
    assert hit.sum() > 1 and np.array_equal(np.isnan(covb), hit) and np.array_equal(covb[~hit], good[~hit])
    nrm.close()


def test_replacing_the_pattern(slc, gpu_ctx, cases, references):
    """a longer pattern, then a shorter one, then none: correct results each time, and device_bytes follows (16 B per pair in two
    buffers rounded to 256 B); an object without a pattern reports what it did before the feature"""
    c, ref = cases["ladder"], references["ladder", False]
    nrm = _norms(slc, gpu_ctx, c)
    base = nrm.info["device_bytes"]
    i, j = cc.all_pairs(c)
    al = lambda n: 2 * ((8 * n + 255) // 256 * 256)
    for n in (7, len(i), 40, 1):
        got = _cov(nrm, i[:n], j[:n])
        assert got.shape == (n,) and cc.cov_error(got, ref, i[:n], j[:n]) <= 1.0
        assert nrm.info["device_bytes"] == base + al(n)
    nrm.set_covariance_pattern([], [])
    assert nrm.info["device_bytes"] == base and nrm.npairs == 0
    with pytest.raises(slc.SLSError) as e:
        nrm.covariance()
    assert e.value.code == slc._capi.SLS_EINVAL
    assert cc.cov_error(_cov(nrm, i[5:9], j[5:9]), ref, i[5:9], j[5:9]) <= 1.0
    nrm.close()


def test_more_pairs_than_the_largest_grid(slc, gpu_ctx, cases, references):
    """2²⁴ + 5 pairs: the grid stops at 2²² blocks of four waves, so the first waves take a second pair.  Every entry equals the
    value the same pair has in a short list, bit for bit."""
    c, ref = cases["T2"], references["T2", False]
    nrm = _norms(slc, gpu_ctx, c)
    i, j = cc.all_pairs(c)
    short = _cov(nrm, i, j)
    assert cc.cov_error(short, ref, i, j) <= 1.0
    n = (1 << 24) + 5
    sel = (np.arange(n, dtype=np.int64) * 7) % len(i)
    got = _cov(nrm, i[sel], j[sel])
    assert got.shape == (n,) and np.array_equal(got, short[sel])
    nrm.close()


def test_readme_chain_end_to_end(slc, gpu_ctx, readme):
    """Plan.execute → ClosedLoopNorms.from_plant(...).load of that same device array.  col_h2 is the objective value of every
    column (default weights: [C1 D12] = I, B1 = I), totals[0] the objective total; the covariance on the neighbour pattern of the
    plant against the dense reference built from the downloaded Φ."""
    P, S, _ = readme
    plan = slc.Plan(gpu_ctx, P, S)
    d = plan.alloc_values()
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == slc._capi.SLS_COL_OK)
    obj, obj_total = plan.objective_values(d)
    nrm = slc.ClosedLoopNorms.from_plant(P, S[0], S[1], max_freq=1, ctx=gpu_ctx).load(d)
    row, col, tot = nrm.h2()
    vx, vu = plan.download(d)
    c = nc.from_values(S[0], S[1], np.concatenate(vx + vu))
    ref = cc.reference(c)
    er, ec, et = nc.rel(row, ref.row), nc.rel(col, ref.col), nc.rel(tot[:1], [ref.row.sum()])
    eo, eto = nc.rel(col, obj), nc.rel(tot[:1], [obj_total])
    print(f"README chain: ‖·‖²_𝓗₂ {tot[0]:.6f}, largest variance {tot[1]:.6f}; rel err row_h2 {er:.2e} col_h2 {ec:.2e} (tol {cc.h2_rtol(c):.2e}) "
          f"total {et:.2e} (tol {cc.total_rtol(c):.2e}); col_h2 against the objective values {eo:.2e}, total {eto:.2e}")
    assert len(obj) == c.Nx
    assert max(er, ec, eo) <= cc.h2_rtol(c) and max(et, eto) <= cc.total_rtol(c)
    assert tot[1] == row.max()
    pi, pj = slc.covariance_pattern_of(P)
    assert len(pi) == 2 * c.Nx - 1 + c.Nu                               # a chain: the diagonal, the first off-diagonal, the inputs
    cov = nrm.set_covariance_pattern(pi, pj).covariance()
    e = cc.cov_error(cov, ref, pi, pj)
    print(f"  covariance on the neighbour pattern: {len(pi)} pairs, worst error / tolerance {e:.3f}")
    assert e <= 1.0
    nrm.close(); plan.close()


def test_error_paths_leave_the_object_usable(slc, gpu_ctx, cases, references):
    """every refusal happens on the host before anything is enqueued: the documented code, and a correct call afterwards"""
    import torch
    c, ref = cases["T2"], references["T2", False]
    EINVAL, EUNSUPPORTED = slc._capi.SLS_EINVAL, slc._capi.SLS_EUNSUPPORTED
    i, j = cc.all_pairs(c)
    nrm = _norms(slc, gpu_ctx, c, load=False)
    base = nrm.info["device_bytes"]
    nrm.set_covariance_pattern(i, j)                                    # a pattern may come before the first load
    d_out = torch.zeros(len(i), dtype=torch.float64, device=_dev())
    for call in (lambda: nrm.covariance(), lambda: nrm.covariance_async(d_out), lambda: nrm.h2(), lambda: nrm.h2_async()):
        with pytest.raises(slc.SLSError, match="no Φ loaded") as e:     # before the first load
            call()
        assert e.value.code == EINVAL
    nrm._keep = _to_dev(c.values)
    nrm.load(nrm._keep)
    good = nrm.covariance()
    assert cc.cov_error(good, ref, i, j) <= 1.0
    lib, ip = slc.load_library(), C.POINTER(C.c_int64)
    one = np.zeros(1, dtype=np.int64)
    bad_lists = (([0, c.N], [0, 0], 1), ([0, 1, 2], [0, -1, 2], 1), ([c.N + 7], [0], 0))
    for pi, pj, at in bad_lists:                                        # an index out of range: the pattern in place is kept
        with pytest.raises(slc.SLSError, match=f"pair {at} ") as e:
            nrm.set_covariance_pattern(pi, pj)
        assert e.value.code == EINVAL
        assert nrm.npairs == len(i) and np.array_equal(nrm.covariance(), good)
    assert lib.sls_norms_cov_pattern(nrm.handle, -1, one.ctypes.data_as(ip), one.ctypes.data_as(ip)) == EINVAL
    assert lib.sls_norms_cov_pattern(nrm.handle, 1, None, one.ctypes.data_as(ip)) == EINVAL
    assert lib.sls_norms_cov_pattern(nrm.handle, 1 << 31, one.ctypes.data_as(ip), one.ctypes.data_as(ip)) == EUNSUPPORTED
    assert lib.sls_norms_cov(nrm.handle, None, None) == EINVAL and "null output" in slc._capi.last_error(gpu_ctx.handle)
    assert lib.sls_norms_cov(None, None, d_out.data_ptr()) == EINVAL
    assert nrm.info["device_bytes"] > base and np.array_equal(nrm.covariance(), good)
    with pytest.raises(ValueError):
        nrm.set_covariance_pattern([0, 1], [0])
    with pytest.raises(ValueError):
        nrm.covariance_async(torch.zeros(len(i) + 1, dtype=torch.float64, device=_dev()))
    assert lib.sls_norms_fetch_cov(nrm.handle, None, None) == 0         # a NULL host array: the pass runs, nothing is copied
    nrm.set_covariance_pattern([], [])                                  # no pattern: refused, then usable again
    with pytest.raises(slc.SLSError, match="no pattern") as e:
        nrm.covariance_async(d_out.data_ptr())
    assert e.value.code == EINVAL
    assert np.array_equal(_cov(nrm, i, j), good)
    nrm.covariance_async(d_out)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), good)
    row, col, tot = nrm.h2()
    assert nc.rel(row, ref.row) <= cc.h2_rtol(c)
    nrm.close()
