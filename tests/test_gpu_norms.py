"""GPU tests of the closed-loop norms (csrc/sls_norms.hip, sls_norms_*): 𝓛₁ row / column sums and the power-iteration bound of
σ_max(G(ω)) per frequency, from a Φ that lives on the device.

References (tests/norms_cases.py, all in long double, sharing no code with the library): dense G[t] and G(ω); row and column
absolute sums; the same power iteration from the same v₀; σ_max by np.linalg.svd.  Tolerances: 𝓛₁ relative 4·(n + 2)·2⁻⁵³ with n
the longest row or column; σ parity HINF_RTOL = 64·2⁻⁵³ (8 × the deviation of a plain complex128 run is below that floor:
test_norms_host.py); σ_max relative 1e-9 at (ω, iters) whose convergence condition test_norms_host.py asserts.

Shapes: the row-length ladder (Nx 24, Nu 6, T 24: rows of 0 … 576 entries straddle every boundary of the 64 entry slots and of
the four-way unroll), T1, T2, Nu0, and HOLES (a row and a column without entries); the README chain end to end.

Largest relative error on an MI355X: 𝓛₁ sums 1.9e-16 (ladder; tolerance 2.6e-13) and 2.0e-16 weighted; σ against the long-double
iteration 2.4e-16 (T2; tolerance 7.1e-15), README chain 1.9e-16; σ against σ_max of the SVD 4.0e-16 (ladder, 320 iterations;
tolerance 1e-9).  (The tests print each figure before they assert: run with -s.)"""
import numpy as np
import pytest

import norms_cases as nc

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(_dev())        # a copy: fixtures are read-only


def _norms(slc, ctx, c, values=None, cz=None, b=None, max_freq=16):
    nrm = slc.ClosedLoopNorms((c.Nx, c.Nu), [c.Sx, c.Su], cz=cz, b=b, max_freq=max_freq, ctx=ctx)
    info = nrm.info
    assert info["n_entries"] == c.n_entries and info["max_freq"] == max_freq and info["device_bytes"] >= 28 * c.n_entries
    d_vals = _to_dev(c.values if values is None else values)
    nrm.load(d_vals)
    nrm._keep = d_vals
    return nrm


@pytest.fixture(scope="module")
def cases():
    return {name: nc.case(name) for name in nc.ALL}


@pytest.fixture(scope="module")
def parity_reference(cases):
    """long-double 𝓛₁ sums and σ of every case at PARITY_OMEGAS, computed once"""
    out = {}
    for name, c in cases.items():
        row, col = nc.l1_reference(nc.dense(c))
        out[name] = (row, col, nc.sigma_reference(c, nc.PARITY_OMEGAS, nc.PARITY_ITERS))
    return out


@pytest.mark.parametrize("name", nc.ALL)
def test_l1_on_every_case(slc, gpu_ctx, cases, parity_reference, name):
    import torch
    c = cases[name]
    row_ref, col_ref, _ = parity_reference[name]
    nrm = _norms(slc, gpu_ctx, c)
    row, col, tot = nrm.l1()
    er, ec = nc.rel(row, row_ref), nc.rel(col, col_ref)
    print(f"{name}: rel err row_l1 {er:.2e} col_l1 {ec:.2e} (tol {nc.l1_rtol(c):.2e})")
    assert er <= nc.l1_rtol(c) and ec <= nc.l1_rtol(c)
    assert tot[0] == row.max() and tot[1] == col.max()                  # bit for bit
    row2, col2, tot2 = nrm.l1()
    assert np.array_equal(row, row2) and np.array_equal(col, col2) and np.array_equal(tot, tot2)
    # the device-output form: the same bits, and NULL outputs are accepted
    d_row = torch.full((c.N,), float("nan"), dtype=torch.float64, device=_dev())
    d_col = torch.full((c.Nx,), float("nan"), dtype=torch.float64, device=_dev())
    d_tot = torch.full((2,), float("nan"), dtype=torch.float64, device=_dev())
    nrm.l1_async(d_row, d_col, d_tot)
    nrm.l1_async(None, None, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_row.cpu().numpy(), row) and np.array_equal(d_col.cpu().numpy(), col) and np.array_equal(d_tot.cpu().numpy(), tot)
    # a NaN written into one read entry: +inf in exactly its row and its column
    tables = slc.norms_tables((c.Nx, c.Nu), [c.Sx, c.Su])
    e = len(tables[1]) // 2
    i = int(np.searchsorted(tables[0], e, side="right")) - 1
    j = int(tables[1][e]) % c.Nx
    bad = np.array(c.values); bad[tables[2][e]] = np.nan
    d_bad = _to_dev(bad)
    nrm.load(d_bad)
    rowb, colb, totb = nrm.l1()
    assert np.array_equal(np.flatnonzero(np.isinf(rowb)), [i]) and np.array_equal(np.flatnonzero(np.isinf(colb)), [j])
    assert np.isposinf(rowb[i]) and np.isposinf(colb[j]) and np.isposinf(totb).all()
    keep = np.ones(c.N, dtype=bool); keep[i] = False
    keepc = np.ones(c.Nx, dtype=bool); keepc[j] = False
    assert np.array_equal(rowb[keep], row[keep]) and np.array_equal(colb[keepc], col[keepc])
    nrm.close()


def test_hinf_lane_layouts_on_the_ladder(slc, gpu_ctx, cases):
    """nfreq = 1 … 65 with max_freq = 65: every SCN class (1, 2, 4, … 64), each with dead lanes, and a second frequency chunk.
    The sigma of a frequency does not depend on the call, the SCN class or the slot it sat in: bit for bit across the nine calls
    (the call of 64 passes its angles in reverse order, so that every frequency changes its slot)."""
    c = cases["ladder"]
    om = np.array(nc.LAYOUT_OMEGAS)
    nrm = _norms(slc, gpu_ctx, c, max_freq=nc.LAYOUT_MAX_FREQ)
    full, peak, arg = nrm.hinf(om, iters=nc.LAYOUT_ITERS)
    assert np.isfinite(full).all() and full.min() > 1.0 and len(np.unique(full)) > 40
    assert peak == full.max() and arg == int(np.argmax(full))
    for nf in nc.LAYOUT_NFREQ:
        sel = np.arange(nf)[::-1] if nf == 64 else np.arange(nf)
        s, pk, ar = nrm.hinf(om[sel], iters=nc.LAYOUT_ITERS)
        assert np.array_equal(s, full[sel]), nf
        assert pk == s.max() and ar == int(np.argmax(s)), nf
    ref = nc.sigma_reference(c, om[:9], nc.LAYOUT_ITERS)
    e = nc.rel(full[:9], ref)
    print(f"ladder layouts: rel err of sigma against the long-double iteration {e:.2e} (tol {nc.HINF_RTOL:.2e})")
    assert e <= nc.HINF_RTOL
    nrm.close()


@pytest.mark.parametrize("name", nc.ALL)
def test_sigma_parity_and_structure(slc, gpu_ctx, cases, parity_reference, name):
    """Against the long-double iteration at the same iters; ω = 0 and ω = π against the iteration on the REAL matrices Σ G[t] and
    Σ (−1)ᵗ G[t]; σ(−ω) = σ(ω) bit for bit; non-decreasing over iters = 1, 2, 4, 8 up to one rounding of the final norm."""
    c = cases[name]
    nrm = _norms(slc, gpu_ctx, c)
    s, _, _ = nrm.hinf(nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS)
    e = nc.rel(s, parity_reference[name][2])
    G0, Gpi = nc.real_matrices(c)
    real = [nc.power_iteration(G.astype(nc.CL), nc.PARITY_ITERS) for G in (G0, Gpi)]
    er = nc.rel(s[:2], real)
    print(f"{name}: rel err of sigma {e:.2e}, of ω = 0, π against the real matrices {er:.2e} (tol {nc.HINF_RTOL:.2e})")
    assert e <= nc.HINF_RTOL and er <= nc.HINF_RTOL
    om = list(nc.PARITY_OMEGAS)
    assert s[om.index(0.3)] == s[om.index(-0.3)] and s[om.index(2.0)] == s[om.index(-2.0)]
    runs = [nrm.hinf(nc.MONOTONE_OMEGAS, iters=k)[0] for k in nc.MONOTONE_ITERS]
    for a, b in zip(runs, runs[1:]):
        assert np.all(b >= a * (1 - 2.0 ** -52)), (name, a, b)
    assert np.all(runs[-1] > runs[0])
    nrm.close()


@pytest.mark.parametrize("name", nc.ALL)
def test_sigma_against_the_svd(slc, gpu_ctx, cases, name):
    c = cases[name]
    om, iters = nc.SVD_OMEGAS[name], nc.SVD_ITERS[name]
    nrm = _norms(slc, gpu_ctx, c)
    s, peak, arg = nrm.hinf(om, iters=iters)
    top = np.array([nc.svd_top2(c, w)[0] for w in om])
    e = nc.rel(s, top)
    print(f"{name}: iters {iters}, rel err against σ_max {e:.2e}")
    assert e <= nc.SVD_RTOL
    assert peak == s.max() and arg == int(np.argmax(s))
    nrm.close()


def test_edges(slc, gpu_ctx, cases):
    import torch
    # T = 1: G = [diag(d)·w; Φu[0]·w] for every ω — the state rows in closed form, sigma independent of ω
    c = cases["T1"]
    cz, b = nc.weights(c)
    nrm = _norms(slc, gpu_ctx, c, cz=cz, b=b)
    row, col, tot = nrm.l1()
    d = c.values[:c.Nx]
    assert np.array_equal(row[:c.Nx], np.abs(d * (cz[:c.Nx] * b)))
    s, _, _ = nrm.hinf([0.0, 0.4, -2.2, np.pi], iters=5)
    assert len(set(s)) == 1
    G = nc.dense(c, cz, b)
    assert nc.rel(s[:1], [nc.power_iteration(G[0].astype(nc.CL), 5)]) <= nc.HINF_RTOL
    nrm.close()
    # a row and a column with no stored-true entry: exactly 0, and the iteration is unharmed
    h = cases["HOLES"]
    nrm = _norms(slc, gpu_ctx, h)
    row, col, _ = nrm.l1()
    assert row[nc.HOLES_EMPTY_ROW_X] == 0 and row[h.Nx + nc.HOLES_EMPTY_ROW_U] == 0 and col[nc.HOLES_EMPTY_COL] == 0
    assert np.count_nonzero(row == 0) == 2 and np.count_nonzero(col == 0) == 1
    # load of a second Φ changes the result and leaves nothing of the first behind: a fresh object gives the same bits
    s1 = nrm.hinf(nc.PARITY_OMEGAS, iters=3)[0]
    second = np.array(h.values) * np.where(np.arange(len(h.values)) % 2 == 0, 0.5, -1.5)
    d_second = _to_dev(second)
    nrm.load(d_second)
    row2, col2, tot2 = nrm.l1()
    s2 = nrm.hinf(nc.PARITY_OMEGAS, iters=3)[0]
    assert not np.array_equal(row2, row) and not np.array_equal(s2, s1)
    fresh = _norms(slc, gpu_ctx, h, values=second)
    rowf, colf, totf = fresh.l1()
    assert np.array_equal(rowf, row2) and np.array_equal(colf, col2) and np.array_equal(totf, tot2)
    assert np.array_equal(fresh.hinf(nc.PARITY_OMEGAS, iters=3)[0], s2)
    fresh.close(); nrm.close()
    # device outputs of hinf: the same bits as the fetch, NULL outputs accepted
    lad = cases["ladder"]
    nrm = _norms(slc, gpu_ctx, lad)
    s, pk, ar = nrm.hinf(nc.PARITY_OMEGAS, iters=2)
    d_s = torch.full((len(nc.PARITY_OMEGAS),), float("nan"), dtype=torch.float64, device=_dev())
    d_p = torch.full((2,), float("nan"), dtype=torch.float64, device=_dev())
    nrm.hinf_async(nc.PARITY_OMEGAS, iters=2, sigma=d_s, peak=d_p)
    nrm.hinf_async(nc.PARITY_OMEGAS, iters=2)
    torch.cuda.synchronize()
    assert np.array_equal(d_s.cpu().numpy(), s) and np.array_equal(d_p.cpu().numpy(), [pk, float(ar)])
    nrm.close()


def test_hinf_twiddles_without_the_pinned_buffer(slc, gpu_ctx, cases, monkeypatch):
    """With SLS_PAGEABLE_D2H=1 no pinned buffer is handed out: the twiddles are copied from a pageable array and waited for, and
    the results come straight into the caller's arrays.  σ, peak and argmax equal bitwise those of the run through the pinned buffer.
    T2 is the smallest case whose twiddles are not all 1 (T1: t = 0 only)."""
    monkeypatch.delenv("SLS_PAGEABLE_D2H", raising=False)
    nrm = _norms(slc, gpu_ctx, cases["T2"])
    try:
        s, pk, ar = nrm.hinf(nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS)
        assert len(set(s)) > 1
        monkeypatch.setenv("SLS_PAGEABLE_D2H", "1")
        s2, pk2, ar2 = nrm.hinf(nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS)
        assert np.array_equal(s2, s) and pk2 == pk and ar2 == ar
    finally:
        nrm.close()


@pytest.mark.parametrize("name", ["ladder", "Nu0", "HOLES"])
def test_weights_against_prescaled_values(slc, gpu_ctx, cases, name):
    """cz, b random positive against NULL weights on values pre-scaled on the host: one multiply per entry apart.  Both against
    the long-double reference as well."""
    c = cases[name]
    cz, b = nc.weights(c, seed=3)
    wtd = _norms(slc, gpu_ctx, c, cz=cz, b=b)
    pre = _norms(slc, gpu_ctx, c, values=nc.prescale(c, cz, b))
    rw, cw, tw = wtd.l1()
    rp, cp, tp = pre.l1()
    tol = 4 * nc.U                                                      # (cz·b)·Φ on both sides: the same two roundings
    assert nc.rel(rw, rp) <= tol and nc.rel(cw, cp) <= tol and nc.rel(tw, tp) <= tol
    sw, sp_ = wtd.hinf(nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS)[0], pre.hinf(nc.PARITY_OMEGAS, iters=nc.PARITY_ITERS)[0]
    assert nc.rel(sw, sp_) <= nc.HINF_RTOL
    G = nc.dense(c, cz, b)
    row, col = nc.l1_reference(G)
    e = nc.rel(sw, nc.sigma_reference(c, nc.PARITY_OMEGAS, nc.PARITY_ITERS, cz, b))
    print(f"{name} weighted: rel err row_l1 {nc.rel(rw, row):.2e} col_l1 {nc.rel(cw, col):.2e} sigma {e:.2e}")
    assert nc.rel(rw, row) <= nc.l1_rtol(c) and nc.rel(cw, col) <= nc.l1_rtol(c) and e <= nc.HINF_RTOL
    wtd.close(); pre.close()


def test_readme_chain_end_to_end(slc, gpu_ctx, readme):
    """Plan.execute → ClosedLoopNorms.from_plant(...).load of that same device array; l1 and hinf on 16 frequencies against the
    dense reference built from the downloaded Φ.  Φx[0] = I puts a 1 into every column, so the 𝓔₁ norm is at least 1."""
    P, S, _ = readme
    plan = slc.Plan(gpu_ctx, P, S)
    d = plan.alloc_values()
    plan.execute(d); plan.synchronize()
    assert np.all(plan.fetch_status()[0] == 0)
    nrm = slc.ClosedLoopNorms.from_plant(P, S[0], S[1], max_freq=16, ctx=gpu_ctx).load(d)
    row, col, tot = nrm.l1()
    om = np.linspace(0.0, np.pi, 16)
    s, peak, arg = nrm.hinf(om, iters=nc.PARITY_ITERS)
    vx, vu = plan.download(d)
    c = nc.from_values(S[0], S[1], np.concatenate(vx + vu))
    assert nrm.info["n_entries"] == c.n_entries
    G = nc.dense(c)                                                     # Plant(A, B1, B2): [C1 D12] = I, B1 = I
    row_ref, col_ref = nc.l1_reference(G)
    er, ec = nc.rel(row, row_ref), nc.rel(col, col_ref)
    es = nc.rel(s, nc.sigma_reference(c, om, nc.PARITY_ITERS))
    print(f"README chain: 𝓛₁ {tot[0]:.6f} 𝓔₁ {tot[1]:.6f} peak {peak:.6f} at ω = {om[arg]:.4f}; rel err row_l1 {er:.2e} col_l1 {ec:.2e} "
          f"(tol {nc.l1_rtol(c):.2e}) sigma {es:.2e} (tol {nc.HINF_RTOL:.2e})")
    assert er <= nc.l1_rtol(c) and ec <= nc.l1_rtol(c) and es <= nc.HINF_RTOL
    assert tot[0] == row.max() and tot[1] == col.max() and tot[1] >= 1.0
    assert peak == s.max() and arg == int(np.argmax(s))
    nrm.close(); plan.close()


def test_error_paths_leave_the_object_usable(slc, gpu_ctx, cases):
    c = cases["T2"]
    EINVAL = slc._capi.SLS_EINVAL
    nrm = slc.ClosedLoopNorms((c.Nx, c.Nu), [c.Sx, c.Su], max_freq=4, ctx=gpu_ctx)
    for call in (lambda: nrm.hinf([0.1], iters=2), lambda: nrm.l1()):   # before the first load
        with pytest.raises(slc.SLSError) as e:
            call()
        assert e.value.code == EINVAL
    d_vals = _to_dev(c.values)
    nrm.load(d_vals)
    good = nrm.hinf([0.1, 0.2], iters=2)[0]
    for kw in (dict(omega=[0.1] * 5, iters=2), dict(omega=[0.1], iters=0), dict(omega=[0.1, np.inf], iters=2),
               dict(omega=[np.nan], iters=2), dict(omega=np.zeros(0), iters=2)):
        with pytest.raises(slc.SLSError) as e:
            nrm.hinf(**kw)
        assert e.value.code == EINVAL
        assert np.array_equal(nrm.hinf([0.1, 0.2], iters=2)[0], good)   # still usable, same bits
    for kw in (dict(max_freq=0), dict(dev_slot=7), dict(cz=np.full(c.N, np.inf)), dict(b=np.full(c.Nx, np.nan))):
        with pytest.raises(slc.SLSError) as e:
            slc.ClosedLoopNorms((c.Nx, c.Nu), [c.Sx, c.Su], ctx=gpu_ctx, **kw)
        assert e.value.code == EINVAL
    nrm.close()
