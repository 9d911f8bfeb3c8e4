"""Four-wave twisted kernel, off the factor chain: the setup images built at plan time, the helpers' first static block requested
in the setup, and the downward sweeps of the later passes taking their weights from the table.

What moved: (1) with plan-time static blocks the launch no longer builds the dense image `Ad` of Ã and the weight table `wxt`
(Wx_k = mask_k ⊙ H⁻¹ for every block k): twisted4_prepare_kernel writes both next to the static blocks and the launch copies them;
the rebuild instantiation (SLS_T4_PRESTATIC=0 in lab mode) still builds them in the launch and is the bit-exact reference.
(2) In the three-tile classes `elim_down` and `middle` read the weight from `wxt`, and a downward outward step writes
tmp = Wx_k·Δλ_k together with rq[k] for its successor.  No arithmetic changed: every comparison between the two
instantiations, between two executes and between a subset and a full run is on bit patterns.

What can go wrong: an image indexed by the wrong launch position (column subset, several columns per launch), an image left
stale by a plant update, padding of the images (rows ñx … 8·TR − 1 of `Ad`, row T and the entries beyond ñx of `wxt`), a weight
row off by one block in a sweep (shows where the masks still grow at the meeting block and on weighted columns), a `tmp` entry
of the downward outward sweep that its predecessor did not write (shows on second passes), the four-tile path.

Cases, plants, masks and bounds are those of test_gpu_twisted4_tilesweep.py (its header derives them): against the two-wave
kernel equal statuses and pass counts and |ΔΦ| < 1e-9, the default-weight cases against the C oracle at TOL.

A third part was measured and taken out: output destinations staged in LDS.  The output pass reads the
plan's table as before, so there is no staging limit to test.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_c import TOL
from test_gpu_twisted4_prepared import _index_sets, _masks_of
from test_gpu_twisted4_tilesweep import CASES, FOUR, TWO, NCU, _case, _run, _execute_into_nan

BIT_CASES = ("c10_T7", "c12_mix", "c12_top24", "c10_T17_mix", "load_path", "weighted", "four_tile")
IMAGE_CASES = ("c10_T17_mix", "weighted")
SUBSET_CASE, SUBSET = "c10_T17_mix", [1, 3]

_runs = {}


def _both(slc, gpu_ctx, cid, monkeypatch):
    """The case under the default plan (plan-time blocks and images), the rebuild instantiation and the two-wave kernel: run once."""
    if cid not in _runs:
        P, S, cols, cls, want, _ = _case(slc, cid)
        out = {}
        for key, env, name in (("pre", {}, FOUR + cls), ("rebuild", {"SLS_T4_PRESTATIC": "0"}, FOUR + cls), ("two", {"SLS_TWISTED4": "0"}, TWO + "<")):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
                try:
                    desc = plan.describe()
                    assert name in desc and desc.count(";") == 1, desc
                    if key == "pre":
                        plan.twisted4_images()                      # the default plan keeps the images …
                    elif key == "rebuild":
                        with pytest.raises(slc._capi.SLSError):     # … the rebuild plan none
                            plan.twisted4_images()
                    res = _run(plan)
                finally:
                    plan.close()
            for a in res:
                a.setflags(write=False)
            out[key] = res
        _runs[cid] = out
    return _runs[cid]


def _weights(P, sx):
    """H⁻¹ on the state rows of a column (diagonal C1, unit B1): 1 / c_i²; ones under the default weights."""
    if P.default_weights:
        return np.ones(len(sx))
    c1 = np.asarray(sp.csc_matrix(P.C1)[:P.Nx, :].diagonal())[sx]
    return 1.0 / (c1 * c1)


def _images(P, S, c, TR):
    sx, su = _index_sets(P, S, c)
    n, T = len(sx), len(S[0])
    Ad = np.zeros((8 * TR, 40))
    Ad[:n, :n] = sp.csr_matrix(sp.csc_matrix(P.A))[sx][:, sx].toarray()
    wxt = np.zeros((T + 1, 32))
    wxt[:T, :n] = _masks_of(S, c, sx, su)[:, :n] * _weights(P, sx)
    return Ad, wxt


# ---- host (no GPU) ----

def test_cases_are_those_of_the_tilesweep_table(slc):
    assert set(BIT_CASES) <= set(CASES) and set(IMAGE_CASES) <= set(BIT_CASES) and SUBSET_CASE in BIT_CASES
    assert len(CASES[SUBSET_CASE][4]) > len(SUBSET) and SUBSET[0] > 0
    P, S, cols, cls, _, _ = _case(slc, "weighted")
    assert not P.default_weights and _case(slc, "c10_T17_mix")[0].default_weights
    assert np.array_equal(sp.csc_matrix(P.B1).toarray(), np.eye(P.Nx))          # the unit column scale `_weights` assumes
    desc = slc.dist.describe_launches(P, S, [[c] for c in cols], None, NCU)
    assert desc.startswith(FOUR + cls), desc


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("cid", BIT_CASES)
def test_plan_time_images_give_the_bits_of_the_rebuild(slc, gpu_ctx, cid, monkeypatch):
    r = _both(slc, gpu_ctx, cid, monkeypatch)
    (got, st, rs, it), (got0, st0, rs0, it0) = r["pre"], r["rebuild"]
    print(f"{cid}: status {st.tolist()} passes {it.tolist()} residual {rs.max():.1e}; max |Φ − Φ_rebuild| = {np.abs(got - got0).max():.2e}")
    assert np.array_equal(got.view(np.uint64), got0.view(np.uint64))
    assert np.array_equal(st, st0) and np.array_equal(it, it0)
    assert np.array_equal(rs.view(np.uint64), rs0.view(np.uint64))
    if cid == "load_path":
        assert it.max() >= 2, it                                    # every non-fused sweep ran twice


@pytest.mark.gpu
@pytest.mark.parametrize("cid", BIT_CASES)
def test_against_two_wave_kernel_and_oracle(slc, gpu_ctx, cid, monkeypatch):
    want = _case(slc, cid)[4]
    r = _both(slc, gpu_ctx, cid, monkeypatch)
    (got, st, rs, it), (ref, st2, rs2, it2) = r["pre"], r["two"]
    dev = np.abs(got - ref).max()
    err = np.abs(got - want).max() if want is not None else float("nan")
    print(f"{cid}: status {st.tolist()} / {st2.tolist()} passes {it.tolist()} / {it2.tolist()} max |Φ4 − Φ2| = {dev:.2e}, max |Φ4 − Φ_oracle| = {err:.2e}")
    assert np.array_equal(st, st2), (st, st2)
    assert np.array_equal(it, it2), (it, it2)
    assert dev < 1e-9, dev
    if want is not None:
        assert np.all(st == 0), (st, rs)
        assert err < TOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IMAGE_CASES)
def test_images_equal_numpy_construction(slc, gpu_ctx, cid):
    """`Ad` holds values of A unchanged: equal bits.  `wxt` holds 0 or H⁻¹ = 1 / (b²·c²) with b = 1: the host rounds the product and
    the reciprocal once each, as the NumPy line does — at most 2 ulp between two such evaluations whatever their order, and the
    zeros (masked entries, entries beyond ñx, row T) exact."""
    P, S, cols, cls, _, _ = _case(slc, cid)
    TR = 3 if cls in ("<32,10>", "<32,12>") else 4
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        assert FOUR + cls in plan.describe()
        img = plan.twisted4_images()
    finally:
        plan.close()
    assert len(img["Ad"]) == len(cols) and len(img["wxt"]) == len(cols)
    for i, c in enumerate(cols):
        Ad, wxt = _images(P, S, c, TR)
        assert img["Ad"][i].shape == Ad.shape and img["wxt"][i].shape == wxt.shape
        assert np.array_equal(img["Ad"][i].view(np.uint64), Ad.view(np.uint64)), c
        assert np.array_equal(img["wxt"][i] == 0.0, wxt == 0.0) and not np.signbit(img["wxt"][i]).any(), c
        assert np.all(np.abs(img["wxt"][i] - wxt) <= 2 * np.finfo(float).eps * wxt), c
        if P.default_weights:
            assert np.array_equal(img["wxt"][i], wxt)
        else:
            assert len(np.unique(wxt)) > 2                          # real weights, not a 0 / 1 table


@pytest.mark.gpu
def test_plant_update_refreshes_the_images(slc, gpu_ctx):
    """After update_plant with scaled A and B2 on the weighted plant, an execute into a NaN-filled array equals a freshly built
    plan's bit for bit, a second execute equals the first, and the images are those of the fresh plan."""
    P, S, cols, cls, _, _ = _case(slc, "weighted")
    A, B2 = sp.csc_matrix(P.A).copy(), sp.csc_matrix(P.B2).copy()
    A.data = A.data * 1.0625; B2.data = B2.data * 0.875
    Q = slc.Plant(A, P.B1, B2, P.C1, P.D11, P.D12)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    fresh = None
    try:
        assert FOUR + cls in plan.describe()
        first = _execute_into_nan(plan)
        before = plan.twisted4_images()
        plan.update_plant(A=Q.A, B2=Q.B2)
        upd = _execute_into_nan(plan)
        upd2 = _execute_into_nan(plan)
        after = plan.twisted4_images()
        fresh = slc.Plan(gpu_ctx, Q, S, [[c] for c in cols])
        ref = _execute_into_nan(fresh)
        ref_img = fresh.twisted4_images()
    finally:
        plan.close()
        if fresh is not None:
            fresh.close()
    bits = lambda r: r[0].view(np.uint64)
    assert not np.all(np.isnan(first[0])) and np.array_equal(np.isnan(first[0]), np.isnan(ref[0]))
    assert not np.array_equal(bits(first), bits(upd))               # the update changed something
    assert np.array_equal(bits(upd), bits(ref)) and np.array_equal(bits(upd2), bits(upd))
    assert all(np.array_equal(a, b) for a, b in zip(upd[1:], ref[1:])) and all(np.array_equal(a, b) for a, b in zip(upd[1:], upd2[1:]))
    for i in range(len(cols)):
        assert not np.array_equal(before["Ad"][i], after["Ad"][i])
        assert np.array_equal(after["Ad"][i].view(np.uint64), ref_img["Ad"][i].view(np.uint64))
        assert np.array_equal(after["wxt"][i].view(np.uint64), ref_img["wxt"][i].view(np.uint64))
        assert np.array_equal(after["wxt"][i], before["wxt"][i])    # the weights do not depend on A or B2


@pytest.mark.gpu
def test_column_subset_reads_its_own_images(slc, gpu_ctx):
    """execute_columns on a strict subset that does not start at column 0: the kept columns' entries equal the full run's bit for
    bit (images and first static blocks are indexed by launch position), every other entry keeps the NaN it held."""
    import torch
    P, S, cols, cls, _, _ = _case(slc, SUBSET_CASE)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        assert FOUR + cls in plan.describe()
        n = plan.info["n_values"]
        q_of = -np.ones(P.Nx, dtype=np.int64)
        q_of[np.asarray(cols)] = np.arange(len(cols))
        owner = -np.ones(n, dtype=np.int64)
        for masks, offs in ((S[0], plan.off_x), (S[1], plan.off_u)):
            for t, M in enumerate(masks):
                M = sp.csc_matrix(M); M.sort_indices()
                owner[offs[t]:offs[t + 1]] = q_of[np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))]
        full = _execute_into_nan(plan)
        v = torch.full((max(n, 1),), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert plan.execute_columns(v.data_ptr(), SUBSET) == len(SUBSET)
        plan.synchronize()
        part = v.cpu().numpy()[:n].copy()
    finally:
        plan.close()
    kept = np.isin(owner, SUBSET)
    assert kept.any() and (~kept & (owner >= 0)).any() and np.all(full[1] == 0)
    assert not np.isnan(full[0][owner >= 0]).any()
    assert np.array_equal(part[kept].view(np.uint64), full[0][kept].view(np.uint64))
    assert np.isnan(part[~kept]).all()
