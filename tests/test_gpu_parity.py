"""GPU parity tests proper: the HIP path, called through the C ABI, against the oracle / golden vectors.

Tolerance.  BASELINE.json's north_star contract is ‖Φ−Φ_ref‖∞ < 1e-6 with the sparsity pattern bit-exact.
The tests hold the HIP path to TOL = 1e-8 against the FP64 oracle — 100× inside the contract and at the
reference's own Ipopt tolerance (1e-8) — and to exact pattern containment.  Why not tighter: the kernel stops
refining at ‖f − E z‖∞ ≤ 1e-12 and z ∈ range(Eᵀ) exactly, so z − z* = E⁺(Ez − f) is bounded by
1e-12/σ_min⁺(E) ≈ 1e-12 · 1.3e3 on README columns; measured 2e-9."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, flat_phi, split_vals
from oracle_c import TOL, c_oracle_flat as _c_oracle_flat

pytestmark = pytest.mark.gpu


def _flat(slc, P, S, I=None, ctx=None):
    Phix, Phiu, info = slc.SLS_H2(P, S, I, ctx=ctx, return_info=True, dropzeros=False)
    return np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])]), Phix, Phiu, info


def test_readme_chain_matches_golden(slc, gpu_ctx, readme, golden_readme):
    P, S, _ = readme
    got, Phix, Phiu, info = _flat(slc, P, S, ctx=gpu_ctx)
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    assert got.shape == want.shape == (36029,)
    assert np.abs(got - want).max() < TOL
    assert info["n_unsolved"] == 0 and np.all(info["col_status"] == 0)
    assert info["max_residual"] < 1e-12 and info["n_subproblems"] == 59 and info["n_free"] == 36029
    # pattern: bit-exact containment in the masks (values live in the mask's own CSC arrays)
    for F, M in zip(Phix + Phiu, S[0] + S[1]):
        assert np.array_equal(F.indptr, M.indptr) and np.array_equal(F.indices, M.indices)
    # per-column cost Σ‖Φ[:,j]‖² against the oracle's (SURVEY §8c anchors: 1.739859, 23.545630, 18.830872, 22.362423)
    cost = sum(np.asarray(F.multiply(F).sum(axis=0)).ravel() for F in Phix + Phiu)
    assert np.abs(cost - golden_readme["col_cost"]).max() < 1e-8
    assert abs(cost.sum() - 893.3262819770) < 1e-7


def test_readme_closed_loop_localized(slc, gpu_ctx, readme, oracle):
    """README.md:60-76 with the HIP Φ: response confined to |i−30| ≤ 9, dead after T = 29 steps."""
    P, S, _ = readme
    Phix, Phiu = slc.SLS_H2(P, S, ctx=gpu_ctx)
    x, u = oracle.closed_loop(P.A, P.B1, P.B2, Phix, Phiu)
    r, c = np.nonzero(np.abs(x) > 1e-9)
    assert r.min() + 1 >= 21 and r.max() + 1 <= 39 and c.min() + 1 == 51 and c.max() + 1 <= 79


def _weighted_problem(slc):
    g = np.load(os.path.join(GOLDEN, "weighted_chain_phi.npz"))
    Nx = int(g["Nx"])
    Pc = slc.workloads.chain_plant(Nx)
    Nu = Pc.Nu
    C1 = sp.vstack([sp.diags(g["q"]), sp.csc_matrix((Nu, Nx))]).tocsc()
    D12 = sp.vstack([sp.csc_matrix((Nx, Nu)), sp.diags(g["r"])]).tocsc()
    D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nx + Nu, Nx))
    P = slc.Plant(Pc.A, sp.diags(g["b"]).tocsc(), Pc.B2, C1, D11, D12)
    S = slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"]))
    return P, list(S), g


def test_weighted_lqr_with_feedthrough_matches_golden(slc, gpu_ctx):
    """Diagonal Q,R weights, D11 ≠ 0, B1 = diag(b): src/synthesis.jl:42,50-52 beyond the default plant."""
    P, S, g = _weighted_problem(slc)
    got, _, _, info = _flat(slc, P, S, ctx=gpu_ctx)
    want = np.concatenate([g["vals_x"], g["vals_u"]])
    assert np.abs(got - want).max() < TOL
    assert info["n_unsolved"] == 0


def test_multi_column_groups_match_golden(slc, gpu_ctx, readme):
    """𝓘 = [0:20, 20:40, 40:59] (src/synthesis.jl:11 keyword 𝓘): columns solved on their group's s_x, s_u."""
    P, S, _ = readme
    g = np.load(os.path.join(GOLDEN, "grouped_chain_phi.npz"))
    groups = [list(range(0, 20)), list(range(20, 40)), list(range(40, 59))]
    got, _, _, info = _flat(slc, P, S, groups, ctx=gpu_ctx)
    want = np.concatenate([g["vals_x"], g["vals_u"]])
    assert np.abs(got - want).max() < TOL
    assert info["n_unsolved"] == 0 and info["max_nx"] == 40


def test_julia_index_base_one_end_to_end(slc, gpu_ctx, readme, golden_readme):
    """The drop-in call with every index array 1-based, exactly what julia/SLSMI355X.jl hands over (index_base = 1):
    default groups and explicit multi-column groups."""
    P, S, _ = readme
    Phix, Phiu, info = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False, index_base=1)
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    assert np.abs(got - want).max() < TOL and info["n_unsolved"] == 0
    g = np.load(os.path.join(GOLDEN, "grouped_chain_phi.npz"))
    groups = [list(range(0, 20)), list(range(20, 40)), list(range(40, 59))]
    Phix, Phiu, info = slc.SLS_H2(P, S, groups, ctx=gpu_ctx, return_info=True, dropzeros=False, index_base=1)
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    assert np.abs(got - np.concatenate([g["vals_x"], g["vals_u"]])).max() < TOL and info["n_unsolved"] == 0


def test_partial_groups_leave_other_columns_zero(slc, gpu_ctx, readme, golden_readme):
    P, S, _ = readme
    got, Phix, _, info = _flat(slc, P, S, [[5], [40]], ctx=gpu_ctx)
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    cols = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    sel = np.isin(cols, [5, 40])
    assert np.abs(got[sel] - want[sel]).max() < TOL and np.all(got[~sel] == 0.0)
    assert info["n_subproblems"] == 2


def test_infeasible_columns_are_flagged_not_silent(slc, gpu_ctx):
    """Columns with no feasible localized response: the reference never checks Ipopt's status
    (src/synthesis.jl:62-65); this build returns a status word per column and the least-squares point."""
    g = np.load(os.path.join(GOLDEN, "infeasible_chain.npz"))
    P = slc.workloads.chain_plant(int(g["Nx"]))
    S = list(slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"])))
    got, _, _, info = _flat(slc, P, S, ctx=gpu_ctx)
    bad = g["col_resid"] > 1e-9
    assert bad.sum() == 12
    assert np.array_equal(info["col_status"] != 0, bad)
    assert info["n_unsolved"] == 12
    want = np.concatenate([g["vals_x"], g["vals_u"]])
    cols = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = ~np.isin(cols, np.flatnonzero(bad))
    assert np.abs(got[ok] - want[ok]).max() < TOL


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_small_plants_against_live_oracle(slc, gpu_ctx, oracle, seed):
    """Seeded random banded plants with ragged index sets, stored-false mask entries and a column with an
    empty mask; oracle computed live (sizes it finishes in seconds)."""
    rng = np.random.default_rng(seed)
    Nx = int(rng.integers(14, 22))
    bw = int(rng.integers(1, 3))
    A = sp.identity(Nx, format="lil")
    for k in range(1, bw + 1):
        for i in range(Nx - k):
            if rng.random() < 0.9:
                A[i, i + k] = rng.uniform(-0.4, 0.4)
            if rng.random() < 0.9:
                A[i + k, i] = rng.uniform(-0.4, 0.4)
    A = A.tocsc()
    act = sorted(rng.choice(Nx, size=max(3, Nx // 2), replace=False).tolist())
    B2 = sp.csc_matrix((rng.uniform(0.5, 1.5, len(act)), (act, range(len(act)))), shape=(Nx, len(act)))
    P = slc.Plant(A, sp.identity(Nx, format="csc"), B2)
    d, T = 4 + bw, 10
    Sx, Su = slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5)
    # a stored `false` inside a mask (Julia masks may hold them; the reference tests `.≠ 1`)
    Sx = [m.copy() for m in Sx]
    m = Sx[T // 2].tolil(); r, c = m.nonzero(); k = int(rng.integers(len(r)))
    m = Sx[T // 2].copy(); m.data = m.data.copy()
    m.data[int(rng.integers(m.nnz))] = False
    Sx[T // 2] = m
    S = [Sx, list(Su)]
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ox, ou, dg = oracle.SLS_H2(Po, S, return_diag=True)
    want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
    got, _, _, info = _flat(slc, P, S, ctx=gpu_ctx)
    feasible = np.array([d_["resid"] < 1e-9 for d_ in dg])
    assert np.array_equal(info["col_status"] == 0, feasible)
    cols = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(cols, np.flatnonzero(feasible))
    assert np.abs(got[ok] - want[ok]).max() < TOL


def test_plan_execute_paths_agree(slc, gpu_ctx, readme, golden_readme):
    """sls_h2_sf_plan / sls_plan_execute (device-resident, mask-order and packed) ≡ sls_h2_sf_solve."""
    P, S, _ = readme
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    plan = slc.Plan(gpu_ctx, P, S)
    assert plan.info["n_subproblems"] == 59 and plan.info["n_values"] == 36029
    d = plan.alloc_values(packed=False)
    plan.execute(d, packed=False); plan.synchronize()
    vx, vu = plan.download(d)
    got = np.concatenate(vx + vu)
    assert np.abs(got - want).max() < TOL
    st, rs, it = plan.fetch_status()
    assert np.all(st == 0) and rs.max() < 1e-12 and it.max() <= 3
    # shard [10, 30): only its columns are written
    plan2 = slc.Plan(gpu_ctx, P, S, None, (10, 30))
    d2 = plan2.alloc_values(packed=False)
    plan2.execute(d2); plan2.synchronize()
    got2 = np.concatenate(sum(plan2.download(d2), []))
    cols = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    sel = (cols >= 10) & (cols < 30)
    assert np.abs(got2[sel] - want[sel]).max() < TOL and np.all(got2[~sel] == 0)
    avg_ms, n = plan.kernel_time_ms()
    assert n == 1 and avg_ms > 0
    plan.close(); plan2.close()


def test_two_device_slots_in_one_context(slc, readme, golden_readme):
    """One context over two device slots (both slot → GPU 0 on the 1-GPU box): the in-process
    multi-device split of sls_h2_sf_solve (cost-balanced cuts, per-device packed D2H) reassembles Φ."""
    P, S, _ = readme
    ctx = slc.Context([0, 0])
    got, _, _, info = _flat(slc, P, S, ctx=ctx)
    ctx.close()
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    assert np.abs(got - want).max() < TOL and info["n_devices"] == 2 and info["n_subproblems"] == 59


def test_sharded_solver_single_rank_torch_stream(slc, readme, golden_readme):
    """dist.ColumnShardedH2 at world size 1 on cuda:0 — the bench's step: HIP solve on torch's stream + unpack."""
    import torch
    P, S, _ = readme
    sh = slc.dist.ColumnShardedH2(P, S, None, device="cuda:0")
    vals = sh.step()
    torch.cuda.synchronize()
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    assert np.abs(vals.cpu().numpy() - want).max() < TOL


@pytest.mark.parametrize("name", ["chain1024", "chain4096"])
def test_chain_full_size_properties(slc, gpu_ctx, name):
    """Full-size cases (1024 / 4096 subproblems, d=12, T=40; chain-4096 is BASELINE configs[3]'s plant and the only case that
    runs the throughput variant; its four size classes share one launch, or get one each with SLS_ABSORB=0) through
    size-independent properties:
    (i) FULL-system achievability  Φx[1]=I, Φx[t+1]=AΦx[t]+B2Φu[t], AΦx[T]+B2Φu[T]=0  (README.md:31),
    (ii) pattern ⊆ mask, (iii) shift invariance: interior columns 6 states apart are shifted copies."""
    P, S, _ = slc.workloads.make_workload(name)
    Phix, Phiu, info = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
    assert info["n_unsolved"] == 0 and info["max_residual"] < 1e-11
    T = len(Phix)
    assert abs(Phix[0] - sp.identity(P.Nx)).max() < 1e-12
    worst = 0.0
    for t in range(T - 1):
        worst = max(worst, abs(Phix[t + 1] - (P.A @ Phix[t] + P.B2 @ Phiu[t])).max())
    worst = max(worst, abs(P.A @ Phix[T - 1] + P.B2 @ Phiu[T - 1]).max())
    assert worst < 1e-11
    j = 500
    for t in (1, 7, 20, 39):
        a = Phix[t][:, j].toarray().ravel(); b = Phix[t][:, j + 6].toarray().ravel()
        assert np.abs(a[:-6] - b[6:]).max() < 1e-10
    if name == "chain4096":
        # launch list: the 22 edge columns of three smaller one-wave classes run inside the interior columns' launch (one launch,
        # 2048 waves); SLS_ABSORB=0 gives every class its own launch — same Φ up to the round-off of a different register layout
        plan = slc.Plan(gpu_ctx, P, S); desc = plan.describe(); plan.close()
        assert desc.count("h2_column_wave_kernel") == 1 and "nsub=4096 grid=2048" in desc, desc
        os.environ["SLS_ABSORB"] = "0"
        try:
            plan = slc.Plan(gpu_ctx, P, S); desc0 = plan.describe(); plan.close()
            Qx, Qu, info0 = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
        finally:
            del os.environ["SLS_ABSORB"]
        assert desc0.count("h2_column_wave_kernel") == 4 and "nsub=4074" in desc0, desc0
        assert info0["n_unsolved"] == 0
        assert max(abs(a - b).max() for a, b in zip(Phix + Phiu, Qx + Qu)) < 1e-10


def _two_rank_gpu_worker(rank, world, port, q):
    import sys
    import torch.distributed as dist
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import torch
        import slc_amd
        g = np.load(os.path.join(GOLDEN, "readme_chain_phi.npz"))
        want = np.concatenate([g["vals_x"], g["vals_u"]])
        P, S, _ = slc_amd.workloads.make_workload("readme_chain")
        sh = slc_amd.dist.ColumnShardedH2(P, S, None, device="cuda:0")
        vals = sh.step()
        torch.cuda.synchronize()
        err = float(np.abs(vals.cpu().numpy() - want).max())
        st, rs, it = sh.local.plan.fetch_status()
        q.put((rank, err, sh.group_range, int(sh.local.n_packed), int((st != 0).sum())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_share_one_gpu_sharded_solve():
    """The N>1 product path end to end on the 1-GPU box: two processes, each plans and solves ITS column shard with the
    HIP kernels on cuda:0, packed shards are all-gathered (gloo with host staging here; RCCL on a real multi-GPU node)
    and unpacked on both ranks.  Everything of bench.py --gpus 2 except the RCCL transport itself."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_gpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = sorted(q.get(timeout=480) for _ in range(2))
    for p_ in procs:
        p_.join(60)
        assert p_.exitcode == 0
    assert all(r[1] < TOL for r in res), res
    assert all(r[4] == 0 for r in res)
    assert res[0][2][1] == res[1][2][0] and res[0][3] + res[1][3] == 36029


def _rccl_single_rank_worker(port, q):
    """RCCL process group of ONE rank on cuda:0: the collective + unpack of the N>1 path (always_gather), in its stream-ordered
    form (step) and in its pipelined form (step_async on a side stream, double-buffered) — both must reproduce the golden Φ."""
    import os
    import torch
    import torch.distributed as dist
    import slc_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    P, S, _ = slc_amd.workloads.make_workload("readme_chain")
    g = np.load(os.path.join(GOLDEN, "readme_chain_phi.npz"))
    want = np.concatenate([g["vals_x"], g["vals_u"]])
    sh = slc_amd.dist.ColumnShardedH2(P, S, None, device=dev, always_gather=True)
    assert sh.gather and not sh._direct()
    e_sync = float(np.abs(sh.step().cpu().numpy() - want).max())
    sh.values.zero_()
    for _ in range(5):
        sh.step_async()
    sh.flush()
    torch.cuda.synchronize()
    e_pipe = float(np.abs(sh.values[: sh.n_values].cpu().numpy() - want).max())
    q.put((e_sync, e_pipe, dist.get_backend()))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_rccl_all_gather_path_single_rank():
    """The RCCL transport itself cannot be shared by two ranks on one GPU, so it is rehearsed with a one-rank group:
    init_process_group("nccl"), all_gather_into_tensor of the packed shard on device memory, unpack kernel."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p_ = ctx.Process(target=_rccl_single_rank_worker, args=(port, q))
    p_.start()
    e_sync, e_pipe, backend = q.get(timeout=480)
    p_.join(60)
    assert p_.exitcode == 0 and backend == "nccl"
    assert e_sync < TOL and e_pipe < TOL


@pytest.mark.parametrize("four", ["1", "0"])
@pytest.mark.parametrize("d,expect_cls", [(8, "<32,10"), (12, "<32,14"), (14, "<32,16")])
def test_twisted_kernel_other_npl32_classes(slc, gpu_ctx, d, expect_cls, four, monkeypatch):
    """ñx = 2d+3 = 19 / 27 / 31: the twisted kernels' remaining NPL = 32 classes, whose Gauss–Jordan runs on the 8×8 lane
    grid with 3×3 tiles and four padded rows (NP = 20), and with 4×4 tiles (NP = 28, 32) — on the four-wave kernel (round 3:
    chain + helper wave per direction, the default for at most one column per CU) and on the two-wave kernel (SLS_TWISTED4=0)."""
    monkeypatch.setenv("SLS_TWISTED4", four)
    P = slc.workloads.chain_plant(90)
    S = list(slc.workloads.localization_masks(P.A, P.B2, d, 2 * d + 8, 1.5))
    cols = list(range(33, 57, 2))
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    desc = plan.describe()
    assert ("h2_column_twisted4_kernel" if four == "1" else "h2_column_twisted_kernel") + expect_cls in desc, desc
    plan.close()
    Phix, Phiu, info = slc.SLS_H2(P, S, [[c] for c in cols], ctx=gpu_ctx, return_info=True, dropzeros=False)
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    assert oinfo["status"].max() == 0 and info["n_unsolved"] == 0
    assert np.abs(got - want).max() < TOL


@pytest.mark.parametrize("d,expect", [(20, "<64,48>"), (28, "<64,64>"), (20, "h2_column_tile_kernel"), (28, "h2_column_tile_kernel")])
def test_wide_localization_mid_classes(slc, d, expect, monkeypatch):
    """ñx = 2d+3 = 43 / 59.  Default routing: the tile kernel (faster than the 64-lane one-wave classes on every workload measured,
    DESIGN §5).  SLS_WAVE64=1: the NPL = 64 size classes of the one-wave kernel (one lane per column, scalar broadcasts), kept and
    kept tested."""
    if expect.startswith("<64"):
        monkeypatch.setenv("SLS_WAVE64", "1")
    gpu_ctx = slc.Context([0])
    P = slc.workloads.chain_plant(96)
    S = list(slc.workloads.localization_masks(P.A, P.B2, d, 2 * d + 6, 1.5))
    cols = list(range(30, 66, 3))
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    desc = plan.describe()
    plan.close()
    assert expect in desc and ("wave_kernel" in desc) == expect.startswith("<64"), desc
    Phix, Phiu, info = slc.SLS_H2(P, S, [[c] for c in cols], ctx=gpu_ctx, return_info=True, dropzeros=False)
    gpu_ctx.close()
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    assert oinfo["status"].max() == 0 and info["n_unsolved"] == 0
    assert np.abs(got - want).max() < TOL


def test_grid_plant_general_kernel_and_infeasible_columns(slc, gpu_ctx):
    """BASELINE configs[2] shape (32×32 grid, actuators every 3rd state, d=5, T=20): interior ñx = 85 runs on the
    general workgroup kernel.  Several columns have NO feasible localized response as specified (the reference's
    Ipopt would refuse them too: free < rows); they must come back flagged, the feasible ones must match."""
    P, S, _ = slc.workloads.make_workload("grid32")
    cols = [0, 31, 200, 495, 500, 528, 529, 1023]
    os.environ["SLS_TILE"] = "0"                               # the round-1 workgroup kernel (the default is the tile kernel)
    try:
        plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
        assert "h2_column_general_kernel" in plan.describe()
        plan.close()
        Phix, Phiu, info = slc.SLS_H2(P, S, [[c] for c in cols], ctx=gpu_ctx, return_info=True, dropzeros=False)
    finally:
        del os.environ["SLS_TILE"]
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    feasible = oinfo["status"] == 0
    assert 0 < feasible.sum() < len(cols)                       # both kinds present
    assert np.array_equal(info["col_status"] == 0, feasible)
    colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(colidx, np.asarray(cols)[feasible])
    assert np.abs(got[ok] - want[ok]).max() < TOL
    assert info["max_nx"] == 85


def test_wide_general_kernel_between_96_and_144(slc, gpu_ctx):
    """A 16×16 grid with d = 6: interior ñx = 113 runs on the wide variant of the workgroup kernel (9×9 register tiles, the Ã·Q
    image in the global workspace); status and values against the C restatement."""
    P = slc.workloads.grid_plant(16, 3)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 6, 14, 1.5))
    cols = [119, 136, 0]
    os.environ["SLS_TILE"] = "0"
    try:
        plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
        assert "h2_column_general_kernel<wide>" in plan.describe(), plan.describe()
        assert plan.info["max_nx"] == 113
        plan.close()
        Phix, Phiu, info = slc.SLS_H2(P, S, [[c] for c in cols], ctx=gpu_ctx, return_info=True, dropzeros=False)
    finally:
        del os.environ["SLS_TILE"]
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    feasible = oinfo["status"] == 0
    assert np.array_equal(info["col_status"] == 0, feasible)
    colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(colidx, np.asarray(cols)[feasible])
    assert ok.any() and np.abs(got[ok] - want[ok]).max() < TOL


def test_random_sparse_plant_ragged_classes(slc, gpu_ctx):
    """BASELINE configs[4] family (random sparse A, seeded, d=2 so that it IS localized): ragged ñx over many size
    classes in one call; a sample of columns against the C restatement, the rest through the residual certificate."""
    P = slc.workloads.random_plant(400, 2, 1, seed=5)          # ñx from 1 to 52, ñu up to 97 (> 64 ⇒ general kernel too)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 2, 8, 1.5))
    Phix, Phiu, info = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
    st = info["col_status"]
    cols = list(range(0, 400, 20))
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    feasible = oinfo["status"] == 0
    assert np.array_equal(st[cols] == 0, feasible)
    colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(colidx, np.asarray(cols)[feasible])
    assert ok.any() and np.abs(got[ok] - want[ok]).max() < TOL
    assert info["max_residual"] < 1e-9


@pytest.mark.parametrize("routing", ["default", "tile"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7])
def test_short_horizons(slc, oracle, T, routing, monkeypatch):
    """T = 1, 2 run on the one-wave kernel, T ≥ 3 on the twisted two-wave kernel (middle block at (T−1)/2); with every column
    forced onto the tile kernel the same horizons exercise its block loops (T + 1 = 2 blocks at the least).  Most columns
    are infeasible at these horizons (the response cannot die in T steps); statuses and the feasible values must agree
    with the oracle."""
    if routing == "tile":
        monkeypatch.setenv("SLS_FORCE_GENERAL", "1")
    gpu_ctx = slc.Context([0])
    P = slc.workloads.chain_plant(13)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 3, T, 1.5))
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ox, ou, dg = oracle.SLS_H2(Po, S, return_diag=True)
    want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
    got, _, _, info = _flat(slc, P, S, ctx=gpu_ctx)
    gpu_ctx.close()
    feasible = np.array([d_["resid"] < 1e-9 for d_ in dg])
    assert np.array_equal(info["col_status"] == 0, feasible)
    cols = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(cols, np.flatnonzero(feasible))
    if ok.any():
        assert np.abs(got[ok] - want[ok]).max() < TOL


@pytest.mark.parametrize("routing", ["default", "tile"])
def test_columns_without_reachable_actuators(slc, oracle, routing, monkeypatch):
    """README chain dynamics with only two actuators, at one end: most columns see ñu = 0 (no input within d+1 hops) and
    are infeasible — the response cannot be killed; the columns next to the actuators are feasible.  Statuses and the
    feasible values against the oracle; ñu = 0 exercises the empty-input paths of the kernels — with every column forced
    onto the tile kernel, those of its plain build too."""
    if routing == "tile":
        monkeypatch.setenv("SLS_FORCE_GENERAL", "1")
    gpu_ctx = slc.Context([0])
    Nx, T, d = 14, 10, 3
    Pc = slc.workloads.chain_plant(Nx)
    B2 = sp.identity(Nx, format="csc")[:, [Nx - 2, Nx - 1]]
    P = slc.Plant(Pc.A, Pc.B1, B2)
    S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5))
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ox, ou, dg = oracle.SLS_H2(Po, S, return_diag=True)
    assert min(d_["m"] for d_ in dg) == 0
    want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
    if routing == "tile":
        plan = slc.Plan(gpu_ctx, P, S)
        desc = plan.describe()
        plan.close()
        assert desc.count(";") == 1 and desc.startswith("h2_column_tile_kernel<"), desc
    got, _, _, info = _flat(slc, P, S, ctx=gpu_ctx)
    gpu_ctx.close()
    feasible = np.array([d_["resid"] < 1e-9 for d_ in dg])
    assert np.array_equal(info["col_status"] == 0, feasible)
    cols = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(cols, np.flatnonzero(feasible))
    if ok.any():
        assert np.abs(got[ok] - want[ok]).max() < TOL


def test_column_outside_its_own_index_set_is_trivial(slc, gpu_ctx):
    """A[:,c] = 0 ⇒ s_x = rows((𝓢x[T]·(A≠0))[:,c]) = ∅ does not contain c: the reference's L·Φ·R is then not conformable
    (it throws, src/synthesis.jl:42,50).  The library returns Φ[:,c] = 0 with status SLS_COL_TRIVIAL."""
    Nx = 8
    A = sp.diags(0.5 * np.ones(Nx - 1), -1).tocsc()          # nilpotent: last column is empty
    P = slc.Plant(A, sp.identity(Nx, format="csc"), sp.identity(Nx, format="csc")[:, [0, 3]])
    S = list(slc.workloads.localization_masks(A + sp.identity(Nx), P.B2, 3, 5, 1.0))
    got, _, _, info = _flat(slc, P, S, [[Nx - 1]], ctx=gpu_ctx)
    assert info["col_status"].tolist() == [slc._capi.SLS_COL_TRIVIAL] and np.all(got == 0.0)


def test_one_wave_and_twisted_kernels_agree(slc, readme, golden_readme):
    """SLS_NO_TWISTED=1 forces the one-wave kernel on the README chain, SLS_TWISTED4=0 the two-wave twisted kernel; the default is
    the four-wave twisted kernel.  All three must meet the golden vector (they share the mathematics, not the elimination
    order; the four-wave kernel forms the next block by elimination behind the pivots instead of explicit products)."""
    P, S, _ = readme
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    os.environ["SLS_NO_TWISTED"] = "1"
    try:
        ctx = slc.Context([0])
        plan = slc.Plan(ctx, P, S)
        assert "h2_column_wave_kernel" in plan.describe()
        d = plan.alloc_values(); plan.execute(d); plan.synchronize()
        got1 = np.concatenate(sum(plan.download(d), []))
        plan.close(); ctx.close()
    finally:
        del os.environ["SLS_NO_TWISTED"]
    got = {}
    for four, name in (("0", "h2_column_twisted_kernel"), ("1", "h2_column_twisted4_kernel")):
        os.environ["SLS_TWISTED4"] = four
        try:
            ctx = slc.Context([0])
            plan = slc.Plan(ctx, P, S)
            assert name in plan.describe(), plan.describe()
            d = plan.alloc_values(); plan.execute(d); plan.synchronize()
            got[four] = np.concatenate(sum(plan.download(d), []))
            st, rs, it = plan.fetch_status()
            assert np.all(st == 0) and rs.max() < 1e-12 and it.max() == 2
            plan.close(); ctx.close()
        finally:
            del os.environ["SLS_TWISTED4"]
    for g2 in got.values():
        assert np.abs(g2 - want).max() < TOL and np.abs(got1 - g2).max() < TOL
    assert np.abs(got["0"] - got["1"]).max() < 1e-10          # same block recursion, the products in a different order


def test_twisted_variant_with_pivot_blocks_in_lds(slc, readme, golden_readme):
    """Opt-in variant (SLS_P_LDS=1): P_k stays in LDS, no workspace traffic; slower than the default but
    must give the same Φ."""
    P, S, _ = readme
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    os.environ["SLS_P_LDS"] = "1"
    try:
        ctx = slc.Context([0])
        plan = slc.Plan(ctx, P, S)
        assert "P_in_LDS" in plan.describe()
        d = plan.alloc_values(); plan.execute(d); plan.synchronize()
        got = np.concatenate(sum(plan.download(d), []))
        plan.close(); ctx.close()
    finally:
        del os.environ["SLS_P_LDS"]
    assert np.abs(got - want).max() < TOL


def test_throughput_variant_with_global_vectors(slc, readme, golden_readme):
    """The throughput-regime variant of the one-wave kernel keeps λ and r/q in a global workspace instead of LDS; it is
    selected automatically only for batches larger than the GPU (e.g. chain-4096).  SLS_VEC_GLOBAL=1 forces it on the
    README chain so that it is checked against the golden vector like every other kernel."""
    P, S, _ = readme
    want = np.concatenate([golden_readme["vals_x"], golden_readme["vals_u"]])
    os.environ["SLS_VEC_GLOBAL"] = "1"
    try:
        ctx = slc.Context([0])
        plan = slc.Plan(ctx, P, S)
        assert "h2_column_wave_kernel" in plan.describe()
        d = plan.alloc_values(); plan.execute(d); plan.synchronize()
        got = np.concatenate(sum(plan.download(d), []))
        st, rs, it = plan.fetch_status()
        plan.close(); ctx.close()
    finally:
        del os.environ["SLS_VEC_GLOBAL"]
    assert np.abs(got - want).max() < TOL and np.all(st == 0) and rs.max() < 1e-12


def test_plain_c_host_drop_in_call(tmp_path):
    """examples/solve_readme.c: README plant with Julia's 1-based arrays, masks from sls_localization_masks, the drop-in
    call from a plain C host; exits 0 iff every column is solved and Σ‖Φ‖² matches the oracle's 893.3262819770."""
    import subprocess
    from test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "columns not solved: 0" in r.stdout


def test_random_plant_all_kernel_families_in_one_call(slc, gpu_ctx):
    """Random sparse plant at d = 3 (ñx up to 97, ñu up to 173): wave classes, the workgroup kernel and its wide variant side
    by side in ONE call; a sample of the columns against the C restatement."""
    P = slc.workloads.random_plant(400, 2, 1, seed=5)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 3, 8, 1.5))
    os.environ["SLS_TILE"] = "0"
    try:
        plan = slc.Plan(gpu_ctx, P, S)
        desc = plan.describe()
        plan.close()
        assert "h2_column_general_kernel<wide>" in desc and "h2_column_general_kernel nsub" in desc and \
            ("h2_column_wave_kernel" in desc or "h2_column_twisted_kernel" in desc or "h2_column_twisted4_kernel" in desc), desc
        Phix, Phiu, info = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
    finally:
        del os.environ["SLS_TILE"]
    st = info["col_status"]
    uns = st == slc._capi.SLS_COL_UNSUPPORTED
    cols = [int(c) for c in np.flatnonzero(~uns)[::17]]
    assert len(cols) >= 5
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    feasible = oinfo["status"] == 0
    assert np.array_equal(st[cols] == 0, feasible)
    colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
    ok = np.isin(colidx, np.asarray(cols)[feasible])
    assert ok.any() and np.abs(got[ok] - want[ok]).max() < TOL
    if uns.any():
        assert np.all(got[np.isin(colidx, np.flatnonzero(uns))] == 0.0)


def test_batch_of_plants_equals_separate_solves(slc, gpu_ctx):
    """sls_plan_execute_batch: four different plants in one call, results and statuses identical (bit for bit) to executing
    each plan on its own — the launches only overlap in time."""
    specs = [(59, 9, 29), (40, 6, 20), (23, 6, 18), (59, 5, 12)]
    plans, vals, want = [], [], []
    try:
        for Nx, d, T in specs:
            P = slc.workloads.chain_plant(Nx)
            S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5))
            p = slc.Plan(gpu_ctx, P, S)
            plans.append(p)
            v = p.alloc_values()
            p.execute(v); p.synchronize()
            want.append((np.concatenate([a for part in p.download(v) for a in part]), p.fetch_status()[0].copy()))
            vals.append(p.alloc_values())
        slc.execute_batch(plans, vals)
        plans[0].synchronize()                                  # the null stream joins every plan's stream
        for p, v, (w, st) in zip(plans, vals, want):
            got = np.concatenate([a for part in p.download(v) for a in part])
            assert np.array_equal(got, w)
            assert np.array_equal(p.fetch_status()[0], st)
        with pytest.raises(slc.SLSError):
            slc.execute_batch([plans[0], plans[0]], [vals[0], vals[0]])
    finally:
        for p in plans:
            p.close()


def test_batch_solve_equals_one_call_per_plant(slc, gpu_ctx, oracle):
    """sls_h2_sf_solve_batch: plants of different sizes and weights (one with D11 feed-through) sharing T, solved as one
    block-diagonal composite — each plant's Φ equals its own single-call Φ to rounding (the composite may land in another
    kernel of the same mathematics) and the oracle's to TOL; statuses identical."""
    rng = np.random.default_rng(21)
    T = 20
    plants, masks = [], []
    for Nx, d in ((59, 6), (23, 5), (40, 6)):
        base = slc.workloads.chain_plant(Nx)
        q = rng.uniform(0.5, 2.0, Nx); r = rng.uniform(0.5, 2.0, base.Nu)
        C1 = sp.vstack([sp.diags(q), sp.csc_matrix((base.Nu, Nx))]).tocsc()
        D12 = sp.vstack([sp.csc_matrix((Nx, base.Nu)), sp.diags(r)]).tocsc()
        D11 = (sp.random(Nx + base.Nu, Nx, density=0.03, random_state=int(Nx), format="csc") * 0.1) if Nx == 23 else 0
        P = slc.Plant(base.A, base.B1, base.B2, C1, D11, D12)
        plants.append(P)
        masks.append(list(slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5)))
    res, info = slc.SLS_H2_batch(plants, masks, ctx=gpu_ctx, return_info=True, dropzeros=False)
    res1, info1 = slc.SLS_H2_batch(plants, masks, ctx=gpu_ctx, return_info=True, dropzeros=False, index_base=1)   # Julia's own arrays
    for i, (P, S) in enumerate(zip(plants, masks)):
        assert np.array_equal(info1["col_status"][i], info["col_status"][i])
        for a, b in zip(res1[i][0] + res1[i][1], res[i][0] + res[i][1]):
            assert np.array_equal(a.toarray(), b.toarray())
        Px, Pu, inf1 = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
        assert np.array_equal(info["col_status"][i], inf1["col_status"])
        got = np.concatenate([flat_phi(res[i][0], S[0]), flat_phi(res[i][1], S[1])])
        one = np.concatenate([flat_phi(Px, S[0]), flat_phi(Pu, S[1])])
        assert np.abs(got - one).max() <= 1e-11 * max(1.0, np.abs(one).max())
        Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
        ox, ou = oracle.SLS_H2(Po, S)
        want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        ok = info["col_status"][i][colidx] == 0               # infeasible columns hold a least-squares point: not compared
        assert ok.sum() > 0
        assert np.abs(got - want)[ok].max() <= TOL * max(1.0, np.abs(want).max())
    # mismatched T is refused
    bad = [masks[0], [m[:-1] for m in masks[1]]]
    with pytest.raises((slc.SLSError, ValueError)):
        slc.SLS_H2_batch(plants[:2], bad, ctx=gpu_ctx)


def test_ridge_term_equals_reweighted_plant(slc, oracle):
    """sls_set_ridge (the diagonal instance of the reference's L⁺ hook, src/synthesis.jl:21,52): with default weights and
    B1 = I the ridge-regularised solve equals the plain solve of the plant with [C1 D12] = diag(√(1 + r)) — compared with the
    oracle on that plant (README chain: one-wave / twisted kernels) — and clearing the term restores the plain answer."""
    P, S, _ = slc.workloads.make_workload("readme_chain")
    rng = np.random.default_rng(2)
    rx = rng.uniform(0.0, 2.0, P.Nx); ru = rng.uniform(0.0, 2.0, P.Nu)
    ctx = slc.Context([0])
    try:
        plain = slc.SLS_H2(P, S, ctx=ctx, dropzeros=False)
        ctx.set_ridge(rx, ru)
        Px, Pu, info = slc.SLS_H2(P, S, ctx=ctx, return_info=True, dropzeros=False)
        assert np.all(info["col_status"] == 0)
        C1 = sp.vstack([sp.diags(np.sqrt(1 + rx)), sp.csc_matrix((P.Nu, P.Nx))]).tocsc()
        D12 = sp.vstack([sp.csc_matrix((P.Nx, P.Nu)), sp.diags(np.sqrt(1 + ru))]).tocsc()
        ox, ou = oracle.SLS_H2(oracle.OraclePlant(P.A, P.B1, P.B2, C1, None, D12), S)
        got = np.concatenate([flat_phi(Px, S[0]), flat_phi(Pu, S[1])])
        want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
        assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max())
        base = np.concatenate([flat_phi(plain[0], S[0]), flat_phi(plain[1], S[1])])
        assert np.abs(got - base).max() > 1e-3                        # the term does something
        with pytest.raises(slc.SLSError):
            ctx.set_ridge(-rx, ru)
        with pytest.raises(slc.SLSError):                             # wrong length for this plant
            ctx.set_ridge(rx[:5], None); slc.SLS_H2(P, S, ctx=ctx)
        ctx.set_ridge(None, None)
        again = slc.SLS_H2(P, S, ctx=ctx, dropzeros=False)
        assert np.array_equal(flat_phi(again[0], S[0]), flat_phi(plain[0], S[0]))
    finally:
        ctx.close()


def test_ridge_term_with_dense_hessian_and_coupled_group(slc, oracle):
    """The ridge term inside the CG build (dense [C1 D12]ᵀ[C1 D12], a coupled group): against the joint problem solved in NumPy
    from the oracle's own (E, f, M, m0):  min ‖M z + m0‖² + Σ r z²  s.t.  E z = f  (null-space method)."""
    g = np.load(os.path.join(GOLDEN, "coupled_group_phi.npz"))
    Nx = int(g["Nx"])
    Pc = slc.workloads.chain_plant(Nx)
    Nu = Pc.Nu
    W = sp.csc_matrix((g["dense_W_data"], g["dense_W_indices"], g["dense_W_indptr"]), shape=(Nx + Nu, Nx + Nu))
    B1 = sp.csc_matrix((g["B1_data"], g["B1_indices"], g["B1_indptr"]), shape=(Nx, Nx))
    D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nx + Nu, Nx))
    P = slc.Plant(Pc.A, B1, Pc.B2, W[:, :Nx], D11, W[:, Nx:])
    S = list(slc.workloads.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"])))
    groups = [[6, 7, 8, 9], [15]]
    rng = np.random.default_rng(4)
    rx = rng.uniform(0.1, 1.0, Nx); ru = rng.uniform(0.1, 1.0, Nu)
    ctx = slc.Context([0])
    try:
        ctx.set_ridge(rx, ru)
        Px, Pu, info = slc.SLS_H2(P, S, groups, ctx=ctx, return_info=True, dropzeros=False)
    finally:
        ctx.close()
    assert np.all(info["col_status"] == 0)
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    for cj in groups:
        E, f, M, m0, oi = oracle.assemble_group(Po, cj, S[0], S[1])
        r = np.array([(rx[oi["sx"][rr]] if kind == 0 else ru[oi["su"][rr]]) for (_, kind, rr, _) in oi["var_index"]])
        # null-space method on  min ‖M z + m0‖² + zᵀdiag(r)z  s.t.  E z = f
        zp = np.linalg.lstsq(E, f, rcond=None)[0]
        U, sv, Vt = np.linalg.svd(E)
        Z = Vt[int((sv > 1e-10 * sv.max()).sum()):].T
        H = M.T @ M + np.diag(r)
        y = np.linalg.solve(Z.T @ H @ Z, -Z.T @ (H @ zp + M.T @ m0))
        z = zp + Z @ y
        got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[rr], cj[c]] for (t, kind, rr, c) in oi["var_index"]])
        assert np.abs(got - z).max() <= TOL * max(1.0, np.abs(z).max()), (cj, np.abs(got - z).max())


def test_near_singular_column_keeps_full_pivot_images(slc, oracle, monkeypatch):
    """Regression (round 2): the one-wave kernel's NPL = 32 classes store pivot blocks as their upper half.  On a near-singular
    block the in-register inverse is one-sided, not symmetric to working accuracy, and its mirror image made a feasible column
    (random plant, ñx = 32) stall at 1e-5 and come back SLS_COL_INFEASIBLE.  Blocks that fail a symmetry test now keep their full
    image.  One column per plan on the one-wave kernel (SLS_NO_TWISTED=1), all 36 columns: statuses must agree with the oracle's
    feasibility, feasible columns to 1e-6·(conditioning: the oracle's own residual on them is up to 1e-14)."""
    monkeypatch.setenv("SLS_NO_TWISTED", "1")
    Nx = 36
    A = sp.random(Nx, Nx, density=0.08, random_state=1, format="csc") * 0.5 + sp.eye(Nx, format="csc")
    B2 = sp.eye(Nx, format="csc")[:, ::2]
    P = slc.Plant(A, sp.eye(Nx, format="csc"), B2)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 3, 8, 1.5))
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ctx = slc.Context([0])
    seen32 = False
    try:
        for c in range(Nx):
            z, oi, d = oracle.solve_group(Po, [c], S[0], S[1])
            plan = slc.Plan(ctx, P, S, [[c]])
            desc = plan.describe(); plan.close()
            if "wave_kernel<32," not in desc:
                continue
            seen32 = seen32 or oi["n"] == 32
            Px, Pu, info = slc.SLS_H2(P, S, [[c]], ctx=ctx, return_info=True, dropzeros=False)
            assert (info["col_status"][0] == 0) == (d["resid"] < 1e-9), (c, oi["n"], info["col_status"][0], d["resid"])
            if d["resid"] < 1e-9:
                got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], c] for (t, kind, r, _) in oi["var_index"]])
                assert np.abs(got - z).max() <= 1e-6 * max(1.0, np.abs(z).max()), (c, np.abs(got - z).max())
    finally:
        ctx.close()
    assert seen32


_FUZZ_ORACLE = {}


@pytest.mark.parametrize("seed", [2, 3, 7, 12, 21, 30])
@pytest.mark.parametrize("routing", ["default", "tile"])
def test_fuzz_irregular_plants_against_live_oracle(slc, oracle, seed, routing, monkeypatch):
    """Randomized plants the fixed workloads do not resemble (tools/fuzz_h2.py: irregular sparse A, partial actuation, weights + D11
    on even seeds, 1-based arrays on odd ones, d, T, Nx drawn at random), on the default kernel routing and with every column on
    the tile kernel: status ⇔ oracle feasibility and Φ on the feasible columns.  Columns the oracle itself finds marginal (residual
    between 1e-14 and 1e-6: feasible or infeasible only just) are not judged.  This test class found the packed-block bug
    of DESIGN §3.35."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_h2_problem", os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py"))
    src = open(spec.origin).read().split("modes = {")[0]
    ns = {"__file__": spec.origin}
    exec(compile(src, spec.origin, "exec"), ns)
    P, S, meta = ns["problem"](seed)
    if routing == "tile":
        monkeypatch.setenv("SLS_TILE", "all"); monkeypatch.setenv("SLS_FORCE_GENERAL", "1")
    if seed not in _FUZZ_ORACLE:                       # the oracle's dense SVDs are the slow part: once per seed
        Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
        _FUZZ_ORACLE[seed] = oracle.SLS_H2(Po, S, return_diag=True)
    ox, ou, dg = _FUZZ_ORACLE[seed]
    res = np.array([d_["resid"] for d_ in dg])
    ctx = slc.Context([0])
    try:
        Px, Pu, info = slc.SLS_H2(P, S, ctx=ctx, return_info=True, dropzeros=False, index_base=seed % 2)
    finally:
        ctx.close()
    st = info["col_status"]
    judged = 0
    for c in range(P.Nx):
        if 1e-14 < res[c] < 1e-6:
            continue
        judged += 1
        feas = res[c] <= 1e-14
        assert (st[c] in (0, 3)) == feas, (meta, c, int(st[c]), res[c])
        if feas:
            err = max(max(abs(X[:, c] - O[:, c]).max() for X, O in zip(Px, ox)), max(abs(U[:, c] - O[:, c]).max() for U, O in zip(Pu, ou)))
            assert err <= 1e-7, (meta, c, err)
    assert judged >= P.Nx // 2


def test_one_shot_call_refines_slowly_converging_columns(slc, oracle, monkeypatch):
    """Fuzz seed 77, column 21 (ñx = 12, σ_min(E) = 2e-6): the twisted / one-wave kernels stop at a residual of 4e-10 after 8–12
    passes — accepted (≤ 1e-9), but Φ is then only good to residual/σ_min = 2e-4.  The drop-in call solves such columns (≥ 4 passes,
    residual > 1e-11) once more on the tile kernel's minimal-residual iteration before the download: 1e-13, |ΔΦ| ≈ 2e-10, and it
    says so in sls_stats.n_refined.  SLS_REFINE=0 shows the unrefined answer."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")        # the stagnation rule of rounds 1–2: this test is about the refinement machinery (round 3's rule solves the column in place, see test_slow_consistent_columns_*)
    import importlib.util
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    col = 21
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])
    assert d["resid"] < 1e-12

    def run():
        ctx = slc.Context([0])
        try:
            Px, Pu, info = slc.SLS_H2(P, S, [[col]], ctx=ctx, return_info=True, dropzeros=False)
        finally:
            ctx.close()
        got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
        return np.abs(got - z).max(), info
    err, info = run()
    assert info["col_status"][0] == 0 and info["n_refined"] == 1 and info["max_residual"] < 1e-12
    assert err < 1e-8
    os.environ["SLS_REFINE"] = "0"
    try:
        err0, info0 = run()
    finally:
        del os.environ["SLS_REFINE"]
    assert info0["n_refined"] == 0 and info0["col_status"][0] == 0 and err0 > 1e-6          # what the refinement is for


def test_one_shot_call_refines_on_every_device_slot(slc, oracle, monkeypatch):
    """Several devices (two slots of the one GPU here): each shard travels packed, so the refinement of a shard writes its own packed
    array and the host scatters it over the first pass's values.  The near-singular column must come out refined whichever
    shard it lands in, the other columns must equal the single-device call bit for bit."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")        # the stagnation rule of rounds 1–2: this test is about the refinement machinery (round 3's rule solves the column in place, see test_slow_consistent_columns_*)
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    col = 21
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])
    ctx1 = slc.Context([0])
    try:
        Px1, Pu1, info1 = slc.SLS_H2(P, S, ctx=ctx1, return_info=True, dropzeros=False)
    finally:
        ctx1.close()
    ctx2 = slc.Context([0, 0])
    try:
        Px2, Pu2, info2 = slc.SLS_H2(P, S, ctx=ctx2, return_info=True, dropzeros=False)
    finally:
        ctx2.close()
    assert info1["n_refined"] >= 1 and info2["n_refined"] == info1["n_refined"]
    assert np.array_equal(info1["col_status"], info2["col_status"])
    got = np.array([(Px2 if kind == 0 else Pu2)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
    assert np.abs(got - z).max() < 1e-8
    for A1, A2 in zip(Px1 + Pu1, Px2 + Pu2):
        assert np.array_equal(A1.toarray(), A2.toarray())


def test_resident_plan_refine_attaches_tile_pass(slc, oracle, monkeypatch):
    """The same column through the resident path: sls_plan_execute alone leaves the 2e-4 error (status OK, residual 4e-10);
    sls_plan_refine re-solves it on the tile kernel into the same device array, attaches that pass to the plan — a later execute
    into a fresh array is refined without another call — and the status read reports the refined residual.  A well-conditioned
    neighbour column in the same plan is left alone."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")        # the stagnation rule of rounds 1–2: this test is about the refinement machinery (round 3's rule solves the column in place, see test_slow_consistent_columns_*)
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    col = 21
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])

    def err_of(vx, vu):
        Px, Pu = slc.assemble_phi(S[0], S[1], vx, vu, dropzeros=False)
        got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
        return np.abs(got - z).max()
    ctx = slc.Context([0])
    plan = None
    try:
        plan = slc.Plan(ctx, P, S, [[col], [col + 1]])
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        st0, rs0, it0 = plan.fetch_status()
        e0 = err_of(*plan.download(dv))
        assert st0[0] == 0 and rs0[0] > 1e-11 and e0 > 1e-6                  # accepted, but only to residual/σ_min
        n = plan.refine(dv)
        # the neighbour is infeasible; flagged by a twisted kernel after three or more passes it gets the tile kernel's verdict too
        # (round 3), otherwise it is left alone
        nref = 2 if (st0[1] == 1 and it0[1] >= 3 and "twisted" in plan.describe()) else 1      # (flagged at the second pass: a plain infeasible column, not re-judged)
        assert n == nref
        st1, rs1, it1 = plan.fetch_status()
        assert st1[0] == 0 and rs1[0] < 1e-12 and it1[0] > it0[0]
        assert st1[1] == st0[1] and (nref == 2 or (rs1[1] == rs0[1] and it1[1] == it0[1]))    # the neighbour: same verdict (untouched unless re-judged)
        assert err_of(*plan.download(dv)) < 1e-8
        assert plan.refine(dv) == nref                                       # idempotent: the attached pass is reported, not rebuilt
        dv2 = plan.alloc_values()
        plan.execute(dv2); plan.synchronize()                                # the attached pass runs with every execute
        vx2, vu2 = plan.download(dv2)
        assert err_of(vx2, vu2) < 1e-8
        # ... in the packed layout too: the refinement numbers its free variables where the plan put them
        import torch
        pk = torch.zeros(plan.info["n_packed"], dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        plan.execute(pk.data_ptr(), packed=True); plan.synchronize()
        full = np.zeros(plan.info["n_values"]); full[plan.packed_dest()] = pk.cpu().numpy()
        assert np.array_equal(full, np.concatenate(vx2 + vu2))
    finally:
        if plan is not None:
            plan.close()
        ctx.close()


def test_column_sharded_refine_on_packed_shard(slc, oracle, monkeypatch):
    """ColumnShardedH2.refine on the packed path (always_gather off, but the packed buffer + unpack kernel forced through a
    non-direct solver): the first refine call happens in the PACKED layout, and the unpacked Φ of the next step carries the
    refined column."""
    monkeypatch.setenv("SLS_MAX_ITERS_SLOW", "0")        # the stagnation rule of rounds 1–2: this test is about the refinement machinery (round 3's rule solves the column in place, see test_slow_consistent_columns_*)
    import torch
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](77)
    col = 21
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])
    sh = slc.dist.ColumnShardedH2(P, S, [[col], [col + 1]], device="cuda:0")
    sh._direct = lambda: False                                               # take the packed buffer + unpack route of N > 1
    try:
        def err_now():
            v = sh.step().cpu().numpy()
            nx = [M.nnz for M in S[0]]; nu = [M.nnz for M in S[1]]
            cut = np.cumsum([0] + nx + nu)
            vx = [v[cut[t]:cut[t + 1]] for t in range(len(nx))]; vu = [v[cut[len(nx) + t]:cut[len(nx) + t + 1]] for t in range(len(nu))]
            Px, Pu = slc.assemble_phi(S[0], S[1], vx, vu, dropzeros=False)
            got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
            return np.abs(got - z).max()
        assert err_now() > 1e-6
        assert sh.refine() in (1, 2)             # 2: the infeasible neighbour, flagged by a twisted kernel, is re-judged on the tile kernel as well
        torch.cuda.synchronize()
        assert err_now() < 1e-8
    finally:
        sh.local.plan.close(); sh.ctx.close()


@pytest.mark.parametrize("T", [63, 70])
def test_long_horizon_one_wave_kernel(slc, T, monkeypatch):
    """Horizons around the 64-block boundary of the packed-block bookkeeping (one bit per block in a 64-bit mask; beyond T + 1 = 64
    blocks every block keeps its full image): ñx = 27 chain columns on the one-wave kernel against the C restatement."""
    monkeypatch.setenv("SLS_NO_TWISTED", "1")
    P = slc.workloads.chain_plant(64)
    S = list(slc.workloads.localization_masks(P.A, P.B2, 12, T, 1.5))
    cols = [0, 5, 20, 31, 32, 50, 63]
    ctx = slc.Context([0])
    try:
        plan = slc.Plan(ctx, P, S, [[c] for c in cols]); desc = plan.describe(); plan.close()
        assert "h2_column_wave_kernel<32," in desc, desc
        Phix, Phiu, info = slc.SLS_H2(P, S, [[c] for c in cols], ctx=ctx, return_info=True, dropzeros=False)
    finally:
        ctx.close()
    got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
    want, oinfo = _c_oracle_flat(slc, P, S, cols)
    assert oinfo["status"].max() == 0 and info["n_unsolved"] == 0
    assert np.abs(got - want).max() < TOL


def test_overlapping_groups_are_summed_like_the_reference(slc, gpu_ctx, readme, oracle):
    """A column listed in several groups: the reference solves it once per group (with that group's index sets) and adds the
    contributions — Φ̃ += [Φₓ Φᵤ] per group and the (+) fold of the workers, src/synthesis.jl:24,67.  The drop-in call does
    the same (layers of groups, summed); compared with the oracle's own `+=` accumulation, both index bases."""
    P, S, _ = readme
    I = [list(range(0, 20)), list(range(10, 30)), [25], [25], list(range(40, 45)), [44]]
    Po = oracle.OraclePlant(P.A, P.B1, P.B2)
    ox, ou = oracle.SLS_H2(Po, S, I)
    want = np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])])
    for base in (0, 1):
        Phix, Phiu, info = slc.SLS_H2(P, S, I, ctx=gpu_ctx, return_info=True, dropzeros=False, index_base=base)
        got = np.concatenate([flat_phi(Phix, S[0]), flat_phi(Phiu, S[1])])
        assert info["n_unsolved"] == 0 and len(info["col_status"]) == sum(len(g) for g in I) and np.all(info["col_status"] == 0)
        assert info["n_subproblems"] == sum(len(g) for g in I)
        assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max())
    # column 25 is in three groups: its Φ is not any single group's solution
    single = slc.SLS_H2(P, S, [[25]], ctx=gpu_ctx, dropzeros=False)
    c25 = np.abs(Phix[5][:, 25].toarray()).max() / max(np.abs(single[0][5][:, 25].toarray()).max(), 1e-300)
    assert c25 > 1.5
    # the resident-plan interface keeps one owner per column
    with pytest.raises(slc.SLSError) as ei:
        slc.Plan(gpu_ctx, P, S, groups=I)
    assert ei.value.code == slc._capi.SLS_EINVAL and "more than one group" in str(ei.value)


def test_batch_with_surplus_disturbance_channels_and_ridge(slc, gpu_ctx):
    """sls_h2_sf_solve_batch with a plant whose B1 / D11 have more columns than states (Nw > Nx) in FRONT of another plant, and
    non-identity B1 / D11: every plant must equal its own single call (the composite used to read another plant's B1 column).
    Then the ridge term of sls_set_ridge on a batch of equally sized plants: per-plant weights apply to every plant."""
    rng = np.random.default_rng(5)
    T = 16
    plants, masks = [], []
    for Nx, extra in ((23, 3), (40, 0), (23, 1)):
        base = slc.workloads.chain_plant(Nx)
        b = rng.uniform(0.5, 2.0, Nx)
        B1 = sp.hstack([sp.diags(b), sp.random(Nx, extra, density=0.5, random_state=Nx + extra, format="csc")]).tocsc() if extra else sp.diags(b).tocsc()
        q = rng.uniform(0.5, 2.0, Nx); r = rng.uniform(0.5, 2.0, base.Nu)
        C1 = sp.vstack([sp.diags(q), sp.csc_matrix((base.Nu, Nx))]).tocsc()
        D12 = sp.vstack([sp.csc_matrix((Nx, base.Nu)), sp.diags(r)]).tocsc()
        D11 = (sp.random(Nx + base.Nu, Nx + extra, density=0.05, random_state=7 * Nx + extra, format="csc") * 0.2).tocsc()
        P = slc.Plant(base.A, B1, base.B2, C1, D11, D12)
        plants.append(P)
        masks.append(list(slc.workloads.localization_masks(P.A, P.B2, 5, T, 1.5)))

    def flat(res, S):
        return np.concatenate([flat_phi(res[0], S[0]), flat_phi(res[1], S[1])])

    res, info = slc.SLS_H2_batch(plants, masks, ctx=gpu_ctx, return_info=True, dropzeros=False)
    for i, (P, S) in enumerate(zip(plants, masks)):
        Px, Pu, inf1 = slc.SLS_H2(P, S, ctx=gpu_ctx, return_info=True, dropzeros=False)
        assert np.array_equal(info["col_status"][i], inf1["col_status"])
        one = flat((Px, Pu), S)
        assert np.abs(one).max() > 0.1
        assert np.abs(flat(res[i], S) - one).max() <= 1e-10 * max(1.0, np.abs(one).max())
    ctx = slc.Context([0])
    try:
        same = [plants[0], plants[2]]; smasks = [masks[0], masks[2]]
        rx = rng.uniform(0.0, 2.0, 23); ru = rng.uniform(0.0, 2.0, same[0].Nu)
        ctx.set_ridge(rx, ru)
        resr = slc.SLS_H2_batch(same, smasks, ctx=ctx, dropzeros=False)
        for i, (P, S) in enumerate(zip(same, smasks)):
            one = flat(slc.SLS_H2(P, S, ctx=ctx, dropzeros=False), S)
            assert np.abs(flat(resr[i], S) - one).max() <= 1e-10 * max(1.0, np.abs(one).max())
            assert np.abs(flat(resr[i], S) - flat(res[0 if i == 0 else 2], S)).max() > 1e-3      # the term acts on every plant
        with pytest.raises(slc.SLSError):                                                          # a plant of another size in the batch
            slc.SLS_H2_batch(plants[:2], masks[:2], ctx=ctx)
        again = flat(slc.SLS_H2(same[0], smasks[0], ctx=ctx, dropzeros=False), smasks[0])        # the per-plant term is still in place
        assert np.abs(again - flat(resr[0], smasks[0])).max() <= 1e-10 * max(1.0, np.abs(again).max())
    finally:
        ctx.close()


def test_execute_batch_waits_for_pending_readers_of_its_outputs(slc, gpu_ctx):
    """sls_plan_execute_batch's fork edge: plans 1… run on their own streams, and must not overwrite d_values[i] while work
    enqueued on the caller's stream BEFORE the call still uses it.  The caller's stream is held busy, then writes a sentinel
    into every value array and snapshots it; the batch call enqueued after that must leave the SOLUTION in the arrays (without
    the edge plans 1… ran at once, and the late sentinel write destroyed their result)."""
    import torch
    dev = torch.device("cuda:0")
    specs = [(59, 9, 29), (40, 6, 20), (23, 6, 18)]
    plans, vals, want = [], [], []
    try:
        for Nx, d, T in specs:
            P = slc.workloads.chain_plant(Nx)
            S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, 1.5))
            p = slc.Plan(gpu_ctx, P, S)
            plans.append(p)
            vals.append(torch.zeros(p.info["n_values"], dtype=torch.float64, device=dev))
        st = torch.cuda.current_stream(dev)
        slc.execute_batch(plans, [v.data_ptr() for v in vals], stream=st.cuda_stream)
        st.synchronize()
        want = [v.clone() for v in vals]
        assert all(float(w.abs().max()) > 0.1 for w in want)
        for rep in range(3):
            big = torch.randn(4096, 4096, device=dev)
            for _ in range(40):                                  # tens of ms of work ahead of the sentinel writes
                big = torch.tanh(big @ big * 1e-3)
            snaps = []
            for v in vals:
                v.fill_(7.0)
                snaps.append(v.clone())
            slc.execute_batch(plans, [v.data_ptr() for v in vals], stream=st.cuda_stream)
            st.synchronize()
            for v, w, s in zip(vals, want, snaps):
                assert bool((s == 7.0).all())
                assert torch.equal(v, w)
    finally:
        for p in plans:
            p.close()


@pytest.mark.parametrize("routing", ["default", "one-wave", "tile-all"])
def test_slow_consistent_columns_are_solved_not_flagged(slc, oracle, routing, monkeypatch):
    """A feasible column whose constraint matrix is nearly rank deficient (tools/fuzz_h2.py seed 235, column 52: σ(E) = …, 1.7e-2,
    1.7e-5, 9.0e-7, then exact zeros; the reference hands such a column to Ipopt like any other, src/synthesis.jl:62): the multiplier
    iteration contracts by a constant 0.5–0.8 per pass.  Rounds 1–2 read that as stagnation and flagged the column infeasible at pass
    3; it is now carried to the residual target (still_contracting, sls_device.h) — on the twisted kernels through the drop-in
    call's tile-kernel verdict.  Status OK and |ΔΦ| ≤ residual/σ_min on every kernel routing; the neighbours are as before."""
    for k, v in {"default": {}, "one-wave": {"SLS_NO_TWISTED": "1"}, "tile-all": {"SLS_TILE": "all", "SLS_FORCE_GENERAL": "1"}}[routing].items():
        monkeypatch.setenv(k, v)
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](235)
    col = 52
    Po = oracle.OraclePlant(P.A, P.B1, P.B2, P.C1, P.D11, P.D12)
    z, oi, d = oracle.solve_group(Po, [col], S[0], S[1])
    assert d["resid"] < 1e-13                                     # feasible by the oracle's SVD
    ctx = slc.Context([0])
    try:
        Px, Pu, info = slc.SLS_H2(P, S, [[col], [col + 1]], ctx=ctx, return_info=True, dropzeros=False)
    finally:
        ctx.close()
    assert info["col_status"][0] == 0, info["col_status"]
    got = np.array([(Px if kind == 0 else Pu)[t][(oi["sx"] if kind == 0 else oi["su"])[r], col] for (t, kind, r, _) in oi["var_index"]])
    assert np.abs(got - z).max() < 2e-5                            # residual ≤ 1e-11 over σ_min = 9e-7


@pytest.mark.timeout(600)
def test_bench_collective_path_and_strong_record_on_one_rank():
    """bench.py --force-collective on one rank: everything `--gpus N` runs for N > 1 except a second process — RCCL process group,
    settle steps, pipelined all-gather + unpack of the weak-scaling line, and the extra "strong" record (chain-4096 sharded over
    the ranks, all-gather timed alone, cost imbalance of the cut).  The driver's N = 2, 4, 8 runs are the first time this code
    sees several GPUs: the one-rank rehearsal makes sure nothing in it can fail for a reason other than the rank count."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3",
                        "--force-collective", "--full", "--no-cpu-baseline"], capture_output=True, text=True, env=env, timeout=550)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 1 and d["config"]["unsolved_total"] == 0 and d["value"] > 1e4
    st = d["strong"]
    assert "error" not in st, st
    assert st["n_subproblems"] == 4096 and st["unsolved_total"] == 0 and st["subproblems_per_rank"] == [4096]
    assert st["ms_per_pass"] > 0 and st["all_gather_ms"] > 0 and abs(st["cost_imbalance_max_over_mean"] - 1.0) < 1e-9


@pytest.mark.parametrize("seed", [11, 65, 297])
def test_short_horizon_small_index_sets_take_the_two_wave_kernel(slc, seed, monkeypatch):
    """Ragged latency plans on short horizons (tools/fuzz_h2.py seeds 11, 65, 297: T = 4, 5, 6, index sets of 5–12 states merged into
    the launch's 32-lane class).  The four-wave kernel has an open defect there (residuals of 1e-8…1e-6 that do not contract, columns
    wrongly flagged infeasible — DESIGN §5.1, `sls_api.cpp`), so such launches are routed to the two-wave kernel: the resident plan's
    statuses must equal those of the one-wave kernel and every column both solve must agree to 1e-9.  With the fence lifted
    (SLS_T4_NMIN=0 SLS_T4_TMIN=0) the plan does take the four-wave kernel — the repro the fence is documented with."""
    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "fuzz_h2.py")
    ns = {"__file__": path}
    exec(compile(open(path).read().split("modes = {")[0], path, "exec"), ns)
    P, S, meta = ns["problem"](seed)
    ctx = slc.Context([0])
    try:
        def run():
            plan = slc.Plan(ctx, P, S)
            desc = plan.describe()
            d = plan.alloc_values(); plan.execute(d); plan.synchronize()
            st, rs, it = plan.fetch_status()
            vals = np.concatenate(sum(plan.download(d), []))
            plan.close()
            return desc, st, vals
        desc, st, vals = run()
        assert "h2_column_twisted_kernel" in desc and "twisted4" not in desc, desc
        monkeypatch.setenv("SLS_NO_TWISTED", "1")
        desc1, st1, vals1 = run()
        monkeypatch.delenv("SLS_NO_TWISTED")
        assert "h2_column_wave_kernel" in desc1
        assert np.array_equal(st == 0, st1 == 0)
        colidx = np.concatenate([np.repeat(np.arange(P.Nx), np.diff(M.indptr)) for M in S[0] + S[1]])
        ok = np.isin(colidx, np.flatnonzero(st == 0))
        assert np.abs(vals[ok] - vals1[ok]).max() < 1e-9
        monkeypatch.setenv("SLS_T4_NMIN", "0"); monkeypatch.setenv("SLS_T4_TMIN", "0")
        plan = slc.Plan(ctx, P, S)
        assert "h2_column_twisted4_kernel" in plan.describe()
        plan.close()
    finally:
        ctx.close()
