"""Four-wave twisted kernel: the static blocks S_k built once per plan (twisted4_prepare_kernel) and loaded by the helper waves.

Block k of a column's Schur system has the static part S_k = δI + Wx_k + B̃·Wu_{k−1}·B̃ᵀ + Ã·Wx_{k−1}·Ãᵀ, which holds no factor
and depends only on what a plan fixes.  The prepare kernel builds, per column, δ and the slots a helper wave reads (slot k for
S_k, slot 0 for the upward helper's first block, where δ·w/(δ + w) stands in for Wx_0) with the arithmetic of the in-launch
rebuild; the solve kernel's default instantiation loads them, the other one (SLS_T4_PRESTATIC=0 in lab mode, or a pool beyond
the plan's byte budget) rebuilds them per launch as before.  What can go wrong is therefore (a) a block whose bits differ
from the rebuilt one, (b) a slot that is read but was not built, or built from the wrong time step, (c) a pool left stale by
sls_plan_update_plant, (d) a column that reads another column's pool in a selected run.

Cases: those of test_gpu_twisted4_static.py (imported: a 3-block ramp then 25 reuses; a 5-block ramp; the README-like ramp;
T = 8 and T = 7, where the downward helper rebuilds too; the <32,10> class; the weighted case; rows with 5 > 4 Ã and 3 > 2 B̃
entries) and `four_tile`: chain_plant(90), d = 12, T = 32, α = 1.5, columns range(33, 57, 2): ñx = 27, class <32,14>, 4×4
tiles and 10 stored doubles per lane (built like test_twisted_kernel_other_npl32_classes of test_gpu_parity.py).

Bounds.  Preloaded against rebuild: exact (np.array_equal) on Φ, statuses, pass counts and residuals; the preloaded Φ within
TOL = 1e-8 of the oracle (oracle_c.py; derivation: header of test_gpu_parity.py).  Pool against the NumPy restatement: every
entry is a sum of at most nzA + nzB + 1 ≤ 9 products of O(1) numbers, so ≈ 10 eps·max|S_k|: bound 1e-13·max|S_k|; δ to 1e-14
relative (one product and a maximum).  Plant update and selected columns: exact.

A four-wave launch always runs ONE column per workgroup: kernel selection takes the four-wave kernel only for at most one
column per compute unit and then sets grid = nsub (per_cu = 1; SLS_MAX_PER_CU cannot go below 1, SLS_FULL_GRID does not apply),
so none of the switches of test_gpu_column_reuse.py makes a workgroup of a full execute loop over columns.  The host twin
below asserts grid == nsub for every case; a selected run (execute_columns) also launches one workgroup per kept column.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_c import TOL, c_oracle_flat
from test_gpu_twisted4_static import CASES, _case
from test_gpu_twisted4_prepared import _index_sets, _masks_of, _bits

NCU = 256
FOUR_TILE = "four_tile"
FOUR_TILE_CLS = "h2_column_twisted4_kernel<32,14>"
_ALL = list(CASES) + [FOUR_TILE]
_DEFAULT_WEIGHT = [cid for cid in _ALL if cid != "banded_weighted"]
SENTINEL = 0x7FF8DEAD0000BEEF                 # a quiet-NaN pattern no solve produces

_cache = {}


def _get(slc, cid):
    """(P, S, columns, class string, Φ_oracle, oracle status): the imported cases plus the four-tile one; computed once."""
    if cid != FOUR_TILE:
        return _case(slc, cid)
    if cid not in _cache:
        d = 12
        P = slc.workloads.chain_plant(90)
        S = list(slc.workloads.localization_masks(P.A, P.B2, d, 2 * d + 8, 1.5))
        cols = list(range(33, 57, 2))
        want, oinfo = c_oracle_flat(slc, P, S, cols)
        ostatus = np.array(oinfo["status"])
        want.setflags(write=False); ostatus.setflags(write=False)
        _cache[cid] = (P, S, cols, FOUR_TILE_CLS, want, ostatus)
    return _cache[cid]


# ---- NumPy restatement ----

def _middle(T):
    return (T + 1) // 2 if T >= 7 else (T - 1) // 2


def _slots_read(T, up, down):
    """The slots the helpers read, by the rule in the prepare kernel's comment (twisted4_slot_read): the upward helper produces
    blocks 1 … c — block 1 from slot 0, block 2 always from slot 2, a later block k from slot k unless k < 64 and bit k of the
    upward word lets it reuse its predecessor's; the downward helper produces blocks T … c + 1 — block T always from slot T, a
    later block k from slot k unless k < 64 and bit k of the downward word is set."""
    c = _middle(T)
    read = set()
    if c >= 1:
        read.add(0)
    for k in range(2, c + 1):
        if k == 2 or not (k < 64 and (up >> k) & 1):
            read.add(k)
    for k in range(c + 1, T + 1):
        if k == T or not (k < 64 and (down >> k) & 1):
            read.add(k)
    return read


def _slots_read_by_walking(T, up, down):
    """The same set from a walk through the helper loops as the solve kernel runs them (a cached part exists after any fresh
    block but the upward first; the downward helper's share of the middle block is zeros)."""
    c = _middle(T)
    read = set()
    have = False
    for s in range(1, c + 1):                          # upward: block s
        if have and s < 64 and (up >> s) & 1 and s != 2:
            continue
        read.add(0 if s == 1 else s)
        have = have or s != 1
    have = False
    for s in range(1, T - c + 2):                      # downward: block T − s + 1
        k = T - s + 1
        if k == c or (have and k < 64 and (down >> k) & 1):
            continue
        read.add(k)
        have = True
    return read


def _column_setting(P, S, c):
    """Ã, B̃ (dense), the [T][n + m] mask of column c."""
    sx, su = _index_sets(P, S, c)
    At = sp.csr_matrix(sp.csc_matrix(P.A))[sx][:, sx].toarray()
    Bt = sp.csr_matrix(sp.csc_matrix(P.B2))[sx][:, su].toarray()
    return At, Bt, _masks_of(S, c, sx, su).astype(np.float64)


def _delta(At, Bt):
    return 1e-12 * (1.0 + (At * At).sum(axis=1) + (Bt * Bt).sum(axis=1)).max()


def _static_block(At, Bt, mask, delta, slot, NR):
    """Slot `slot` of a default-weight column as an NR × NR matrix (rows beyond ñx: δ on the diagonal)."""
    n, T = At.shape[0], mask.shape[0]
    k = max(slot, 1)
    wx = lambda t: mask[t, :n] if t < T else np.zeros(n)
    wp = wx(k - 1)
    if slot == 0:
        wp = delta * wp / (delta + wp)
    out = delta * np.eye(NR)
    out[:n, :n] += np.diag(wx(k)) + (At * wp) @ At.T + (Bt * mask[k - 1, n:]) @ Bt.T
    return out


def _stored_entries(Sfull, TR):
    """[TQ][64]: the entries of an (8·TR)² matrix in the pool's order — lane 8·a + b, tiles (ri, cj), ri ≤ cj, row-major."""
    a, b = np.divmod(np.arange(64), 8)
    return np.array([Sfull[a + 8 * ri, b + 8 * cj] for ri in range(TR) for cj in range(ri, TR)])


def _tile_rows(cls):
    return 3 if cls.endswith(("<32,10>", "<32,12>")) else 4


# ---- host twins (no GPU) ----

@pytest.mark.parametrize("cid", _ALL)
def test_cases_route_to_one_workgroup_per_column(slc, cid):
    P, S, cols, cls, want, ostatus = _get(slc, cid)
    desc = slc.dist.describe_launches(P, S, [[c] for c in cols], None, NCU)
    assert desc.startswith(cls + f" nsub={len(cols)} grid={len(cols)} ") and desc.count(";") == 1, desc
    assert np.all(ostatus == 0), ostatus


@pytest.mark.parametrize("cid", ["banded_ramp5", "banded_ramp_to_middle_T7"])
def test_restatement_is_the_diagonal_of_the_schur_system(slc, cid):
    """S_k is the k-th diagonal block of E·H⁻¹·Eᵀ + δI, where row block k of E reads −x_k + Ã·x_{k−1} + B̃·u_{k−1} (x_T does not
    exist) and H⁻¹ is the mask: the restatement is checked against that matrix built whole."""
    P, S, cols, cls, _, _ = _get(slc, cid)
    At, Bt, mask = _column_setting(P, S, cols[len(cols) // 2])
    n, m, T = At.shape[0], Bt.shape[1], mask.shape[0]
    nm = n + m
    E = np.zeros(((T + 1) * n, T * nm))
    for k in range(T + 1):
        if k < T:
            E[k * n:(k + 1) * n, k * nm:k * nm + n] = -np.eye(n)
        if k >= 1:
            E[k * n:(k + 1) * n, (k - 1) * nm:(k - 1) * nm + n] = At
            E[k * n:(k + 1) * n, (k - 1) * nm + n:k * nm] = Bt
    delta = _delta(At, Bt)
    M = (E * mask.ravel()) @ E.T + delta * np.eye((T + 1) * n)
    for k in range(1, T + 1):
        got = _static_block(At, Bt, mask, delta, k, 24)
        assert np.allclose(got[:n, :n], M[k * n:(k + 1) * n, k * n:(k + 1) * n], rtol=0, atol=1e-14)
        assert np.array_equal(got, got.T) and np.array_equal(got[n:, n:], delta * np.eye(24 - n))
    # slot 0: block 1 after block 0 = δI + Wx_0 (diagonal) has been eliminated
    w0 = mask[0, :n]
    schur = M[n:2 * n, n:2 * n] - At @ np.diag(w0 * (1.0 / (delta + w0)) * w0) @ At.T
    assert np.allclose(_static_block(At, Bt, mask, delta, 0, 24)[:n, :n], schur, rtol=0, atol=1e-12)


@pytest.mark.parametrize("cid", _ALL)
def test_slot_rule_equals_a_walk_through_the_helper_loops(slc, cid):
    P, S, cols, cls, _, _ = _get(slc, cid)
    T = len(S[0])
    c = _middle(T)
    for col in cols:
        sx, su = _index_sets(P, S, col)
        up, down = _bits(_masks_of(S, col, sx, su))
        read = _slots_read(T, up, down)
        assert read == _slots_read_by_walking(T, up, down)
        assert {0, 2, T} <= read and 1 not in read and max(read) == T
        assert T - 1 in read or T - 1 <= c            # block T − 1 never reuses block T's part: Wx_T = 0, so its bit is never set
    # the shapes the cases were chosen for (last column): blocks T and T − 1 are always fresh on the way down; a third fresh
    # block there means the ramp reaches the meeting block
    down_reads = len([k for k in read if k > c])
    if cid == "chain_ramp3_reuse25":
        assert len([k for k in read if 1 <= k <= c]) <= 4 and down_reads == 2, sorted(read)
    if cid in ("banded_ramp_to_middle_T8", "banded_ramp_to_middle_T7"):
        assert down_reads >= 3, sorted(read)


# ---- GPU ----

def _run(plan):
    dv = plan.alloc_values()
    plan.execute(dv); plan.synchronize()
    st, rs, it = (np.asarray(a).copy() for a in plan.fetch_status())
    return np.concatenate(sum(plan.download(dv), [])), st, rs, it


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ALL)
def test_preloaded_blocks_give_the_bits_of_the_rebuild(slc, gpu_ctx, cid, monkeypatch):
    P, S, cols, cls, want, ostatus = _get(slc, cid)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        desc = plan.describe()
        plan.twisted4_static()                                  # the default plan keeps a pool
        got, st, rs, it = _run(plan)
    finally:
        plan.close()
    monkeypatch.setenv("SLS_T4_PRESTATIC", "0")                 # lab mode (conftest.py): the rebuild instantiation
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        desc0 = plan.describe()
        with pytest.raises(slc._capi.SLSError):
            plan.twisted4_static()
        got0, st0, rs0, it0 = _run(plan)
    finally:
        plan.close()
    err = np.abs(got - want).max()
    print(f"{cid}: {desc} status {st.tolist()} residual {rs.max():.1e} passes {it.tolist()} max |Φ − Φ_oracle| = {err:.2e}, "
          f"max |Φ − Φ_rebuild| = {np.abs(got - got0).max():.2e}")
    assert cls in desc and desc == desc0, (desc, desc0)
    assert np.all(ostatus == 0) and np.all(st == 0), (ostatus, st, rs)
    assert np.array_equal(got, got0)
    assert np.array_equal(st, st0) and np.array_equal(it, it0) and np.array_equal(rs, rs0)
    assert err < TOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _DEFAULT_WEIGHT)
def test_pool_equals_numpy_restatement(slc, gpu_ctx, cid):
    P, S, cols, cls, _, _ = _get(slc, cid)
    T, TR = len(S[0]), _tile_rows(cls)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        assert cls in plan.describe()
        pool = plan.twisted4_static()
        bits = plan.twisted4_tables()["bits"]
    finally:
        plan.close()
    assert pool["valid"].shape == (len(cols), T + 1) and len(pool["blocks"]) == len(cols)
    worst = 0.0
    for i, c in enumerate(cols):
        At, Bt, mask = _column_setting(P, S, c)
        up, down = _bits(mask.astype(np.uint8))
        assert [int(b) for b in bits[i]] == [up, down]
        delta = _delta(At, Bt)
        assert abs(pool["delta"][i] - delta) <= 1e-14 * delta, (pool["delta"][i], delta)
        read = _slots_read(T, up, down)
        valid = set(np.flatnonzero(pool["valid"][i]).tolist())
        assert read <= valid, (c, sorted(read), sorted(valid))
        blocks = pool["blocks"][i]
        assert blocks.shape == (T + 1, TR * (TR + 1) // 2, 64)
        for slot in sorted(valid):
            exp = _stored_entries(_static_block(At, Bt, mask, pool["delta"][i], slot, 8 * TR), TR)
            dev = np.abs(blocks[slot] - exp).max() / np.abs(exp).max()
            worst = max(worst, dev)
            assert dev <= 1e-13, (c, slot, dev)
    print(f"{cid}: max |S − S_numpy| / max |S| = {worst:.2e} over the valid slots of {len(cols)} columns")


def _scaled(slc, P):
    A, B2 = sp.csc_matrix(P.A).copy(), sp.csc_matrix(P.B2).copy()
    A.data = A.data * 1.0625; B2.data = B2.data * 0.875
    return slc.Plant(A, P.B1, B2)


@pytest.mark.gpu
def test_plant_update_rebuilds_pool_and_delta(slc, gpu_ctx):
    """After sls_plan_update_plant with scaled A and B2 the pool, δ, the slot flags and Φ equal, bit for bit, those of a plan
    freshly built from the new values."""
    P, S, cols, cls, _, _ = _get(slc, "banded_ramp5")
    Q = _scaled(slc, P)
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    fresh = None
    try:
        before = plan.twisted4_static()
        _run(plan)
        plan.update_plant(A=Q.A, B2=Q.B2)
        after = plan.twisted4_static()
        got, st, rs, it = _run(plan)
        fresh = slc.Plan(gpu_ctx, Q, S, [[c] for c in cols])
        ref = fresh.twisted4_static()
        got_f, st_f, rs_f, it_f = _run(fresh)
    finally:
        plan.close()
        if fresh is not None:
            fresh.close()
    assert not np.array_equal(before["delta"], after["delta"])               # the update changed something
    assert np.array_equal(after["delta"].view(np.uint64), ref["delta"].view(np.uint64))
    assert np.array_equal(after["valid"], ref["valid"]) and np.array_equal(after["valid"], before["valid"])
    for a, r in zip(after["blocks"], ref["blocks"]):
        assert np.array_equal(a.view(np.uint64), r.view(np.uint64))
    assert np.all(st == 0) and np.array_equal(st, st_f) and np.array_equal(it, it_f) and np.array_equal(rs, rs_f)
    assert np.array_equal(got, got_f)


@pytest.mark.gpu
def test_selected_columns_read_their_own_pool(slc, gpu_ctx):
    """execute_columns on a strict subset that does not start at column 0: the kept columns' entries equal the full run's bit
    for bit, every other entry keeps the sentinel."""
    import torch
    P, S, cols, cls, _, _ = _get(slc, "banded_ramp5")
    subs = [2, 3, 5, 7]
    plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
    try:
        n = plan.info["n_values"]
        q_of = -np.ones(P.Nx, dtype=np.int64)
        q_of[np.asarray(cols)] = np.arange(len(cols))
        owner = -np.ones(n, dtype=np.int64)
        for masks, offs in ((S[0], plan.off_x), (S[1], plan.off_u)):
            for t, M in enumerate(masks):
                M = sp.csc_matrix(M); M.sort_indices()
                owner[offs[t]:offs[t + 1]] = q_of[np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))]
        arrays = []
        for run in ("full", "subset"):
            v = torch.from_numpy(np.full(max(n, 1), SENTINEL, dtype=np.uint64).view(np.float64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            if run == "full":
                plan.execute(v.data_ptr())
            else:
                assert plan.execute_columns(v.data_ptr(), subs) == len(subs)
            plan.synchronize()
            arrays.append(v.cpu().numpy().view(np.uint64)[:n].copy())
        st = plan.fetch_status()[0].copy()
    finally:
        plan.close()
    full, part = arrays
    kept = np.isin(owner, subs)
    assert kept.any() and np.all(st == 0)
    assert np.all(full[owner >= 0] != SENTINEL)
    assert np.array_equal(part[kept], full[kept])
    assert np.all(part[~kept] == SENTINEL)
