"""Four-wave twisted kernel: the chain wave takes its scaled pivot row from the record it publishes for the helper.

What moved: the chain wave's owner lanes of pivot p + 1 (lane-grid row (p + 1) mod 8) scale their row with the predicted
reciprocal and publish it — the record the helper reads, flag included — right after the FMAs of pivot p that touch it, and every
lane of the chain wave reads the record of its grid column back instead of fetching the row with ds_bpermute and scaling it a
second time.  Pivot 0 of a block is published behind receive(); the last pivot of a block publishes nothing.  Same operands,
same operations, same hand-off rule: Φ, residuals, status words and pass counts must be those of the commit before, bit for
bit (tests/golden/twisted4_records_parent.npz, recorded on the device with that commit's library by
make_golden_twisted4_records.py).  Two further exchanges through records — the pivot column, and the helper's column form of X —
were measured slower and are not in the kernel; they passed these tests too.

What can go wrong: a record read before its store or from another pivot's slot (shows at every size), the publish of a pivot
that is not eliminated or a missing one at the last pivot (ñx not a multiple of 8: 13, 16 | 17, 19, 21, 23), the owner row's wrap at
p = 8 and 16 (every case), the full grid ñx = 24 (c12_top24), the shortest horizon (c10_T7: halves of 4 and 3 blocks), records of a
later block overwriting those the helper still reads, or a flag raised for a record not yet stored (long halves: c10_T17_mix,
load_path), the second pass (load_path), weighted columns, the four-tile class with its six-double records (four_tile).

Cases, plants, masks and bounds are those of test_gpu_twisted4_tilesweep.py (its header derives them): against the two-wave
kernel equal statuses and pass counts and |ΔΦ| < 1e-9, the default-weight cases against the C oracle at TOL.  Each case runs
once under the default plan, once under SLS_T4_PRESTATIC=0 and once on the two-wave kernel; the tests share the runs.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle_c import TOL
from test_gpu_twisted4_tilesweep import CASES, FOUR, TWO, NCU, _case, _run

RECORD_CASES = ("c10_T7", "c12_mix", "c12_top24", "c10_T17_mix", "load_path", "weighted", "four_tile")
CLASS_OF = {"c10_T7": "<32,10>", "c10_T17_mix": "<32,10>", "c12_mix": "<32,12>", "c12_top24": "<32,12>", "load_path": "<32,12>",
            "weighted": "<32,12>", "four_tile": "<32,14>"}
PLANS = (("pre", {}), ("rebuild", {"SLS_T4_PRESTATIC": "0"}))

_runs = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "twisted4_records_parent.npz"))


def _all(slc, gpu_ctx, cid, monkeypatch):
    """The case under the default plan, the rebuild instantiation and the two-wave kernel: run once, never modified."""
    if cid not in _runs:
        P, S, cols, cls, _, _ = _case(slc, cid)
        out = {}
        for key, env, name in (PLANS[0] + (FOUR + cls,), PLANS[1] + (FOUR + cls,), ("two", {"SLS_TWISTED4": "0"}, TWO + "<")):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                plan = slc.Plan(gpu_ctx, P, S, [[c] for c in cols])
                try:
                    desc = plan.describe()
                    assert name in desc and desc.count(";") == 1, desc
                    res = _run(plan)
                finally:
                    plan.close()
            for a in res:
                a.setflags(write=False)
            out[key] = res
        _runs[cid] = out
    return _runs[cid]


# ---- host (no GPU) ----

@pytest.mark.parametrize("cid", RECORD_CASES)
def test_record_cases_exist_and_route_to_their_class(slc, cid):
    assert cid in CASES and CASES[cid][6] == CLASS_OF[cid]
    P, S, cols, cls, _, _ = _case(slc, cid)
    desc = slc.dist.describe_launches(P, S, [[c] for c in cols], None, NCU)
    assert desc.startswith(FOUR + CLASS_OF[cid] + f" nsub={len(cols)} grid={len(cols)} ") and desc.count(";") == 1, desc


def test_record_cases_cover_the_edges_they_are_chosen_for(slc):
    nx = {cid: CASES[cid][5] for cid in RECORD_CASES}
    assert CASES["c10_T7"][2] == 7                                          # the shortest four-wave horizon
    assert any(n % 8 for cid in RECORD_CASES for n in nx[cid])              # a guarded last pivot that is not a tile edge
    assert 16 in nx["c10_T17_mix"] and 17 in nx["c10_T17_mix"]              # … and the tile edge itself, both sides
    assert min(min(v) for v in nx.values()) > 8 and max(nx["c12_top24"]) == 24      # the owner row wraps; the full three-tile grid
    assert not _case(slc, "weighted")[0].default_weights
    assert CLASS_OF["four_tile"] == "<32,14>" and max(nx["four_tile"]) > 24


def test_golden_holds_every_case_under_both_plans(golden):
    want = {f"{cid}/{key}/{part}" for cid in RECORD_CASES for key, _ in PLANS for part in ("phi", "status", "resid", "passes")}
    assert set(golden.files) == want
    for cid in RECORD_CASES:
        assert golden[f"{cid}/pre/phi"].dtype == np.float64 and np.count_nonzero(golden[f"{cid}/pre/phi"]) > 0
        assert len(golden[f"{cid}/pre/status"]) == len(CASES[cid][4])
    assert golden["load_path/pre/passes"].max() >= 2                        # the second pass is in the recording


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("key", [k for k, _ in PLANS])
@pytest.mark.parametrize("cid", RECORD_CASES)
def test_bits_of_the_parent_commit(slc, gpu_ctx, golden, cid, key, monkeypatch):
    got, st, rs, it = _all(slc, gpu_ctx, cid, monkeypatch)[key]
    g = {part: golden[f"{cid}/{key}/{part}"] for part in ("phi", "status", "resid", "passes")}
    print(f"{cid} [{key}]: status {st.tolist()} passes {it.tolist()} residual {rs.max():.1e}; max |Φ − Φ_parent| = {np.abs(got - g['phi']).max():.2e}, "
          f"{np.count_nonzero(got.view(np.uint64) != g['phi'].view(np.uint64))} of {got.size} values differ in bits")
    assert got.shape == g["phi"].shape
    assert np.array_equal(got.view(np.uint64), g["phi"].view(np.uint64))
    assert np.array_equal(rs.view(np.uint64), g["resid"].astype(rs.dtype).view(np.uint64))
    assert np.array_equal(st, g["status"]) and np.array_equal(it, g["passes"])


@pytest.mark.gpu
@pytest.mark.parametrize("key", [k for k, _ in PLANS])
@pytest.mark.parametrize("cid", RECORD_CASES)
def test_against_two_wave_kernel_and_oracle(slc, gpu_ctx, cid, key, monkeypatch):
    want = _case(slc, cid)[4]
    r = _all(slc, gpu_ctx, cid, monkeypatch)
    (got, st, rs, it), (ref, st2, rs2, it2) = r[key], r["two"]
    dev = np.abs(got - ref).max()
    err = np.abs(got - want).max() if want is not None else float("nan")
    print(f"{cid} [{key}]: status {st.tolist()} / {st2.tolist()} passes {it.tolist()} / {it2.tolist()} max |Φ4 − Φ2| = {dev:.2e}, max |Φ4 − Φ_oracle| = {err:.2e}")
    assert np.array_equal(st, st2), (st, st2)
    assert np.array_equal(it, it2), (it, it2)
    assert dev < 1e-9, dev
    if cid == "load_path":
        assert it.max() >= 2 and it2.max() >= 2, (it, it2)
    if want is not None:
        assert np.all(st == 0), (st, rs)
        assert err < TOL, err
