"""Host twin of tests/test_gpu_wave_ladder.py: everything about the wave kernels' size ladder (tests/wave_cases.py) that can be
proven without a GPU — the index-set sizes, the references' feasibility on every compared column, the launch list of every plan
for 256 CUs and the LDS step of the one-wave kernel's `us` alias — so that the shapes are known good before a GPU is used, and a
later change to the masks, the reduction or the routing cannot quietly take a full class off the ladder."""
import re

import numpy as np
import pytest

import wave_cases as wc

_SIZES = [11, 12, 13, 15, 16, 17, 19, 20, 21, 23, 24, 25, 27, 28, 29, 31, 32, 33, 39, 40, 41, 47, 48, 49, 63, 64, 65, 62, 63]


def test_capacities_are_the_library_s(slc):
    """CLASSES restates wave_class (sls_device.h): held to the header's own table, so that a new class cannot go untested."""
    import os
    with open(os.path.join(os.path.dirname(slc.__file__), "csrc", "sls_device.h")) as f:
        m = re.search(r"tab\[kNumWaveClasses\] = \{(.*?)\};", f.read())
    assert tuple((int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", m.group(1))) == wc.CLASSES
    assert wc.CAPS == (12, 16, 20, 24, 28, 32, 40, 48, 64)
    assert [wc.size_of(l) for l in wc.LABELS] == _SIZES and wc.SMALL == tuple(_SIZES[:18])
    lower = 0
    for cap, targets in wc.CLASS_TARGETS.items():
        # the columns of a class: every ladder size above the class below, the largest one on the capacity
        assert targets == tuple(n for n in wc.TARGETS[:27] if lower < n <= cap) and targets[-1] == cap
        lower = cap
    assert tuple(wc.CLASS_TARGETS) == wc.CAPS


@pytest.mark.parametrize("name", wc.PROBLEMS)
def test_ladder_hits_every_target_size(slc, oracle, name):
    """ñx of the 29 ladder columns is exactly the targets, by the oracle's reduction and by the library's own; the two agree on
    the index sets themselves, every column is in its own set, d_c ≤ 40, and the columns are three apart or more."""
    picks = wc.pick_columns(slc)
    assert [l for l, _, _ in picks] == list(wc.LABELS) and max(d for _, _, d in picks) <= 40
    cols = sorted(c for _, c, _ in picks)
    assert len(set(cols)) == 29 and min(np.diff(cols)) >= 3 and cols[0] >= 1 and cols[-1] <= wc.NX - 2
    ours = wc.index_sets(slc, name)
    lib = wc.library_index_sets(slc, name)
    assert [len(sx) for sx, _ in ours] == _SIZES
    assert [len(sx) for sx, _ in lib] == _SIZES
    for (sx, su), (lx, lu), (_, c, _) in zip(ours, lib, picks):
        assert np.array_equal(np.sort(sx), np.sort(lx)) and np.array_equal(np.sort(su), np.sort(lu))
        assert c in sx


def test_horizon_cut_keeps_the_index_sets(slc, oracle):
    """α = 128 gives every column its full width at the first step after t = 0: the index sets at T = 2, 3, 4, 31, 32 are the
    ladder's."""
    base = wc.index_sets(slc, "act_all")
    for Th in wc.CUT_T:
        assert len(wc.problem(slc, "act_all", Th)["S"][0]) == Th
        for (sx, su), (bx, bu) in zip(wc.index_sets(slc, "act_all", Th), base):
            assert np.array_equal(sx, bx) and np.array_equal(su, bu), Th


def test_input_counts_and_the_nu_fence(slc, oracle):
    """ñu as the issue of this ladder records it: ñx + 1 (end columns) or ñx + 2 (interior) on act_all, 4 … 23 on readme_act.
    The fence pair of wave_class_of: ñu = 64 on the end column with ñx = 63, 65 on the interior one; ñx = 62 has 63."""
    nu_all = {l: len(su) for l, (_, su) in zip(wc.LABELS, wc.index_sets(slc, "act_all"))}
    nu_rdm = {l: len(su) for l, (_, su) in zip(wc.LABELS, wc.index_sets(slc, "readme_act"))}
    for l, m in nu_all.items():
        assert m == wc.size_of(l) + (2 if wc.size_of(l) % 2 and l != "63e" else 1), (l, m)
    assert (min(nu_rdm.values()), max(nu_rdm.values())) == (4, 23), nu_rdm
    assert (nu_all[62], nu_all["63e"], nu_all[63], nu_all[64]) == (63, 64, 65, 65)
    for f in wc.FENCES:
        if f["nu"] is not None:
            assert tuple(nu_all[l] for l in f["targets"]) == f["nu"], f["id"]
    assert any(f["nu"] == (64, 65) for f in wc.FENCES)
    assert nu_rdm[64] <= 64 and nu_rdm[65] <= 64         # the readme_act fence is the one on ñx alone


@pytest.mark.parametrize("name,Th", [(p, wc.T) for p in wc.PROBLEMS] + [("act_all", Th) for Th in wc.CUT_T])
def test_reference_feasibility(slc, oracle, name, Th):
    """The cap on columns left out of the comparison: none on act_all (every horizon) and weighted; on readme_act exactly the
    column with ñx = 11, which the reference flags (status 1).  Every other column has status 0 and a residual under the
    project's bound (1e-12 for the C restatement, 1e-9 for the NumPy oracle), and max |Φ| above 0.1, so that the absolute
    tolerance means something."""
    pr, ref = wc.problem(slc, name, Th), wc.reference(slc, name, Th)
    n = {"act_all": 29, "readme_act": 28, "weighted": 18}[name] if Th == wc.T else 18
    assert len(pr["targets"]) == len(ref["status"]) == len(ref["resid"]) == n
    out = tuple(l for l, f in zip(pr["targets"], ref["feasible"]) if not f)
    assert out == wc.LEFT_OUT[name] and len(out) == (1 if name == "readme_act" else 0), (out, ref["status"], ref["resid"])
    for l, st, rs in zip(pr["targets"], ref["status"], ref["resid"]):
        if l in out:
            assert st != 0 and rs > 1e-6, (l, st, rs)            # flagged, and by a wide margin
        else:
            assert st == 0 and rs < wc.tile_cases.residual_bound(name), (l, st, rs)
    assert ref["big"][ref["feasible"]].min() > 0.1, ref["big"]
    print(f"{name} T={Th}: reference in {wc.oracle_seconds[(name, Th)]:.2f} s, worst residual of a compared column "
          f"{ref['resid'][ref['feasible']].max():.1e}, smallest max|Φ| {ref['big'][ref['feasible']].min():.3f}")


@pytest.mark.parametrize("cid", wc.IDS + wc.FENCE_IDS)
def test_wave_launch_lists_on_256_cus(slc, cid, monkeypatch):
    """Kernel selection alone, for 256 CUs: every plan of every case gets its pinned launch list (kernel with template
    arguments, nsub, grid == nsub).  A class plan is one launch in the class under test whose largest column fills the class
    (on act_all under SLS_WAVE64=1 the columns past the ñu fence show as a tile launch); a fence plan is one column in a wave
    class and one on the tile kernel."""
    case = wc.get(cid)
    pr = wc.problem(slc, case["problem"], case["T"])
    sizes = dict(zip(wc.LABELS, (len(sx) for sx, _ in wc.index_sets(slc, case["problem"], case["T"]))))
    wc.set_knobs(monkeypatch, case["env"])
    for pl in wc.plans_of(case):
        desc = slc.dist.describe_launches(pr["P"], pr["S"], wc.groups_of(slc, pl["targets"]), None, wc.NCU)
        assert wc.short(desc) == pl["pinned"], (pl["cap"], desc)
        L = wc.son_cases.launches(desc)
        assert all(grid == nsub for _, nsub, grid in L) and sum(nsub for _, nsub, _ in L) == len(pl["targets"]), desc
        wave = [(k, nsub) for k, nsub, _ in L if "tile" not in k]
        tile = [nsub for k, nsub, _ in L if "tile" in k]
        if pl["cap"] is None:
            assert len(wave) == 1 and wave[0][1] == 1 and tile == [1], desc
            continue
        assert len(wave) == 1 and wave[0][0].split("<")[1].startswith("%d,%d" % wc.CLASSES[wc.CAPS.index(pl["cap"])]), desc
        assert set(pl["targets"]) <= set(pr["targets"])          # every column of the plan has a reference
        if tile:
            assert cid == "act_all-T8-wave64" and pl["cap"] == 64 and tile == [2] and wave[0][1] == 1, desc
        else:
            assert max(sizes[l] for l in pl["targets"]) == pl["cap"], desc      # the largest column fills the class


def test_table_names_every_class_at_full_capacity():
    """Each of the nine one-wave classes, six two-wave classes and four four-wave classes appears in at least one pinned
    single-launch list of a plan whose largest column equals the capacity; every family, problem and horizon is in the table,
    and at T = 2 every family is pinned to the one-wave kernel."""
    full = {pl["pinned"].split(" ")[0] for c in wc.CASES for pl in c["plans"] if ";" not in pl["pinned"] and pl["targets"][-1] == pl["cap"]}
    for npl, rpl in wc.CLASSES:
        assert f"h2_column_wave_kernel<{npl},{rpl}>" in full, (npl, rpl)
    for npl, rpl in wc.CLASSES[:6]:
        assert f"h2_column_twisted_kernel<{npl},{rpl},P_in_workspace>" in full, (npl, rpl)
        assert f"h2_column_twisted_kernel<{npl},{rpl},P_in_LDS>" in full, (npl, rpl)
    for npl, rpl in wc.CLASSES[2:6]:
        assert f"h2_column_twisted4_kernel<{npl},{rpl}>" in full, (npl, rpl)
    assert {(c["problem"], c["T"], c["family"]) for c in wc.CASES} == (
        {(p, 8, f) for p in wc.PROBLEMS for f in ("four", "two", "one")}
        | {("act_all", 8, "two_plds"), ("act_all", 8, "wave64"), ("readme_act", 8, "wave64")}
        | {("act_all", Th, f) for Th in (2, 3, 4, 31, 32) for f in ("four", "two", "one")})
    for c in wc.CASES:
        assert [pl["cap"] for pl in c["plans"]] == list(wc.CAPS[6:] if c["family"] == "wave64" else wc.CAPS[:6]), c["id"]
        if c["T"] == 2:
            assert all(pl["pinned"].startswith("h2_column_wave_kernel<") for pl in c["plans"]), c["id"]
        elif c["family"] == "four":
            assert [pl["pinned"].split("<")[0] for pl in c["plans"]] == ["h2_column_twisted_kernel"] * 2 + ["h2_column_twisted4_kernel"] * 4


def test_us_alias_ends_between_T31_and_T32(slc, monkeypatch):
    """The one-wave kernel's `us` shares the matrix image while T·mcap ≤ NP·(NPL + 1) (wave_kernel_lds_bytes): on class <32,12>
    with the plan's mcap = 25 that is 775 ≤ 792 at T = 31 and 800 > 792 at T = 32, and the launch's LDS goes 37 312 → 44 272
    bytes — 6 960 = 8·(T·mcap at T = 32) + the horizon's own 560 bytes, the step of the classes that do not change layout."""
    mcap = max(len(su) for l, (_, su) in zip(wc.LABELS, wc.index_sets(slc, "act_all")) if l in wc.CLASS_TARGETS[24])
    assert mcap == 25 and 31 * mcap <= 24 * 33 < 32 * mcap
    wc.set_knobs(monkeypatch, wc.FAMILIES["one"])
    lds = {}
    for Th in (30, 31, 32):
        if Th in wc.CUT_T:
            pr = wc.problem(slc, "act_all", Th)
            P, S = pr["P"], pr["S"]
        else:
            P = wc.problem(slc, "act_all")["P"]
            S = wc.tile_cases.composite_masks(slc, P.A, P.B2, wc.pick_columns(slc), Th, wc.CUT_ALPHA)
        desc = slc.dist.describe_launches(P, S, wc.groups_of(slc, wc.CLASS_TARGETS[24]), None, wc.NCU)
        assert desc.startswith("h2_column_wave_kernel<32,12> "), desc
        lds[Th] = int(re.search(r"lds=(\d+)", desc).group(1))
    assert (lds[31], lds[32]) == (37312, 44272), lds
    assert lds[32] - lds[31] == (lds[31] - lds[30]) + 8 * 32 * mcap, lds
