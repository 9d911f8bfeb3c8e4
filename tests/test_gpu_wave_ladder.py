"""The one-wave, two-wave and four-wave column kernels where an index set fills its size class, against the oracle.

These kernels size their lane grid, LDS carve and pivot tiles by a class (NPL, RPL) of capacity (64/NPL)·RPL = 12, 16, 20, 24,
28, 32, 40, 48 or 64 states, and a merged launch runs every column in the launch's largest class, rows from ñx up to the capacity
being padding.  A column with ñx equal to the capacity is the only one without padding: its last row group, the last lane of the
8×8 grid and the last pivot tile hold live data.  The uniform-mask chains of the other tests never get there (an interior column
has the odd size 2d + 3, every capacity is even, and the even end columns run in the class of the odd largest one).  Here
(tests/wave_cases.py): chain_plant(120) under a composite mask whose ladder columns have ñx = capacity − 1, capacity and
capacity + 1 for all nine capacities, as the problems
  act_all     B2 = I (ñu = ñx + 1 or + 2)
  readme_act  the README actuators (ñu = 4 … 23)
  weighted    act_all with diagonal LQR weights, B1 = diag(b) and a sparse D11
at T = 8, and act_all again at T = 2, 3, 4 (below T = 3 the twisted kernels hand over to the one-wave kernel) and T = 31, 32 (the
last horizon at which the one-wave kernel's `us` shares the matrix image on class <32,12>, and the first at which it has a block
of its own).  One test is one (problem, T, family) — family: "four" the default route, "two" SLS_TWISTED4=0, "one"
SLS_NO_TWISTED=1, "two_plds" SLS_P_LDS=1, "wave64" SLS_WAVE64=1 — and holds one plan per class, of that class's two or three
ladder columns alone, so that the launch's class is the class under test and its largest column fills it.  Three more plans sit
on the fences where a column leaves the wave kernels for the tile kernel (ñu = 63 | 65, ñu = 64 | 65, ñx = 64 | 65).  The host
twin tests/test_wave_cases_host.py proves without a GPU that every size is hit, which columns the reference finds feasible and
that every plan's launch list for 256 CUs is the pinned one.

Per plan: (1) the live describe() is the host's and names the pinned kernel, nsub and grid; (2) col_status is 0 exactly where the
reference finds the column feasible; (3) |Φ − Φ_ref| ≤ TOL = 1e-8 (oracle_c.TOL, the suite's bound) on every feasible column;
(4) Φ outside the plan's columns is exactly zero; (5) a second execute of the same plan is bit-identical.  The reference is the C
restatement of the oracle for the default weights and the NumPy oracle for "weighted", computed once per session per (problem, T)
and never modified.

Largest |Φ_gpu − Φ_ref| per family, measured on an MI355X (TOL = 1e-8; all 30 tests pass in 4.4 s, 0.02 – 0.45 s each):
  four      1.8e-11  (readme_act, <16,4> ñx = 16, which the default route gives to the two-wave kernel; four-wave classes 2.8e-14)
  two       1.8e-11  (the same column; 6.6e-13 at the most on the NPL = 32 classes)
  one       1.8e-09  (readme_act, <16,4> ñx = 16; 1.6e-10 at ñx = 12, 5.4e-10 at 15, 9.6e-11 at 24: the level at which the one-wave
                      kernel's multiplier iteration stops on this problem at every size, full class or not; 5.6e-15 on act_all)
  two_plds  1.1e-16
  wave64    4.3e-14  (readme_act; 3.8e-14 on act_all)
  fences    2.8e-14
act_all is at 5.8e-15 at the most on every family and horizon, weighted at 3.0e-14.
What the ladder sees, shown once with a value-only edit to a scratch copy of the kernels (never committed): the x-weight of row
capacity − 1 staged as padding (`lane < n && lane < NP − 1`) fails 23 of these 30 tests, every one at ñx = capacity only, on the
classes whose full column sits at the right end of the chain (16, 24, 32, 48: its last row is state 119, a live entry of Φx);
on a left-end column the last row is the boundary ring state, whose Φx is masked out, so this edit changes nothing there.
"""
import numpy as np
import pytest

import wave_cases as wc
from wave_cases import TOL

pytestmark = pytest.mark.gpu

worst = {}                                  # {family: worst |Φ − Φ_ref| seen this session}, printed by every test


def _device_ncu():
    import torch
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert ncu == wc.NCU, f"the cases of this module are pinned for {wc.NCU} compute units; this device reports {ncu}"


def _run_plan(slc, ctx, pr, groups):
    """A fresh plan of the given single-column groups, executed twice, each time into a zeroed value array of its own: describe(), the mask-order values and
    fetch_status() of the first execute, the values of the second."""
    plan = slc.Plan(ctx, pr["P"], pr["S"], groups)
    try:
        desc = plan.describe()
        d = plan.alloc_values()
        plan.execute(d); plan.synchronize()
        vals = np.concatenate(sum(plan.download(d), []))
        st = plan.fetch_status()[0].copy()
        d2 = plan.alloc_values()                                 # zeroed: the second execute has to write every value again
        plan.execute(d2); plan.synchronize()
        again = np.concatenate(sum(plan.download(d2), []))
    finally:
        plan.close()
    return desc, vals, st, again


def _check_case(slc, ctx, case, monkeypatch):
    _device_ncu()
    pr = wc.problem(slc, case["problem"], case["T"])
    ref = wc.reference(slc, case["problem"], case["T"])
    feasible = dict(zip(pr["targets"], ref["feasible"].tolist()))
    family = case.get("family", "fence")
    wc.set_knobs(monkeypatch, case["env"])
    report, failures = [], []
    for pl in wc.plans_of(case):
        groups = wc.groups_of(slc, pl["targets"])
        cls = "fence" if pl["cap"] is None else "<%d,%d>" % wc.CLASSES[wc.CAPS.index(pl["cap"])]
        desc, vals, st, again = _run_plan(slc, ctx, pr, groups)
        # (1) the live launch list
        assert desc == slc.dist.describe_launches(pr["P"], pr["S"], groups, None, wc.NCU), desc
        assert wc.short(desc) == pl["pinned"], desc
        assert len(st) == len(groups)
        mine = np.zeros(len(vals), dtype=bool)
        for label, (c,), s in zip(pl["targets"], groups, st.tolist()):
            tag = f"{family} {cls} ñx={label}"
            sel = pr["colidx"] == c
            mine |= sel
            # (2) statuses on every column of the plan
            if (s == 0) != feasible[label]:
                failures.append(f"{tag}: col_status {s}, reference {'feasible' if feasible[label] else 'infeasible'}")
            # (3) values on the feasible columns
            if feasible[label]:
                err = float(np.abs(vals[sel] - ref["flat"][sel]).max())
                report.append(f"{tag}: {err:.1e}")
                worst[family] = max(worst.get(family, 0.0), err)
                if not err <= TOL:
                    failures.append(f"{tag}: |Φ − Φ_ref| = {err:.2e} > {TOL:g}")
        # (4) nothing outside the plan's columns
        if np.any(vals[~mine] != 0.0):
            failures.append(f"{family} {cls}: {int(np.count_nonzero(vals[~mine]))} nonzero values outside the plan's columns")
        # (5) determinism
        if not np.array_equal(vals, again):
            failures.append(f"{family} {cls}: the second execute differs in {int(np.count_nonzero(vals != again))} values, "
                            f"by {np.abs(vals - again).max():.2e} at the most")
    print(f"{case['id']}: worst |Φ − Φ_ref| per (family, class, ñx):  " + ";  ".join(report))
    print("worst per family so far: " + ", ".join(f"{f} {e:.1e}" for f, e in sorted(worst.items())))
    assert not failures, f"{case['id']}: " + " | ".join(failures) + " || all columns: " + "; ".join(report)


@pytest.mark.parametrize("cid", wc.IDS)
def test_full_classes(slc, oracle, gpu_ctx, cid, monkeypatch):
    """One (problem, T, family): a plan per class whose largest column fills the class; the five checks of the module docstring."""
    _check_case(slc, gpu_ctx, wc.get(cid), monkeypatch)


@pytest.mark.parametrize("cid", wc.FENCE_IDS)
def test_fences(slc, oracle, gpu_ctx, cid, monkeypatch):
    """A two-column plan on a fence of wave_class_of: one column in class <64,64>, the other on the tile kernel."""
    _check_case(slc, gpu_ctx, wc.get(cid), monkeypatch)
