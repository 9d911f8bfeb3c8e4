"""Golden plan footprints: what plan construction leaves observable, recorded from LIVE plans on an MI355X.

   plan_footprints.json   {"commit": the commit whose build was recorded, "ncu": CU count of the recording device,
                           "cases": {case name: {"workspace_bytes", "n_packed", "n_values", "describe"} or {"refused": text}},
                           "residual": {"res_inf", "halo_inf", "res_l1", "totals"} of the block-diagonal plant}

tests/test_gpu_plan_build.py builds every case again and asserts equality, so a change of plan construction (arena layout, scratch
workspace, four-wave pools, kernel selection) that moves a byte shows up.  The numbers must come from the build BEFORE such a
change: check out and build that commit elsewhere, then run, from this tree and on the GPU box,
    python tests/golden/make_golden_plan_footprints.py COMMIT --lib /path/to/that/libsls_mi355x.so [OUTPUT.json]
(without --lib the library of this tree is recorded).  Review the diff of the JSON like code.
The knobs of a case only act in lab mode; they are set around the construction of that one plan.
`Plan` always builds the packed layout (sls_h2_sf_plan); the plans without it belong to the one-shot calls, which show no footprint.
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "plan_footprints.json")


def _case(name, plant="readme_chain", env=None, objective="h2", route="masks", updatable_weights=False, group_range=None):
    return dict(name=name, plant=plant, env=dict(env or {}), objective=objective, route=route, updatable_weights=updatable_weights,
                group_range=group_range)


def cases():
    return [
        _case("readme_chain"),
        _case("readme_chain/shard", group_range=(20, 41)),
        _case("readme_chain/weights_updatable", updatable_weights=True),
        _case("readme_chain/localized", route="localized"),
        _case("readme_chain/SLS_T4_PRESTATIC=0", env={"SLS_T4_PRESTATIC": "0"}),
        _case("readme_chain/SLS_TWISTED4=0", env={"SLS_TWISTED4": "0"}),
        _case("readme_chain/SLS_HOST_TABLES=1", env={"SLS_HOST_TABLES": "1"}),
        _case("grid6", plant="grid6"),
        _case("chain40_T3/sum_of_norms", plant="chain40_T3", objective="sum_of_norms"),
        _case("readme_chain/empty_shard", group_range=(7, 7)),
    ]


_problems = {}


def problem(slc, plant):
    """(P, [Sx, Su], (d, T, alpha)) of a plant key, cached."""
    if plant not in _problems:
        wl = slc.workloads
        if plant == "readme_chain":
            P, dTa = wl.chain_plant(59), (9, 29, 1.5)
        elif plant == "grid6":                         # 36 states, index sets up to the whole grid: several launches
            P, dTa = wl.grid_plant(6, 3), (5, 8, 1.5)
        elif plant == "chain40_T3":
            P, dTa = wl.chain_plant(40), (2, 3, 1.5)
        elif plant == "chain24_T4":
            P, dTa = wl.chain_plant(24), (3, 4, 1.5)
        elif plant == "two_blocks":                    # 2 blocks of 3 states, T = 2, (A≠0)² at t = 1: every index set is its block, no halo row
            A3 = wl.chain_plant(3).A
            A = sp.block_diag([A3, A3], format="csc")
            B2 = sp.identity(6, format="csc")[:, [0, 3]]
            P, dTa = slc.Plant(A, sp.identity(6, format="csc"), B2), (3, 2, 2.0)
        else:
            raise KeyError(plant)
        _problems[plant] = (P, list(wl.localization_masks(P.A, P.B2, *dTa)), dTa)
    return _problems[plant]


class knobs:
    """The case's SLS_* variables, set for the duration of one plan construction."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(slc, ctx, case):
    """The case's live plan on `ctx`."""
    P, S, (d, T, alpha) = problem(slc, case["plant"])
    with knobs(case["env"]):
        if case["route"] == "localized":
            return slc.Plan.localized(ctx, P, d, T, alpha, objective=case["objective"], updatable_weights=case["updatable_weights"])
        return slc.Plan(ctx, P, S, None, case["group_range"], objective=case["objective"], updatable_weights=case["updatable_weights"])


def footprint(slc, ctx, case):
    """What the golden file holds of a case: built on a context that lends its arena, scratch and streams (no other plan alive)."""
    try:
        plan = build(slc, ctx, case)
    except slc._capi.SLSError as e:
        return {"refused": str(e)}
    try:
        return {"workspace_bytes": int(plan.info["workspace_bytes"]), "n_packed": int(plan.info["n_packed"]),
                "n_values": int(plan.info["n_values"]), "describe": plan.describe()}
    finally:
        plan.close()


def two_blocks_residual(slc, ctx):
    """sls_plan_fetch_residual of the solved block-diagonal plant: a plan whose halo list is empty."""
    P, S, _ = problem(slc, "two_blocks")
    plan = slc.Plan(ctx, P, S)
    try:
        dv = plan.alloc_values()
        plan.execute(dv); plan.synchronize()
        r = plan.residual(dv)
        return {"res_inf": [float(v) for v in r[0]], "halo_inf": [float(v) for v in r[1]], "res_l1": [float(v) for v in r[2]],
                "totals": [float(r[3]), float(r[4])]}
    finally:
        plan.close()


def main():
    os.environ.setdefault("SLS_LAB", "1")
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    args = sys.argv[1:]
    lib = None
    if "--lib" in args:
        i = args.index("--lib")
        lib = args[i + 1]
        del args[i:i + 2]
    if not args:
        raise SystemExit(__doc__)
    import slc_amd as slc
    if lib:
        slc._capi.LIB_PATH = os.path.abspath(lib)
    import torch
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    out = {}
    for case in cases():
        ctx = slc.Context([0])
        out[case["name"]] = footprint(slc, ctx, case)
        ctx.close()
        print(case["name"], "->", out[case["name"]], flush=True)
    ctx = slc.Context([0])
    res = two_blocks_residual(slc, ctx)
    ctx.close()
    print("two_blocks residual ->", res, flush=True)
    with open(args[1] if len(args) > 1 else OUT, "w") as f:
        json.dump({"commit": args[0], "ncu": ncu, "cases": out, "residual": res,
                   "how": "python tests/golden/make_golden_plan_footprints.py COMMIT --lib LIBRARY_OF_THAT_COMMIT (see the script's header)"},
                  f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
