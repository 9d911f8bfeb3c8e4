"""Golden launch lists: `Plan.describe()` of a fixed case list, recorded from LIVE plans on an MI355X.

   launch_lists.json   {"ncu": CU count of the recording device, "cases": {case name: describe string}}

tests/test_host.py recomputes every string without a device (sls_debug_describe_launches with the recorded CU count) and
compares character for character, so a routing change shows up on a machine without a GPU.  After an INTENDED routing change,
regenerate on the GPU box and review the diff of the JSON like code:
    python tests/golden/make_golden_launch_lists.py [OUTPUT.json]
The knobs of a case only act in lab mode; they are set around the construction of that one plan.
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "launch_lists.json")


def _case(name, plant, env=None, objective="h2", shard=None):
    return dict(name=name, plant=plant, env=dict(env or {}), objective=objective, shard=shard)


def cases(slc):
    c = [_case(w, w) for w in slc.workloads.WORKLOADS]
    for k in ("SLS_TWISTED4=0", "SLS_NO_TWISTED=1", "SLS_P_LDS=1", "SLS_VEC_GLOBAL=1"):
        c.append(_case("readme_chain/" + k, "readme_chain", dict([k.split("=")])))
    c.append(_case("chain59_T5", "chain59_T5"))                                       # trips the four-wave fence (T ≤ 6, ñx ≤ 12)
    c.append(_case("chain59_T5/fence_off", "chain59_T5", {"SLS_T4_NMIN": "0", "SLS_T4_TMIN": "0"}))
    c.append(_case("chain4096/SLS_ABSORB=0", "chain4096", {"SLS_ABSORB": "0"}))
    c.append(_case("chain4096/shard3of8", "chain4096", shard=(3, 8)))
    c.append(_case("chain512_d20/SLS_WAVE64=1", "chain512_d20", {"SLS_WAVE64": "1"}))
    for k in ("SLS_TILE=0", "SLS_TILE=large", "SLS_FORCE_GENERAL=1", "SLS_TILE_BIG=all", "SLS_TILE_BIG=0", "SLS_TILE_ONE_PER_CU=1"):
        c.append(_case("grid32/" + k, "grid32", dict([k.split("=")])))
    for w in ("chain4096", "grid32"):
        c.append(_case(w + "/sum_of_norms", w, objective="sum_of_norms"))
        c.append(_case(w + "/sum_of_norms/SLS_SON_TILE=1", w, {"SLS_SON_TILE": "1"}, objective="sum_of_norms"))
    c.append(_case("dense_hessian_chain", "dense_hessian_chain"))                     # tests/test_gpu_tile.py: general_weights_phi.npz
    c.append(_case("coupled_groups_chain", "coupled_groups_chain"))                   # tests/test_gpu_tile.py: coupled_group_phi.npz
    return c


_problems = {}


def problem(slc, plant):
    """(P, [Sx, Su], groups) of a case's plant key; cached, the masks of the large workloads take seconds."""
    if plant in _problems:
        return _problems[plant]
    wl = slc.workloads
    groups = None
    if plant in wl.WORKLOADS:
        P, S, _ = wl.make_workload(plant)
    elif plant == "chain59_T5":
        P = wl.chain_plant(59)
        S = list(wl.localization_masks(P.A, P.B2, 9, 5, 3.0))
    elif plant in ("dense_hessian_chain", "coupled_groups_chain"):
        coupled = plant == "coupled_groups_chain"
        g = np.load(os.path.join(HERE, "coupled_group_phi.npz" if coupled else "general_weights_phi.npz"))
        pre = "dense_" if coupled else ""
        Nx = int(g["Nx"])
        Pc = wl.chain_plant(Nx)
        Nz = Nx + Pc.Nu
        W = sp.csc_matrix((g[pre + "W_data"], g[pre + "W_indices"], g[pre + "W_indptr"]), shape=(Nz, Nz))
        D11 = sp.csc_matrix((g["D11_data"], g["D11_indices"], g["D11_indptr"]), shape=(Nz, Nx))
        if coupled:
            B1 = sp.csc_matrix((g["B1_data"], g["B1_indices"], g["B1_indptr"]), shape=(Nx, Nx))
            gp, gc = g["group_ptr"], g["group_cols"]
            groups = [[int(c) for c in gc[gp[i]:gp[i + 1]]] for i in range(len(gp) - 1)]
        else:
            B1 = sp.diags(g["b"]).tocsc()
        P = slc.Plant(Pc.A, B1, Pc.B2, W[:, :Nx], D11, W[:, Nx:])
        S = list(wl.localization_masks(P.A, P.B2, int(g["d"]), int(g["T"]), float(g["alpha"])))
    else:
        raise KeyError(plant)
    _problems[plant] = (P, S, groups)
    return _problems[plant]


def group_range(slc, case, P, S, groups):
    if case["shard"] is None:
        return None
    i, n = case["shard"]
    cuts = slc.dist.shard_groups(P, S, groups, n)
    return int(cuts[i]), int(cuts[i + 1])


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


def main():
    os.environ.setdefault("SLS_LAB", "1")
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    import slc_amd as slc
    import torch
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    ctx = slc.Context([0])
    out = {}
    for case in cases(slc):
        P, S, groups = problem(slc, case["plant"])
        with knobs(case["env"]):
            plan = slc.Plan(ctx, P, S, groups, group_range(slc, case, P, S, groups), objective=case["objective"])
            out[case["name"]] = plan.describe()
            plan.close()
        print(case["name"], "->", out[case["name"]], flush=True)
    ctx.close()
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump({"ncu": ncu, "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
