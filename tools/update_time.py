"""Resident plan: new plant values through Plan.update_plant against destroying and rebuilding the plan.

Per step, host clock around work that ends in a stream synchronise, same process, same device, the three variants alternating
round by round:
  update(host)   + execute   Plan.update_plant with NumPy nzval arrays (pinned staging), then Plan.execute
  update(device) + execute   Plan.update_plant with torch tensors already on the device, then Plan.execute
  rebuild        + execute   Plan.close() + Plan(...) on the new plant (symbolic pass, allocation, uploads), then Plan.execute
The plant alternates between P and perturb(P) of tests/update_cases.py (every stored value of A and B2 scaled by a factor in
[0.8, 1.2], seed 5), so every step really changes the numbers; at the end the updated plan's Φ is compared with the rebuilt
plan's on the same plant.  Every timed window holds as many steps as fill --window seconds (default 0.5), sized from the warm-up.
Usage: python tools/update_time.py [--rounds R] [--window S] [--json FILE] [workload ...]      (default: readme_chain chain4096)"""
import argparse, json, os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
import scipy.sparse as sp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import slc_amd
import torch
from update_cases import perturb


def measure(name, rounds, window):
    P, S, meta = slc_amd.workloads.make_workload(name)
    S = [list(S[0]), list(S[1])]
    plants = [P, perturb(P)]
    host = [(sp.csc_matrix(Q.A).data.copy(), sp.csc_matrix(Q.B2).data.copy()) for Q in plants]
    dev = [(torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")) for a, b in host]
    torch.cuda.synchronize()
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    dv = torch.zeros(plan.info["n_values"], dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    out = {"workload": name, "Nx": P.Nx, "T": len(S[0]), "n_values": int(plan.info["n_values"]), "nnz_A": int(host[0][0].size),
           "nnz_B2": int(host[0][1].size), "launches": plan.describe()}
    state = {"plan": plan, "k": 0}

    def step_update(src):
        state["k"] ^= 1
        a, b = src[state["k"]]
        state["plan"].update_plant(A=a, B2=b)
        state["plan"].execute(dv.data_ptr()); state["plan"].synchronize()

    def step_rebuild():
        state["k"] ^= 1
        state["plan"].close()
        state["plan"] = slc_amd.Plan(ctx, plants[state["k"]], S)
        state["plan"].execute(dv.data_ptr()); state["plan"].synchronize()

    def step_execute():
        state["plan"].execute(dv.data_ptr()); state["plan"].synchronize()

    variants = {"execute_only": step_execute, "update_host+execute": lambda: step_update(host),
                "update_device+execute": lambda: step_update(dev), "rebuild+execute": step_rebuild}
    steps = {}
    for k, f in variants.items():        # warm every variant (code objects, pinned buffer, cached arenas), then size its window
        for _ in range(3):
            f()
        t0 = time.perf_counter()
        for _ in range(5):
            f()
        steps[k] = max(5, int(np.ceil(window / ((time.perf_counter() - t0) / 5))))
    out["steps_per_window"] = steps
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            n = steps[k]
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            times[k].append(1e3 * (time.perf_counter() - t0) / n)
    for k, v in times.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "rounds": len(v)}
    # same plant through both routes: the updated plan against a rebuilt one
    plan = state["plan"]
    plan.update_plant(A=host[1][0], B2=host[1][1]); plan.execute(dv.data_ptr()); plan.synchronize()
    upd = dv.cpu().numpy().copy()
    assert plan.update_result() == 0
    plan.close()
    plan = slc_amd.Plan(ctx, plants[1], S)
    plan.execute(dv.data_ptr()); plan.synchronize()
    out["max_abs_diff_updated_vs_rebuilt"] = float(np.abs(upd - dv.cpu().numpy()).max())
    out["n_not_ok"] = int((plan.fetch_status()[0] != 0).sum())
    plan.close(); ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["readme_chain", "chain4096"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for w in a.workloads:
        r = measure(w, a.rounds, a.window)
        res.append(r)
        print(json.dumps(r), flush=True)
        u, d, b = (r[k + "_ms"]["median"] for k in ("update_host+execute", "update_device+execute", "rebuild+execute"))
        print(f"{w}: execute {r['execute_only_ms']['median']:.3f} ms | update(host)+execute {u:.3f} ms | update(device)+execute {d:.3f} ms | "
              f"rebuild+execute {b:.3f} ms | updated vs rebuilt max |ΔΦ| {r['max_abs_diff_updated_vs_rebuilt']:.1e}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
