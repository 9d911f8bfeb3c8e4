"""Resident plan: new LQR weights through Plan.update_weights against destroying and rebuilding the plan.

Per step, host clock around work that ends in a stream synchronise, same process, same device, the variants alternating round by
round (the method of tools/update_time.py):
  execute                     Plan.execute alone on the weighted plan the update variants work on
  execute (flagged)           Plan.execute on a plan of the identity-weight plant built with updatable_weights=True (hinv = 1 records)
  execute (unflagged)         Plan.execute on a plan of the same identity-weight plant without the flag (no weight records)
  update(host)   + execute    Plan.update_weights with NumPy diagonals (pinned staging), then Plan.execute
  update(device) + execute    Plan.update_weights with torch tensors already on the device, then Plan.execute
  rebuild        + execute    Plan.close() + Plan(..., updatable_weights=True) on the re-weighted plant, then Plan.execute
The weights alternate between the two draws of tests/weights_cases.py (seeds 11 and 12: every diagonal value in [0.5, 2]), so
every step really changes the numbers; at the end the updated plan's Φ is compared with the rebuilt plan's on the same weights.
Every timed window holds as many steps as fill --window seconds (default 0.5), sized from the warm-up.
Usage: python tools/weights_time.py [--rounds R] [--window S] [--json FILE] [workload ...]      (default: readme_chain chain4096)"""
import argparse, json, os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import slc_amd
import torch
from weights_cases import SEED_A, SEED_B, diagonals, with_weights


def measure(name, rounds, window):
    P, S, meta = slc_amd.workloads.make_workload(name)
    S = [list(S[0]), list(S[1])]
    host = [diagonals(P, SEED_A), diagonals(P, SEED_B)]
    plants = [with_weights(P, c, d) for c, d in host]
    dev = [(torch.from_numpy(c).to("cuda:0"), torch.from_numpy(d).to("cuda:0")) for c, d in host]
    torch.cuda.synchronize()
    ctx = slc_amd.Context([0])
    plain = slc_amd.Plan(ctx, P, S)                                    # identity weights, no flag: no weight records
    ident = slc_amd.Plan(ctx, P, S, updatable_weights=True)            # identity weights, flag: hinv = 1 records
    plan = slc_amd.Plan(ctx, plants[0], S, updatable_weights=True)
    dv = torch.zeros(plan.info["n_values"], dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    out = {"workload": name, "Nx": P.Nx, "Nu": P.Nu, "T": len(S[0]), "n_values": int(plan.info["n_values"]), "launches": plan.describe(),
           "launches_unflagged": plain.describe()}
    state = {"plan": plan, "k": 0}

    def step_update(src):
        state["k"] ^= 1
        c, d = src[state["k"]]
        state["plan"].update_weights(C1=c, D12=d)
        state["plan"].execute(dv.data_ptr()); state["plan"].synchronize()

    def step_rebuild():
        state["k"] ^= 1
        state["plan"].close()
        state["plan"] = slc_amd.Plan(ctx, plants[state["k"]], S, updatable_weights=True)
        state["plan"].execute(dv.data_ptr()); state["plan"].synchronize()

    def step_of(p):
        def f():
            p.execute(dv.data_ptr()); p.synchronize()
        return f

    def step_execute():
        state["plan"].execute(dv.data_ptr()); state["plan"].synchronize()

    variants = {"execute_only": step_execute, "execute_flagged": step_of(ident), "execute_unflagged": step_of(plain), "update_host+execute": lambda: step_update(host),
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
    # same weights through both routes: the updated plan against a rebuilt one
    plan = state["plan"]
    plan.update_weights(C1=host[1][0], D12=host[1][1]); plan.execute(dv.data_ptr()); plan.synchronize()
    upd = dv.cpu().numpy().copy()
    assert plan.update_weights_result() == 0
    plan.close()
    plan = slc_amd.Plan(ctx, plants[1], S, updatable_weights=True)
    plan.execute(dv.data_ptr()); plan.synchronize()
    out["max_abs_diff_updated_vs_rebuilt"] = float(np.abs(upd - dv.cpu().numpy()).max())
    out["n_not_ok"] = int((plan.fetch_status()[0] != 0).sum())
    plan.close(); ident.close(); plain.close(); ctx.close()
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
        m = {k: r[k + "_ms"]["median"] for k in ("execute_only", "execute_flagged", "execute_unflagged", "update_host+execute", "update_device+execute", "rebuild+execute")}
        print(f"{w}: execute {m['execute_only']:.3f} ms | identity plant: flagged {m['execute_flagged']:.3f} ms, unflagged {m['execute_unflagged']:.3f} ms | update(host)+execute "
              f"{m['update_host+execute']:.3f} ms | update(device)+execute {m['update_device+execute']:.3f} ms | rebuild+execute "
              f"{m['rebuild+execute']:.3f} ms | updated vs rebuilt max |ΔΦ| {r['max_abs_diff_updated_vs_rebuilt']:.1e}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
