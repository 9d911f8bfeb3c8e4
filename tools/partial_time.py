"""Resident plan: re-solving only the columns a local plant change touched against solving all of them.

Plant: chain-4096 (d = 12, T = 40).  Each step changes ONE entry of A (A[2048, 2048], alternating between two values, so every
step really changes it) through Plan.update_plant's device path, then solves:
  update + execute_dirty   tracking on: the update marks the touched subproblems, Plan.execute_dirty re-solves those
  update + execute         the same update, then the full Plan.execute
  execute                  the full execute alone
Per step, host clock around work that ends in a stream synchronise; same process, same device, the variants alternating round by
round; every timed window holds as many steps as fill --window seconds (default 0.5), sized from the warm-up.  At the end the
array kept current by execute_dirty is compared, bit for bit, with a full execute of the same plan.

--full-only times the full execute alone and needs nothing newer than Plan.execute; with --root DIR the package is imported from
another checkout (its own built library), which is how the commit before this feature is timed: alternate the two processes
in one job.
Usage: python tools/partial_time.py [--full-only] [--root DIR] [--rounds R] [--window S] [--json FILE]"""
import argparse, json, os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
import scipy.sparse as sp


def measure(slc_amd, torch, rounds, window, full_only):
    P, S, meta = slc_amd.workloads.make_workload("chain4096")
    S = [list(S[0]), list(S[1])]
    A = sp.csc_matrix(P.A)
    i = P.Nx // 2
    k = int(A.indptr[i] + np.flatnonzero(A.indices[A.indptr[i]:A.indptr[i + 1]] == i)[0])
    vals = [A.data.copy(), A.data.copy()]
    vals[1][k] += 0.05
    dev = [torch.from_numpy(a).to("cuda:0") for a in vals]
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    dv = torch.zeros(plan.info["n_values"], dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    out = {"workload": "chain4096", "Nx": P.Nx, "T": len(S[0]), "n_subproblems": int(plan.info["n_subproblems"]),
           "changed_entry": [i, i], "launches": plan.describe(), "full_only": bool(full_only)}
    state = {"k": 0}

    def step_execute():
        plan.execute(dv.data_ptr()); plan.synchronize()

    def step_update_full():
        state["k"] ^= 1
        plan.update_plant(A=dev[state["k"]])
        plan.execute(dv.data_ptr()); plan.synchronize()

    def step_update_dirty():
        state["k"] ^= 1
        plan.update_plant(A=dev[state["k"]])
        state["n_solved"] = plan.execute_dirty(dv.data_ptr()); plan.synchronize()

    variants = {"execute": step_execute}
    if not full_only:
        plan.track_changes()
        variants.update({"update+execute": step_update_full, "update+execute_dirty": step_update_dirty})
    steps = {}
    for name, f in variants.items():     # warm every variant (code objects, lazy buffers), then size its window
        for _ in range(3):
            f()
        t0 = time.perf_counter()
        for _ in range(5):
            f()
        steps[name] = max(5, int(np.ceil(window / ((time.perf_counter() - t0) / 5))))
    out["steps_per_window"] = steps
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            if name == "update+execute_dirty":          # the full variant left marks behind: the timed steps start clean, Φ current
                plan.execute(dv.data_ptr()); plan.clear_dirty(); plan.synchronize()
            n = steps[name]
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            times[name].append(1e3 * (time.perf_counter() - t0) / n)
    for name, v in times.items():
        out[name + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "rounds": len(v)}
    if not full_only:
        out["n_solved_per_step"] = int(state["n_solved"])
        kept = dv.cpu().numpy().view(np.uint64).copy()
        plan.execute(dv.data_ptr()); plan.synchronize()
        out["kept_equals_full_execute_bitwise"] = bool(np.array_equal(kept, dv.cpu().numpy().view(np.uint64)))
    out["n_not_ok"] = int((plan.fetch_status()[0] != 0).sum())
    plan.close(); ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--full-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import slc_amd
    import torch
    r = measure(slc_amd, torch, a.rounds, a.window, a.full_only)
    r["root"] = os.path.abspath(a.root)
    print(json.dumps(r), flush=True)
    line = f"chain4096: execute {r['execute_ms']['median']:.3f} ms"
    if not a.full_only:
        line += (f" | update+execute {r['update+execute_ms']['median']:.3f} ms | update+execute_dirty {r['update+execute_dirty_ms']['median']:.3f} ms"
                 f" ({r['n_solved_per_step']} of {r['n_subproblems']} subproblems) | bitwise equal to a full execute: {r['kept_equals_full_execute_bitwise']}")
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)
