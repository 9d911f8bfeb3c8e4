"""Robust-stability margins of an ensemble (sls_margin_run: three launches for all scenarios) against what a user had to do before
for the 𝓔₁ half alone: per scenario `Plan.update_plant` + `Plan.residual`, which overwrites the plan's design values and gives
column sums only.  sls_margin_run: HIP events around a batch of calls enqueued back to back on one stream, the batch sized from the
warm-up round to last about 0.2 s (50 … 5000 calls).  The loop waits on the host in every residual, so it is timed by the wall
clock around nscen update + residual pairs and reported per scenario and per ensemble.  Both contenders alternate in one process for ROUNDS rounds after a warm-up round; median (min – max).  Also printed:
n_defect, device bytes, and the first-call cost (plan + load + the first fetch, wall clock).
Usage: python tools/margin_time.py [workload:nscen ...]      (default: readme_chain:1 readme_chain:64 chain4096:64)"""
import os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import slc_amd

ROUNDS, WINDOW_MS = 7, 200.0

def measure(name, nscen):
    P, S, meta = slc_amd.workloads.make_workload(name)
    dev = torch.device("cuda:0")
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    d = plan.alloc_values(); plan.execute(d); plan.synchronize()
    plan.residual(d)                                              # the plan's first residual builds its halo lists: not counted
    a0, b0 = (np.array(v) for v in plan.plant_values())
    rng = np.random.default_rng(11)
    A = a0[:, None] * rng.uniform(0.99, 1.01, (a0.size, nscen))
    B = b0[:, None] * rng.uniform(0.99, 1.01, (b0.size, nscen))
    t0 = time.perf_counter()
    mg = slc_amd.RobustMargin(ctx, P, S, nscen=nscen)
    mg.load(d)
    mg.margins()
    first = 1e3 * (time.perf_counter() - t0)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        d_A, d_B = torch.from_numpy(np.ascontiguousarray(A)).to(dev), torch.from_numpy(np.ascontiguousarray(B)).to(dev)
        d_tot = torch.empty((2, nscen), dtype=torch.float64, device=dev)
    mg.set_plant(d_A, d_B, per_scenario=True, stream=s)
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    calls = [50]

    def margin():
        e0.record(stream)
        for _ in range(calls[0]):
            mg.run_async(totals=d_tot, stream=s)
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / calls[0]

    e1_loop = np.zeros(nscen)

    def loop():
        t = time.perf_counter()
        for k in range(nscen):
            plan.update_plant(A=np.ascontiguousarray(A[:, k]), B2=np.ascontiguousarray(B[:, k]))
            e1_loop[k] = plan.residual(d).e1_norm
        return 1e3 * (time.perf_counter() - t)

    t_m, t_l = [], []
    for r in range(ROUNDS + 1):                                   # round 0 is the warm-up of both
        for dst, f in ((t_m, margin), (t_l, loop)):
            v = f()
            if r:
                dst.append(v)
            elif f is margin:
                calls[0] = int(min(5000, max(50, WINDOW_MS / v)))
    plan.update_plant(A=a0, B2=b0)                                # the design values back
    e1 = d_tot.cpu().numpy()[1]
    f = lambda v, k=1.0: "%.4f ms (%.4f – %.4f)" % (float(np.median(v)) / k, min(v) / k, max(v) / k)
    print(f"{name} nscen={nscen}: Nx={P.Nx} Nu={P.Nu} T={meta['T']} entries={mg.n_entries} n_defect={mg.n_defect} "
          f"device {mg.device_bytes / 1e6:.3f} MB (scratch {8e-6 * mg.n_defect * nscen:.3f} MB, plant values {mg.plant_bytes / 1e6:.3f} MB); "
          f"first call (plan + load + fetch) {first:.1f} ms")
    print(f"  {'sls_margin_run, whole ensemble (𝓛₁ and 𝓔₁)':52s}: {f(t_m)} per call   {f(t_m, nscen)} per scenario   ({calls[0]} calls per batch)")
    print(f"  {'update_plant + residual per scenario (𝓔₁ only)':52s}: {f(t_l)} per ensemble   {f(t_l, nscen)} per scenario")
    print(f"  ratio loop / margin per ensemble: {np.median(t_l) / np.median(t_m):.1f}×;  largest |𝓔₁ margin − 𝓔₁ loop| "
          f"{float(np.abs(e1 - e1_loop).max()):.2e} (the loop's Δ also counts Φx[0] − I)")
    mg.close(); plan.close(); ctx.close()

for arg in (sys.argv[1:] or ["readme_chain:1", "readme_chain:64", "chain4096:64"]):
    name, _, n = arg.partition(":")
    measure(name, int(n or 1))
