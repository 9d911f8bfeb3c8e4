"""Stand-alone controller step (sls_controller_step: plain launches, one per step) against the unchanged closed-loop simulator's
per-step time (sls_closed_loop_last_ms / (steps − 1): hipGraph replay), whose per-entry work is identical.  Controller: HIP events
around STEPS steps enqueued back to back on one stream, after a warm-up; the two are alternated in one process for ROUNDS rounds;
median and min – max per step, and bytes per step (12 B × n_entries) over the median.  Φ comes from the plan's execute and stays
on the device.  The table of DESIGN.md §3.10.
Usage: python tools/controller_time.py [workload:nscen ...]      (default: readme_chain:1 readme_chain:64 chain4096:1)"""
import os, sys
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import slc_amd

STEPS, WARM, ROUNDS, SIM_STEPS = 2000, 200, 7, 250

def measure(name, nscen):
    P, S, meta = slc_amd.workloads.make_workload(name)
    dev = torch.device("cuda:0")
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    d = plan.alloc_values(); plan.execute(d); plan.synchronize()
    loop = slc_amd.ClosedLoop(ctx, P, S)
    ctl = slc_amd.Controller(ctx, P, S, nscen=nscen)
    ctl.load(d)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    rng = np.random.default_rng(0)
    with torch.cuda.stream(stream):
        d_w = torch.from_numpy(0.01 * rng.standard_normal((SIM_STEPS, P.Nw, nscen))).to(dev)
        d_xs = torch.empty((SIM_STEPS, P.Nx, nscen), dtype=torch.float64, device=dev)
        d_us = torch.empty((SIM_STEPS, max(P.Nu, 1), nscen), dtype=torch.float64, device=dev)
        d_x = torch.zeros((P.Nx, nscen), dtype=torch.float64, device=dev)   # the step's loads and FMAs do not depend on the values
        d_u = torch.empty((P.Nu, nscen), dtype=torch.float64, device=dev)
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_ctl, t_sim = [], []
    for r in range(ROUNDS + 1):                                   # round 0 is the warm-up of both (graph capture included)
        ctl.reset(stream=s)
        for _ in range(WARM):
            ctl.step(d_x, u=d_u, stream=s)
        e0.record(stream)
        for _ in range(STEPS):
            ctl.step(d_x, u=d_u, stream=s)
        e1.record(stream)
        stream.synchronize()
        loop.run(d, d_w.data_ptr(), SIM_STEPS, nscen, d_xs.data_ptr(), d_us.data_ptr(), stream=s)
        stream.synchronize()
        if r:
            t_ctl.append(1e3 * e0.elapsed_time(e1) / STEPS)
            t_sim.append(1e3 * loop.last_ms() / (SIM_STEPS - 1))
    assert torch.isfinite(d_u).all() and torch.isfinite(d_xs).all()
    byts = 12.0 * ctl.n_entries
    f = lambda t: "%.2f µs (%.2f – %.2f)" % (float(np.median(t)), min(t), max(t))
    print(f"{name} nscen={nscen}: Nx={P.Nx} Nu={P.Nu} T={meta['T']} entries={ctl.n_entries} ({byts / 1e6:.3f} MB per step)")
    print(f"  controller step, {STEPS} plain launches back to back : {f(t_ctl)}   {byts / np.median(t_ctl) / 1e3:.1f} GB/s")
    print(f"  simulator step, graph replay of {SIM_STEPS - 1} launches      : {f(t_sim)}   {byts / np.median(t_sim) / 1e3:.1f} GB/s")
    ctl.close(); loop.close(); plan.close(); ctx.close()

for arg in (sys.argv[1:] or ["readme_chain:1", "readme_chain:64", "chain4096:1"]):
    name, _, n = arg.partition(":")
    measure(name, int(n or 1))
