"""Ensemble rollout (sls_rollout_run: plain launches, one per step) against the two ways the library offered before it: the
closed-loop simulator (sls_closed_loop_last_ms / (steps − 1): hipGraph replay, design plant only, x / u / ŵ of all steps kept)
and the stand-alone controller interleaved with a torch sparse plant (controller step, then x ← A·x + w_k + B₂·u on the same
stream: what a user had to write for a plant that is not the design model).  HIP events around STEPS steps enqueued back to back on
one stream, after a warm-up run; the contenders are alternated in one process for ROUNDS rounds; median and min – max per step.
Rollout rows: recording off (cost and peaks only), recording on, and per-scenario plant values (the same kernel reading other
numbers).  Bytes per step of the model of DESIGN.md §3.14: 12 B × n_entries + 8 B × (nnz(A) + nnz(B₂)) × nscen.
Usage: python tools/rollout_time.py [workload:nscen ...]      (default: readme_chain:1 chain4096:64)"""
import os, sys
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import slc_amd

STEPS, ROUNDS = 250, 7

def measure(name, nscen):
    P, S, meta = slc_amd.workloads.make_workload(name)
    dev = torch.device("cuda:0")
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    d = plan.alloc_values(); plan.execute(d); plan.synchronize()
    loop = slc_amd.ClosedLoop(ctx, P, S)
    ctl = slc_amd.Controller(ctx, P, S, nscen=nscen)
    ctl.load(d)
    ro = slc_amd.Rollout(ctx, P, S, nscen=nscen)
    ro.load(d)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    rng = np.random.default_rng(0)
    A, B2 = P.A.tocsr(), P.B2.tocsr()
    with torch.cuda.stream(stream):
        d_w = torch.from_numpy(0.01 * rng.standard_normal((STEPS, P.Nw, nscen))).to(dev)
        d_xs = torch.empty((STEPS, P.Nx, nscen), dtype=torch.float64, device=dev)
        d_us = torch.empty((STEPS, max(P.Nu, 1), nscen), dtype=torch.float64, device=dev)
        d_x = torch.zeros((P.Nx, nscen), dtype=torch.float64, device=dev)
        d_u = torch.empty((P.Nu, nscen), dtype=torch.float64, device=dev)
        fa = torch.from_numpy(rng.uniform(0.8, 1.2, (ro.nnz_A, nscen)) * np.asarray(P.A.data)[:, None]).to(dev)
        fb = torch.from_numpy(rng.uniform(0.8, 1.2, (ro.nnz_B2, nscen)) * np.asarray(P.B2.data)[:, None]).to(dev)
        tA = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                     torch.from_numpy(A.data), size=A.shape, dtype=torch.float64, device=dev)
        tB = torch.sparse_csr_tensor(torch.from_numpy(B2.indptr.astype(np.int64)), torch.from_numpy(B2.indices.astype(np.int64)),
                                     torch.from_numpy(B2.data), size=B2.shape, dtype=torch.float64, device=dev)
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        e0.record(stream); f(); e1.record(stream)
        stream.synchronize()
        return 1e3 * e0.elapsed_time(e1) / STEPS

    def rollout(record, per_scenario):
        def f():
            ro.run(STEPS, w=d_w, x=d_xs if record else None, u=d_us if record and P.Nu else None, stream=s)
        if per_scenario:
            ro.set_plant(fa, fb, per_scenario=True, stream=s)
        else:
            ro.set_plant(torch.from_numpy(np.asarray(P.A.data)).to(dev), torch.from_numpy(np.asarray(P.B2.data)).to(dev), stream=s)
        ro.reset(stream=s)
        stream.synchronize()
        return timed(f)

    def interleaved():
        def f():
            with torch.cuda.stream(stream):
                for k in range(STEPS):
                    ctl.step(d_x, u=d_u, stream=s)
                    d_x.copy_(torch.sparse.mm(tA, d_x) + d_w[k] + torch.sparse.mm(tB, d_u))
        ctl.reset(stream=s); d_x.zero_()
        stream.synchronize()
        return timed(f)

    rows = {"rollout, cost and peaks only": lambda: rollout(False, False), "rollout, x and u recorded": lambda: rollout(True, False),
            "rollout, per-scenario plants, recorded": lambda: rollout(True, True),
            "controller step + torch sparse plant": interleaved}
    t = {k: [] for k in rows}
    t_sim = []
    skipped = {}
    for r in range(ROUNDS + 1):                                   # round 0 is the warm-up of all (graph capture included)
        for k, f in rows.items():
            if k in skipped:
                continue
            try:
                v = f()
            except RuntimeError as e:                             # a torch build without sparse FP64 mat-mat: say so, measure the rest
                skipped[k] = str(e).splitlines()[0]
                continue
            if r:
                t[k].append(v)
        loop.run(d, d_w.data_ptr(), STEPS, nscen, d_xs.data_ptr(), d_us.data_ptr(), stream=s)
        stream.synchronize()
        if r:
            t_sim.append(1e3 * loop.last_ms() / (STEPS - 1))
    assert torch.isfinite(d_xs).all() and np.isfinite(ro.stats(stream=s)[0]).all()
    byts = 12.0 * ro.n_entries + 8.0 * (ro.nnz_A + ro.nnz_B2) * nscen
    f = lambda v: "%.2f µs (%.2f – %.2f)" % (float(np.median(v)), min(v), max(v))
    print(f"{name} nscen={nscen}: Nx={P.Nx} Nu={P.Nu} T={meta['T']} entries={ro.n_entries} nnz(A)+nnz(B2)={ro.nnz_A + ro.nnz_B2} "
          f"({byts / 1e6:.3f} MB per step; state {ro.state_bytes / 1e6:.3f} MB, plant values {ro.plant_bytes / 1e6:.3f} MB, both independent of steps)")
    for k in rows:
        if k in skipped:
            print(f"  {k:44s}: not measured ({skipped[k]})")
        else:
            print(f"  {k:44s}: {f(t[k])} per step   {byts / np.median(t[k]) / 1e3:.1f} GB/s of the model")
    print(f"  {'simulator, graph replay (design plant only)':44s}: {f(t_sim)} per step   {12.0 * ro.n_entries / np.median(t_sim) / 1e3:.1f} GB/s of its model")
    ro.close(); ctl.close(); loop.close(); plan.close(); ctx.close()

for arg in (sys.argv[1:] or ["readme_chain:1", "chain4096:64"]):
    name, _, n = arg.partition(":")
    measure(name, int(n or 1))
