"""Closed-loop norm passes (sls_norms_l1, sls_norms_hinf) on a solved Φ that stays on the device.  HIP events around the calls
enqueued on one stream, after a warm-up, over ROUNDS rounds: median and min – max per call.  l1: REPS calls back to back per round.
hinf: one call of NFREQ frequencies and ITERS iterations per round (its twiddle upload included), and the bytes of the traffic
model of DESIGN.md §3.11 — 12 B · entries · ⌈nfreq/SCN⌉ · 2 passes · iters — over the median.  The line of DESIGN.md §3.11.
Usage: python tools/norms_time.py [workload:nfreq:iters ...]      (default: readme_chain:64:32 chain4096:64:32)"""
import os, sys
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import slc_amd

REPS, ROUNDS = 20, 7

def measure(name, nfreq, iters):
    P, S, meta = slc_amd.workloads.make_workload(name)
    dev = torch.device("cuda:0")
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    d = plan.alloc_values(); plan.execute(d); plan.synchronize()
    nrm = slc_amd.ClosedLoopNorms.from_plant(P, S[0], S[1], max_freq=nfreq, ctx=ctx).load(d)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        d_tot = torch.empty(2, dtype=torch.float64, device=dev)
        d_sig = torch.empty(nfreq, dtype=torch.float64, device=dev)
        d_peak = torch.empty(2, dtype=torch.float64, device=dev)
    om = np.linspace(0.0, np.pi, nfreq)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_l1, t_h = [], []
    for r in range(ROUNDS + 1):                                   # round 0 is the warm-up of both
        e0.record(stream)
        for _ in range(REPS):
            nrm.l1_async(totals=d_tot, stream=s)
        e1.record(stream)
        stream.synchronize()
        if r:
            t_l1.append(1e3 * e0.elapsed_time(e1) / REPS)
        e0.record(stream)
        nrm.hinf_async(om, iters=iters, sigma=d_sig, peak=d_peak, stream=s)
        e1.record(stream)
        stream.synchronize()
        if r:
            t_h.append(e0.elapsed_time(e1))
    assert torch.isfinite(d_tot).all() and torch.isfinite(d_sig).all()
    n = nrm.info["n_entries"]
    scn = 1
    while scn < 64 and scn < nfreq:
        scn *= 2
    model = 12.0 * n * -(-nfreq // scn) * 2 * iters
    tot, pk = d_tot.cpu().numpy(), d_peak.cpu().numpy()
    print(f"{name}: Nx={P.Nx} Nu={P.Nu} T={meta['T']} entries={n} device bytes={nrm.info['device_bytes']}")
    print(f"  L1 norm {tot[0]:.6f}  E1 norm {tot[1]:.6f}  peak sigma {pk[0]:.6f} at omega {om[int(pk[1])]:.4f} (grid of {nfreq}, {iters} iterations)")
    print(f"  l1, {REPS} calls back to back                : %.2f µs (%.2f – %.2f) per call" % (float(np.median(t_l1)), min(t_l1), max(t_l1)))
    print(f"  hinf, nfreq={nfreq} (SCN {scn}) iters={iters}, one call : %.3f ms (%.3f – %.3f)   model {model / 1e6:.2f} MB, {model / np.median(t_h) / 1e6:.1f} GB/s"
          % (float(np.median(t_h)), min(t_h), max(t_h)))
    nrm.close(); plan.close(); ctx.close()

for arg in (sys.argv[1:] or ["readme_chain:64:32", "chain4096:64:32"]):
    name, nf, it = (arg.split(":") + ["64", "32"])[:3]
    measure(name, int(nf), int(it))
