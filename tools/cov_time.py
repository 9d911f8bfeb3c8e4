"""𝓗₂-share and covariance passes (sls_norms_h2, sls_norms_cov) on a solved Φ that stays on the device, beside what they replace:
the download of Φ to the host.  HIP events around the calls enqueued on one stream, after a warm-up round, over ROUNDS rounds:
median and min – max per call, REPS calls back to back per round.  The covariance pattern is the neighbour pattern of the plant
(`covariance_pattern_of`: the upper triangle of (A ≠ 0) ∪ I on the state rows and the diagonal of the input rows).
Byte models (12 B per entry = value + key): h2 reads the value of every entry in both orders and no key, 16 B · entries; cov reads,
per pair, the keys and values of both row lists at most once, 12 B · Σ_p (len i_p + len j_p) — an upper bound, since the longer
list is only probed inside the windows the shorter one selects and a value is fetched on a hit only.  Rows shared by several
pairs are re-read from cache, so the rate over the model is a cache rate wherever the tables fit one.
The download is `Plan.download` (device → host, all Φ[t]), host clock around a call that ends synchronised, same rounds.
The table of DESIGN.md §3.12.
Usage: python tools/cov_time.py [--out FILE] [workload ...]      (default: readme_chain chain4096)"""
import os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import slc_amd

REPS, ROUNDS = 200, 7
lines = []

def say(s):
    print(s, flush=True)
    lines.append(s)

def measure(name):
    P, S, meta = slc_amd.workloads.make_workload(name)
    dev = torch.device("cuda:0")
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    d = plan.alloc_values(); plan.execute(d); plan.synchronize()
    nrm = slc_amd.ClosedLoopNorms.from_plant(P, S[0], S[1], max_freq=1, ctx=ctx).load(d)
    pi, pj = slc_amd.covariance_pattern_of(P)
    nrm.set_covariance_pattern(pi, pj)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        d_row = torch.empty(P.Nx + P.Nu, dtype=torch.float64, device=dev)
        d_tot = torch.empty(2, dtype=torch.float64, device=dev)
        d_cov = torch.empty(len(pi), dtype=torch.float64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_h2, t_cov, t_dl = [], [], []
    for r in range(ROUNDS + 1):                                   # round 0 is the warm-up of all three
        for t, call in ((t_h2, lambda: nrm.h2_async(row_h2=d_row, totals=d_tot, stream=s)), (t_cov, lambda: nrm.covariance_async(d_cov, stream=s))):
            e0.record(stream)
            for _ in range(REPS):
                call()
            e1.record(stream)
            stream.synchronize()
            if r:
                t.append(1e3 * e0.elapsed_time(e1) / REPS)
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        vx, vu = plan.download(d)
        c1 = time.perf_counter()
        if r:
            t_dl.append(1e3 * (c1 - c0))
    assert torch.isfinite(d_tot).all() and torch.isfinite(d_cov).all() and torch.isfinite(d_row).all()
    info = nrm.info
    n = info["n_entries"]
    row_len = np.diff(slc_amd.norms_tables(P, S)[0])
    m_h2 = 16.0 * n
    m_cov = 12.0 * float((row_len[pi] + row_len[pj]).sum())
    phi_bytes = 8.0 * sum(len(v) for v in vx + vu)
    tot = d_tot.cpu().numpy()
    med = lambda t: float(np.median(t))
    say(f"{name}: Nx={P.Nx} Nu={P.Nu} T={meta['T']} entries={n} pairs={len(pi)} device bytes={info['device_bytes']}")
    say(f"  squared H2 norm {tot[0]:.6f}  largest variance {tot[1]:.6f}  largest RMS {np.sqrt(tot[1]):.6f}")
    say(f"  h2, {REPS} calls back to back   : %.2f µs (%.2f – %.2f) per call   model {m_h2 / 1e6:.2f} MB, {m_h2 / med(t_h2) / 1e3:.1f} GB/s"
        % (med(t_h2), min(t_h2), max(t_h2)))
    say(f"  cov, {REPS} calls back to back  : %.2f µs (%.2f – %.2f) per call   model {m_cov / 1e6:.2f} MB, {m_cov / med(t_cov) / 1e3:.1f} GB/s"
        % (med(t_cov), min(t_cov), max(t_cov)))
    say(f"  download of Φ ({phi_bytes / 1e6:.2f} MB)   : %.3f ms (%.3f – %.3f) per call, {phi_bytes / med(t_dl) / 1e6:.2f} GB/s — %.0f × (h2 + cov)"
        % (med(t_dl), min(t_dl), max(t_dl), 1e3 * med(t_dl) / (med(t_h2) + med(t_cov))))
    nrm.close(); plan.close(); ctx.close()

args = sys.argv[1:]
out = None
if "--out" in args:
    k = args.index("--out")
    out = args[k + 1]
    del args[k:k + 2]
for name in (args or ["readme_chain", "chain4096"]):
    measure(name)
if out:
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
