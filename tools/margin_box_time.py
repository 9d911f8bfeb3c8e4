"""Worst-case 𝓛₁ margin over a box of plants (sls_margin_box_run: two launches for all boxes) against what a user could do before:
rows decouple, so V = 2^max_i b_i plants per box — plant v gives every row its vertex v mod 2^b_i — go through sls_margin_run as
V scenarios, and the host takes the per-row maximum.  Radius ε·|a⁰| round the design plant (ε = 0.01), so every stored coefficient
is active.  Both are timed by HIP events around a batch of calls enqueued back to back on one stream, the batch sized from the
warm-up round to last about 0.2 s (20 … 5000 calls); the baseline's time is its device passes alone — the download of
[Nx][nscen·V] row sums and the host maximum are not counted.  Both alternate in one process for ROUNDS rounds after a warm-up
round; median (min – max).  Also printed: the longest active list, the vertex sums per scenario, device bytes, the worst norm, and
the largest relative difference between the two results.
Usage: python tools/margin_box_time.py [workload:nscen ...]      (default: readme_chain:1 readme_chain:64 chain4096:8)"""
import os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import slc_amd

ROUNDS, WINDOW_MS, EPS = 7, 200.0, 0.01


def bit_of_entry(A, B2):
    """per CSC entry of A and of B₂: the position of its coefficient in its row's active list (A by ascending column, then B₂) when
    every stored coefficient is active; and the list length per row"""
    out, count = [], np.zeros(A.shape[0], dtype=np.int64)
    for M in (A, B2):
        M = sp.csc_matrix(M).copy(); M.sort_indices()
        pos = sp.csc_matrix((np.arange(1, M.nnz + 1, dtype=np.float64), M.indices, M.indptr), shape=M.shape).tocsr()
        pos.sort_indices()
        rank = np.arange(pos.nnz) - np.repeat(pos.indptr[:-1], np.diff(pos.indptr))
        bit = np.zeros(M.nnz, dtype=np.int64)
        bit[pos.data.astype(np.int64) - 1] = rank + np.repeat(count, np.diff(pos.indptr))
        out.append(bit)
        count = count + np.diff(pos.indptr)
    return out[0], out[1], count


def measure(name, nscen):
    P, S, meta = slc_amd.workloads.make_workload(name)
    dev = torch.device("cuda:0")
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    d = plan.alloc_values(); plan.execute(d); plan.synchronize()
    a0, b0 = (np.array(v) for v in plan.plant_values())
    bitA, bitB, bits = bit_of_entry(P.A, P.B2)
    V = 1 << int(bits.max())
    t0 = time.perf_counter()
    mg = slc_amd.RobustMargin(ctx, P, S, nscen=nscen)
    mg.load(d)
    mg.set_radius(relative=EPS)
    box = mg.box_margins()
    first = 1e3 * (time.perf_counter() - t0)
    assert mg.box_max_bits == int(bits.max()) and mg.box_inexact_rows == 0
    # the baseline: scenario s·V + v is plant v of box s (all boxes share the design centre here)
    v = np.arange(V)
    A = a0[:, None] + np.where((v[None, :] >> bitA[:, None]) & 1, 1.0, -1.0) * (EPS * np.abs(a0))[:, None]
    B = b0[:, None] + np.where((v[None, :] >> bitB[:, None]) & 1, 1.0, -1.0) * (EPS * np.abs(b0))[:, None]
    base = slc_amd.RobustMargin(ctx, P, S, nscen=nscen * V)
    base.load(d)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        d_A = torch.from_numpy(np.ascontiguousarray(np.tile(A, (1, nscen)))).to(dev)
        d_B = torch.from_numpy(np.ascontiguousarray(np.tile(B, (1, nscen)))).to(dev)
        d_row = torch.empty((P.Nx, nscen * V), dtype=torch.float64, device=dev)
        d_wc = torch.empty((P.Nx, nscen), dtype=torch.float64, device=dev)
        d_tot = torch.empty((nscen,), dtype=torch.float64, device=dev)
    base.set_plant(d_A, d_B, per_scenario=True, stream=s)
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = {"box": 20, "base": 20}

    def timed(key, call):
        e0.record(stream)
        for _ in range(calls[key]):
            call()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / calls[key]

    run = {"box": lambda: mg.box_run_async(row_wc=d_wc, totals=d_tot, stream=s), "base": lambda: base.run_async(row_l1=d_row, stream=s)}
    t = {"box": [], "base": []}
    for r in range(ROUNDS + 1):                                   # round 0 is the warm-up of both
        for key in ("box", "base"):
            ms = timed(key, run[key])
            if r:
                t[key].append(ms)
            else:
                calls[key] = int(min(5000, max(20, WINDOW_MS / ms)))
    wc = d_wc.cpu().numpy()
    by_hand = d_row.cpu().numpy().reshape(P.Nx, nscen, V).max(axis=2)
    assert np.array_equal(wc, box["row_wc"])
    rel = float(np.max(np.abs(wc - by_hand) / np.maximum(np.abs(by_hand), 1e-300)))
    f = lambda x, k=1.0: "%.4f ms (%.4f – %.4f)" % (float(np.median(x)) / k, min(x) / k, max(x) / k)
    print(f"{name} nscen={nscen} ε={EPS}: Nx={P.Nx} Nu={P.Nu} T={meta['T']} n_defect={mg.n_defect} longest active list {mg.box_max_bits} "
          f"vertex sums per scenario {mg.box_vertex_sums} box arena {mg.box_device_bytes / 1e6:.3f} MB (object {mg.device_bytes / 1e6:.3f} MB; "
          f"baseline object with {nscen * V} scenarios {base.device_bytes / 1e6:.3f} MB); first call (plan + load + set_radius + fetch) {first:.1f} ms; "
          f"worst ‖D‖_𝓛₁ over the box {box['l1_wc'][0]:.6f}")
    print(f"  {'sls_margin_box_run, all boxes':58s}: {f(t['box'])} per call   {f(t['box'], nscen)} per box   ({calls['box']} calls per batch)")
    print(f"  {f'sls_margin_run on {V} vertex plants per box (device only)':58s}: {f(t['base'])} per call   {f(t['base'], nscen)} per box   ({calls['base']} calls per batch)")
    print(f"  ratio baseline / box per call: {np.median(t['base']) / np.median(t['box']):.2f}×;  largest relative |box − per-row maximum of the baseline| {rel:.2e}")
    base.close(); mg.close(); plan.close(); ctx.close()


for arg in (sys.argv[1:] or ["readme_chain:1", "readme_chain:64", "chain4096:8"]):
    name, _, n = arg.partition(":")
    measure(name, int(n or 1))
