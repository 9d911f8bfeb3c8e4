"""Device time of the objective evaluation (sls_plan_objective: csrc/sls_objective.hip) next to the solve it follows and to
what a caller had to do without it: Plan.download plus a NumPy sum.  One line per plan, all from the same process and run:
HIP-event time of the evaluation (median of `reps` calls on the stream the execute ran on), the bytes it reads (8 B per free
value, 4 B of destination and 1 B of mask per slot), the plan's own sls_plan_kernel_time_ms, and the download + sum.
Usage: python tools/objective_time.py [workload ...]      (default: readme_chain chain4096 grid32)"""
import os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slc_amd
import torch

reps = 20
for name in (sys.argv[1:] or ["readme_chain", "chain4096", "grid32"]):
    P, S, meta = slc_amd.workloads.make_workload(name)
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    n_values, n_packed = plan.info["n_values"], plan.info["n_packed"]
    vals = torch.zeros(n_values, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        plan.execute(vals.data_ptr(), stream=st)
    torch.cuda.synchronize()
    plan.kernel_time_ms()                                  # drop the warm-up launches
    for _ in range(5):
        plan.execute(vals.data_ptr(), stream=st)
    torch.cuda.synchronize()
    solve_ms, _ = plan.kernel_time_ms()
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        col, tot = plan.objective_values_async(vals.data_ptr(), stream=st)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    obj_ms = float(np.median(ms[2:]))
    t0 = time.perf_counter()
    vx, vu = plan.download(vals.data_ptr())
    host_total = sum(float(np.dot(v, v)) for v in vx + vu)
    host_ms = 1e3 * (time.perf_counter() - t0)
    T = plan.info["T"]
    import scipy.sparse as sp
    last = sp.csc_matrix(S[0][-1]); lastu = sp.csc_matrix(S[1][-1])
    Ab = (sp.csc_matrix(P.A) != 0).astype(np.int32)
    nx = np.diff(((sp.csc_matrix((np.ones(last.nnz, dtype=np.int32), last.indices, last.indptr), shape=last.shape) @ Ab).tocsc()).indptr)
    nu = np.diff(((sp.csc_matrix((np.ones(lastu.nnz, dtype=np.int32), lastu.indices, lastu.indptr), shape=lastu.shape) @ Ab).tocsc()).indptr)
    slots = int(T * (nx + nu).sum())
    read_bytes = 8 * n_packed + 5 * slots
    print(f"{name}: objective {obj_ms:.4f} ms ({read_bytes / 1e6:.2f} MB read, {read_bytes / obj_ms / 1e6:.1f} GB/s), "
          f"solve kernels {solve_ms:.4f} ms (ratio {obj_ms / solve_ms:.3f}), download + NumPy sum {host_ms:.3f} ms; "
          f"total {float(tot.item()):.10f} (host sum {host_total:.10f})")
    plan.close(); ctx.close()
