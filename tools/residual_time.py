"""Device time of the achievability residual (sls_plan_residual: csrc/sls_residual.hip) beside the objective evaluation
(sls_plan_objective) on the same resident plan, and beside what a caller had to do without it: Plan.download of Φ.

Per workload, all in one process: the plan's first residual call on its own (it builds the halo lists on the host and uploads
them — host clock, ends in a stream synchronise); then, alternating round by round, HIP-event time around `batch` back-to-back
calls of each C entry point, outputs allocated once, on the stream the execute ran on (a batch is sized from the warm-up to fill --window seconds; the number
reported is the time per call, median / min / max over the rounds); the host clock of one Plan.residual (the fetch form: launch,
copy of 3n + 2 doubles, wait); the plan's own sls_plan_kernel_time_ms; one Plan.download.  Prints one JSON line per workload.
Usage: python tools/residual_time.py [--rounds R] [--window S] [workload ...]      (default: readme_chain chain4096)"""
import argparse, json, os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slc_amd
import torch


def measure(name, rounds, window):
    P, S, meta = slc_amd.workloads.make_workload(name)
    ctx = slc_amd.Context([0])
    plan = slc_amd.Plan(ctx, P, S)
    vals = torch.zeros(plan.info["n_values"], dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    for _ in range(3):
        plan.execute(vals.data_ptr(), stream=st)
    torch.cuda.synchronize()
    plan.kernel_time_ms()                                  # drop the warm-up launches
    for _ in range(5):
        plan.execute(vals.data_ptr(), stream=st)
    torch.cuda.synchronize()
    solve_ms, _ = plan.kernel_time_ms()
    t0 = time.perf_counter()
    first = plan.residual(vals.data_ptr(), stream=st)      # the halo build + the first launch (code object load included)
    first_ms = 1e3 * (time.perf_counter() - t0)

    # the C entry points with outputs allocated once: a batch then holds the launches alone, no tensor allocation between them
    n = max(int(plan.info["n_subproblems"]), 1)
    out_r = torch.empty(3 * n + 2, dtype=torch.float64, device="cuda:0")
    out_o = torch.empty(n + 1, dtype=torch.float64, device="cuda:0")
    pr, po, lib, chk = out_r.data_ptr(), out_o.data_ptr(), plan._lib, slc_amd._capi.check

    def residual():
        chk(lib.sls_plan_residual(plan.handle, st, vals.data_ptr(), 0, pr, pr + 8 * n, pr + 16 * n, pr + 24 * n), ctx.handle)

    def objective():
        chk(lib.sls_plan_objective(plan.handle, st, vals.data_ptr(), 0, po, po + 8 * n), ctx.handle)

    def batch_ms(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            f()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    variants = {"residual": residual, "objective": objective}
    batch = {}
    for k, f in variants.items():                          # warm, then size the batch
        batch_ms(f, 5)
        batch[k] = max(10, int(np.ceil(1e3 * window / max(batch_ms(f, 20), 1e-4))))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            times[k].append(batch_ms(f, batch[k]))
    fetch = []
    for _ in range(rounds + 2):
        t0 = time.perf_counter()
        r = plan.residual(vals.data_ptr())
        fetch.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    plan.download(vals.data_ptr())
    download_ms = 1e3 * (time.perf_counter() - t0)
    same = all(np.array_equal(a, b) for a, b in zip(first[:3], r[:3])) and first[3:] == r[3:]
    out = {"workload": name, "Nx": P.Nx, "T": len(S[0]), "n_subproblems": int(plan.info["n_subproblems"]),
           "n_values": int(plan.info["n_values"]), "solve_kernels_ms": solve_ms, "first_call_ms": first_ms,
           "calls_per_batch": batch, "fetch_form_host_ms": float(np.median(fetch[2:])), "download_ms": download_ms,
           "max_inf": r.max_inf, "e1_norm": r.e1_norm, "halo_inf_max": float(r.halo_inf.max()), "bitwise_repeatable": bool(same),
           "n_not_ok": int((plan.fetch_status()[0] != 0).sum())}
    for k, v in times.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "rounds": len(v)}
    plan.close(); ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("workloads", nargs="*", default=["readme_chain", "chain4096"])
    a = ap.parse_args()
    for name in a.workloads:
        r = measure(name, a.rounds, a.window)
        print(json.dumps(r), flush=True)
        print(f"{name}: residual {r['residual_ms']['median']:.4f} ms per call (objective {r['objective_ms']['median']:.4f} ms, solve kernels "
              f"{r['solve_kernels_ms']:.4f} ms); first call {r['first_call_ms']:.2f} ms, fetch form {r['fetch_form_host_ms']:.3f} ms on the host, "
              f"Plan.download {r['download_ms']:.2f} ms; max res_inf {r['max_inf']:.2e}, E1 norm {r['e1_norm']:.2e}", flush=True)
