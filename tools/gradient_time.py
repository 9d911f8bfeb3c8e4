"""Device time of the gradient pass (sls_plan_gradient: csrc/sls_gradient.hip) and what SLS_PLAN_MULTIPLIERS costs the solve.

Per workload, all in one process: a plan built with the flag (every column on the one-wave kernel, which exports λ) and a plan
of the same plant without it; the flagged plan's first gradient call on its own (it builds the entry tables on the host and
uploads them — host clock, ends in a stream synchronise); then, alternating round by round after a warm-up, HIP-event time
around `batch` back-to-back calls of: execute of the flagged plan, execute of the unflagged plan, the gradient pass (outputs
allocated once, on the stream the execute ran on).  A batch is sized from the warm-up to fill --window seconds; the number
reported is the time per call, median / min / max over the rounds.  Prints one JSON line per workload.
Usage: python tools/gradient_time.py [--rounds R] [--window S] [workload ...]      (default: readme_chain chain4096)"""
import argparse, json, os, sys, time
os.environ.setdefault("SLS_LAB", "1")      # diagnostic knobs are honoured in lab mode only
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slc_amd
import torch


def measure(name, rounds, window):
    P, S, meta = slc_amd.workloads.make_workload(name)
    ctx = slc_amd.Context([0])
    flagged = slc_amd.Plan(ctx, P, S, multipliers=True)
    plain = slc_amd.Plan(ctx, P, S)
    vf = torch.zeros(flagged.info["n_values"], dtype=torch.float64, device="cuda:0")
    vp = torch.zeros(plain.info["n_values"], dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    for _ in range(3):
        flagged.execute(vf.data_ptr(), stream=st); plain.execute(vp.data_ptr(), stream=st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = flagged.gradient(vf.data_ptr(), stream=st)      # the table build + the first launch (code object load included)
    torch.cuda.synchronize()
    first_ms = 1e3 * (time.perf_counter() - t0)
    gA = torch.empty(max(P.A.nnz, 1), dtype=torch.float64, device="cuda:0")
    gB = torch.empty(max(P.B2.nnz, 1), dtype=torch.float64, device="cuda:0")
    lib, chk = flagged._lib, slc_amd._capi.check

    def gradient():
        chk(lib.sls_plan_gradient(flagged.handle, st, vf.data_ptr(), 0, None, gA.data_ptr(), gB.data_ptr(), None, None), ctx.handle)

    def batch_ms(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            f()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    variants = {"execute_flagged": lambda: flagged.execute(vf.data_ptr(), stream=st),
                "execute_unflagged": lambda: plain.execute(vp.data_ptr(), stream=st), "gradient": gradient}
    batch = {}
    for k, f in variants.items():                          # warm, then size the batch
        batch_ms(f, 5)
        batch[k] = max(10, int(np.ceil(1e3 * window / max(batch_ms(f, 20), 1e-4))))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            times[k].append(batch_ms(f, batch[k]))
    again = flagged.gradient(vf.data_ptr(), stream=st)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(first, again))
    dphi = float((vf - vp).abs().max())
    out = {"workload": name, "Nx": P.Nx, "T": len(S[0]), "n_subproblems": int(flagged.info["n_subproblems"]),
           "launches_flagged": flagged.describe(), "launches_unflagged": plain.describe(), "first_call_ms": first_ms,
           "calls_per_batch": batch, "bitwise_repeatable": bool(same), "max_abs_phi_difference": dphi,
           "n_not_ok": int((flagged.fetch_status()[0] != 0).sum()), "max_abs_gA": float(first[0].abs().max())}
    for k, v in times.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "rounds": len(v)}
    flagged.close(); plain.close(); ctx.close()
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
        print(f"{name}: gradient {r['gradient_ms']['median']:.4f} ms per call; execute {r['execute_flagged_ms']['median']:.4f} ms with the flag, "
              f"{r['execute_unflagged_ms']['median']:.4f} ms without; first gradient call {r['first_call_ms']:.2f} ms", flush=True)
