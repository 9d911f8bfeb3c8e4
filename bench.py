#!/usr/bin/env python3
"""bench.py — throughput of the batched HIP 𝓗₂ SLS solve (the hot path of BASELINE.json's north_star).

  python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run, one rank per GPU)
          [--full] [--dump-outputs DIR]

A plain run measures the headline figure only: setup, W warmup steps, K timed steps, the result line.  --full adds the
measurements that take runs of their own: the one-shot drop-in call (config.oneshot_call, config.wall_clock_to_phi_ms),
cpu_baseline (N=1) and the "strong" record (N>1, or one rank with --force-collective).
--dump-outputs DIR writes what the last timed step computed — the mask-order Φ value array every rank holds after a step
(Φx[t] then Φu[t], each in its mask's CSC order) — to DIR/phi_values.npy in float64.  Beyond 64 MB a fixed, seeded sample
is written instead, its positions in DIR/phi_values_index.npy.  The inputs depend on the arguments only.

Workload.  N=1 is BASELINE.json configs[1] exactly: the README chain (Nx=59, Nu=20, d=9, T=29, α=1.5; README.md:43-57),
59 localized subproblems per step.  N>1 keeps the per-GPU work fixed (weak scaling of the sharded path): the same chain
recipe with Nx = 59·N states, columns cut into N contiguous cost-balanced shards, one RCCL all-gather of the packed
shards per step reassembles {Φx[t],Φu[t]} on every rank.
A step = one pass of the hot path over the whole batch of columns: the device-resident solve (sls_plan_execute) on this
rank's shard + (N>1) the all-gather + the unpack into the mask-order value array (N=1: the solve writes that array
itself).  Consecutive steps are independent solves: for N>1 the gather + unpack of step k run on a side stream while
step k+1 solves (dist.ColumnShardedH2.step_async), every step doing its full work inside the timed region.  Inputs (shared operator A,B2 in CSR,
index sets, masks, destination tables) are resident in HBM before the timed region; the symbolic pass and the H2D upload
are setup (timed separately, reported in config).
value = subproblems attempted by all ranks per second (whole job); solved_per_s counts only those that ended SLS_COL_OK
(equal on the README chain; grid-32 and the random plants have infeasible columns as specified).  dtype f64.  vs_baseline
null (the reference publishes no number).  N>1 with --full adds a "strong" record to the same line: ONE fixed
plant (chain Nx=4096, d=12, T=40) sharded over the N ranks — ms per pass, the all-gather alone, the cost imbalance of the cut.
roofline: FP64 compute bound (≈146 flop/B ≫ ridge).  achieved = F_alg of this rank's shard ÷ average
device time of the solve kernel (HIP events on the launch stream inside libsls); peak = 78.6 TFLOP/s, the public
MI355X FP64 vector/matrix figure (the in-container microarch guide lists no FP64 rate).  bound = "mfma" when the
launch list contains the FP64-MFMA tile kernel (ñx > 64: grid-32, random10000), "fp64_valu" when only the wave kernels run
(README chain, chain-4096) — those issue no MFMA instruction.  traffic = HBM bytes per launch from separate rocprofv3 PMC
passes of this same command, committed under profiles/ (bench.py cannot read PMC counters itself): an OFFLINE measurement, the
commit it was taken at is in the file.
cpu_baseline: the oracle's C restatement (oracle/sls_oracle_c.c, canonical block-tridiagonal Cholesky) timed on this
box's host cores on the same 59 README columns, repeated to fill a bounded sample ("port"; rank 0, N=1, --full only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP64_TFLOPS = 78.6
DUMP_MAX_BYTES = 64_000_000          # --dump-outputs: payload of all files together, .npy headers included


def dump_outputs(out_dir, values):
    """Writes the mask-order Φ value array of the last step (float64) to out_dir/phi_values.npy.  Above DUMP_MAX_BYTES a
    fixed sample (seed 0, ascending positions) is written instead, with its positions as float64 in phi_values_index.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    v = values.detach().cpu().numpy().astype(np.float64, copy=False)
    cap = (DUMP_MAX_BYTES - 2 * 4096) // 8
    if v.size <= cap:
        np.save(os.path.join(out_dir, "phi_values.npy"), v)
        return
    idx = np.sort(np.random.default_rng(0).choice(v.size, cap // 2, replace=False))
    np.save(os.path.join(out_dir, "phi_values.npy"), v[idx])
    np.save(os.path.join(out_dir, "phi_values_index.npy"), idx.astype(np.float64))


def cpu_baseline(max_seconds=12.0):
    """Times the oracle's C port (checker code, never the product) on the README columns."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import sls_oracle as o
    import sls_oracle_cport as cp
    P = o.readme_chain()
    S = o.readme_masks(P.A, P.B2, 9, 29, 1.5)
    recs = cp.prepare(P, S, range(P.Nx))
    best = None
    ncores = os.cpu_count() or 1
    for threads in sorted({1, min(ncores, 16), ncores}):
        reps = 8 if threads == 1 else 8 * threads
        batch = recs * reps
        cp.solve_batch(recs * threads, 29, threads)   # warm the thread pool
        t_used, n_done = 0.0, 0
        while t_used < max_seconds / 3 and n_done < 200000:
            _, resid, status, _, dt, used = cp.solve_batch(batch, 29, threads)
            assert status.max() == 0 and resid.max() < 1e-9
            t_used += dt; n_done += len(batch)
        rate = n_done / t_used
        if best is None or rate > best["value"]:
            best = dict(value=rate, unit="subproblems/s", cores=threads, cores_total=ncores, kind="port",
                        sample=f"{n_done} README-chain columns (59 distinct, repeated) in {t_used:.2f} s, "
                               f"C block-tridiagonal Cholesky + refinement, OpenMP over columns, model build excluded")
    best["value"] = round(best["value"], 1)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="auto", help="auto = chain with Nx=59·gpus (README chain at 1 GPU); or a name from workloads.WORKLOADS")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline figure: one-shot drop-in call, cpu_baseline, strong record")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the Φ values of the last timed step to DIR/phi_values.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip cpu_baseline")
    ap.add_argument("--objective", default="h2", choices=["h2", "sum_of_norms"],
                    help="sum_of_norms = the column-separable 𝓗∞ bound (BASELINE configs[3] as named; an extension, no reference exists)")
    ap.add_argument("--no-strong", action="store_true", help="--full, N > 1: skip the extra strong-scaling record (chain-4096 sharded over the ranks)")
    ap.add_argument("--force-collective", action="store_true",
                    help="one rank only: still create the RCCL process group and run the all-gather + unpack of the N>1 path")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 or args.force_collective:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    import slc_amd
    wl = slc_amd.workloads
    t0 = time.perf_counter()
    if args.workload == "auto":
        Nx = 59 * world
        P = wl.chain_plant(59) if world == 1 else wl.chain_plant(Nx)
        d, T, alpha = 9, 29, 1.5
        S = list(wl.localization_masks(P.A, P.B2, d, T, alpha))
        wname = "README chain Nx=59 Nu=20 d=9 T=29 alpha=1.5 (BASELINE configs[1])" if world == 1 else \
            f"README chain recipe at Nx={Nx} (59 columns per GPU) d=9 T=29 alpha=1.5"
    else:
        P, S, meta = wl.make_workload(args.workload)
        d, T, alpha = meta["d"], meta["T"], meta["alpha"]
        wname = args.workload
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    sh = slc_amd.dist.ColumnShardedH2(P, S, None, device=device, always_gather=args.force_collective, objective=args.objective)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    n_sub_total = P.Nx

    # step_async: the gather + unpack of pass k overlap the solve of pass k+1 (side stream, double-buffered); every pass
    # does the full work and flush() + synchronize() close the timed region
    if sh.gather:
        # The first process that uses RCCL on a box runs its collectives ≈3× slower for the first few thousand of them
        # (measured with a one-rank group: 0.43 ms per step over steps 20..220, 0.146 ms after 3000 steps or in any later
        # process), long after the W warmup steps a caller asks for.  Settle untimed before the contract's warmup.
        t_settle = time.perf_counter()
        n_settle = 0
        while n_settle < 2000 or (time.perf_counter() - t_settle < 1.0 and n_settle < 20000):
            for _ in range(100):
                sh.step_async()
            sh.flush()
            torch.cuda.synchronize()
            n_settle += 100
    for _ in range(args.warmup):
        sh.step_async()
    sh.flush()
    torch.cuda.synchronize()
    sh.local.plan.kernel_time_ms()          # reset the event accumulator
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sh.step_async()
    sh.flush()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, sh.values[: sh.n_values])      # every rank holds the whole array after a step
    kern_ms, n_launch = sh.local.plan.kernel_time_ms()
    st, rs, it = sh.local.plan.fetch_status()
    n_bad = int((st != 0).sum())
    n_bad_total = n_bad
    if world > 1:
        tb = torch.tensor([n_bad], dtype=torch.int64, device=device)
        dist.all_reduce(tb, op=dist.ReduceOp.SUM)
        n_bad_total = int(tb.item())
    info = sh.local.info

    # --full, N > 1: the informative sharding case next to the weak-scaling `value` — ONE fixed plant (chain Nx = 4096, d = 12, T = 40:
    # BASELINE configs[3]'s plant under the 𝓗₂ objective) cut over the N ranks: time per pass of the sharded path (solve of
    # the shard + all-gather + unpack, max over ranks), the all-gather alone, and the predicted-cost imbalance of the cut
    strong = None
    if args.full and (world > 1 or args.force_collective) and args.workload == "auto" and not args.no_strong:      # (one rank + --force-collective: rehearsal of this block on a single GPU)
        try:
            Ps, Ss, ms = wl.make_workload("chain4096")
            shs = slc_amd.dist.ColumnShardedH2(Ps, Ss, None, device=device, objective="h2")
            cuts, per_cost, imb = slc_amd.dist.shard_cost_report(Ps, Ss, None, world)
            for _ in range(5):
                shs.step_async()
            shs.flush(); torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
            k2 = 20
            t1 = time.perf_counter()
            for _ in range(k2):
                shs.step_async()
            shs.flush(); torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
            el = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=device)
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dist.barrier(); torch.cuda.synchronize()
            e0.record()
            for _ in range(k2):
                shs._all_gather(shs.gathered, shs.packed)
            e1.record(); torch.cuda.synchronize()
            ag = torch.tensor([e0.elapsed_time(e1) / k2], dtype=torch.float64, device=device)
            dist.all_reduce(ag, op=dist.ReduceOp.MAX)
            sts, _, _ = shs.local.plan.fetch_status()
            bad = torch.tensor([int((sts != 0).sum())], dtype=torch.int64, device=device)
            dist.all_reduce(bad, op=dist.ReduceOp.SUM)
            strong = {"workload": "chain Nx=4096 d=12 T=40 (BASELINE configs[3]'s plant, H2 objective), columns sharded over the ranks",
                      "scaling": "strong", "n_subproblems": int(Ps.Nx), "steps": k2,
                      "ms_per_pass": round(1e3 * float(el.item()) / k2, 5),
                      "subproblems_per_s": round(Ps.Nx * k2 / float(el.item()), 1),
                      "all_gather_ms": round(float(ag.item()), 5),
                      "all_gather_bytes_per_rank": int(shs.max_packed) * 8,
                      "cost_imbalance_max_over_mean": round(imb, 5),
                      "subproblems_per_rank": [int(cuts[r + 1] - cuts[r]) for r in range(world)],
                      "unsolved_total": int(bad.item())}
            del shs
        except Exception as e:   # the extra record must never take the contract line down
            strong = {"error": str(e)}

    # PCIe-inclusive one-shot drop-in call (symbolic pass + H2D + solve + D2H per call) — --full only, reported in config, never `value`
    oneshot = None
    if args.full and rank == 0 and world == 1:
        try:
            octx = slc_amd.Context([local_rank])
            slc_amd.SLS_H2(P, S, ctx=octx, objective=args.objective, return_info=True)
            best = None
            for _ in range(3):
                t1 = time.perf_counter()
                _, _, oi = slc_amd.SLS_H2(P, S, ctx=octx, return_info=True, objective=args.objective)
                w = time.perf_counter() - t1
                if best is None or w < best[0]:
                    best = (w, oi)
            oi = best[1]
            lib_ms = 1e3 * (oi["t_symbolic_s"] + oi["t_upload_s"] + oi["t_solve_s"] + oi["t_download_s"])
            oneshot = {"library_ms": round(lib_ms, 3), "symbolic_ms": round(1e3 * oi["t_symbolic_s"], 3),
                       "h2d_ms": round(1e3 * oi["t_upload_s"], 3), "solve_ms": round(1e3 * oi["t_solve_s"], 3),
                       "d2h_ms": round(1e3 * oi["t_download_s"], 3), "python_wrapper_wall_ms": round(1e3 * best[0], 3),
                       "subproblems_per_s_incl_pcie": round(n_sub_total / (lib_ms * 1e-3), 1)}
            # the same call through the device-resident symbolic route (sls_h2_sf_solve_localized: the plan is built from
            # (A, B2, d, α, T) on the device, no mask crosses PCIe) — H2 objective, default plant weights
            if args.objective == "h2":
                try:
                    import ctypes as C
                    from slc_amd import _capi
                    mm = _capi.Marshalled(P, [], [], None); mm.dims.T = int(T)
                    dpt = C.POINTER(C.c_double)
                    vx = [__import__("numpy").zeros(max(int(M.nnz), 1)) for M in S[0]]; vu = [__import__("numpy").zeros(max(int(M.nnz), 1)) for M in S[1]]
                    pxa = (dpt * T)(*[a.ctypes.data_as(dpt) for a in vx]); pua = (dpt * T)(*[a.ctypes.data_as(dpt) for a in vu])
                    bestl = None
                    for _ in range(4):
                        stl = _capi.sls_stats()
                        rcl = octx._lib.sls_h2_sf_solve_localized(octx.handle, C.byref(mm.dims), C.byref(mm.plant), int(d), float(alpha), pxa, pua, None, C.byref(stl))
                        _capi.check(rcl, octx.handle)
                        dl = stl.asdict()
                        msl = 1e3 * (dl["t_symbolic_s"] + dl["t_upload_s"] + dl["t_solve_s"] + dl["t_download_s"])
                        if bestl is None or msl < bestl[0]:
                            bestl = (msl, dl)
                    oneshot["device_resident_route"] = {"library_ms": round(bestl[0], 3), "symbolic_ms": round(1e3 * bestl[1]["t_symbolic_s"], 3),
                                                        "h2d_ms": round(1e3 * bestl[1]["t_upload_s"], 3), "solve_ms": round(1e3 * bestl[1]["t_solve_s"], 3),
                                                        "d2h_ms": round(1e3 * bestl[1]["t_download_s"], 3)}
                except Exception as e2:
                    oneshot["device_resident_route"] = {"error": str(e2)}
            octx.close()
        except Exception as e:
            oneshot = {"error": str(e)}

    if rank == 0:
        achieved = info["flops_alg"] / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
        # HBM traffic per launch: measured offline with rocprofv3 PMC passes of this same command (bench.py cannot read
        # PMC counters itself) and committed under profiles/; null when this workload has no committed measurement.
        traffic, traffic_src = None, None
        for tf in ("r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", tf)))
                tkey = wname if args.objective == "h2" else wname + " [sum_of_norms]"
                if world == 1 and tkey in tj:
                    traffic = tj[tkey]["bytes_per_launch"]
                    traffic_src = f"profiles/{tf} (offline rocprofv3 PMC passes, commit {tj[tkey].get('commit', 'round 1')})"
                    break
            except Exception:
                pass
        desc = sh.local.plan.describe()
        bound = "mfma" if "h2_column_tile_kernel" in desc else "fp64_valu"
        oneshot_ms = oneshot.get("library_ms") if isinstance(oneshot, dict) else None
        out = {
            "metric": "SLS subproblems/sec (whole node)",
            "value": round(n_sub_total * args.steps / elapsed, 1),
            "unit": "subproblems/s",
            # `value` counts every subproblem the pass attempts (a column flagged infeasible has been factored and iterated on
            # like any other); solved_per_s counts only those that ended SLS_COL_OK
            "solved_per_s": round((n_sub_total - n_bad_total) * args.steps / elapsed, 1),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 5),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": wname if args.objective == "h2" else wname + " [objective: sum of norms, the column-separable H-infinity bound; extension, no reference exists]",
                       "objective": args.objective, "Nx": int(P.Nx), "Nu": int(P.Nu), "d": d, "T": T, "alpha": alpha,
                       "subproblems_per_step": int(n_sub_total), "subproblems_rank0": int(info["n_subproblems"]),
                       "max_nx": int(info["max_nx"]), "max_nu": int(info["max_nu"]),
                       "phi_values": int(info["n_values"]),
                       # what a caller of the drop-in call waits for Φ: symbolic pass + H2D + solve + D2H inside the library
                       # (--full; null in a plain run)
                       "wall_clock_to_phi_ms": oneshot_ms,
                       "resident_step_ms": round(1e3 * elapsed / args.steps, 5),
                       "setup_symbolic_upload_s": round(t_setup, 4), "mask_generation_s": round(t_gen, 4),
                       "unsolved_rank0": n_bad, "unsolved_total": n_bad_total, "max_residual_rank0": float(rs.max()) if len(rs) else 0.0,
                       "max_refinement_passes": int(it.max()) if len(it) else 0,
                       "oneshot_call": oneshot,
                       "parallelism": f"columns sharded over {world} GPU(s), one all-gather" if world > 1 else "single GPU"},
            "roofline": {"bound": bound, "achieved": round(achieved, 6), "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / PEAK_FP64_TFLOPS, 8), "traffic": traffic, "traffic_source": traffic_src,
                         "kernel": desc, "kernel_avg_ms": round(kern_ms, 6),
                         "kernel_launches": int(n_launch), "flops_alg_per_launch": info["flops_alg"],
                         "bytes_alg_per_launch": info["bytes_alg"],
                         "hbm_GBps_alg": round(info["bytes_alg"] / (kern_ms * 1e-3) / 1e9, 4) if kern_ms > 0 else 0.0},
        }
        if strong is not None:
            out["strong"] = strong
        if args.objective != "h2":
            # F_alg counts the 𝓗₂ solve (factor + one pass) once; the ADMM steps on top of it are not algorithmic flops of
            # anything the reference computes — the fraction is reported for the 𝓗₂ part only and says so
            out["roofline"]["note"] = "flops_alg is the H2 solve's (SURVEY §8d); the sum-of-norms loop runs max_refinement_passes ADMM steps on top"
        if args.full and world == 1 and not args.no_cpu_baseline and args.objective == "h2":
            try:
                out["cpu_baseline"] = cpu_baseline()
            except Exception as e:   # the checker must never take the measurement down
                out["cpu_baseline"] = {"value": None, "unit": "subproblems/s", "cores": 0, "kind": "port",
                                       "sample": f"unavailable: {e}"}
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
