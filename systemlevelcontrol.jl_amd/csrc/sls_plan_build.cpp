// sls_plan_build.cpp — how a resident plan comes to be and goes (include/sls_mi355x.h; the plan: sls_plan.h): sls_h2_sf_plan and
// plan_create (host symbolic pass), plan_finish (the second half, shared with sls_h2_sf_plan_localized of
// sls_symbolic_device.cpp), sls_plan_destroy — what construction borrows from the context or creates, destruction gives back —
// and the refinement, which builds a second plan (attach_refinement, sls_plan_refine).
//   sls_h2_sf_plan       ≙ the per-column set-up the reference redoes inside the loop
//                           (src/reduction.jl:11-27, src/synthesis.jl:40-43,57-60)
// plan_finish is a sequence of steps.  Their host arithmetic — solver parameters and knobs, the sum-of-norms weights check, kernel
// selection, the scratch and four-wave pool layouts — is in sls_routing.cpp, the arena's in sls_arena.h (both without HIP); the
// steps here borrow, allocate, declare and launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_dropin_host.h"
#include "sls_object.h"
#include "sls_plan.h"

using namespace sls;

namespace {

// Device memory of a plan comes from ONE arena (sls_arena.h: one hipMalloc or none, one staged H2D copy).  A README-sized plan
// used to spend 2 ms in ~25 hipMalloc/hipMemcpy calls for a 0.2 ms solve: it has ~15 tables of a few KB and each synchronous
// pageable copy costs ≈20 µs.  Tables above this size are copied in place, from the caller's memory.
constexpr size_t kInPlaceAbove = 256u << 10;

struct CompactTables { const uint64_t* d_cmask = nullptr; const int32_t* d_cbase = nullptr; const int64_t* d_coff = nullptr; };

// Aux streams (launches 1… of a plan).  Launches of a handful of workgroups (the edge classes of a chain: 6–8 columns) go to
// streams of the LOWEST priority: the launch with the most work — launch 0, on the caller's stream — then gets its workgroups
// placed first and the stragglers take what is left, instead of 22 workgroups scattered over CUs that each lose a slot for the
// whole pass (chain-4096: 1.95 → 1.75 ms).  Launches of real size keep the default priority (random10000_d2 with eleven of them:
// 62.6 ms, against 66.5 ms when they all ran at low priority).  SLS_AUX_PRIORITY=0: default priority for all.
hipError_t create_aux_stream(hipStream_t* st, bool low) {
  int least = 0, greatest = 0;
  const char* e = sls_knob("SLS_AUX_PRIORITY");
  if (low && !(e && e[0] == '0') && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, least);
  return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}

// the plan's main stream: the slot's when no live plan has it, the context's refinement stream for the refinement plan of the
// drop-in call (a hipStreamCreate per call cost 3 ms), else one of its own
int take_main_stream(sls_plan* pl, bool refinement) {
  sls_ctx* ctx = pl->ctx;
  sls_ctx::Slot& sl = ctx->slots[pl->slot];
  hipError_t e = hipSetDevice(pl->dev);
  if (e != hipSuccess) return hipfail(ctx, e, "hipSetDevice");
  if (sl.streams_in_use == 0) {
    if (sl.streams.empty()) {
      hipStream_t st0 = nullptr;
      e = hipStreamCreateWithFlags(&st0, hipStreamNonBlocking);
      if (e != hipSuccess) return hipfail(ctx, e, "hipStreamCreate");
      sl.streams.push_back(st0);
    }
    pl->stream = sl.streams[0]; pl->streams_borrowed = true; sl.streams_in_use = 1;
  } else if (refinement) {
    if (!sl.refine_stream) {
      e = hipStreamCreateWithFlags(&sl.refine_stream, hipStreamNonBlocking);
      if (e != hipSuccess) return hipfail(ctx, e, "hipStreamCreate");
    }
    pl->stream = sl.refine_stream; pl->stream_external = true;
  } else {
    e = hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hipfail(ctx, e, "hipStreamCreate");
  }
  for (int i = 0; i < kEventPool; ++i) { pl->ev_start[i] = nullptr; pl->ev_stop[i] = nullptr; }   // created on first use
  pl->events_ok = true;
  { const char* e = sls_knob("SLS_EXEC_MARKERS"); pl->exec_markers = e && e[0] == '1'; }   // lab mode, read once per plan
  return 0;
}

// solver parameters, then kernel selection (sls_routing.cpp): the launch list in submission order, its workspace layout, S.order
// launch by launch
int select_kernels(sls_plan* pl, const sls_dims* dims, const PlanOpts& opt, const SolverKnobs& knobs, RoutingResult& route) {
  Symbolic& S = pl->sym;
  KernelParams& kp = pl->kp;
  kp.T = (int32_t)S.T; kp.nsub = (int32_t)S.subs.size();
  kp.objective = (dims->flags & SLS_SOLVE_SUM_OF_NORMS) ? 1 : 0;
  knobs.apply(kp);
  std::string msg;
  int rc = kp.objective == 1 ? check_sum_of_norms_weights(S, msg) : 0;
  if (!rc) rc = build_launch_list(S, kp.T, kp.objective, pl->ctx->ncu[pl->slot], opt.force_tile, RoutingKnobs::from_env(), route, msg, opt.multipliers);
  if (rc) return fail(pl->ctx, rc, msg);
  pl->launches = std::vector<sls_plan::Launch>(route.launches.begin(), route.launches.end());
  pl->has_tile = route.has_tile;
  pl->too_large_subs = route.too_large;
  pl->info_unsupported = (int64_t)route.too_large.size();
  kp.w_nzA = S.max_row_A; kp.w_nzAc = S.max_row_At; kp.w_nzB = S.max_row_B; kp.w_nzBc = S.max_row_Bt;
  return 0;
}

// the operator and the per-subproblem tables; `dt`: index sets and compact tables are used where they sit on the device
void declare_tables(sls_plan* pl, Arena& ar, const DeviceTables* dt, bool want_packed, CompactTables& ct) {
  const Symbolic& S = pl->sym;
  KernelParams& kp = pl->kp;
  ar.table(S.A_csr.ptr, &kp.A_rowptr); ar.table(S.A_csr.idx, &kp.A_colidx); ar.table(S.A_csr.val, &kp.A_val);
  ar.table(S.At_csr.ptr, &kp.At_rowptr); ar.table(S.At_csr.idx, &kp.At_colidx); ar.table(S.At_csr.val, &kp.At_val);
  ar.table(S.B_csr.ptr, &kp.B_rowptr); ar.table(S.B_csr.idx, &kp.B_colidx); ar.table(S.B_csr.val, &kp.B_val);
  ar.table(S.Bt_csr.ptr, &kp.Bt_rowptr); ar.table(S.Bt_csr.idx, &kp.Bt_colidx); ar.table(S.Bt_csr.val, &kp.Bt_val);
  ar.table(S.subs, &kp.subs); ar.table(S.order, &kp.order);
  if (dt) kp.idx_pool = dt->d_idx; else ar.table(S.idx_pool, &kp.idx_pool);
  ar.table(S.w_pool, &kp.w_pool);
  if (S.compact) {
    // tables expanded on the device (expand_tables_kernel) from the compact form: 16 B per (column, time step) uploaded
    // instead of 5 B per masked position
    if (dt) ct = CompactTables{dt->d_cmask, dt->d_cbase, dt->d_coff};
    else { ar.table(S.cmask, &ct.d_cmask); ar.table(S.cbase, &ct.d_cbase); ar.table(S.coff, &ct.d_coff); }
    ar.buffer((size_t)std::max<int64_t>(S.md_total, 1), const_cast<uint8_t**>(&kp.mask_pool));
    ar.buffer((size_t)std::max<int64_t>(S.md_total, 1), const_cast<int32_t**>(&pl->d_dest));
  } else {
    ar.table(S.mask_pool, &kp.mask_pool);
    ar.table(S.dest_pool, &pl->d_dest);
  }
  if (want_packed) ar.table(S.pdest_pool, &pl->d_pdest);
}

// the scratch workspaces (never initialised, never read before written) come from the context's cache; a second live plan
// gets its own
int take_scratch(sls_plan* pl, const RoutingResult& route) {
  sls_ctx* ctx = pl->ctx;
  sls_ctx::Slot& sl = ctx->slots[pl->slot];
  const ScratchLayout lay = scratch_layout(route.fac_doubles, route.vec_doubles, route.big_bytes);
  void* sbase = nullptr;
  hipError_t e = hipSuccess;
  if (!sl.scratch_in_use) {
    if (sl.scratch_bytes < lay.bytes) {
      if (sl.scratch) (void)hipFree(sl.scratch);
      sl.scratch = nullptr; sl.scratch_bytes = 0;
      e = hipMalloc(&sl.scratch, lay.bytes);
      if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc (scratch workspace)");
      sl.scratch_bytes = lay.bytes;
    }
    sbase = sl.scratch; sl.scratch_in_use = true; pl->scratch_borrowed = true;
  } else {
    e = hipMalloc(&pl->own_scratch, lay.bytes);
    if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc (scratch workspace)");
    sbase = pl->own_scratch;
  }
  pl->info.workspace_bytes += (int64_t)lay.bytes;
  pl->kp.fac_ws = reinterpret_cast<double*>(sbase);
  pl->kp.vec_ws = route.vec_doubles ? pl->kp.fac_ws + lay.vec_off : nullptr;
  if (route.big_bytes) pl->d_big = static_cast<unsigned char*>(sbase) + lay.big_off;
  return 0;
}

// launches 1… get a stream (the slot's, while the plan has the slot's streams) and the event that joins them back
int take_aux_streams(sls_plan* pl) {
  sls_ctx* ctx = pl->ctx;
  sls_ctx::Slot& sl = ctx->slots[pl->slot];
  size_t n_lo = 0;
  for (size_t li = 1; li < pl->launches.size(); ++li) {
    const bool low = (int64_t)pl->launches[li].grid * 16 <= ctx->ncu[pl->slot];
    if (pl->streams_borrowed) {
      std::vector<hipStream_t>& pool = low ? sl.streams_lo : sl.streams;
      const size_t idx = low ? n_lo++ : li;
      while (pool.size() <= idx) {
        hipStream_t st = nullptr;
        if (create_aux_stream(&st, low) != hipSuccess) return fail(ctx, SLS_EHIP, "aux stream creation failed");
        pool.push_back(st);
      }
      pl->launches[li].stream = pool[idx];
    } else if (create_aux_stream(&pl->launches[li].stream, low) != hipSuccess) {
      return fail(ctx, SLS_EHIP, "aux stream creation failed");
    }
    if (hipEventCreateWithFlags(&pl->launches[li].done, hipEventDisableTiming) != hipSuccess)
      return fail(ctx, SLS_EHIP, "aux event creation failed");
  }
  if (pl->launches.size() > 1 && hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming) != hipSuccess)
    return fail(ctx, SLS_EHIP, "fork event creation failed");
  return 0;
}

// what the solve and the calls on a resident plan write: status words, work queues, objective, operator and weights updates
void declare_state(sls_plan* pl, Arena& ar, const SolverKnobs& knobs) {
  Symbolic& S = pl->sym;
  KernelParams& kp = pl->kp;
  const size_t ns = (size_t)std::max(kp.nsub, 1);
  pl->status_init.assign(ns, SLS_COL_OK);
  for (int32_t q : pl->too_large_subs) pl->status_init[(size_t)S.subs[q].out_index] = SLS_COL_UNSUPPORTED;
  ar.table(pl->status_init, const_cast<const int32_t**>(&kp.status));   // the kernels overwrite the words of what they solve
  ar.buffer(ns, &kp.resid);
  ar.buffer(ns, &kp.iters);
  ar.buffer(std::max<size_t>(pl->launches.size(), 1), &pl->d_counters);   // tile kernel work queues
  // objective evaluation: dense columns and coupled groups go to the general build, one workgroup each; their z_t is staged
  // in LDS when the largest of them fits 48 KiB
  int64_t need = 0;
  for (size_t q = 0; q < S.subs.size(); ++q) {
    const SubDesc& sd = S.subs[q];
    if (sd.has_w != 2 && sd.has_w != 3) continue;
    pl->obj_gen.push_back((int32_t)q);
    need = std::max<int64_t>(need, (int64_t)(sd.has_w == 3 ? sd.pad_ : 1) * (sd.n + sd.m));
  }
  pl->obj_lds_doubles = (int)std::min<int64_t>(need, 6144);
  ar.table(S.obj_pool, &pl->d_obj); ar.table(pl->obj_gen, &pl->d_gen);
  ar.buffer(ns + 1, &pl->d_colobj);
  if (knobs.dbg_level) ar.buffer(ns * 8, &kp.dbg);                        // SLS_PHASE_TIMERS
  // operator update: every plan can take new values of A / B2 (the device-resident route's operator comes through here too)
  build_operator_value_map(S, pl->opmap);
  ar.table(pl->opmap.row_pos, &pl->d_upd_pos); ar.table(pl->opmap.zero, &pl->d_upd_zero);
  ar.buffer(std::max<size_t>(pl->opmap.row_pos.size(), 1), &pl->d_upd_stage); ar.buffer(1, &pl->d_upd_rejected);
  if (S.wu.updatable) {
    // weights update (SLS_PLAN_WEIGHTS_UPDATABLE): what sls_plan_update_weights reads and writes besides w_pool
    ar.table(S.wu.b2, &pl->d_w_b2); ar.table(S.wu.owner, &pl->d_w_owner); ar.table(S.wu.diag, const_cast<const double**>(&pl->d_w_diag));
    if (!S.wu.ridge.empty()) ar.table(S.wu.ridge, &pl->d_w_ridge);
    ar.buffer((size_t)(S.Nx + S.Nu), &pl->d_w_stage); ar.buffer(1, &pl->d_w_rejected);
  }
}

// the four-wave launches' records, and their static blocks and setup images when the plan keeps them (t4_pool_layout)
void declare_t4_pools(sls_plan* pl, Arena& ar, const SolverKnobs& knobs) {
  const KernelParams& kp = pl->kp;
  const T4Pools pools = t4_pool_layout(std::vector<LaunchSpec>(pl->launches.begin(), pl->launches.end()), kp.T, knobs.t4_prestatic);
  for (size_t li = 0; li < pl->launches.size(); ++li) static_cast<T4Slot&>(pl->launches[li]) = pools.slots[li];
  pl->t4_records = pools.records; pl->t4s_doubles = pools.static_doubles; pl->t4i_doubles = pools.image_doubles;
  if (!pools.records) return;
  pl->t4_stride = twisted4_record_bytes(kp.w_nzA, kp.w_nzAc, kp.w_nzB, kp.w_nzBc, kp.T);
  ar.buffer((size_t)(pl->t4_records * pl->t4_stride), &pl->d_t4);
  if (pools.keep_static) { ar.buffer((size_t)pl->t4s_doubles, &pl->d_t4s); ar.buffer((size_t)pl->t4i_doubles, &pl->d_t4i); }
}

// Where the arena's memory comes from: the context keeps one allocation for reuse (a drop-in call builds and drops a plan per
// call: a hipMalloc + hipFree pair of tens of MB costs ≈0.2 ms, of a few hundred KB ≈30 µs); a second live plan gets its own.
// The small tables are staged in the slot's pinned buffer when it fits (a pageable source costs the runtime one more copy and
// ≈15 µs); status / residual words and the other small buffers are cleared on the plan's stream, the big workspaces need none.
int commit_plan_arena(sls_plan* pl, Arena& ar) {
  sls_ctx* ctx = pl->ctx;
  const Arena::Layout lay = ar.lay_out(kInPlaceAbove);
  sls_ctx::Slot* sl = (ctx_is_live(ctx) && pl->slot < (int)ctx->slots.size()) ? &ctx->slots[pl->slot] : nullptr;
  const size_t want = std::max<size_t>(lay.total, 256);
  void* base = nullptr;
  hipError_t e = hipSuccess;
  if (sl && !sl->arena_in_use) {
    if (sl->arena_bytes < want || sl->arena_bytes > 4 * want + (64u << 20)) {      // too small, or wastefully large
      if (sl->arena) (void)hipFree(sl->arena);
      sl->arena = nullptr; sl->arena_bytes = 0;
      e = hipMalloc(&sl->arena, want);
      if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc (plan arena)");
      sl->arena_bytes = want;
    }
    base = sl->arena; sl->arena_in_use = true; pl->arena_borrowed = true;
  } else {
    e = hipMalloc(&base, want);
    if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc (plan arena)");
    pl->dev_allocs.push_back(base);
  }
  pl->info.workspace_bytes += (int64_t)lay.total;
  unsigned char* stage = lay.staged_end ? slot_pinned(ctx, pl->slot, lay.staged_end) : nullptr;
  if (int rc = ar.commit_in(ctx, base, lay, stage, "hipMemcpy H2D (plan arena)")) return rc;
  return ar.clear(ctx, base, lay, pl->stream, "hipMemset");
}

// The plan's own set-up work on its stream, behind the clear: table expansion, then the four-wave launches' records behind the
// tables they read.  The host waits for that stream only — a device-wide wait here would also wait for whatever the caller has
// in flight on other streams (an RCCL collective, another plan).
int run_setup_kernels(sls_plan* pl, const CompactTables& ct) {
  const KernelParams& kp = pl->kp;
  hipError_t e = hipSuccess;
  if (pl->sym.compact) {
    e = launch_expand_tables(kp.subs, kp.nsub, kp.T, ct.d_cmask, ct.d_cbase, ct.d_coff, const_cast<uint8_t*>(kp.mask_pool),
                             const_cast<int32_t*>(pl->d_dest), pl->stream);
    if (e != hipSuccess) return hipfail(pl->ctx, e, "launch expand_tables_kernel");
  }
  e = launch_twisted4_prepares(pl, pl->stream);
  if (e != hipSuccess) return hipfail(pl->ctx, e, "launch twisted4_prepare_kernel");
  e = hipStreamSynchronize(pl->stream);
  if (e != hipSuccess) return hipfail(pl->ctx, e, "hipStreamSynchronize (plan set-up)");
  return 0;
}

// SLS_PLAN_MULTIPLIERS: the buffer every execute exports λ into — an allocation of its own, not part of workspace_bytes;
// cleared once, so that a slot no execute has written yet (and the lanes beyond a 16-lane class's rows) reads as 0
int take_multiplier_buffer(sls_plan* pl) {
  const size_t bytes = (size_t)std::max(pl->kp.nsub, 1) * (size_t)mu_slot_doubles(pl->kp.T) * sizeof(double);
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, bytes);
  if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMalloc (multiplier buffer)");
  pl->dev_allocs.push_back(d);
  e = hipMemsetAsync(d, 0, bytes, pl->stream);
  if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMemsetAsync (multiplier buffer)");
  pl->grad.d_mu = static_cast<double*>(d);
  pl->kp.mu = pl->grad.d_mu; pl->kp.mu_stride = mu_slot_doubles(pl->kp.T);
  return 0;
}

// sls_plan_info, and the big host pools go: nothing reads them after the upload
void fill_info_and_drop_pools(sls_plan* pl, double t_symbolic_s, double t_upload_s) {
  Symbolic& S = pl->sym;
  sls_plan_info& I = pl->info;
  I.n_subproblems = pl->kp.nsub; I.n_values = S.n_values;
  I.n_values_x = S.off_x[S.T]; I.n_values_u = S.n_values - S.off_x[S.T];
  I.n_packed = S.n_packed; I.max_nx = S.max_n; I.max_nu = S.max_m; I.T = (int32_t)S.T; I.device = pl->dev;
  I.flops_alg = S.flops_alg; I.bytes_alg = S.bytes_alg; I.t_symbolic_s = t_symbolic_s; I.t_upload_s = t_upload_s;
  pool_vec<uint8_t>().swap(S.mask_pool);
  pool_vec<int32_t>().swap(S.dest_pool);
  pool_vec<int32_t>().swap(S.pdest_pool);
  pool_vec<int32_t>().swap(S.idx_pool);
  pool_vec<uint64_t>().swap(S.cmask); pool_vec<int32_t>().swap(S.cbase); pool_vec<int64_t>().swap(S.coff);
}

}  // namespace

hipError_t sls::launch_twisted4_prepares(sls_plan* pl, hipStream_t stream) {
  for (const auto& L : pl->launches) {
    if (!(L.kind == LaunchKind::Twisted && L.four)) continue;
    KernelParams q = pl->kp;
    q.order_off = L.order_off; q.nsub = L.nsub; q.t4_stride = pl->t4_stride;
    q.w_mcap = L.mcap;
    q.t4_static = pl->d_t4s ? pl->d_t4s + L.t4s_off : nullptr; q.t4_static_stride = L.t4s_stride;
    q.t4_images = pl->d_t4s ? pl->d_t4i + L.t4i_off : nullptr; q.t4_images_stride = L.t4i_stride;
    hipError_t e = launch_twisted4_prepare(L.cls, q, pl->d_t4 + L.t4_off * pl->t4_stride, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int sls::plan_create(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                     int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t group_begin, int64_t group_end,
                     bool want_packed, const PlanOpts& opt, sls_plan** plan_out) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (!plan_out) return fail(ctx, SLS_EINVAL, "null plan_out");
  *plan_out = nullptr;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "dev_slot out of range");
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(ctx, rc, msg);
  if (!ctx->ridge_x.empty() || !ctx->ridge_u.empty()) {
    if ((!ctx->ridge_x.empty() && (int64_t)ctx->ridge_x.size() != dims->Nx) || (!ctx->ridge_u.empty() && (int64_t)ctx->ridge_u.size() != dims->Nu))
      return fail(ctx, SLS_EINVAL, "sls_set_ridge: the weights' lengths do not match this plant's Nx / Nu");
    if (dims->flags & SLS_SOLVE_SUM_OF_NORMS) return fail(ctx, SLS_EUNSUPPORTED, "the ridge term is not built for the sum-of-norms objective");
    in.reg_x = ctx->ridge_x.empty() ? nullptr : ctx->ridge_x.data();
    in.reg_u = ctx->ridge_u.empty() ? nullptr : ctx->ridge_u.data();
  }

  sls_plan* pl = new (std::nothrow) sls_plan();
  if (!pl) return fail(ctx, SLS_ENOMEM, "out of memory");
  pl->ctx = ctx; pl->dev = ctx->devs[dev_slot]; pl->slot = dev_slot;
  pl->gbeg = group_begin; pl->gend = group_end; pl->ngroups_in = ngroups;
  const double t0 = now_s();
  pl->sym.want_packed = want_packed;
  if (opt.force_tile && want_packed && opt.pk_override) pl->sym.pk_override = *opt.pk_override;
  {
    const char* e = sls_knob("SLS_HOST_TABLES");       // "1": mask / destination tables built on the host (diagnostics)
    const bool host_tables = opt.host_tables >= 0 ? opt.host_tables != 0 : (e && e[0] == '1');
    pl->sym.compact = !want_packed && !host_tables;
  }

  rc = build_symbolic(in, group_begin, group_end, pl->sym, msg);
  if (rc) { delete pl; return fail(ctx, rc, msg); }
  return plan_finish(ctx, dev_slot, dims, pl, t0, want_packed, opt, nullptr, plan_out);
}

// second half of plan creation (contract: sls_plan.h).  What reaches the device, in this order: one hipMalloc or none, one staged
// H2D copy, one copy per large table, the clear on the plan's stream, expand_tables, the four-wave prepares; then the host
// waits for the plan's stream, once.
int sls::plan_finish(sls_ctx* ctx, int dev_slot, const sls_dims* dims, sls_plan* pl, double t0, bool want_packed, const PlanOpts& opt,
                     const DeviceTables* dt, sls_plan** plan_out) {
  const double t1 = now_s();
  auto bail = [&](int code) { sls_plan_destroy(pl); return code; };
  DebugTicker tick("sls plan", 28);
  int rc = take_main_stream(pl, opt.force_tile);
  if (rc) return bail(rc);
  tick("setdevice+stream");
  const SolverKnobs knobs = SolverKnobs::from_env();
  RoutingResult route;
  Arena ar;
  CompactTables ct;
  if ((rc = select_kernels(pl, dims, opt, knobs, route))) return bail(rc);
  declare_tables(pl, ar, dt, want_packed, ct);
  if ((rc = take_scratch(pl, route)) || (rc = take_aux_streams(pl))) return bail(rc);
  declare_state(pl, ar, knobs);
  declare_t4_pools(pl, ar, knobs);
  tick("launch list + requests");
  if ((rc = commit_plan_arena(pl, ar))) return bail(rc);
  tick("arena commit (malloc+H2D)");
  if (opt.multipliers && (rc = take_multiplier_buffer(pl))) return bail(rc);
  if ((rc = run_setup_kernels(pl, ct))) return bail(rc);
  const double t2 = now_s();
  tick("set-up stream synchronize");
  fill_info_and_drop_pools(pl, t1 - t0, t2 - t1);
  *plan_out = pl;
  return 0;
}

// Refinement (which columns and why: select_refinement_groups, sls_dropin_host.h; contract: sls_plan.h)
int sls::attach_refinement(sls_plan* pl, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                           int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, hipStream_t stream, double* d_values,
                           int64_t* n_refined, std::vector<int32_t>& stt, std::vector<double>& res, std::vector<int32_t>& its, int packed) {
  sls_ctx* ctx = pl->ctx;
  *n_refined = 0;
  const int64_t ns = pl->info.n_subproblems;
  stt.resize(ns); its.resize(ns); res.resize(ns);
  if (ns == 0) return 0;
  if (pl->refine) { *n_refined = pl->refine->info.n_subproblems; return sls_plan_fetch_status(pl, stt.data(), res.data(), its.data()); }
  int rc = fetch_status_raw(pl, stt.data(), res.data(), its.data());
  if (rc) return rc;
  const bool all_tile = pl->launches.size() == 1 && pl->launches[0].kind == LaunchKind::Tile;
  if (all_tile) return 0;
  std::vector<int64_t> gptr_all, gcols_all;
  Inputs in0{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  normalise_groups(in0, gptr_all, gcols_all);
  if (pl->gend > (int64_t)gptr_all.size() - 1 || gptr_all[pl->gend] - gptr_all[pl->gbeg] != ns)
    return fail(ctx, SLS_EINVAL, "sls_plan_refine: the group list does not match the one this plan was built from");
  std::vector<int32_t> cls((size_t)ns);
  for (int64_t q = 0; q < ns; ++q) cls[(size_t)q] = pl->sym.subs[q].cls;
  std::vector<char> on_twisted((size_t)ns, 0);
  for (const auto& L : pl->launches)
    if (L.kind == LaunchKind::Twisted)
      for (int i = 0; i < L.nsub; ++i) {
        const int64_t q = pl->sym.order[(size_t)L.order_off + i];
        if (q >= 0 && q < ns) on_twisted[(size_t)q] = 1;
      }
  std::vector<int64_t> rg_ptr, rg_cols, rg_dst;
  select_refinement_groups(pl->gbeg, pl->gend, gptr_all, gcols_all, dims->index_base, cls.data(), on_twisted.data(), stt.data(), its.data(),
                           res.data(), rg_ptr, rg_cols, rg_dst);
  if (rg_dst.empty()) return 0;
  const int64_t nrg = (int64_t)rg_ptr.size() - 1;
  sls_plan* rp = nullptr;
  // a plan with the packed layout gets a refinement that numbers its free variables where the plan put them (pk_base of the
  // refined subproblems), so that either layout of d_values can be written in place
  const bool with_packed = pl->d_pdest != nullptr;
  if (packed && !with_packed) return fail(ctx, SLS_EINVAL, "this plan was built without the packed layout");
  std::vector<int64_t> pk_over;
  if (with_packed) for (int64_t q : rg_dst) pk_over.push_back(pl->sym.pk_base[q]);
  PlanOpts ropt; ropt.force_tile = true; ropt.pk_override = &pk_over;
  rc = plan_create(ctx, pl->slot, dims, P, Sx, Su, nrg, rg_ptr.data(), rg_cols.data(), 0, nrg, with_packed, ropt, &rp);
  if (rc) return rc;
  rc = sls_plan_execute(rp, stream, d_values, packed);
  if (rc == 0) rc = sls_plan_synchronize(rp, stream);
  if (rc) { sls_plan_destroy(rp); return rc; }
  pl->refine = rp; pl->refine_dst = std::move(rg_dst);
  *n_refined = rp->info.n_subproblems;
  return sls_plan_fetch_status(pl, stt.data(), res.data(), its.data());       // merged with the refinement's
}

extern "C" {

int sls_h2_sf_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                   const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                   int64_t group_begin, int64_t group_end, sls_plan** plan_out) {
  PlanOpts opt;
  opt.multipliers = dims && (dims->flags & SLS_PLAN_MULTIPLIERS) != 0;
  return plan_create(ctx, dev_slot, dims, P, Sx, Su, ngroups, group_ptr, group_cols, group_begin, group_end, true, opt, plan_out);
}

void sls_plan_destroy(sls_plan* plan) {
  if (!plan) return;
  if (plan->refine) { sls_plan_destroy(plan->refine); plan->refine = nullptr; }
  (void)hipSetDevice(plan->dev);
  const bool ctx_alive = ctx_is_live(plan->ctx);
  // a stream lent by the context (slot stream, refinement stream) died with it: sls_destroy has waited for nothing, hipFree below does
  const bool stream_gone = !ctx_alive && (plan->streams_borrowed || plan->stream_external);
  if (plan->stream && !stream_gone) (void)hipStreamSynchronize(plan->stream);
  for (void* d : plan->dev_allocs) (void)hipFree(d);
  if (plan->events_ok)
    for (int i = 0; i < kEventPool; ++i) { if (plan->ev_start[i]) (void)hipEventDestroy(plan->ev_start[i]); if (plan->ev_stop[i]) (void)hipEventDestroy(plan->ev_stop[i]); }
  for (auto& L : plan->launches) {
    if (L.done) (void)hipEventDestroy(L.done);
    if (L.stream && !plan->streams_borrowed) (void)hipStreamDestroy(L.stream);
  }
  if (plan->ev_fork) (void)hipEventDestroy(plan->ev_fork);
  if (plan->ev_done) (void)hipEventDestroy(plan->ev_done);
  if (plan->ev_batch) (void)hipEventDestroy(plan->ev_batch);
  if (plan->ev_batch_done) (void)hipEventDestroy(plan->ev_batch_done);
  if (plan->ev_upd) (void)hipEventDestroy(plan->ev_upd);
  if (plan->stream && !plan->streams_borrowed && !plan->stream_external) (void)hipStreamDestroy(plan->stream);
  if (ctx_alive && plan->slot < (int)plan->ctx->slots.size()) {
    if (plan->streams_borrowed) plan->ctx->slots[plan->slot].streams_in_use = 0;
    if (plan->scratch_borrowed) plan->ctx->slots[plan->slot].scratch_in_use = false;
    if (plan->arena_borrowed) plan->ctx->slots[plan->slot].arena_in_use = false;
    if (plan->ltab_borrowed) plan->ctx->slots[plan->slot].ltab_in_use = false;
  }
  if (plan->own_scratch) (void)hipFree(plan->own_scratch);
  delete plan;
}

int sls_plan_refine(sls_plan* plan, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                    int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, void* hip_stream, double* d_values,
                    int packed, int64_t* n_refined) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!dims || !P || !Sx || !Su || !d_values) return fail(plan->ctx, SLS_EINVAL, "null argument");
  if (dims->flags & SLS_SOLVE_SUM_OF_NORMS) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_refine: 𝓗₂ objective only");
  if (plan->kp.objective != 0) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_refine: 𝓗₂ objective only");
  if (ngroups != plan->ngroups_in) return fail(plan->ctx, SLS_EINVAL, "sls_plan_refine: the group list does not match the one this plan was built from");
  if (plan->grad.d_mu) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_refine: a plan built with SLS_PLAN_MULTIPLIERS takes no refinement (the tile pass would leave stale multipliers)");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  int64_t nr = 0;
  std::vector<int32_t> stt, its; std::vector<double> res;
  int rc = attach_refinement(plan, dims, P, Sx, Su, ngroups, group_ptr, group_cols, reinterpret_cast<hipStream_t>(hip_stream), d_values, &nr,
                             stt, res, its, packed);
  if (n_refined) *n_refined = nr;
  return rc;
}

}  // extern "C"
