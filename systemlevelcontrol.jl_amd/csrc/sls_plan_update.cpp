// sls_plan_update.cpp — what changes a resident plan after sls_plan_build.cpp built it (include/sls_mi355x.h; the plan: sls_plan.h):
//   partial re-solve   sls_plan_execute_columns, sls_plan_track_changes, sls_plan_execute_dirty, sls_plan_clear_dirty,
//                      sls_plan_fetch_dirty                                                        
//   plant update       sls_plan_update_plant, sls_plan_update_result, sls_plan_fetch_plant
//   weights update     sls_plan_update_weights, sls_plan_update_weights_result, sls_plan_fetch_weights   
// The two update calls differ in checks, kernel and tracking; staging, closing sequence and the counter's read exist once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_object.h"
#include "sls_plan.h"
#include "sls_weights.h"

using namespace sls;

namespace {

// The device buffers of the partial re-solve, made by the first call that needs them: one allocation, cleared, plus the table
// of the launches' slices of `order`.  Not counted in workspace_bytes, which describes the plan as sls_h2_sf_plan left it.
int partial_ensure(sls_plan* plan) {
  sls_plan::Partial& pt = plan->part;
  if (pt.ready) return 0;
  const size_t ns = (size_t)std::max<int64_t>(plan->kp.nsub, 1), nl = std::max<size_t>(plan->launches.size(), 1);
  const size_t nop = (size_t)std::max<int64_t>(plan->opmap.nnzA + plan->opmap.nnzB, 1), nx = (size_t)std::max<int64_t>(plan->sym.Nx, 1);
  size_t no = 1;
  std::vector<int32_t> tab(3 * nl, 0);
  for (size_t li = 0; li < plan->launches.size(); ++li) {
    const auto& L = plan->launches[li];
    no = std::max(no, (size_t)L.order_off + (size_t)L.nsub);
    tab[3 * li] = L.order_off; tab[3 * li + 1] = L.nsub; tab[3 * li + 2] = (L.kind == LaunchKind::Tile && L.gw) ? 1 : 0;
  }
  Arena ar;
  ar.buffer(ns, &pt.dirty); ar.buffer(ns, &pt.marks); ar.buffer(nop, &pt.chg); ar.buffer(nx, &pt.row_chg);
  ar.buffer(no, &pt.sel_order); ar.buffer(no, &pt.sel_pos); ar.buffer(2 * nl, &pt.count);
  const size_t buffer_bytes = ar.bytes();                  // the table, declared last, lies behind what is cleared
  ar.table(tab, &pt.launch_tab);
  void* base = nullptr;
  if (int rc = ar.commit(plan->ctx, &base, "hipMalloc (partial re-solve buffers)", "hipMemcpy H2D (partial re-solve launch table)")) return rc;
  plan->dev_allocs.push_back(base);
  HIPCHK(plan->ctx, hipMemset(base, 0, buffer_bytes));
  pt.h_count.assign(2 * nl, 0);
  pt.ready = true;
  return 0;
}

// The selected run over the subproblems marked in `d_marks` (by out_index).  compact_order_kernel builds the launch lists on
// `st`; the host then WAITS for `st` — the one host wait of the partial re-solve — to read the per-launch counts (two int32 per
// launch), because grids and skipped launches are decided on the host.  No timing events: sls_plan_kernel_time_ms keeps
// averaging full executes.  Ends with the run's end on `st` as last_done (ev_done): what status reads and downloads wait for.
// clear_marks: the marks are zeroed on `st` inside the run (sls_plan_execute_dirty), once the compaction has read them.
int execute_marked(sls_plan* plan, hipStream_t st, double* d_values, int packed, uint8_t* d_marks, bool clear_marks, int64_t* n_solved) {
  sls_plan::Partial& pt = plan->part;
  const size_t nl = plan->launches.size();
  KernelParams kp = plan->kp;
  kp.out = d_values;
  kp.dest_pool = packed ? plan->d_pdest : plan->d_dest;
  CompactOrderParams cp{};
  cp.subs = kp.subs; cp.order = kp.order; cp.launch_tab = pt.launch_tab; cp.marks = d_marks;
  cp.sel_order = pt.sel_order; cp.sel_pos = pt.sel_pos; cp.count = pt.count; cp.nlaunch = (int32_t)nl;
  hipError_t e = launch_compact_order(cp, st);
  if (e != hipSuccess) return hipfail(plan->ctx, e, "launch compact_order_kernel");
  if (nl) HIPCHK(plan->ctx, hipMemcpyAsync(pt.h_count.data(), pt.count, 2 * nl * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(plan->ctx, hipStreamSynchronize(st));
  int64_t items = 0, cols = 0;
  for (size_t li = 0; li < nl; ++li) { items += pt.h_count[li]; cols += pt.h_count[nl + li]; }
  if (n_solved) *n_solved = cols;
  const size_t nmarks = (size_t)plan->kp.nsub;
  if (!plan->ev_done) HIPCHK(plan->ctx, hipEventCreateWithFlags(&plan->ev_done, hipEventDisableTiming));
  SelectedRun sel{pt.sel_order, pt.sel_pos, pt.h_count.data()};
  if (items > 0 && one_kernel_run(plan, st, &sel)) {
    // one kernel: ev_done is the stop event of its dispatch, no marker behind it.  The marks go first — the host has waited for
    // the compaction, their only reader — so that the kernel's end is still the end of the run.
    if (clear_marks) HIPCHK(plan->ctx, hipMemsetAsync(d_marks, 0, nmarks, st));
    const LaunchEvents le{nullptr, plan->ev_done};
    if (int rc = enqueue_launches(plan, kp, st, &sel, &le)) return rc;
    plan->last_done = plan->ev_done;
    return 0;
  }
  if (items > 0) if (int rc = enqueue_launches(plan, kp, st, &sel)) return rc;
  if (clear_marks) HIPCHK(plan->ctx, hipMemsetAsync(d_marks, 0, nmarks, st));
  HIPCHK(plan->ctx, hipEventRecord(plan->ev_done, st));
  plan->last_done = plan->ev_done;
  return 0;
}

int partial_args(sls_plan* plan, double* d_values, int packed, const char* who) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (plan->refine) return fail(plan->ctx, SLS_EUNSUPPORTED, std::string(who) + ": a refinement is attached to this plan (it re-solves columns of its own after every full execute)");
  if (!d_values && plan->info.n_packed > 0) return fail(plan->ctx, SLS_EINVAL, "null device value pointer");
  if (packed && !plan->d_pdest) return fail(plan->ctx, SLS_EINVAL, "this plan was built without the packed layout");
  return 0;
}

// Shared by the two update calls.  Behind the update kernel on `st`: the four-wave kernel's plan-time data (prepared records,
// static blocks, setup images, weight tables) are the only other place that holds operator values and weights; then the end.
int record_update(sls_plan* plan, hipStream_t st) {
  hipError_t e = launch_twisted4_prepares(plan, st);
  if (e != hipSuccess) return hipfail(plan->ctx, e, "launch twisted4_prepare_kernel");
  HIPCHK(plan->ctx, hipEventRecord(plan->ev_upd, st));
  plan->upd_recorded = true;
  return 0;
}

// Which columns are near-singular depends on the plant and on the weights: an attached refinement goes — last, only when the
// update is enqueued in full (a failure before leaves it attached), and after the last execute, which runs it, has ended; the
// caller runs sls_plan_refine again with the new values.
int drop_refinement(sls_plan* plan) {
  if (!plan->refine) return 0;
  if (int rc = wait_plan_done(plan)) return rc;
  sls_plan_destroy(plan->refine);
  plan->refine = nullptr; plan->refine_dst.clear();
  return 0;
}

// What the update entry points read back (dst = NULL: an array the caller does not want): behind the last update (an event edge
// into the plan's own stream), copied there and waited for there — nothing else on the device is waited for.
int read_behind_update(sls_plan* plan, void* dst, const void* d_src, size_t bytes) {
  if (!dst || bytes == 0) return 0;
  if (plan->upd_recorded) HIPCHK(plan->ctx, hipStreamWaitEvent(plan->stream, plan->ev_upd, 0));
  return fetch_to_host(plan->ctx, plan->slot, plan->stream, dst, d_src, bytes);
}

// the refusal counter of the device path: nothing recorded → 0, else the counter behind the last update
int read_refusals(sls_plan* plan, bool recorded, const unsigned long long* d_counter, int64_t* n_rejected) {
  *n_rejected = 0;
  if (!recorded) return 0;
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  unsigned long long n = 0;
  if (int rc = read_behind_update(plan, &n, d_counter, sizeof(n))) return rc;
  *n_rejected = (int64_t)n;
  return 0;
}

}  // namespace

extern "C" {

int sls_plan_execute_columns(sls_plan* plan, void* hip_stream, double* d_values, int packed, const int64_t* subs, int64_t nsubs,
                             int64_t* n_solved) {
  if (n_solved) *n_solved = 0;
  if (int rc = partial_args(plan, d_values, packed, "sls_plan_execute_columns")) return rc;
  if (nsubs < 0 || (nsubs > 0 && !subs)) return fail(plan->ctx, SLS_EINVAL, "sls_plan_execute_columns: bad subproblem list");
  const int64_t ns = plan->kp.nsub;
  for (int64_t i = 0; i < nsubs; ++i) {
    if (subs[i] < 0 || subs[i] >= ns)
      return fail(plan->ctx, SLS_EINVAL, "sls_plan_execute_columns: subproblem " + std::to_string(subs[i]) + " is outside 0 .. " + std::to_string(ns - 1));
    if (i > 0 && subs[i] <= subs[i - 1])
      return fail(plan->ctx, SLS_EINVAL, "sls_plan_execute_columns: the subproblem list must be strictly ascending (position " + std::to_string(i) + ")");
  }
  if (nsubs == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = partial_ensure(plan)) return rc;
  sls_plan::Partial& pt = plan->part;
  pt.h_marks.assign((size_t)ns, 0);
  for (int64_t i = 0; i < nsubs; ++i) pt.h_marks[(size_t)subs[i]] = 1;
  // h_marks belongs to the plan and execute_marked waits for `st` before it returns: the copy has read it by then
  HIPCHK(plan->ctx, hipMemcpyAsync(pt.marks, pt.h_marks.data(), (size_t)ns, hipMemcpyHostToDevice, st));
  return execute_marked(plan, st, d_values, packed, pt.marks, false, n_solved);
}

int sls_plan_track_changes(sls_plan* plan, int on) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  sls_plan::Partial& pt = plan->part;
  if (!on) { pt.track = false; return 0; }
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = partial_ensure(plan)) return rc;
  // the marks are cleared behind the last update and the last execute, on the plan's own stream, and waited for
  hipStream_t ps = plan->stream;
  if (plan->upd_recorded) HIPCHK(plan->ctx, hipStreamWaitEvent(ps, plan->ev_upd, 0));
  if (plan->last_done) HIPCHK(plan->ctx, hipStreamWaitEvent(ps, plan->last_done, 0));
  HIPCHK(plan->ctx, hipMemsetAsync(pt.dirty, 0, (size_t)std::max<int64_t>(plan->kp.nsub, 1), ps));
  HIPCHK(plan->ctx, hipStreamSynchronize(ps));
  pt.track = true;
  return 0;
}

int sls_plan_execute_dirty(sls_plan* plan, void* hip_stream, double* d_values, int packed, int64_t* n_solved) {
  if (n_solved) *n_solved = 0;
  if (int rc = partial_args(plan, d_values, packed, "sls_plan_execute_dirty")) return rc;
  sls_plan::Partial& pt = plan->part;
  if (!pt.ready || plan->kp.nsub == 0) return 0;          // tracking was never on: no mark exists
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  return execute_marked(plan, st, d_values, packed, pt.dirty, true, n_solved);
}

int sls_plan_clear_dirty(sls_plan* plan, void* hip_stream) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!plan->part.ready || plan->kp.nsub == 0) return 0;
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  HIPCHK(plan->ctx, hipMemsetAsync(plan->part.dirty, 0, (size_t)plan->kp.nsub, reinterpret_cast<hipStream_t>(hip_stream)));
  return 0;
}

int sls_plan_fetch_dirty(sls_plan* plan, uint8_t* dirty) {
  if (!plan || (!dirty && plan->kp.nsub > 0)) return fail(nullptr, SLS_EINVAL, "null argument");
  const size_t n = (size_t)plan->kp.nsub;
  if (n == 0) return 0;
  if (!plan->part.ready) { std::fill(dirty, dirty + n, (uint8_t)0); return 0; }   // tracking was never on
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = wait_plan_done(plan)) return rc;            // an sls_plan_execute_dirty clears the marks before its end
  return read_behind_update(plan, dirty, plan->part.dirty, n);
}

int sls_plan_update_plant(sls_plan* plan, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!A_nzval && !B2_nzval) return 0;
  sls_ctx* ctx = plan->ctx;
  const OperatorValueMap& M = plan->opmap;
  if (!on_device) {                        // everything is checked before anything is enqueued: a refused update leaves the plan as it was
    std::string msg;
    if (int rc = check_operator_update(M, A_nzval, B2_nzval, msg)) return fail(ctx, rc, msg);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(ctx, hipSetDevice(plan->dev));
  if (!plan->ev_upd) HIPCHK(ctx, hipEventCreateWithFlags(&plan->ev_upd, hipEventDisableTiming));
  const KernelParams& kp = plan->kp;
  OperatorUpdateParams up{};
  up.nnzA = M.nnzA; up.nnzB = M.nnzB;
  up.row_pos = plan->d_upd_pos; up.zero = plan->d_upd_zero;
  up.A_val = const_cast<double*>(kp.A_val); up.At_val = const_cast<double*>(kp.At_val);
  up.B_val = const_cast<double*>(kp.B_val); up.Bt_val = const_cast<double*>(kp.Bt_val);
  up.rejected = plan->d_upd_rejected;
  up.newA = A_nzval; up.newB = B2_nzval;
  if (!on_device) {                        // host arrays are not kept after return: A's values, then B2's, into the staging array
    if (int rc = stage_to_device(ctx, plan->slot, st, plan->d_upd_stage, A_nzval, (size_t)M.nnzA, B2_nzval, (size_t)M.nnzB)) return rc;
    up.newA = A_nzval ? plan->d_upd_stage : nullptr;
    up.newB = B2_nzval ? plan->d_upd_stage + M.nnzA : nullptr;
  }
  if (plan->part.track) {
    // before operator_update_kernel overwrites the old values: the entries this update changes, then the subproblems they touch
    sls_plan::Partial& pt = plan->part;
    ChangedEntriesParams cp{};
    cp.up = up; cp.rowA = kp.At_colidx; cp.rowB = kp.Bt_colidx; cp.chg = pt.chg; cp.row_chg = pt.row_chg;
    HIPCHK(ctx, hipMemsetAsync(pt.row_chg, 0, (size_t)std::max<int64_t>(plan->sym.Nx, 1), st));
    hipError_t et = launch_changed_entries(cp, st);
    if (et != hipSuccess) return hipfail(ctx, et, "launch changed_entries_kernel");
    MarkAffectedParams mp{};
    mp.subs = kp.subs; mp.nsub = kp.nsub; mp.idx_pool = kp.idx_pool;
    mp.A_rowptr = kp.A_rowptr; mp.A_colidx = kp.A_colidx; mp.B_rowptr = kp.B_rowptr; mp.B_colidx = kp.B_colidx;
    mp.nnzA = M.nnzA; mp.chg = pt.chg; mp.row_chg = pt.row_chg; mp.dirty = pt.dirty;
    et = launch_mark_affected(mp, st);
    if (et != hipSuccess) return hipfail(ctx, et, "launch mark_affected_kernel");
  }
  HIPCHK(ctx, hipMemsetAsync(plan->d_upd_rejected, 0, sizeof(unsigned long long), st));
  hipError_t e = launch_operator_update(up, st);
  if (e != hipSuccess) return hipfail(ctx, e, "launch operator_update_kernel");
  if (int rc = record_update(plan, st)) return rc;
  return drop_refinement(plan);
}

int sls_plan_update_result(sls_plan* plan, int64_t* n_rejected) {
  if (!plan || !n_rejected) return fail(nullptr, SLS_EINVAL, "null argument");
  return read_refusals(plan, plan->upd_recorded, plan->d_upd_rejected, n_rejected);
}

int sls_plan_fetch_plant(sls_plan* plan, double* A_nzval, double* B2_nzval) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  // At_val / Bt_val are the CSC nzval order itself
  if (int rc = read_behind_update(plan, A_nzval, plan->kp.At_val, (size_t)plan->opmap.nnzA * sizeof(double))) return rc;
  return read_behind_update(plan, B2_nzval, plan->kp.Bt_val, (size_t)plan->opmap.nnzB * sizeof(double));
}

int sls_plan_update_weights(sls_plan* plan, void* hip_stream, const double* c1_diag, const double* d12_diag, int on_device) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  sls_ctx* ctx = plan->ctx;
  const Symbolic::UpdatableWeights& W = plan->sym.wu;
  if (!W.updatable) return fail(ctx, SLS_EINVAL, "sls_plan_update_weights: plan not built with SLS_PLAN_WEIGHTS_UPDATABLE");
  if (!c1_diag && !d12_diag) return fail(ctx, SLS_EINVAL, "sls_plan_update_weights: c1_diag and d12_diag are both NULL");
  const int64_t Nx = plan->sym.Nx, Nu = plan->sym.Nu;
  if (!on_device) {                        // everything is checked before anything is enqueued: a refused update leaves the plan as it was
    std::string msg;
    if (int rc = check_weights_update(W, Nx, Nu, c1_diag, d12_diag, msg)) return fail(ctx, rc, msg);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(ctx, hipSetDevice(plan->dev));
  if (!plan->ev_upd) HIPCHK(ctx, hipEventCreateWithFlags(&plan->ev_upd, hipEventDisableTiming));
  const KernelParams& kp = plan->kp;
  WeightsUpdateParams wp{};
  wp.subs = kp.subs; wp.nsub = kp.nsub; wp.idx_pool = kp.idx_pool; wp.Nx = Nx; wp.Nu = Nu;
  wp.b2 = plan->d_w_b2; wp.owner = plan->d_w_owner; wp.ridge = plan->d_w_ridge;
  wp.w_pool = const_cast<double*>(kp.w_pool); wp.diag = plan->d_w_diag; wp.rejected = plan->d_w_rejected;
  wp.dirty = plan->part.track ? plan->part.dirty : nullptr;
  wp.new_c1 = c1_diag; wp.new_d12 = d12_diag;
  if (!on_device) {                        // as the operator update: C1's values, then D12's, into the staging array
    if (int rc = stage_to_device(ctx, plan->slot, st, plan->d_w_stage, c1_diag, (size_t)Nx, d12_diag, (size_t)Nu)) return rc;
    wp.new_c1 = c1_diag ? plan->d_w_stage : nullptr;
    wp.new_d12 = d12_diag ? plan->d_w_stage + Nx : nullptr;
  }
  HIPCHK(ctx, hipMemsetAsync(plan->d_w_rejected, 0, sizeof(unsigned long long), st));
  hipError_t e = launch_weights_update(wp, st);
  if (e != hipSuccess) return hipfail(ctx, e, "launch weights_update_kernel");
  if (int rc = record_update(plan, st)) return rc;
  plan->w_upd_recorded = true;
  return drop_refinement(plan);
}

int sls_plan_update_weights_result(sls_plan* plan, int64_t* n_rejected) {
  if (!plan || !n_rejected) return fail(nullptr, SLS_EINVAL, "null argument");
  return read_refusals(plan, plan->w_upd_recorded, plan->d_w_rejected, n_rejected);
}

int sls_plan_fetch_weights(sls_plan* plan, double* c1_diag, double* d12_diag) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!plan->sym.wu.updatable) return fail(plan->ctx, SLS_EINVAL, "sls_plan_fetch_weights: plan not built with SLS_PLAN_WEIGHTS_UPDATABLE");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  const size_t nx = (size_t)plan->sym.Nx, nu = (size_t)plan->sym.Nu;
  if (int rc = read_behind_update(plan, c1_diag, plan->d_w_diag, nx * sizeof(double))) return rc;
  return read_behind_update(plan, d12_diag, plan->d_w_diag + nx, nu * sizeof(double));
}

}  // extern "C"
