// sls_api.cpp — implementation of include/sls_mi355x.h (the drop-in C ABI): the context, the error plumbing, the slot's pinned
// staging paths, and what runs and reads a resident plan (execute, batch, synchronize, status, objective, residual, describe,
// timing, values, download, scatter).  Plans are built and destroyed in sls_plan_build.cpp; plant and weights updates and partial
// re-solves of a plan are in sls_plan_update.cpp, the one-shot calls built on plans (sls_h2_sf_solve ≙ SLS_𝓗₂(P, 𝓢; 𝓘),
// src/synthesis.jl:11-32) in sls_dropin.cpp, the three device symbolic passes (sls_localization_masks_device,
// sls_index_sets_device, sls_h2_sf_plan_localized) in sls_symbolic_device.cpp, the exports of include/sls_mi355x_debug.h in
// sls_debug.cpp.
//
// Host side of the path that replaces reference src/synthesis.jl:11-72:
//   sls_plan_execute     ≙ the @distributed loop body's solve   (src/synthesis.jl:46-62)
//   sls_plan_download    ≙ the scatter into Φx[t], Φu[t]         (src/synthesis.jl:65-67)
// No CPU fallback exists: without a gfx950 device every compute entry point fails
// with SLS_ENODEVICE / SLS_EHIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_device.h"
#include "sls_dropin_host.h"
#include "sls_internal.h"
#include "sls_object.h"
#include "sls_objective.h"
#include "sls_plan.h"
#include "sls_residual.h"
#include "sls_routing.h"
#include "sls_symbolic.h"

namespace {
std::mutex g_err_mu;
std::string g_last_error;
void set_global_error(const std::string& s) { std::lock_guard<std::mutex> l(g_err_mu); g_last_error = s; }
std::set<const void*> g_live_ctx;   // a plan may outlive its context (host-language GC order): checked before touching it
}  // namespace

namespace sls {
int fail(sls_ctx* ctx, int code, const std::string& msg) {
  // a plan / loop object may report through a context that its owner has already destroyed (host-language GC order)
  if (ctx && ctx_is_live(ctx)) ctx->err = msg;
  set_global_error(msg);
  return code;
}
int hipfail(sls_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, SLS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
bool ctx_is_live(const sls_ctx* ctx) {
  std::lock_guard<std::mutex> l(g_err_mu);
  return g_live_ctx.count(ctx) > 0;
}
double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int wait_plan_done(sls_plan* pl) {
  if (pl->last_done) {
    hipError_t e = hipEventSynchronize(pl->last_done);
    if (e != hipSuccess) return hipfail(pl->ctx, e, "hipEventSynchronize (plan done)");
  }
  return 0;
}
}  // namespace sls

using namespace sls;

// The context slot's pinned staging memory (created on first use, 8 MiB): nullptr when unavailable or too small.
unsigned char* sls::slot_pinned(sls_ctx* ctx, int slot, size_t bytes) {
  if (!ctx_is_live(ctx) || slot < 0 || slot >= (int)ctx->slots.size() || sls_knob("SLS_PAGEABLE_D2H")) return nullptr;
  sls_ctx::Slot& sl = ctx->slots[slot];
  if (sl.pinned_pending) { (void)hipEventSynchronize(sl.pinned_busy); sl.pinned_pending = false; }   // an update's H2D copy still reads it
  constexpr size_t kBytes = 8u << 20;
  if (!sl.pinned) {
    if (hipHostMalloc(&sl.pinned, kBytes, hipHostMallocDefault) != hipSuccess) { sl.pinned = nullptr; return nullptr; }
    sl.pinned_bytes = kBytes;
  }
  return bytes <= sl.pinned_bytes ? static_cast<unsigned char*>(sl.pinned) : nullptr;
}

int sls::pinned_read_until(sls_ctx* ctx, int slot, hipStream_t st) {
  sls_ctx::Slot& sl = ctx->slots[slot];
  if (!sl.pinned_busy) HIPCHK(ctx, hipEventCreateWithFlags(&sl.pinned_busy, hipEventDisableTiming));
  HIPCHK(ctx, hipEventRecord(sl.pinned_busy, st));
  sl.pinned_pending = true;
  return 0;
}

int sls::stage_to_device(sls_ctx* ctx, int slot, hipStream_t st, double* d_stage, const double* a, size_t na, const double* b, size_t nb) {
  double* pin = reinterpret_cast<double*>(slot_pinned(ctx, slot, (na + nb) * sizeof(double)));
  const bool has_a = a && na, has_b = b && nb;
  if (pin && has_a) { std::memcpy(pin, a, na * sizeof(double)); a = pin; }
  if (pin && has_b) { std::memcpy(pin + na, b, nb * sizeof(double)); b = pin + na; }
  if (has_a) HIPCHK(ctx, hipMemcpyAsync(d_stage, a, na * sizeof(double), hipMemcpyHostToDevice, st));
  if (has_b) HIPCHK(ctx, hipMemcpyAsync(d_stage + na, b, nb * sizeof(double), hipMemcpyHostToDevice, st));
  if (pin) return pinned_read_until(ctx, slot, st);
  HIPCHK(ctx, hipStreamSynchronize(st));               // no pinned buffer (or too small): the copies have read the caller's arrays
  return 0;
}

int sls::fetch_to_host(sls_ctx* ctx, int slot, hipStream_t st, void* dst, const void* d_src, size_t bytes) {
  unsigned char* pin = slot_pinned(ctx, slot, bytes);
  HIPCHK(ctx, hipMemcpyAsync(pin ? static_cast<void*>(pin) : dst, d_src, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (pin) std::memcpy(dst, pin, bytes);
  return 0;
}

// (contract: sls_internal.h)  1 MiB chunks through kDlLanes lanes, each a host thread with its own stream and pinned chunk — DMA at
// link speed into pinned memory, then a host copy whose first-touch page faults are spread over the lanes and overlap the other DMA.
int sls::pinned_download(sls_ctx* ctx, int slot, int dev, const void* d_src, const std::vector<int64_t>& beg, const std::vector<void*>& ptrs) {
  constexpr int kDlLanes = 8;
  constexpr int64_t kChunk = (1ll << 20) / 8;          // elements per chunk
  const int64_t nsl = (int64_t)ptrs.size(), n_total = beg[nsl];
  if (n_total == 0) return 0;
  if (!ctx_is_live(ctx) || slot >= (int)ctx->slots.size() || sls_knob("SLS_PAGEABLE_D2H")) return 1;
  sls_ctx::Slot& sl = ctx->slots[slot];
  (void)slot_pinned(ctx, slot, (size_t)kDlLanes * kChunk * 8);
  while (sl.pinned && (int)sl.dl_streams.size() < kDlLanes) {
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
    sl.dl_streams.push_back(st);
  }
  if (!sl.pinned || (int)sl.dl_streams.size() != kDlLanes) return 1;
  const int64_t nchunks = (n_total + kChunk - 1) / kChunk;
  const int lanes = (int)std::min<int64_t>(kDlLanes, nchunks);
  std::vector<hipError_t> errs(lanes, hipSuccess);
  const unsigned char* src = static_cast<const unsigned char*>(d_src);
  host_parallel(lanes, [&](int ln) {
    hipError_t e = hipSetDevice(dev);
    unsigned char* stage = static_cast<unsigned char*>(sl.pinned) + (int64_t)ln * kChunk * 8;
    int64_t sli = 0;                                         // slice cursor (chunks of one lane ascend)
    for (int64_t ch = ln; ch < nchunks && e == hipSuccess; ch += lanes) {
      const int64_t b = ch * kChunk, en = std::min(n_total, b + kChunk);
      e = hipMemcpyAsync(stage, src + b * 8, (size_t)(en - b) * 8, hipMemcpyDeviceToHost, sl.dl_streams[ln]);
      if (e == hipSuccess) e = hipStreamSynchronize(sl.dl_streams[ln]);
      if (e != hipSuccess) break;
      while (sli < nsl - 1 && beg[sli + 1] <= b) ++sli;
      for (int64_t s2 = sli; s2 < nsl && beg[s2] < en; ++s2) {
        const int64_t lo = std::max(b, beg[s2]), hi = std::min(en, beg[s2 + 1]);
        if (hi > lo) std::memcpy(static_cast<unsigned char*>(ptrs[s2]) + (lo - beg[s2]) * 8, stage + (lo - b) * 8, (size_t)(hi - lo) * 8);
      }
    }
    errs[ln] = e;
  });
  for (hipError_t e : errs) if (e != hipSuccess) return hipfail(ctx, e, "pinned D2H");
  return 0;
}

namespace {

// Fold the timing events of finished launches into the accumulator.  blocking = false (the hot path, when the pool is
// full): only launches the GPU has already completed are folded (hipEventQuery) — the host never waits; events still in
// flight stay in the pool, compacted to its front.
int fold_events(sls_plan* pl, bool blocking = true) {
  int kept = 0;
  for (int i = 0; i < pl->ev_used; ++i) {
    float ms = 0.f;
    hipError_t e = blocking ? hipEventSynchronize(pl->ev_stop[i]) : hipEventQuery(pl->ev_stop[i]);
    if (!blocking && e == hipErrorNotReady) {
      std::swap(pl->ev_start[kept], pl->ev_start[i]); std::swap(pl->ev_stop[kept], pl->ev_stop[i]);
      ++kept;
      continue;
    }
    if (e != hipSuccess) return hipfail(pl->ctx, e, "hipEventSynchronize");
    e = hipEventElapsedTime(&ms, pl->ev_start[i], pl->ev_stop[i]);
    if (e != hipSuccess) return hipfail(pl->ctx, e, "hipEventElapsedTime");
    pl->ev_acc_ms += ms; pl->ev_acc_n += 1;
  }
  pl->ev_used = kept;
  return 0;
}

}  // namespace

extern "C" {

int sls_abi_version(void) { return SLS_ABI_VERSION; }

const char* sls_last_error(const sls_ctx* ctx) {
  if (ctx) return ctx->err.c_str();
  std::lock_guard<std::mutex> l(g_err_mu);
  static thread_local std::string copy;
  copy = g_last_error;
  return copy.c_str();
}

int sls_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { set_global_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); return SLS_ENODEVICE; }
  return n;
}

sls_ctx* sls_create(const int* devs, int ndev, uint32_t flags) {
  int navail = 0;
  hipError_t e = hipGetDeviceCount(&navail);
  if (e != hipSuccess || navail <= 0) {
    set_global_error(std::string("sls_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                     "); this library has no CPU fallback");
    return nullptr;
  }
  if (ndev <= 0) { set_global_error("sls_create: ndev must be >= 1"); return nullptr; }
  sls_ctx* ctx = new (std::nothrow) sls_ctx();
  if (!ctx) { set_global_error("sls_create: out of memory"); return nullptr; }
  ctx->flags = flags;
  for (int i = 0; i < ndev; ++i) {
    const int d = devs ? devs[i] : i;
    if (d < 0 || d >= navail) {
      set_global_error("sls_create: device ordinal " + std::to_string(d) + " out of range (" + std::to_string(navail) + " visible)");
      delete ctx; return nullptr;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, d);
    if (e != hipSuccess) { set_global_error(std::string("hipGetDeviceProperties: ") + hipGetErrorString(e)); delete ctx; return nullptr; }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
      set_global_error(std::string("sls_create: device ") + std::to_string(d) + " is " + prop.gcnArchName +
                       ", kernels are built for gfx950 only");
      delete ctx; return nullptr;
    }
    ctx->devs.push_back(d);
    ctx->ncu.push_back(prop.multiProcessorCount);
    ctx->slots.emplace_back();
  }
  { std::lock_guard<std::mutex> l(g_err_mu); g_live_ctx.insert(ctx); }
  return ctx;
}

void sls_destroy(sls_ctx* ctx) {
  if (!ctx) return;
  { std::lock_guard<std::mutex> l(g_err_mu); g_live_ctx.erase(ctx); }
  for (size_t i = 0; i < ctx->slots.size(); ++i) {
    (void)hipSetDevice(ctx->devs[i]);
    for (hipStream_t st : ctx->slots[i].streams) if (st) (void)hipStreamDestroy(st);
    for (hipStream_t st : ctx->slots[i].streams_lo) if (st) (void)hipStreamDestroy(st);
    if (ctx->slots[i].refine_stream) (void)hipStreamDestroy(ctx->slots[i].refine_stream);
    if (ctx->slots[i].scratch) (void)hipFree(ctx->slots[i].scratch);
    if (ctx->slots[i].arena) (void)hipFree(ctx->slots[i].arena);
    if (ctx->slots[i].ltab) (void)hipFree(ctx->slots[i].ltab);
    for (hipStream_t st : ctx->slots[i].dl_streams) if (st) (void)hipStreamDestroy(st);
    if (ctx->slots[i].pinned_busy) { (void)hipEventSynchronize(ctx->slots[i].pinned_busy); (void)hipEventDestroy(ctx->slots[i].pinned_busy); }
    if (ctx->slots[i].pinned) (void)hipHostFree(ctx->slots[i].pinned);
  }
  delete ctx;
}

int sls_set_ridge(sls_ctx* ctx, int64_t nx, const double* rx, int64_t nu, const double* ru) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (nx < 0 || nu < 0 || (nx > 0 && !rx) || (nu > 0 && !ru)) return fail(ctx, SLS_EINVAL, "bad ridge arguments");
  for (int64_t i = 0; i < nx; ++i) if (!(rx[i] >= 0.0)) return fail(ctx, SLS_EINVAL, "ridge weights must be ≥ 0");
  for (int64_t i = 0; i < nu; ++i) if (!(ru[i] >= 0.0)) return fail(ctx, SLS_EINVAL, "ridge weights must be ≥ 0");
  ctx->ridge_x.assign(rx, rx + nx);
  ctx->ridge_u.assign(ru, ru + nu);
  return 0;
}

int sls_sparsity_dim_reduction(const sls_dims* dims, const sls_csc_f64* A, const sls_csc_bool* Sx_last,
                               const sls_csc_bool* Su_last, const int64_t* cj, int64_t ncj, int64_t* sx_out,
                               int64_t* nsx, int64_t* su_out, int64_t* nsu) {
  if (!dims || !A || !Sx_last || !Su_last || (!cj && ncj > 0) || !nsx || !nsu) return fail(nullptr, SLS_EINVAL, "null argument");
  // masks are addressed as "the last of T": present a T = 1 view
  sls_dims d1 = *dims; d1.T = 1;
  sls_plant P{}; P.A = A;
  Inputs in{&d1, &P, Sx_last, Su_last, 0, nullptr, nullptr};
  std::vector<int64_t> c0(ncj);
  for (int64_t i = 0; i < ncj; ++i) {
    c0[i] = cj[i] - dims->index_base;
    if (c0[i] < 0 || c0[i] >= dims->Nx) return fail(nullptr, SLS_EINVAL, "column out of range");
  }
  GroupSets gs; std::string msg;
  int rc = group_index_sets(in, c0.data(), ncj, gs, msg);
  if (rc) return fail(nullptr, rc, msg);
  if (sx_out) for (size_t i = 0; i < gs.sx_first.size(); ++i) sx_out[i] = gs.sx_first[i] + dims->index_base;
  if (su_out) for (size_t i = 0; i < gs.su_first.size(); ++i) su_out[i] = gs.su_first[i] + dims->index_base;
  *nsx = (int64_t)gs.sx_first.size(); *nsu = (int64_t)gs.su_first.size();
  return 0;
}

int sls_localization_masks(const sls_dims* dims, const sls_csc_f64* A, const sls_csc_f64* B2, int64_t d, double alpha,
                           int64_t* nnz_x, int64_t* nnz_u, int64_t* const* colptr_x, int64_t* const* rowval_x,
                           int64_t* const* colptr_u, int64_t* const* rowval_u) {
  if (!dims || !A || !B2 || !nnz_x || !nnz_u) return fail(nullptr, SLS_EINVAL, "null argument");
  std::string msg;
  int rc = localization_masks(dims, A, B2, d, alpha, nnz_x, nnz_u, colptr_x, rowval_x, colptr_u, rowval_u, msg);
  return rc ? fail(nullptr, rc, msg) : 0;
}

int sls_shard_groups(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                     int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int nshards, int64_t* cuts) {
  if (nshards <= 0 || !cuts) return fail(nullptr, SLS_EINVAL, "nshards must be >= 1");
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  std::vector<double> cost;
  rc = group_costs(in, cost, msg);
  if (rc) return fail(nullptr, rc, msg);
  balanced_cuts(cost, nshards, cuts);
  return 0;
}

int sls_h2_sf_packed_layout(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                            int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t group_begin,
                            int64_t group_end, int64_t* n_packed, int64_t* n_values, int64_t* dest, sls_plan_info* info) {
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  Symbolic S;
  const double t0 = now_s();
  rc = build_symbolic(in, group_begin, group_end, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  if (n_packed) *n_packed = S.n_packed;
  if (n_values) *n_values = S.n_values;
  if (dest) std::copy(S.packed_to_final.begin(), S.packed_to_final.end(), dest);
  if (info) {
    sls_plan_info I{};
    I.n_subproblems = (int64_t)S.subs.size(); I.n_values = S.n_values; I.n_values_x = S.off_x[S.T];
    I.n_values_u = S.n_values - S.off_x[S.T]; I.n_packed = S.n_packed; I.max_nx = S.max_n; I.max_nu = S.max_m;
    I.T = (int32_t)S.T; I.device = -1; I.flops_alg = S.flops_alg; I.bytes_alg = S.bytes_alg;
    I.t_symbolic_s = now_s() - t0;
    *info = I;
  }
  return 0;
}

int sls_plan_get_info(const sls_plan* plan, sls_plan_info* info) {
  if (!plan || !info) return fail(nullptr, SLS_EINVAL, "null argument");
  *info = plan->info;
  return 0;
}

int sls_plan_value_offsets(const sls_plan* plan, int64_t* off_x, int64_t* off_u) {
  if (!plan || !off_x || !off_u) return fail(nullptr, SLS_EINVAL, "null argument");
  std::copy(plan->sym.off_x.begin(), plan->sym.off_x.end(), off_x);
  std::copy(plan->sym.off_u.begin(), plan->sym.off_u.end(), off_u);
  return 0;
}

extern "C++" bool sls::one_kernel_run(const sls_plan* plan, hipStream_t st, const SelectedRun* sel) {
  if (plan->exec_markers || plan->launches.size() != 1 || plan->has_tile) return false;   // has_tile: a counter memset goes first
  if (sel && sel->count[0] <= 0) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;       // a capturing stream keeps the recorded events: they become graph nodes
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
  // A full execute takes the dispatch path only behind an execute of this plan that is still in flight: that is where a record
  // queues a marker the kernel then waits for.  A caller that waits for every execute gains nothing from it (no marker is queued
  // on an idle stream), and the host wait for a dispatch with bound events was measured 7 µs longer than the wait for a marker.
  return sel || (plan->last_done && hipEventQuery(plan->last_done) == hipErrorNotReady);
}

extern "C++" int sls::enqueue_launches(sls_plan* plan, const KernelParams& kp, hipStream_t st, const SelectedRun* sel, const LaunchEvents* ev) {
  const bool multi = plan->launches.size() > 1;
  if (plan->grad.d_mu) plan->grad.executed = true;      // every run of a flagged plan rewrites the multiplier slots it solves
  if (plan->has_tile) HIPCHK(plan->ctx, hipMemsetAsync(plan->d_counters, 0, plan->launches.size() * sizeof(int32_t), st));
  if (multi) HIPCHK(plan->ctx, hipEventRecord(plan->ev_fork, st));
  for (size_t li = 0; li < plan->launches.size(); ++li) {
    const auto& L = plan->launches[li];
    const int nsub = sel ? sel->count[li] : L.nsub;
    if (sel && nsub <= 0) continue;
    const int grid = sel ? std::min(L.grid, nsub) : L.grid;
    hipStream_t ls = (li == 0) ? st : L.stream;
    if (li > 0) HIPCHK(plan->ctx, hipStreamWaitEvent(ls, plan->ev_fork, 0));
    KernelParams q = kp;
    q.order_off = L.order_off; q.nsub = nsub; q.fac_stride = L.fac_stride;
    if (sel) q.order = sel->order;
    q.fac_ws = kp.fac_ws + L.fac_off;
    hipError_t e;
    const bool tile = L.kind == LaunchKind::Tile;
    if (tile || L.kind == LaunchKind::Workgroup) {
      q.nmax = L.nmax; q.mmax = L.mmax; q.nnzA_cap = L.nnzA_cap; q.nnzB_cap = L.nnzB_cap;
      q.vec_in_lds = L.vec_in_lds; q.vec_stride = L.vec_stride; q.vec_ws = kp.vec_ws ? kp.vec_ws + L.vec_off : nullptr;
      q.tile_oth_rows = L.oth_rows;
      q.work_counter = tile ? plan->d_counters + li : nullptr;
      q.big_ws = L.big ? plan->d_big + L.big_off : nullptr; q.big_stride = L.big_stride;
      e = tile ? launch_tile(q, grid, L.lds, ls, L.mlds, L.two_per_cu, L.gw, L.big, ev) : launch_general(q, grid, L.lds, ls, L.wide, ev);
    } else {
      q.w_mcap = L.mcap; q.w_nm_max = L.nm_max; q.w_pl_off = L.pl_off;
      q.work_counter = (kp.objective == 1 && L.kind == LaunchKind::OneWave) ? plan->d_counters + li : nullptr;
      q.vec_in_lds = L.vec_in_lds; q.vec_stride = L.vec_stride; q.vec_ws = kp.vec_ws ? kp.vec_ws + L.vec_off : nullptr;
      if (L.four) {
        q.t4_rec = plan->d_t4 + L.t4_off * plan->t4_stride; q.t4_stride = plan->t4_stride;
        q.t4_pos = sel ? sel->pos + L.order_off : nullptr;
        q.t4_static = plan->d_t4s ? plan->d_t4s + L.t4s_off : nullptr; q.t4_static_stride = L.t4s_stride;
        q.t4_images = plan->d_t4s ? plan->d_t4i + L.t4i_off : nullptr; q.t4_images_stride = L.t4i_stride;
      }
      e = (L.kind == LaunchKind::Twisted) ? (L.four ? launch_twisted4(L.cls, q, grid, L.lds, ls, ev) : launch_twisted(L.cls, q, grid, L.lds, ls, ev))
                        : launch_wave(L.cls, q, grid, L.lds, ls, ev);
    }
    if (e != hipSuccess) return hipfail(plan->ctx, e, "kernel launch");
    if (li > 0) {
      HIPCHK(plan->ctx, hipEventRecord(L.done, ls));
      HIPCHK(plan->ctx, hipStreamWaitEvent(st, L.done, 0));
    }
  }
  return 0;
}

int sls_plan_execute(sls_plan* plan, void* hip_stream, double* d_values, int packed) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!d_values && plan->info.n_packed > 0) return fail(plan->ctx, SLS_EINVAL, "null device value pointer");
  if (plan->kp.nsub == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);   // NULL = HIP's null stream (torch's default stream)
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (packed && !plan->d_pdest) return fail(plan->ctx, SLS_EINVAL, "this plan was built without the packed layout");
  KernelParams kp = plan->kp;
  kp.out = d_values;
  kp.dest_pool = packed ? plan->d_pdest : plan->d_dest;
  if (plan->ev_used == kEventPool) { int rc = fold_events(plan, false); if (rc) return rc; }   // never blocks the host
  const int ev = plan->ev_used;
  const bool timed = ev < kEventPool;      // pool still full of launches in flight: this one goes untimed
  if (timed && !plan->ev_start[ev]) {
    HIPCHK(plan->ctx, hipEventCreate(&plan->ev_start[ev]));
    HIPCHK(plan->ctx, hipEventCreate(&plan->ev_stop[ev]));
  }
  // One solve kernel and nothing else (no forked size classes, no counter memset, no refinement behind it): the events ride on
  // the kernel's own dispatch packet and no hipEventRecord is made.  A record on a busy stream queues a marker, a barrier packet
  // with a completion signal of its own, so marker → kernel → marker were three dependent hand-offs in the queue where the
  // result needs one.  The timed interval is then the dispatch's begin → end; last_done is the same handle as on the marker path.
  if (!plan->refine && one_kernel_run(plan, st, nullptr)) {
    if (!timed && !plan->ev_done) HIPCHK(plan->ctx, hipEventCreateWithFlags(&plan->ev_done, hipEventDisableTiming));
    const LaunchEvents le = timed ? LaunchEvents{plan->ev_start[ev], plan->ev_stop[ev]} : LaunchEvents{nullptr, plan->ev_done};
    if (int rc = enqueue_launches(plan, kp, st, nullptr, &le)) return rc;
    if (timed) plan->ev_used = ev + 1;
    plan->last_done = le.stop;
    return 0;
  }
  if (timed) HIPCHK(plan->ctx, hipEventRecord(plan->ev_start[ev], st));
  // size classes run concurrently (enqueue_launches)
  if (int rc = enqueue_launches(plan, kp, st, nullptr)) return rc;
  if (plan->refine) {                      // attached by sls_plan_refine: after the joins above, same stream, same array, same layout
    int rc = sls_plan_execute(plan->refine, hip_stream, d_values, packed);
    if (rc) return rc;
  }
  // The end of this execute on the caller's stream: a timed execute's stop event is that point already (two event records per
  // execute, not three); only an untimed one records the dedicated event.  An event handle stays the same object when
  // fold_events compacts the pool, and a stop event is recorded again only at the end of a later execute, which then points
  // last_done at it.
  if (timed) {
    HIPCHK(plan->ctx, hipEventRecord(plan->ev_stop[ev], st));
    plan->ev_used = ev + 1;
    plan->last_done = plan->ev_stop[ev];
  } else {
    if (!plan->ev_done) HIPCHK(plan->ctx, hipEventCreateWithFlags(&plan->ev_done, hipEventDisableTiming));
    HIPCHK(plan->ctx, hipEventRecord(plan->ev_done, st));
    plan->last_done = plan->ev_done;
  }
  return 0;
}

int sls_plan_execute_batch(sls_plan* const* plans, int nplans, void* hip_stream, double* const* d_values, int packed) {
  if (nplans < 0 || (nplans > 0 && (!plans || !d_values))) return fail(nullptr, SLS_EINVAL, "null argument");
  if (nplans == 0) return 0;
  for (int i = 0; i < nplans; ++i) {
    if (!plans[i]) return fail(nullptr, SLS_EINVAL, "null plan in batch");
    if (plans[i]->dev != plans[0]->dev) return fail(plans[i]->ctx, SLS_EINVAL, "plans of one batch must live on the same device");
    for (int j = 0; j < i; ++j)
      if (plans[j] == plans[i]) return fail(plans[i]->ctx, SLS_EINVAL, "a plan appears twice in the batch");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  sls_plan* p0 = plans[0];
  HIPCHK(p0->ctx, hipSetDevice(p0->dev));
  if (nplans == 1) return sls_plan_execute(p0, hip_stream, d_values[0], packed);
  // plan 0 runs on the caller's stream itself; the others on their plan-owned streams, each made to wait for the caller's
  // stream first (fork edge: one event recorded on hip_stream) and joined back into it by one event.  The fork edge is what
  // makes the usual loop safe — execute_batch, a consumer of d_values[i] queued on hip_stream, execute_batch again: without
  // it the second call's kernels on plan i's stream could overwrite d_values[i] while that consumer still reads it (a plan
  // reads nothing the caller's stream produces, but it WRITES what earlier work there may still read).  A cross-queue wait
  // costs ≈50 µs on this stack; SLS_BATCH_FORK=0 drops the edge for callers that never recycle d_values[i] that way.
  static const bool fork = [] { const char* e = sls_knob("SLS_BATCH_FORK"); return !(e && e[0] == '0'); }();
  if (fork) {
    if (!p0->ev_batch) HIPCHK(p0->ctx, hipEventCreateWithFlags(&p0->ev_batch, hipEventDisableTiming));
    HIPCHK(p0->ctx, hipEventRecord(p0->ev_batch, st));
  }
  for (int i = 1; i < nplans; ++i) {
    sls_plan* pl = plans[i];
    if (fork) HIPCHK(pl->ctx, hipStreamWaitEvent(pl->stream, p0->ev_batch, 0));
    int rc = sls_plan_execute(pl, pl->stream, d_values[i], packed);
    if (rc) return rc;
    if (!pl->ev_batch_done) HIPCHK(pl->ctx, hipEventCreateWithFlags(&pl->ev_batch_done, hipEventDisableTiming));
    HIPCHK(pl->ctx, hipEventRecord(pl->ev_batch_done, pl->stream));
  }
  int rc = sls_plan_execute(p0, hip_stream, d_values[0], packed);
  if (rc) return rc;
  for (int i = 1; i < nplans; ++i) HIPCHK(plans[i]->ctx, hipStreamWaitEvent(st, plans[i]->ev_batch_done, 0));   // join
  return 0;
}

int sls_plan_synchronize(sls_plan* plan, void* hip_stream) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  HIPCHK(plan->ctx, hipStreamSynchronize(st));
  return 0;
}

int sls_plan_packed_dest(const sls_plan* plan, int64_t* dest) {
  if (!plan || (!dest && plan->info.n_packed > 0)) return fail(nullptr, SLS_EINVAL, "null argument");
  std::copy(plan->sym.packed_to_final.begin(), plan->sym.packed_to_final.end(), dest);
  return 0;
}

int sls_plan_fetch_status(sls_plan* plan, int32_t* col_status, double* residual, int32_t* iters) {
  int rc = fetch_status_raw(plan, col_status, residual, iters);
  if (rc || !plan->refine) return rc;
  // the refined subproblems report the tile kernel's outcome (iterations of both passes added up)
  sls_plan* rp = plan->refine;
  const size_t nr = (size_t)rp->kp.nsub;
  std::vector<int32_t> st2(nr), it2(nr); std::vector<double> rs2(nr);
  rc = fetch_status_raw(rp, st2.data(), rs2.data(), it2.data());
  if (rc) return rc;
  for (size_t k = 0; k < nr && k < plan->refine_dst.size(); ++k) {
    const int64_t d = plan->refine_dst[k];
    if (col_status) col_status[d] = st2[k];
    if (residual) residual[d] = rs2[k];
    if (iters) iters[d] += it2[k];
  }
  return 0;
}

extern "C++" int sls::fetch_status_raw(sls_plan* plan, int32_t* col_status, double* residual, int32_t* iters) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = wait_plan_done(plan)) return rc;
  const size_t n = (size_t)plan->kp.nsub;
  if (n == 0) return 0;
  // three small arrays: queued together into the slot's pinned buffer and waited for once (a synchronous hipMemcpy each costs
  // ≈20 µs of latency — a sixth of a README solve)
  if (unsigned char* pin = slot_pinned(plan->ctx, plan->slot, n * 16)) {
    hipStream_t st = plan->stream;
    if (col_status) HIPCHK(plan->ctx, hipMemcpyAsync(pin, plan->kp.status, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (residual) HIPCHK(plan->ctx, hipMemcpyAsync(pin + n * 8, plan->kp.resid, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (iters) HIPCHK(plan->ctx, hipMemcpyAsync(pin + n * 4, plan->kp.iters, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(plan->ctx, hipStreamSynchronize(st));
    if (col_status) std::memcpy(col_status, pin, n * sizeof(int32_t));
    if (residual) std::memcpy(residual, pin + n * 8, n * sizeof(double));
    if (iters) std::memcpy(iters, pin + n * 4, n * sizeof(int32_t));
    return 0;
  }
  if (col_status) HIPCHK(plan->ctx, hipMemcpy(col_status, plan->kp.status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (residual) HIPCHK(plan->ctx, hipMemcpy(residual, plan->kp.resid, n * sizeof(double), hipMemcpyDeviceToHost));
  if (iters) HIPCHK(plan->ctx, hipMemcpy(iters, plan->kp.iters, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

int sls_plan_objective(sls_plan* plan, void* hip_stream, const double* d_values, int packed, double* d_col_objective, double* d_total) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!d_values && plan->info.n_packed > 0) return fail(plan->ctx, SLS_EINVAL, "null device value pointer");
  if (packed && !plan->d_pdest) return fail(plan->ctx, SLS_EINVAL, "this plan was built without the packed layout");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (plan->kp.nsub == 0) {
    if (d_total) HIPCHK(plan->ctx, hipMemsetAsync(d_total, 0, sizeof(double), st));
    return 0;
  }
  ObjectiveParams op{};
  op.subs = plan->kp.subs; op.nsub = plan->kp.nsub; op.T = plan->kp.T; op.objective = plan->kp.objective;
  op.ngen = (int32_t)plan->obj_gen.size(); op.gen_list = plan->d_gen;
  op.mask_pool = plan->kp.mask_pool; op.dest = packed ? plan->d_pdest : plan->d_dest;
  op.w_pool = plan->kp.w_pool; op.obj_pool = plan->d_obj; op.values = d_values;
  op.col_objective = d_col_objective ? d_col_objective : plan->d_colobj;
  hipError_t e = launch_objective(op, plan->obj_lds_doubles, d_total, st);
  if (e != hipSuccess) return hipfail(plan->ctx, e, "launch objective kernels");
  return 0;
}

int sls_plan_fetch_objective(sls_plan* plan, const double* d_values, int packed, double* col_objective, double* total) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  const size_t n = (size_t)plan->kp.nsub;
  if (n == 0) { if (total) *total = 0.0; return 0; }
  hipStream_t st = plan->stream;
  // the execute that wrote d_values may have run on another stream: the plan's stream waits for its end first
  if (plan->last_done) HIPCHK(plan->ctx, hipStreamWaitEvent(st, plan->last_done, 0));
  if (int rc = sls_plan_objective(plan, st, d_values, packed, plan->d_colobj, plan->d_colobj + n)) return rc;
  const size_t bytes = (n + 1) * sizeof(double);
  if (unsigned char* pin = slot_pinned(plan->ctx, plan->slot, bytes)) {
    HIPCHK(plan->ctx, hipMemcpyAsync(pin, plan->d_colobj, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(plan->ctx, hipStreamSynchronize(st));
    if (col_objective) std::memcpy(col_objective, pin, n * sizeof(double));
    if (total) std::memcpy(total, pin + n * sizeof(double), sizeof(double));
    return 0;
  }
  HIPCHK(plan->ctx, hipStreamSynchronize(st));
  if (col_objective) HIPCHK(plan->ctx, hipMemcpy(col_objective, plan->d_colobj, n * sizeof(double), hipMemcpyDeviceToHost));
  if (total) HIPCHK(plan->ctx, hipMemcpy(total, plan->d_colobj + n, sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int sls_ctx_want_objective(sls_ctx* ctx, int on) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  ctx->want_objective = on != 0;
  return 0;
}

int sls_ctx_last_objective(sls_ctx* ctx, double* col_objective, int64_t n, double* total) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (ctx->obj_state == 2)
    return fail(ctx, SLS_EUNSUPPORTED, "the last solve summed layers of overlapping groups: no single objective belongs to a column there");
  if (ctx->obj_state != 1) return fail(ctx, SLS_EINVAL, "no solve has run on this context with sls_ctx_want_objective on");
  if (n != (int64_t)ctx->last_objective.size()) return fail(ctx, SLS_EINVAL, "sls_ctx_last_objective: n is not the number of subproblems of the last solve");
  if (col_objective) std::copy(ctx->last_objective.begin(), ctx->last_objective.end(), col_objective);
  if (total) *total = ctx->last_total;
  return 0;
}

// ---- achievability residual against the full plant: sls_plan_residual, sls_plan_fetch_residual ----

// The device buffers of the residual pass, made by the first call that needs them.  The halo H(q) follows from the index sets
// and the CSC halves of the operator's pattern (build_halo_rows); the host copy of the index sets is gone after plan creation
// (and never existed for sls_h2_sf_plan_localized), so they are read back from the device once — a host wait, first use only.
static int residual_ensure(sls_plan* plan) {
  sls_plan::Residual& rs = plan->resid;
  if (rs.ready) return 0;
  const Symbolic& S = plan->sym;
  const size_t ns = (size_t)plan->kp.nsub;
  if (S.subs.size() != ns || S.sub_col.size() != ns) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_residual: this plan keeps no column list");
  int64_t nidx = 0;
  for (const SubDesc& sd : S.subs) nidx = std::max<int64_t>(nidx, std::max(sd.off_sx + sd.n, sd.off_su + sd.m));
  std::vector<int32_t> idx((size_t)std::max<int64_t>(nidx, 1), 0);
  if (nidx > 0) HIPCHK(plan->ctx, hipMemcpy(idx.data(), plan->kp.idx_pool, (size_t)nidx * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> hp;
  std::vector<int32_t> hr;
  build_halo_rows(S.At_csr, S.Bt_csr, S.subs.data(), (int64_t)ns, idx.data(), S.sub_col.data(), hp, hr);
  Arena ar;
  ar.table(S.sub_col, &rs.sub_col); ar.table(hp, &rs.halo_ptr); ar.table(hr, &rs.halo_rows);     // hr may be empty: nothing to copy
  ar.buffer(3 * ns + 2, &rs.out);
  void* base = nullptr;
  if (int rc = ar.commit(plan->ctx, &base, "hipMalloc (residual tables)", "hipMemcpy H2D (residual tables)")) return rc;
  plan->dev_allocs.push_back(base);
  rs.ready = true;
  return 0;
}

int sls_plan_residual(sls_plan* plan, void* hip_stream, const double* d_values, int packed, double* d_res_inf, double* d_halo_inf,
                      double* d_res_l1, double* d_totals) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!d_values) return fail(plan->ctx, SLS_EINVAL, "null device value pointer");
  if (packed && !plan->d_pdest) return fail(plan->ctx, SLS_EINVAL, "this plan was built without the packed layout");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (plan->kp.nsub == 0) {
    if (d_totals) HIPCHK(plan->ctx, hipMemsetAsync(d_totals, 0, 2 * sizeof(double), st));
    return 0;
  }
  if (int rc = residual_ensure(plan)) return rc;
  const KernelParams& kp = plan->kp;
  const size_t n = (size_t)kp.nsub;
  ResidualParams rp{};
  rp.subs = kp.subs; rp.nsub = kp.nsub; rp.T = kp.T;
  rp.idx_pool = kp.idx_pool; rp.mask_pool = kp.mask_pool; rp.dest = packed ? plan->d_pdest : plan->d_dest;
  rp.A_rowptr = kp.A_rowptr; rp.A_colidx = kp.A_colidx; rp.A_val = kp.A_val;
  rp.B_rowptr = kp.B_rowptr; rp.B_colidx = kp.B_colidx; rp.B_val = kp.B_val;
  rp.sub_col = plan->resid.sub_col; rp.halo_ptr = plan->resid.halo_ptr; rp.halo_rows = plan->resid.halo_rows;
  rp.values = d_values;
  rp.res_inf = d_res_inf ? d_res_inf : plan->resid.out;
  rp.halo_inf = d_halo_inf ? d_halo_inf : plan->resid.out + n;
  rp.res_l1 = d_res_l1 ? d_res_l1 : plan->resid.out + 2 * n;
  hipError_t e = launch_residual(rp, d_totals, st);
  if (e != hipSuccess) return hipfail(plan->ctx, e, "launch residual kernels");
  return 0;
}

int sls_plan_fetch_residual(sls_plan* plan, const double* d_values, int packed, double* res_inf, double* halo_inf, double* res_l1,
                            double* totals) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!d_values) return fail(plan->ctx, SLS_EINVAL, "null device value pointer");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  const size_t n = (size_t)plan->kp.nsub;
  if (n == 0) { if (totals) totals[0] = totals[1] = 0.0; return 0; }
  hipStream_t st = plan->stream;
  // the execute that wrote d_values and the update that wrote the operator may have run on other streams
  if (plan->last_done) HIPCHK(plan->ctx, hipStreamWaitEvent(st, plan->last_done, 0));
  if (plan->upd_recorded) HIPCHK(plan->ctx, hipStreamWaitEvent(st, plan->ev_upd, 0));
  if (int rc = residual_ensure(plan)) return rc;
  double* out = plan->resid.out;
  if (int rc = sls_plan_residual(plan, st, d_values, packed, out, out + n, out + 2 * n, out + 3 * n)) return rc;
  const size_t bytes = (3 * n + 2) * sizeof(double);
  std::vector<double> stage_v;
  double* stage = reinterpret_cast<double*>(slot_pinned(plan->ctx, plan->slot, bytes));
  if (!stage) { stage_v.resize(3 * n + 2); stage = stage_v.data(); }
  HIPCHK(plan->ctx, hipMemcpyAsync(stage, out, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(plan->ctx, hipStreamSynchronize(st));
  if (res_inf) std::memcpy(res_inf, stage, n * sizeof(double));
  if (halo_inf) std::memcpy(halo_inf, stage + n, n * sizeof(double));
  if (res_l1) std::memcpy(res_l1, stage + 2 * n, n * sizeof(double));
  if (totals) std::memcpy(totals, stage + 3 * n, 2 * sizeof(double));
  return 0;
}

// ---- gradient of the 𝓗₂ cost in A, B2 and the LQR diagonals: sls_plan_gradient, sls_plan_fetch_gradient ----

// The tables and buffers of the gradient pass, made by the first call that needs them: like the residual's halo lists they
// follow from the index sets, which are read back from the device once — a host wait, first use only.
static int gradient_ensure(sls_plan* plan) {
  sls_plan::Gradient& gr = plan->grad;
  if (gr.ready) return 0;
  const Symbolic& S = plan->sym;
  const size_t ns = (size_t)plan->kp.nsub;
  if (S.subs.size() != ns || S.b_zero.size() != ns) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_gradient: this plan keeps no column list");
  int64_t nidx = 0;
  for (const SubDesc& sd : S.subs) nidx = std::max<int64_t>(nidx, std::max(sd.off_sx + sd.n, sd.off_su + sd.m));
  std::vector<int32_t> idx((size_t)std::max<int64_t>(nidx, 1), 0);
  if (nidx > 0) HIPCHK(plan->ctx, hipMemcpy(idx.data(), plan->kp.idx_pool, (size_t)nidx * sizeof(int32_t), hipMemcpyDeviceToHost));
  GradientTables G;
  build_gradient_tables(S.At_csr, S.Bt_csr, S.subs.data(), (int64_t)ns, idx.data(), G);
  if (G.nnzA + G.nnzB > INT32_MAX) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_gradient: more than 2³¹ − 1 stored entries");
  int64_t need = 0;
  for (const SubDesc& sd : S.subs) need = std::max<int64_t>(need, (int64_t)(S.T + 1) * sd.n + (int64_t)S.T * (sd.n + sd.m));
  gr.lds_doubles = (int)std::min<int64_t>(need, 8000);                    // λ and z of a column in LDS when they fit 64 000 B
  gr.nnzA = G.nnzA; gr.nnzB = G.nnzB;
  const bool wu = S.wu.updatable;
  Arena ar;
  ar.table(S.b_zero, &gr.b_zero);
  ar.table(G.ent_ptr, &gr.ent_ptr); ar.table(G.ent, &gr.ent); ar.table(G.inv_ptr, &gr.inv_ptr); ar.table(G.inv_slot, &gr.inv_slot);
  if (wu) { ar.table(G.w_base, &gr.w_base); ar.table(G.winv_ptr, &gr.winv_ptr); ar.table(G.winv_slot, &gr.winv_slot); }
  ar.buffer((size_t)std::max<int64_t>(G.ent_ptr[ns], 1), &gr.contrib);
  if (wu) ar.buffer((size_t)std::max<int64_t>(G.w_base[ns], 1), &gr.wcontrib);
  ar.buffer(ns, &gr.col_weight);
  ar.buffer((size_t)(G.nnzA + G.nnzB + S.Nx + S.Nu + 1), &gr.out);
  void* base = nullptr;
  if (int rc = ar.commit(plan->ctx, &base, "hipMalloc (gradient tables)", "hipMemcpy H2D (gradient tables)")) return rc;
  plan->dev_allocs.push_back(base);
  gr.ready = true;
  return 0;
}

int sls_plan_gradient(sls_plan* plan, void* hip_stream, const double* d_values, int packed, const double* d_col_weight,
                      double* d_gA, double* d_gB2, double* d_gc1, double* d_gd12) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!plan->grad.d_mu) return fail(plan->ctx, SLS_EINVAL, "sls_plan_gradient: the plan was built without SLS_PLAN_MULTIPLIERS");
  if (!plan->grad.executed) return fail(plan->ctx, SLS_EINVAL, "sls_plan_gradient: no execute has run on this plan yet");
  if ((d_gc1 || d_gd12) && !plan->sym.wu.updatable)
    return fail(plan->ctx, SLS_EINVAL, "sls_plan_gradient: the weight derivatives need a plan built with SLS_PLAN_WEIGHTS_UPDATABLE");
  if (!d_values && plan->info.n_packed > 0) return fail(plan->ctx, SLS_EINVAL, "null device value pointer");
  if (packed && !plan->d_pdest) return fail(plan->ctx, SLS_EINVAL, "this plan was built without the packed layout");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (plan->kp.nsub == 0) return 0;
  if (int rc = gradient_ensure(plan)) return rc;
  // behind the execute that wrote d_values and the multipliers, and behind the plan's last update (the diagonals, the records)
  if (plan->last_done) HIPCHK(plan->ctx, hipStreamWaitEvent(st, plan->last_done, 0));
  if (plan->upd_recorded || plan->w_upd_recorded) HIPCHK(plan->ctx, hipStreamWaitEvent(st, plan->ev_upd, 0));
  const KernelParams& kp = plan->kp;
  const sls_plan::Gradient& gr = plan->grad;
  GradientParams gp{};
  gp.subs = kp.subs; gp.nsub = kp.nsub; gp.T = kp.T;
  gp.mask_pool = kp.mask_pool; gp.dest = packed ? plan->d_pdest : plan->d_dest; gp.values = d_values;
  gp.mu = gr.d_mu; gp.obj_pool = plan->d_obj; gp.b_zero = gr.b_zero; gp.status = kp.status; gp.col_weight = d_col_weight;
  gp.ent_ptr = gr.ent_ptr; gp.ent = gr.ent; gp.inv_ptr = gr.inv_ptr; gp.inv_slot = gr.inv_slot; gp.contrib = gr.contrib;
  gp.nnzA = gr.nnzA; gp.nnzB = gr.nnzB; gp.gA = d_gA; gp.gB2 = d_gB2;
  if (d_gc1 || d_gd12) {
    gp.b2 = plan->d_w_b2; gp.diag = plan->d_w_diag; gp.w_base = gr.w_base; gp.winv_ptr = gr.winv_ptr; gp.winv_slot = gr.winv_slot;
    gp.wcontrib = gr.wcontrib; gp.Nx = plan->sym.Nx; gp.Nu = plan->sym.Nu; gp.gc1 = d_gc1; gp.gd12 = d_gd12;
  }
  hipError_t e = launch_gradient(gp, gr.lds_doubles, st);
  if (e != hipSuccess) return hipfail(plan->ctx, e, "launch gradient kernels");
  return 0;
}

int sls_plan_fetch_gradient(sls_plan* plan, const double* d_values, int packed, const double* col_weight,
                            double* gA, double* gB2, double* gc1, double* gd12, int64_t* n_skipped) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!plan->grad.d_mu) return fail(plan->ctx, SLS_EINVAL, "sls_plan_gradient: the plan was built without SLS_PLAN_MULTIPLIERS");
  if (!plan->grad.executed) return fail(plan->ctx, SLS_EINVAL, "sls_plan_gradient: no execute has run on this plan yet");
  if ((gc1 || gd12) && !plan->sym.wu.updatable)
    return fail(plan->ctx, SLS_EINVAL, "sls_plan_gradient: the weight derivatives need a plan built with SLS_PLAN_WEIGHTS_UPDATABLE");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (n_skipped) *n_skipped = 0;
  const size_t n = (size_t)plan->kp.nsub;
  if (n == 0) return 0;
  if (int rc = gradient_ensure(plan)) return rc;
  hipStream_t st = plan->stream;
  sls_plan::Gradient& gr = plan->grad;
  if (col_weight) {
    if (int rc = stage_to_device(plan->ctx, plan->slot, st, gr.col_weight, col_weight, n, nullptr, 0)) return rc;
  }
  const size_t nA = (size_t)gr.nnzA, nB = (size_t)gr.nnzB, Nx = (size_t)plan->sym.Nx, Nu = (size_t)plan->sym.Nu;
  double* o = gr.out;
  if (int rc = sls_plan_gradient(plan, st, d_values, packed, col_weight ? gr.col_weight : nullptr, gA ? o : nullptr, gB2 ? o + nA : nullptr,
                                 gc1 ? o + nA + nB : nullptr, gd12 ? o + nA + nB + Nx : nullptr)) return rc;
  std::vector<double> host(nA + nB + Nx + Nu + 1);
  if (int rc = fetch_to_host(plan->ctx, plan->slot, st, host.data(), o, host.size() * sizeof(double))) return rc;
  if (gA) std::memcpy(gA, host.data(), nA * sizeof(double));
  if (gB2) std::memcpy(gB2, host.data() + nA, nB * sizeof(double));
  if (gc1) std::memcpy(gc1, host.data() + nA + nB, Nx * sizeof(double));
  if (gd12) std::memcpy(gd12, host.data() + nA + nB + Nx, Nu * sizeof(double));
  if (n_skipped) {
    std::vector<int32_t> stt(n);
    if (int rc = fetch_status_raw(plan, stt.data(), nullptr, nullptr)) return rc;
    for (int32_t s : stt) *n_skipped += (s != SLS_COL_OK && s != SLS_COL_TRIVIAL);
  }
  return 0;
}

int sls_plan_fetch_multipliers(sls_plan* plan, int64_t sub, double* mu, int64_t len) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!plan->grad.d_mu) return fail(plan->ctx, SLS_EINVAL, "sls_plan_fetch_multipliers: the plan was built without SLS_PLAN_MULTIPLIERS");
  if (!plan->grad.executed) return fail(plan->ctx, SLS_EINVAL, "sls_plan_fetch_multipliers: no execute has run on this plan yet");
  if (sub < 0 || sub >= plan->kp.nsub || (size_t)sub >= plan->sym.subs.size()) return fail(plan->ctx, SLS_EINVAL, "sls_plan_fetch_multipliers: sub out of range");
  const SubDesc& sd = plan->sym.subs[(size_t)sub];
  const int64_t T = plan->kp.T, n = sd.n;
  if (!mu && len == 0) return (int)((T + 1) * n);                       // the size query
  if (!mu || len != (T + 1) * n) return fail(plan->ctx, SLS_EINVAL, "sls_plan_fetch_multipliers: mu must hold (T+1)·ñx doubles");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = wait_plan_done(plan)) return rc;
  hipStream_t st = plan->stream;
  if (plan->w_upd_recorded) HIPCHK(plan->ctx, hipStreamWaitEvent(st, plan->ev_upd, 0));
  const size_t slot = (size_t)mu_slot_doubles((int)T);
  std::vector<double> lam(slot);
  double scale[2] = {1.0, 0.0};
  if (int rc = fetch_to_host(plan->ctx, plan->slot, st, lam.data(), plan->grad.d_mu + (size_t)sub * slot, slot * sizeof(double))) return rc;
  if (int rc = fetch_to_host(plan->ctx, plan->slot, st, scale, plan->d_obj + 2 * (size_t)sub, sizeof scale)) return rc;
  const double f = column_factor(sd.has_w, scale[0]);
  for (int64_t k = 0; k <= T; ++k)
    for (int64_t a = 0; a < n; ++a) mu[k * n + a] = f * lam[(size_t)(k * kMuLd + a)];
  return 0;
}

int sls_plan_describe(const sls_plan* plan, char* buf, int64_t buflen) {
  if (!plan || !buf || buflen <= 0) return fail(nullptr, SLS_EINVAL, "null argument");
  std::string d;
  for (const auto& L : plan->launches) d += describe_launch(L);
  std::snprintf(buf, (size_t)buflen, "%s", d.c_str());
  return 0;
}

int sls_plan_kernel_time_ms(sls_plan* plan, double* avg_ms, int64_t* n_launches) {
  if (!plan || !avg_ms) return fail(nullptr, SLS_EINVAL, "null argument");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  int rc = fold_events(plan);
  if (rc) return rc;
  *avg_ms = plan->ev_acc_n ? plan->ev_acc_ms / (double)plan->ev_acc_n : 0.0;
  if (n_launches) *n_launches = plan->ev_acc_n;
  plan->ev_acc_ms = 0.0; plan->ev_acc_n = 0;
  return 0;
}

int sls_plan_alloc_values(sls_plan* plan, int packed, double** d_values_out) {
  if (!plan || !d_values_out) return fail(nullptr, SLS_EINVAL, "null argument");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  const size_t n = (size_t)std::max<int64_t>(packed ? plan->info.n_packed : plan->info.n_values, 1);
  void* d = nullptr;
  HIPCHK(plan->ctx, hipMalloc(&d, n * sizeof(double)));
  hipError_t e = hipMemset(d, 0, n * sizeof(double));
  if (e != hipSuccess) { (void)hipFree(d); return hipfail(plan->ctx, e, "hipMemset"); }
  *d_values_out = reinterpret_cast<double*>(d);
  return 0;
}

int sls_plan_free_values(sls_plan* plan, double* d_values) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (d_values) HIPCHK(plan->ctx, hipFree(d_values));
  return 0;
}

int sls_plan_download(sls_plan* plan, const double* d_values, double* const* phix_vals, double* const* phiu_vals) {
  if (!plan || !phix_vals || !phiu_vals) return fail(nullptr, SLS_EINVAL, "null argument");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  const Symbolic& S = plan->sym;
  // waits for this plan's last sls_plan_execute, not for the device: a d_values produced by other work of the caller (the
  // unpack of an all-gather on a side stream) has to be complete, or ordered by sls_plan_synchronize on that stream, before this call
  if (int rc = wait_plan_done(plan)) return rc;
  for (int64_t t = 0; t < S.T; ++t) {
    if (S.off_x[t + 1] > S.off_x[t] && !phix_vals[t]) return fail(plan->ctx, SLS_EINVAL, "null phix_vals[t]");
    if (S.off_u[t + 1] > S.off_u[t] && !phiu_vals[t]) return fail(plan->ctx, SLS_EINVAL, "null phiu_vals[t]");
  }
  // small Φ (README: 2T slices of a few KB): one D2H into a staging buffer, then host copies.  Large Φ: the mask-order array
  // is cut into 1 MiB chunks that kDlLanes host threads bring over concurrently, each through its own stream and pinned
  // chunk (DMA at link speed into pinned memory, then a host copy into the caller's pageable slices — whose first-touch
  // page faults are spread over the lanes, and overlap the other lanes' DMA).  A pageable hipMemcpy per slice ran at
  // 14 GB/s (chain-4096: 43 MB in 3.1 ms).
  const bool direct = S.n_values * (int64_t)sizeof(double) > (4ll << 20);
  if (!direct && S.n_values > 0) {
    const double* stage = reinterpret_cast<const double*>(slot_pinned(plan->ctx, plan->slot, (size_t)S.n_values * sizeof(double)));
    if (!stage) { plan->host_stage.resize((size_t)S.n_values); stage = plan->host_stage.data(); }
    HIPCHK(plan->ctx, hipMemcpy(const_cast<double*>(stage), d_values, (size_t)S.n_values * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t t = 0; t < S.T; ++t) {
      const int64_t nx = S.off_x[t + 1] - S.off_x[t], nu = S.off_u[t + 1] - S.off_u[t];
      if (nx > 0) std::memcpy(phix_vals[t], stage + S.off_x[t], (size_t)nx * sizeof(double));
      if (nu > 0) std::memcpy(phiu_vals[t], stage + S.off_u[t], (size_t)nu * sizeof(double));
    }
    return 0;
  }
  if (S.n_values == 0) return 0;
  {
    // slice table: flat offset → caller's array
    const int64_t T = S.T;
    std::vector<int64_t> beg(2 * T + 1);
    std::vector<void*> ptrs(2 * T);
    for (int64_t t = 0; t < T; ++t) { beg[t] = S.off_x[t]; ptrs[t] = phix_vals[t]; beg[T + t] = S.off_u[t]; ptrs[T + t] = phiu_vals[t]; }
    beg[2 * T] = S.n_values;
    const int rc = pinned_download(plan->ctx, plan->slot, plan->dev, d_values, beg, ptrs);
    if (rc <= 0) return rc;                 // 0 done, < 0 error; > 0: pinned path unavailable
  }
  for (int64_t t = 0; t < S.T; ++t) {                      // fallback: pageable copies, slice by slice
    const int64_t nx = S.off_x[t + 1] - S.off_x[t], nu = S.off_u[t + 1] - S.off_u[t];
    if (nx > 0) HIPCHK(plan->ctx, hipMemcpy(phix_vals[t], d_values + S.off_x[t], (size_t)nx * sizeof(double), hipMemcpyDeviceToHost));
    if (nu > 0) HIPCHK(plan->ctx, hipMemcpy(phiu_vals[t], d_values + S.off_u[t], (size_t)nu * sizeof(double), hipMemcpyDeviceToHost));
  }
  return 0;
}

int sls_scatter_f64(sls_ctx* ctx, int dev_slot, void* hip_stream, const double* d_src, const int64_t* d_idx, int64_t n,
                    double* d_dst) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "dev_slot out of range");
  if (n < 0 || (n > 0 && (!d_src || !d_idx || !d_dst))) return fail(ctx, SLS_EINVAL, "bad scatter arguments");
  HIPCHK(ctx, hipSetDevice(ctx->devs[dev_slot]));
  hipError_t e = launch_scatter(d_src, d_idx, n, d_dst, reinterpret_cast<hipStream_t>(hip_stream));
  if (e != hipSuccess) return hipfail(ctx, e, "launch scatter_f64_kernel");
  return 0;
}

}  // extern "C"
