// sls_api.cpp — implementation of include/sls_mi355x.h (the drop-in C ABI): the context, its pinned staging buffer, and the resident
// plans (build, execute, batch, status, objective, residual, download, destroy).  Plant and weights updates and partial re-solves
// of a plan are in sls_plan_update.cpp, the one-shot calls built on plans (sls_h2_sf_solve ≙ SLS_𝓗₂(P, 𝓢; 𝓘),
// src/synthesis.jl:11-32) in sls_dropin.cpp, the three device symbolic passes (sls_localization_masks_device,
// sls_index_sets_device, sls_h2_sf_plan_localized) in sls_symbolic_device.cpp, the exports of include/sls_mi355x_debug.h in
// sls_debug.cpp.
//
// Host side of the path that replaces reference src/synthesis.jl:11-72:
//   sls_h2_sf_plan       ≙ the per-column set-up the reference redoes inside the loop
//                           (src/reduction.jl:11-27, src/synthesis.jl:40-43,57-60)
//   sls_plan_execute     ≙ the @distributed loop body's solve   (src/synthesis.jl:46-62)
//   sls_plan_download    ≙ the scatter into Φx[t], Φu[t]         (src/synthesis.jl:65-67)
// No CPU fallback exists: without a gfx950 device every compute entry point fails
// with SLS_ENODEVICE / SLS_EHIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_device.h"
#include "sls_dropin_host.h"
#include "sls_internal.h"
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

namespace {
constexpr int64_t kT4StaticBudget = 64ll << 20;   // bytes of plan-time static blocks a plan may hold (four-wave kernel)

// Device memory of a plan comes from ONE allocation: requests are recorded first and committed together (one hipMalloc,
// one staged H2D copy).  A README-sized plan used to spend 2 ms in ~25 hipMalloc/hipMemcpy calls for a 0.2 ms solve.
template <class V>
int upload(sls_plan* pl, const V& v, const typename V::value_type** out) {
  using T = typename V::value_type;
  sls_plan::ArenaReq r{};
  r.src = v.empty() ? nullptr : static_cast<const void*>(v.data());
  r.bytes = v.size() * sizeof(T);
  r.out = reinterpret_cast<void**>(const_cast<T**>(out));
  pl->arena_reqs.push_back(r);
  return 0;
}
template <class T>
int dalloc(sls_plan* pl, size_t count, T** out) {
  sls_plan::ArenaReq r{};
  r.src = nullptr; r.bytes = count * sizeof(T); r.out = reinterpret_cast<void**>(out); r.zero = true;
  pl->arena_reqs.push_back(r);
  return 0;
}
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

}  // namespace

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

int arena_commit(sls_plan* pl) {
  auto al = [](size_t b) { return (std::max<size_t>(b, 16) + 255) / 256 * 256; };
  constexpr size_t kSmall = 256u << 10;
  // order: small uploads (staged on the host and copied with ONE hipMemcpy — a README plan has ~15 tables of a few KB
  // and each synchronous pageable copy costs ≈20 µs), then large uploads (copied in place), then scratch
  auto rank = [&](const sls_plan::ArenaReq& r) { return r.src == nullptr ? 2 : (r.bytes <= kSmall ? 0 : 1); };
  std::stable_sort(pl->arena_reqs.begin(), pl->arena_reqs.end(),
                   [&](const sls_plan::ArenaReq& a, const sls_plan::ArenaReq& b) { return rank(a) < rank(b); });
  size_t total = 0, small_bytes = 0;
  for (auto& r : pl->arena_reqs) { r.off = total; total += al(r.bytes); if (rank(r) == 0) small_bytes = total; }
  void* base = nullptr;
  hipError_t e = hipSuccess;
  {
    // the context keeps one arena for reuse (a drop-in call builds and drops a plan per call: a hipMalloc + hipFree pair of
    // tens of MB costs ≈0.2 ms, of a few hundred KB ≈30 µs); a second live plan gets its own
    sls_ctx::Slot* sl = (ctx_is_live(pl->ctx) && pl->slot < (int)pl->ctx->slots.size()) ? &pl->ctx->slots[pl->slot] : nullptr;
    const size_t want = std::max<size_t>(total, 256);
    if (sl && !sl->arena_in_use) {
      if (sl->arena_bytes < want || sl->arena_bytes > 4 * want + (64u << 20)) {      // too small, or wastefully large
        if (sl->arena) (void)hipFree(sl->arena);
        sl->arena = nullptr; sl->arena_bytes = 0;
        e = hipMalloc(&sl->arena, want);
        if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMalloc (plan arena)");
        sl->arena_bytes = want;
      }
      base = sl->arena; sl->arena_in_use = true; pl->arena_borrowed = true;
    } else {
      e = hipMalloc(&base, want);
      if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMalloc (plan arena)");
      pl->dev_allocs.push_back(base);
    }
  }
  pl->info.workspace_bytes += (int64_t)total;
  if (small_bytes) {
    // staged in the slot's pinned buffer when it fits (a pageable source costs the runtime one more copy and ≈15 µs)
    std::vector<unsigned char> stage_v;
    unsigned char* stage = slot_pinned(pl->ctx, pl->slot, small_bytes);
    if (!stage) { stage_v.resize(small_bytes); stage = stage_v.data(); }
    for (auto& r : pl->arena_reqs)
      if (rank(r) == 0 && r.bytes) std::memcpy(stage + r.off, r.src, r.bytes);
    e = hipMemcpy(base, stage, small_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMemcpy H2D (plan arena, staged tables)");
  }
  for (auto& r : pl->arena_reqs) {
    if (rank(r) == 1) {
      e = hipMemcpy(static_cast<unsigned char*>(base) + r.off, r.src, r.bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMemcpy H2D (plan arena)");
    }
  }
  // status / residual words are cleared (one memset over their contiguous range); the big workspaces need no clear
  size_t z0 = total, z1 = 0;
  for (auto& r : pl->arena_reqs) {
    *r.out = static_cast<unsigned char*>(base) + r.off;
    if (!r.src && r.zero && r.bytes <= (1u << 20)) { z0 = std::min(z0, r.off); z1 = std::max(z1, r.off + r.bytes); }
  }
  if (z1 > z0) {
    bool contiguous = true;
    for (auto& r : pl->arena_reqs)
      if (!r.src && r.off >= z0 && r.off < z1 && !(r.zero && r.bytes <= (1u << 20))) contiguous = false;
    if (contiguous) {
      e = hipMemsetAsync(static_cast<unsigned char*>(base) + z0, 0, z1 - z0, pl->stream);
      if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMemset");
    } else {
      for (auto& r : pl->arena_reqs)
        if (!r.src && r.zero && r.bytes <= (1u << 20)) {
          e = hipMemsetAsync(static_cast<unsigned char*>(base) + r.off, 0, r.bytes, pl->stream);
          if (e != hipSuccess) return hipfail(pl->ctx, e, "hipMemset");
        }
    }
  }
  pl->arena_reqs.clear();
  return 0;
}

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

int sls_h2_sf_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                   const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                   int64_t group_begin, int64_t group_end, sls_plan** plan_out) {
  return plan_create(ctx, dev_slot, dims, P, Sx, Su, ngroups, group_ptr, group_cols, group_begin, group_end, true, PlanOpts{}, plan_out);
}

// (extern "C++": declared in sls_plan.h with C++ linkage, defined here inside the extern "C" block of the ABI)
extern "C++" int sls::plan_create(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                                  const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                                  int64_t group_begin, int64_t group_end, bool want_packed, const PlanOpts& opt, sls_plan** plan_out) {
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

// second half of plan creation (contract: sls_plan.h)
extern "C++" int sls::plan_finish(sls_ctx* ctx, int dev_slot, const sls_dims* dims, sls_plan* pl, double t0, bool want_packed,
                                  const PlanOpts& opt, const DeviceTables* dt, sls_plan** plan_out) {
  int rc = 0;
  const double t1 = now_s();
  Symbolic& S = pl->sym;

  auto bail = [&](int code) { sls_plan_destroy(pl); return code; };
  const bool dbg_t = sls_knob("SLS_DEBUG_TIMING") != nullptr;
  double tdbg = now_s();
  auto tick = [&](const char* what) { if (dbg_t) { const double n = now_s(); std::fprintf(stderr, "[sls plan] %-28s %8.3f ms\n", what, 1e3 * (n - tdbg)); tdbg = n; } };
  hipError_t e = hipSetDevice(pl->dev);
  if (e != hipSuccess) return bail(hipfail(ctx, e, "hipSetDevice"));
  {
    sls_ctx::Slot& sl = ctx->slots[dev_slot];
    if (sl.streams_in_use == 0) {
      if (sl.streams.empty()) {
        hipStream_t st0 = nullptr;
        e = hipStreamCreateWithFlags(&st0, hipStreamNonBlocking);
        if (e != hipSuccess) return bail(hipfail(ctx, e, "hipStreamCreate"));
        sl.streams.push_back(st0);
      }
      pl->stream = sl.streams[0]; pl->streams_borrowed = true; sl.streams_in_use = 1;
    } else if (opt.force_tile) {
      // the refinement plan of the drop-in call: a stream of its own kept by the context (a hipStreamCreate per call cost 3 ms)
      if (!sl.refine_stream) {
        e = hipStreamCreateWithFlags(&sl.refine_stream, hipStreamNonBlocking);
        if (e != hipSuccess) return bail(hipfail(ctx, e, "hipStreamCreate"));
      }
      pl->stream = sl.refine_stream; pl->stream_external = true;
    } else {
      e = hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking);
      if (e != hipSuccess) return bail(hipfail(ctx, e, "hipStreamCreate"));
    }
  }
  for (int i = 0; i < kEventPool; ++i) { pl->ev_start[i] = nullptr; pl->ev_stop[i] = nullptr; }   // created on first use
  pl->events_ok = true;
  tick("setdevice+stream");

  KernelParams& kp = pl->kp;
  kp.T = (int32_t)S.T; kp.nsub = (int32_t)S.subs.size();
  kp.delta_rel = 1e-12; kp.tol = 1e-12; kp.tol_ok = 1e-9; kp.max_iters = 8;   // δ scan: tools/iters_hist.py, DESIGN.md §3
  kp.stag = 0.5;
  kp.objective = (dims->flags & SLS_SOLVE_SUM_OF_NORMS) ? 1 : 0;
  kp.son_maxit = 4000; kp.son_tol = 1e-9;
  if (const char* e = sls_knob("SLS_SON_MAXIT")) kp.son_maxit = std::max(1, std::atoi(e));
  if (const char* e = sls_knob("SLS_SON_TOL")) kp.son_tol = std::atof(e);
  kp.son_anderson = 1;
  if (const char* e = sls_knob("SLS_SON_ANDERSON")) kp.son_anderson = e[0] != '0';
  kp.son_aa_start = 20;
  if (const char* e = sls_knob("SLS_SON_AA_START")) kp.son_aa_start = std::max(0, std::atoi(e));
  if (kp.objective == 1) {
    // diagonal weights without feed-through only: a dense Hessian or a D11 column would change the cone structure
    for (const SubDesc& sd : S.subs) {
      bool bad = sd.has_w >= 2;
      if (sd.has_w == 1) for (int32_t i = 0; i < sd.n + sd.m && !bad; ++i) bad = S.w_pool[(size_t)sd.off_w + sd.n + sd.m + i] != 0.0;
      if (bad) return bail(fail(ctx, SLS_EUNSUPPORTED, "SLS_SOLVE_SUM_OF_NORMS needs a diagonal [C1 D12]'[C1 D12] and D11 = 0"));
    }
  }
  kp.delta_first = 1e-15;            // one-wave (throughput) kernel only: DESIGN.md §5
  if (const char* e = sls_knob("SLS_DELTA_FIRST")) kp.delta_first = std::atof(e);   // 0 = single attempt with delta_rel
  if (const char* e = sls_knob("SLS_STAG")) kp.stag = std::atof(e);   // experiments only
  if (const char* e = sls_knob("SLS_MAX_ITERS")) kp.max_iters = std::max(1, std::atoi(e));   // experiments only
  kp.max_iters_slow = 48;
  if (const char* e = sls_knob("SLS_MAX_ITERS_SLOW")) kp.max_iters_slow = std::max(0, std::atoi(e));   // 0: rounds 1–2 rule
  if (const char* e = sls_knob("SLS_TOL")) kp.tol = std::atof(e);
  if (const char* e = sls_knob("SLS_DELTA_REL")) kp.delta_rel = std::atof(e);
  const int ncu = ctx->ncu[dev_slot];

  // kernel selection (sls_routing.cpp): the launch list in submission order, its workspace layout, S.order launch by launch
  RoutingResult route;
  {
    std::string msg;
    rc = build_launch_list(S, kp.T, kp.objective, ncu, opt.force_tile, RoutingKnobs::from_env(), route, msg);
    if (rc) return bail(fail(ctx, rc, msg));
  }
  pl->launches = std::vector<sls_plan::Launch>(route.launches.begin(), route.launches.end());
  pl->has_tile = route.has_tile;
  pl->too_large_subs = route.too_large;
  pl->info_unsupported = (int64_t)route.too_large.size();
  kp.w_nzA = S.max_row_A; kp.w_nzAc = S.max_row_At; kp.w_nzB = S.max_row_B; kp.w_nzBc = S.max_row_Bt;

#define UP(vec, field)                                         \
  do { int rc__ = upload(pl, vec, &kp.field); if (rc__) return bail(rc__); } while (0)
  UP(S.A_csr.ptr, A_rowptr); UP(S.A_csr.idx, A_colidx); UP(S.A_csr.val, A_val);
  UP(S.At_csr.ptr, At_rowptr); UP(S.At_csr.idx, At_colidx); UP(S.At_csr.val, At_val);
  UP(S.B_csr.ptr, B_rowptr); UP(S.B_csr.idx, B_colidx); UP(S.B_csr.val, B_val);
  UP(S.Bt_csr.ptr, Bt_rowptr); UP(S.Bt_csr.idx, Bt_colidx); UP(S.Bt_csr.val, Bt_val);
  UP(S.subs, subs); UP(S.order, order);
  if (dt) kp.idx_pool = dt->d_idx; else UP(S.idx_pool, idx_pool);
  UP(S.w_pool, w_pool);
  const uint64_t* d_cmask = nullptr; const int32_t* d_cbase = nullptr; const int64_t* d_coff = nullptr;
  if (S.compact) {
    // tables expanded on the device (expand_tables_kernel) from the compact form: 16 B per (column, time step) uploaded
    // instead of 5 B per masked position
    if (dt) { d_cmask = dt->d_cmask; d_cbase = dt->d_cbase; d_coff = dt->d_coff; }
    else if ((rc = upload(pl, S.cmask, &d_cmask)) || (rc = upload(pl, S.cbase, &d_cbase)) || (rc = upload(pl, S.coff, &d_coff))) return bail(rc);
    if ((rc = dalloc(pl, (size_t)std::max<int64_t>(S.md_total, 1), const_cast<uint8_t**>(&kp.mask_pool)))) return bail(rc);
    if ((rc = dalloc(pl, (size_t)std::max<int64_t>(S.md_total, 1), const_cast<int32_t**>(&pl->d_dest)))) return bail(rc);
  } else {
    UP(S.mask_pool, mask_pool);
    if ((rc = upload(pl, S.dest_pool, &pl->d_dest))) return bail(rc);
  }
#undef UP
  if (want_packed && (rc = upload(pl, S.pdest_pool, &pl->d_pdest))) return bail(rc);
  {
    const size_t fac_need = route.fac_doubles, vec_need = route.vec_doubles, big_need = route.big_bytes;
    // the two big scratch workspaces (never initialised, never read before written) come from the context's cache
    const size_t need = (std::max<size_t>(fac_need, 1) + vec_need + 32) * sizeof(double) + 512 + big_need + 256;
    sls_ctx::Slot& sl = ctx->slots[dev_slot];
    void* sbase = nullptr;
    if (!sl.scratch_in_use) {
      if (sl.scratch_bytes < need) {
        if (sl.scratch) (void)hipFree(sl.scratch);
        sl.scratch = nullptr; sl.scratch_bytes = 0;
        e = hipMalloc(&sl.scratch, need);
        if (e != hipSuccess) return bail(hipfail(ctx, e, "hipMalloc (scratch workspace)"));
        sl.scratch_bytes = need;
      }
      sbase = sl.scratch; sl.scratch_in_use = true; pl->scratch_borrowed = true;
    } else {
      e = hipMalloc(&pl->own_scratch, need);
      if (e != hipSuccess) return bail(hipfail(ctx, e, "hipMalloc (scratch workspace)"));
      sbase = pl->own_scratch;
    }
    pl->info.workspace_bytes += (int64_t)need;
    kp.fac_ws = reinterpret_cast<double*>(sbase);
    kp.vec_ws = vec_need ? kp.fac_ws + ((fac_need + 31) / 32) * 32 : nullptr;
    if (big_need) {
      const size_t boff = ((((fac_need + 31) / 32) * 32 + vec_need + 32) * sizeof(double) + 255) / 256 * 256;
      pl->d_big = static_cast<unsigned char*>(sbase) + boff;
    }
  }
  size_t n_lo = 0;
  for (size_t li = 1; li < pl->launches.size(); ++li) {
    sls_ctx::Slot& sl = ctx->slots[dev_slot];
    const bool low = (int64_t)pl->launches[li].grid * 16 <= ncu;
    if (pl->streams_borrowed) {
      std::vector<hipStream_t>& pool = low ? sl.streams_lo : sl.streams;
      const size_t idx = low ? n_lo++ : li;
      while (pool.size() <= idx) {
        hipStream_t st = nullptr;
        if (create_aux_stream(&st, low) != hipSuccess) return bail(fail(ctx, SLS_EHIP, "aux stream creation failed"));
        pool.push_back(st);
      }
      pl->launches[li].stream = pool[idx];
    } else if (create_aux_stream(&pl->launches[li].stream, low) != hipSuccess) {
      return bail(fail(ctx, SLS_EHIP, "aux stream creation failed"));
    }
    if (hipEventCreateWithFlags(&pl->launches[li].done, hipEventDisableTiming) != hipSuccess)
      return bail(fail(ctx, SLS_EHIP, "aux event creation failed"));
  }
  if (pl->launches.size() > 1 && hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming) != hipSuccess)
    return bail(fail(ctx, SLS_EHIP, "fork event creation failed"));
  pl->status_init.assign((size_t)std::max(kp.nsub, 1), SLS_COL_OK);
  for (int32_t q : pl->too_large_subs) pl->status_init[(size_t)S.subs[q].out_index] = SLS_COL_UNSUPPORTED;
  if ((rc = upload(pl, pl->status_init, const_cast<const int32_t**>(&kp.status)))) return bail(rc);   // the kernels overwrite the words of what they solve
  if ((rc = dalloc(pl, (size_t)std::max(kp.nsub, 1), &kp.resid))) return bail(rc);
  if ((rc = dalloc(pl, (size_t)std::max(kp.nsub, 1), &kp.iters))) return bail(rc);
  if ((rc = dalloc(pl, (size_t)std::max<size_t>(pl->launches.size(), 1), &pl->d_counters))) return bail(rc);   // tile kernel work queues
  {
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
    if ((rc = upload(pl, S.obj_pool, &pl->d_obj)) || (rc = upload(pl, pl->obj_gen, &pl->d_gen))) return bail(rc);
    if ((rc = dalloc(pl, (size_t)std::max(kp.nsub, 1) + 1, &pl->d_colobj))) return bail(rc);
  }
  if (const char* lv = sls_knob("SLS_PHASE_TIMERS")) {
    if ((rc = dalloc(pl, (size_t)std::max(kp.nsub, 1) * 8, &kp.dbg))) return bail(rc);
    kp.dbg_level = std::max(1, std::atoi(lv));
  }
  if (const char* ko = sls_knob("SLS_KNOCK_OUT")) kp.knock_out = std::atoi(ko);
  {
    // operator update: every plan can take new values of A / B2 (the device-resident route's operator comes through here too)
    build_operator_value_map(S, pl->opmap);
    const size_t nop = pl->opmap.row_pos.size();
    if ((rc = upload(pl, pl->opmap.row_pos, &pl->d_upd_pos)) || (rc = upload(pl, pl->opmap.zero, &pl->d_upd_zero))) return bail(rc);
    if ((rc = dalloc(pl, std::max<size_t>(nop, 1), &pl->d_upd_stage)) || (rc = dalloc(pl, 1, &pl->d_upd_rejected))) return bail(rc);
  }
  if (S.wu.updatable) {
    // weights update (SLS_PLAN_WEIGHTS_UPDATABLE): what sls_plan_update_weights reads and writes besides w_pool, all from the arena
    const size_t nv = (size_t)(S.Nx + S.Nu);
    if ((rc = upload(pl, S.wu.b2, &pl->d_w_b2)) || (rc = upload(pl, S.wu.owner, &pl->d_w_owner)) ||
        (rc = upload(pl, S.wu.diag, const_cast<const double**>(&pl->d_w_diag)))) return bail(rc);
    if (!S.wu.ridge.empty() && (rc = upload(pl, S.wu.ridge, &pl->d_w_ridge))) return bail(rc);
    if ((rc = dalloc(pl, nv, &pl->d_w_stage)) || (rc = dalloc(pl, 1, &pl->d_w_rejected))) return bail(rc);
  }
  for (auto& L : pl->launches)
    if (L.kind == LaunchKind::Twisted && L.four) {
      L.t4_off = pl->t4_records; pl->t4_records += L.nsub;
      L.t4s_stride = twisted4_static_doubles(L.cls, kp.T);
      L.t4s_off = pl->t4s_doubles; pl->t4s_doubles += L.t4s_stride * L.nsub;
      L.t4i_stride = twisted4_image_doubles(L.cls, kp.T);
      L.t4i_off = pl->t4i_doubles; pl->t4i_doubles += L.t4i_stride * L.nsub;
    }
  if (pl->t4_records) {
    pl->t4_stride = twisted4_record_bytes(kp.w_nzA, kp.w_nzAc, kp.w_nzB, kp.w_nzBc, kp.T);
    if ((rc = dalloc(pl, (size_t)(pl->t4_records * pl->t4_stride), &pl->d_t4))) return bail(rc);
    // A four-wave launch has at most one column per compute unit, a column (T + 1) slots of 3 or 5 KiB: the README chain takes
    // 5.3 MiB, 256 columns at T = 29 take 23 MiB.  Beyond the budget (256 columns: horizons past 84 in the three-tile classes,
    // past 50 in the four-tile ones) the plan keeps no pool and its launches use the rebuild instantiation.  The setup images
    // (15 KiB a column on the README chain: 0.9 MiB) belong to the same decision and the same budget.
    const char* pre = sls_knob("SLS_T4_PRESTATIC");
    if (!(pre && pre[0] == '0') && (pl->t4s_doubles + pl->t4i_doubles) * (int64_t)sizeof(double) <= kT4StaticBudget)
      if ((rc = dalloc(pl, (size_t)pl->t4s_doubles, &pl->d_t4s)) || (rc = dalloc(pl, (size_t)pl->t4i_doubles, &pl->d_t4i))) return bail(rc);
  }
  tick("launch list + requests");
  if ((rc = arena_commit(pl))) return bail(rc);
  tick("arena commit (malloc+H2D)");
  if (S.compact) {
    e = launch_expand_tables(kp.subs, kp.nsub, kp.T, d_cmask, d_cbase, d_coff, const_cast<uint8_t*>(kp.mask_pool),
                             const_cast<int32_t*>(pl->d_dest), pl->stream);
    if (e != hipSuccess) return bail(hipfail(ctx, e, "launch expand_tables_kernel"));
  }
  // four-wave launches: the per-column records, behind the tables they read (same stream)
  e = launch_twisted4_prepares(pl, pl->stream);
  if (e != hipSuccess) return bail(hipfail(ctx, e, "launch twisted4_prepare_kernel"));
  // the plan's own set-up work (status clear, table expansion) ran on the plan's stream: wait for that stream only — a
  // device-wide wait here would also wait for whatever the caller has in flight on other streams (an RCCL collective, another plan)
  e = hipStreamSynchronize(pl->stream);
  if (e != hipSuccess) return bail(hipfail(ctx, e, "hipStreamSynchronize (plan set-up)"));
  const double t2 = now_s();
  tick("set-up stream synchronize");

  sls_plan_info& I = pl->info;
  I.n_subproblems = kp.nsub; I.n_values = S.n_values;
  I.n_values_x = S.off_x[S.T]; I.n_values_u = S.n_values - S.off_x[S.T];
  I.n_packed = S.n_packed; I.max_nx = S.max_n; I.max_nu = S.max_m; I.T = (int32_t)S.T; I.device = pl->dev;
  I.flops_alg = S.flops_alg; I.bytes_alg = S.bytes_alg; I.t_symbolic_s = t1 - t0; I.t_upload_s = t2 - t1;
  // the big host pools are no longer needed
  pool_vec<uint8_t>().swap(S.mask_pool);
  pool_vec<int32_t>().swap(S.dest_pool);
  pool_vec<int32_t>().swap(S.pdest_pool);
  pool_vec<int32_t>().swap(S.idx_pool);
  pool_vec<uint64_t>().swap(S.cmask); pool_vec<int32_t>().swap(S.cbase); pool_vec<int64_t>().swap(S.coff);
  *plan_out = pl;
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

extern "C++" int sls::enqueue_launches(sls_plan* plan, const KernelParams& kp, hipStream_t st, const SelectedRun* sel) {
  const bool multi = plan->launches.size() > 1;
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
      e = tile ? launch_tile(q, grid, L.lds, ls, L.mlds, L.two_per_cu, L.gw, L.big) : launch_general(q, grid, L.lds, ls, L.wide);
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
      e = (L.kind == LaunchKind::Twisted) ? (L.four ? launch_twisted4(L.cls, q, grid, L.lds, ls) : launch_twisted(L.cls, q, grid, L.lds, ls))
                        : launch_wave(L.cls, q, grid, L.lds, ls);
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
  auto al = [](size_t b) { return (std::max<size_t>(b, 16) + 255) / 256 * 256; };
  const size_t o_col = 0, o_ptr = o_col + al(4 * ns), o_rows = o_ptr + al(8 * (ns + 1)), o_out = o_rows + al(4 * hr.size()),
               total = o_out + al(8 * (3 * ns + 2));
  unsigned char* base = nullptr;
  HIPCHK(plan->ctx, hipMalloc(reinterpret_cast<void**>(&base), total));
  plan->dev_allocs.push_back(base);
  HIPCHK(plan->ctx, hipMemcpy(base + o_col, S.sub_col.data(), 4 * ns, hipMemcpyHostToDevice));
  HIPCHK(plan->ctx, hipMemcpy(base + o_ptr, hp.data(), 8 * (ns + 1), hipMemcpyHostToDevice));
  if (!hr.empty()) HIPCHK(plan->ctx, hipMemcpy(base + o_rows, hr.data(), 4 * hr.size(), hipMemcpyHostToDevice));
  rs.sub_col = reinterpret_cast<const int32_t*>(base + o_col);
  rs.halo_ptr = reinterpret_cast<const int64_t*>(base + o_ptr);
  rs.halo_rows = reinterpret_cast<const int32_t*>(base + o_rows);
  rs.out = reinterpret_cast<double*>(base + o_out);
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

// Refinement (which columns and why: select_refinement_groups, sls_dropin_host.h; contract: sls_plan.h)
extern "C++" int sls::attach_refinement(sls_plan* pl, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                                        const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                                        hipStream_t stream, double* d_values, int64_t* n_refined, std::vector<int32_t>& stt,
                                        std::vector<double>& res, std::vector<int32_t>& its, int packed) {
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

int sls_plan_refine(sls_plan* plan, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                    int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, void* hip_stream, double* d_values,
                    int packed, int64_t* n_refined) {
  if (!plan) return fail(nullptr, SLS_EINVAL, "null plan");
  if (!dims || !P || !Sx || !Su || !d_values) return fail(plan->ctx, SLS_EINVAL, "null argument");
  if (dims->flags & SLS_SOLVE_SUM_OF_NORMS) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_refine: 𝓗₂ objective only");
  if (plan->kp.objective != 0) return fail(plan->ctx, SLS_EUNSUPPORTED, "sls_plan_refine: 𝓗₂ objective only");
  if (ngroups != plan->ngroups_in) return fail(plan->ctx, SLS_EINVAL, "sls_plan_refine: the group list does not match the one this plan was built from");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  int64_t nr = 0;
  std::vector<int32_t> stt, its; std::vector<double> res;
  int rc = attach_refinement(plan, dims, P, Sx, Su, ngroups, group_ptr, group_cols, reinterpret_cast<hipStream_t>(hip_stream), d_values, &nr,
                             stt, res, its, packed);
  if (n_refined) *n_refined = nr;
  return rc;
}

}  // extern "C"
