// sls_rollout.hip — streaming closed-loop rollout of a resident Φ against an ensemble of plants: sls_rollout_* of
// include/sls_mi355x.h.
//
// Semantics, memory, the ring check, the owners of the accumulators and the traffic model: sls_rollout.h.  One step is ONE kernel
// launch: one wave per state row and scenario chunk plus one wave per orphan actuator, closed_loop_step_kernel
// (sls_closed_loop.hip) restated — lanes = (entry slot le, scenario slot ls), lane = le·SCN + ls, four entries in flight per lane,
// (a0 + a1) + (a2 + a3), then the xor-shuffle sum over the entry slots; the plant row and the fma chain over B₂ in the
// simulator's order — so that with the design plant x and u are bit for bit what the simulator computes.  The two differences:
// plant values are read at [e][scen] (contiguous along the scenario lanes), and ŵ comes from the controller's mirrored ring, with
// x_k − β_k for the entries of lag 1.
//
// The step counter lives on the host and advances at enqueue; the ring slot and the buffer parity are launch arguments, which is
// why a run refuses a capturing stream.  The arena, load and set_plant are the shared ones of sls_object.h.  load, reset, run,
// stats and the device paths of set_plant / set_weights allocate nothing and never wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "../../include/sls_mi355x_debug.h"
#include "sls_internal.h"
#include "sls_object.h"
#include "sls_rollout.h"
#include "sls_symbolic.h"
#include "sls_wave_util.h"

namespace {

using sls::RolloutParams;

constexpr int kWavesPerBlock = 4;

// one scenario per thread, rows ascending (sls_rollout.h: STATS)
__global__ void rollout_stats_kernel(const double* __restrict__ acc_cost, const double* __restrict__ acc_peak, int Nx, int Nu, long long ns,
                                     double* __restrict__ cost, double* __restrict__ peak_x, double* __restrict__ peak_u) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  double c = 0.0, px = 0.0, pu = 0.0;
  for (int r = 0; r < Nx; ++r) {
    c = c + acc_cost[(long long)r * ns + s];
    px = fmax(px, acc_peak[(long long)r * ns + s]);
  }
  for (int r = Nx; r < Nx + Nu; ++r) {
    c = c + acc_cost[(long long)r * ns + s];
    pu = fmax(pu, acc_peak[(long long)r * ns + s]);
  }
  if (cost) cost[s] = c;
  if (peak_x) peak_x[s] = px;
  if (peak_u) peak_u[s] = pu;
}

// s: ring slot of this step, par: which copies hold x_k and β_k.  w [Nw][nscen] or NULL; x_rec [Nx][nscen] / u_rec [Nu][nscen]
// or NULL: where x_k and u_k of this step are recorded.
template <int SCN>
__global__ void __launch_bounds__(64 * kWavesPerBlock)
rollout_step_kernel(RolloutParams p, int s, int par, const double* __restrict__ w, double* __restrict__ x_rec, double* __restrict__ u_rec) {
  constexpr int NE = 64 / SCN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ls = lane % SCN, le = lane / SCN;
  const int row = blockIdx.x * kWavesPerBlock + wave;
  const long long scen = (long long)blockIdx.y * SCN + ls;
  if (row >= p.Nx + p.n_orphan) return;
  const bool live = scen < p.nscen;
  const long long sc = live ? scen : 0;                       // dead lanes read scenario 0 and never write
  const long long ns = p.nscen;
  const long long Nx = p.Nx;
  const double* hist = p.hist + sls::controller_window_end(s, p.R, Nx) * ns + sc;
  const double* xk = p.x + (long long)par * Nx * ns + sc;
  const double* bk = p.beta + (long long)par * Nx * ns + sc;
  // ŵ_{k+1−τ}[c] for hoff = τ·Nx − c: lag 1 (hoff ≤ Nx) is x_k[c] − β_k[c], not in the ring yet; older lags from the window
  auto rd = [&](long long h) { return h <= Nx ? xk[(Nx - h) * ns] - bk[(Nx - h) * ns] : hist[-h * ns]; };
  auto fir = [&](int beg, int end) {                           // this lane's share of Σ_e vals[e]·ŵ
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;               // four entries in flight per lane: the row is a latency chain otherwise
    int e = beg + le;
    for (; e + 3 * NE < end; e += 4 * NE) {
      const double v0 = p.vals[e], v1 = p.vals[e + NE], v2 = p.vals[e + 2 * NE], v3 = p.vals[e + 3 * NE];
      const long long h0 = p.hoff[e], h1 = p.hoff[e + NE], h2 = p.hoff[e + 2 * NE], h3 = p.hoff[e + 3 * NE];
      if (h0 > Nx) {                                             // a row ascends in the lag: all four are older than lag 1 —
        a0 = fma(v0, hist[-h0 * ns], a0);                        // the simulator's loop body, four independent loads
        a1 = fma(v1, hist[-h1 * ns], a1);
        a2 = fma(v2, hist[-h2 * ns], a2);
        a3 = fma(v3, hist[-h3 * ns], a3);
      } else {                                                   // the lag-1 prefix of the row (and the group that straddles its end)
        a0 = fma(v0, rd(h0), a0);
        a1 = fma(v1, rd(h1), a1);
        a2 = fma(v2, rd(h2), a2);
        a3 = fma(v3, rd(h3), a3);
      }
    }
    for (; e < end; e += NE) a0 = fma(p.vals[e], rd(p.hoff[e]), a0);
    return (a0 + a1) + (a2 + a3);
  };
  // the owner of accumulator row `arow` counts v (called by the lanes le == 0 && live only)
  // The owner of accumulator row `arow` counts v.  What it needs — the weight and the two accumulator values — is loaded by
  // `fetch` BEFORE the row sums it belongs to, so that the round trip overlaps with them; `count` then only computes and stores.
  struct Acc { double wgt, cost, peak; };
  const bool writer = le == 0 && live;
  auto fetch = [&](bool mine, long long arow, const double* wgt) {
    Acc a{0.0, 0.0, 0.0};
    if (mine) { a.wgt = *wgt; a.cost = p.acc_cost[arow * ns + scen]; a.peak = p.acc_peak[arow * ns + scen]; }
    return a;
  };
  auto count = [&](const Acc& a, long long arow, double v) {
    const double t = a.wgt * v;
    p.acc_cost[arow * ns + scen] = fma(t, t, a.cost);
    p.acc_peak[arow * ns + scen] = fmax(a.peak, fabs(v));
  };
  if (row >= p.Nx) {                                           // actuator that drives no state: u only, counted here
    const int j = p.orphan[row - p.Nx];
    const Acc au = fetch(writer, Nx + j, p.r + j);
    const double uj = sls::lane_group_sum<SCN>(fir(p.u_ptr[j], p.u_ptr[j + 1]));
    if (writer) {
      if (u_rec) u_rec[(long long)j * ns + scen] = uj;
      count(au, Nx + j, uj);
    }
    return;
  }
  const int i = row;
  const long long at = (long long)i * ns + scen;
  const long long nxt = (long long)(par ^ 1) * Nx * ns + at, cur = (long long)par * Nx * ns + at;
  const Acc ax = fetch(writer, i, p.q + i);
  double xv = 0.0, bv = 0.0;                                   // x_k[i], β_k[i] of the lane that stores ŵ_k[i]
  if (writer) { xv = p.x[cur]; bv = p.beta[cur]; }
  const double beta = sls::lane_group_sum<SCN>(fir(p.beta_ptr[i], p.beta_ptr[i + 1]));
  double part = 0.0;                                           // A⁽ˢ⁾·x_k + B1·w_k, this lane's share
  for (int e = p.A_ptr[i] + le; e < p.A_ptr[i + 1]; e += NE) part = fma(p.A_val[(long long)e * ns + sc], xk[(long long)p.A_idx[e] * ns], part);
  if (w) {
    const double* __restrict__ wk = w + sc;
    for (int e = p.B1_ptr[i] + le; e < p.B1_ptr[i + 1]; e += NE) part = fma(p.B1_val[e], wk[(long long)p.B1_idx[e] * ns], part);
  }
  double xi = sls::lane_group_sum<SCN>(part);
  for (int e = p.B2_ptr[i]; e < p.B2_ptr[i + 1]; ++e) {
    const int j = p.B2_idx[e];
    const bool mine = writer && p.B2_own[e];
    const Acc au = fetch(mine, Nx + j, p.r + j);
    const double uj = sls::lane_group_sum<SCN>(fir(p.u_ptr[j], p.u_ptr[j + 1]));
    xi = fma(p.B2_val[(long long)e * ns + sc], uj, xi);
    if (writer && u_rec) u_rec[(long long)j * ns + scen] = uj;
    if (mine) count(au, Nx + j, uj);
  }
  if (!writer) return;
  const double wv = xv - bv;                                   // ŵ_k[i] into both copies of slot s
  p.x[nxt] = xi;
  p.beta[nxt] = beta;
  p.hist[(long long)s * Nx * ns + at] = wv;
  p.hist[(long long)(s + p.R) * Nx * ns + at] = wv;
  if (x_rec) x_rec[at] = xv;
  count(ax, i, xv);
}

template <int SCN>
hipError_t launch_step(const RolloutParams& p, int s, int par, const double* w, double* x_rec, double* u_rec, hipStream_t st) {
  const int rows = p.Nx + p.n_orphan;
  dim3 grid((rows + kWavesPerBlock - 1) / kWavesPerBlock, (unsigned)((p.nscen + SCN - 1) / SCN));
  hipLaunchKernelGGL(rollout_step_kernel<SCN>, grid, dim3(64 * kWavesPerBlock), 0, st, p, s, par, w, x_rec, u_rec);
  return hipGetLastError();
}

hipError_t launch_rollout_step(int scn, const RolloutParams& p, int s, int par, const double* w, double* x_rec, double* u_rec,
                               hipStream_t st) {
  switch (scn) {
    case 1: return launch_step<1>(p, s, par, w, x_rec, u_rec, st);
    case 2: return launch_step<2>(p, s, par, w, x_rec, u_rec, st);
    case 4: return launch_step<4>(p, s, par, w, x_rec, u_rec, st);
    case 8: return launch_step<8>(p, s, par, w, x_rec, u_rec, st);
    case 16: return launch_step<16>(p, s, par, w, x_rec, u_rec, st);
    case 32: return launch_step<32>(p, s, par, w, x_rec, u_rec, st);
    default: return launch_step<64>(p, s, par, w, x_rec, u_rec, st);
  }
}

}  // namespace

struct sls_rollout {
  sls_ctx* ctx = nullptr;
  int dev = 0;
  int64_t n_entries = 0;
  void* arena = nullptr;               // tables, Φ in row order, weights, plant values, staging, results, state
  const int32_t* d_perm = nullptr;
  double *d_vals = nullptr, *d_q = nullptr, *d_r = nullptr;
  sls::PlantEnsemble plant;
  double* d_result = nullptr;          // [3][nscen]: cost, peak_x, peak_u of sls_rollout_fetch
  RolloutParams kp{};
  int scn = 1;                         // scenario slots per wave: smallest power of two ≥ nscen, at most 64
  size_t state_off = 0, state_bytes = 0, plant_bytes = 0;   // the state is one contiguous range: what reset clears
  int64_t k = 0;                       // steps enqueued since the last reset
  bool loaded = false;
};

using namespace sls;

namespace {

int enqueue_stats(sls_rollout* L, hipStream_t st, double* d_cost, double* d_peak_x, double* d_peak_u) {
  if (!d_cost && !d_peak_x && !d_peak_u) return 0;
  const int bs = 64;
  hipLaunchKernelGGL(rollout_stats_kernel, dim3((unsigned)((L->kp.nscen + bs - 1) / bs)), dim3(bs), 0, st, L->kp.acc_cost, L->kp.acc_peak,
                     L->kp.Nx, L->kp.Nu, L->kp.nscen, d_cost, d_peak_x, d_peak_u);
  HIPCHK(L->ctx, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int sls_rollout_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                     int64_t nscen, sls_rollout** out) {
  int rc = check_plan_args(ctx, "sls_rollout_plan", out, dims && P && Sx && Su, dev_slot, nscen);
  if (rc) return rc;
  RolloutTables Tb;
  std::string msg;
  rc = build_rollout_tables(dims, P, Sx, Su, Tb, msg);
  if (rc) return fail(ctx, rc, "sls_rollout_plan: " + msg);
  FirOperator& F = Tb.F;
  if (F.Nx + F.Nu > 0x7ffffff0LL) return fail(ctx, SLS_EUNSUPPORTED, "sls_rollout_plan: Nx + Nu exceeds int32");
  if ((rc = PlantEnsemble::check_size(ctx, "sls_rollout_plan", F.A.val.size(), F.B2.val.size(), nscen))) return rc;
  sls_rollout* L = new (std::nothrow) sls_rollout();
  if (!L) return fail(ctx, SLS_ENOMEM, "sls_rollout_plan: out of memory");
  L->ctx = ctx; L->dev = ctx->devs[dev_slot];
  L->n_entries = (int64_t)F.hoff.size();
  hipError_t e = hipSetDevice(L->dev);
  if (e != hipSuccess) { delete L; return hipfail(ctx, e, "hipSetDevice"); }
  // one arena: uploaded tables first, then the buffers the object owns
  Arena ar;
  RolloutParams& kp = L->kp;
  ar.table(F.beta_ptr, &kp.beta_ptr); ar.table(F.u_ptr, &kp.u_ptr); ar.table(F.hoff, &kp.hoff); ar.table(F.perm, &L->d_perm);
  ar.table(F.A.ptr, &kp.A_ptr); ar.table(F.A.idx, &kp.A_idx); ar.table(F.B1.ptr, &kp.B1_ptr); ar.table(F.B1.idx, &kp.B1_idx);
  ar.table(F.B1.val, &kp.B1_val); ar.table(F.B2.ptr, &kp.B2_ptr); ar.table(F.B2.idx, &kp.B2_idx); ar.table(F.orphan, &kp.orphan);
  L->plant.lay_out_tables(ar, Tb.A_src, Tb.B2_src);
  ar.table(Tb.b2_owner, &kp.B2_own);
  const std::vector<double> ones((size_t)(F.Nx + F.Nu), 1.0);
  ar.table(ones, &kp.q);                                       // q then r
  ar.buffer((size_t)L->n_entries, &L->d_vals);
  L->plant_bytes = L->plant.lay_out_values(ar, nscen);
  ar.buffer((size_t)(3 * nscen), &L->d_result);
  L->state_off = ar.bytes();
  ar.buffer((size_t)controller_hist_doubles(F.Nx, F.T, nscen), &kp.hist);
  ar.buffer((size_t)controller_beta_doubles(F.Nx, nscen), &kp.beta);
  ar.buffer((size_t)(2 * F.Nx * nscen), &kp.x);
  ar.buffer((size_t)((F.Nx + F.Nu) * nscen), &kp.acc_cost);
  ar.buffer((size_t)((F.Nx + F.Nu) * nscen), &kp.acc_peak);
  L->state_bytes = ar.bytes() - L->state_off;
  rc = ar.commit(ctx, &L->arena, "hipMalloc (rollout)", "hipMemcpy H2D (rollout tables)");
  if (rc) { delete L; return rc; }
  L->d_q = const_cast<double*>(kp.q); L->d_r = L->d_q + F.Nx;
  kp.r = L->d_r;
  kp.vals = L->d_vals; kp.A_val = L->plant.d_A_val; kp.B2_val = L->plant.d_B2_val;
  kp.Nx = (int32_t)F.Nx; kp.Nu = (int32_t)F.Nu; kp.Nw = (int32_t)F.Nw; kp.T = (int32_t)F.T; kp.R = (int32_t)controller_ring_slots(F.T);
  kp.n_orphan = (int32_t)F.orphan.size();
  kp.nscen = nscen;
  L->scn = scenario_slots(nscen);
  rc = L->plant.init_from(ctx, P, "sls_rollout_plan: upload");
  if (!rc) {
    e = hipMemset(static_cast<unsigned char*>(L->arena) + L->state_off, 0, L->state_bytes);   // the state after a reset
    if (e == hipSuccess) e = hipDeviceSynchronize();           // plan time may wait; the calls below do not
    if (e != hipSuccess) rc = hipfail(ctx, e, "sls_rollout_plan: upload");
  }
  if (rc) { (void)hipFree(L->arena); delete L; return rc; }
  *out = L;
  return 0;
}

int sls_rollout_load(sls_rollout* L, void* hip_stream, const double* d_values) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_load: null rollout");
  if (!d_values && L->n_entries > 0) return fail(L->ctx, SLS_EINVAL, "sls_rollout_load: null device pointer");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  // Φ: mask order → row order
  if (int rc = launch_gather_phi(L->ctx, d_values, L->d_perm, L->n_entries, L->d_vals, static_cast<hipStream_t>(hip_stream))) return rc;
  L->loaded = true;
  return 0;
}

int sls_rollout_set_plant(sls_rollout* L, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device, int per_scenario) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_set_plant: null rollout");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  return L->plant.set(L->ctx, static_cast<hipStream_t>(hip_stream), A_nzval, B2_nzval, on_device, per_scenario);
}

int sls_rollout_set_weights(sls_rollout* L, void* hip_stream, const double* q, const double* rr, int on_device) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_set_weights: null rollout");
  sls_ctx* ctx = L->ctx;
  HIPCHK(ctx, hipSetDevice(L->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (q) HIPCHK(ctx, hipMemcpyAsync(L->d_q, q, (size_t)L->kp.Nx * sizeof(double), kind, st));
  if (rr && L->kp.Nu > 0) HIPCHK(ctx, hipMemcpyAsync(L->d_r, rr, (size_t)L->kp.Nu * sizeof(double), kind, st));
  if (!on_device && (q || rr)) HIPCHK(ctx, hipStreamSynchronize(st));   // the caller's arrays are free on return
  return 0;
}

int sls_rollout_reset(sls_rollout* L, void* hip_stream, const double* d_x0) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_reset: null rollout");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  HIPCHK(L->ctx, hipMemsetAsync(static_cast<unsigned char*>(L->arena) + L->state_off, 0, L->state_bytes, st));
  if (d_x0) HIPCHK(L->ctx, hipMemcpyAsync(L->kp.x, d_x0, (size_t)L->kp.Nx * L->kp.nscen * sizeof(double), hipMemcpyDeviceToDevice, st));
  L->k = 0;
  return 0;
}

int sls_rollout_run(sls_rollout* L, void* hip_stream, const double* d_w, int64_t steps, double* d_x, double* d_u) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_run: null rollout");
  sls_ctx* ctx = L->ctx;
  if (steps < 0) return fail(ctx, SLS_EINVAL, "sls_rollout_run: steps must be >= 0");
  if (!L->loaded) return fail(ctx, SLS_EINVAL, "sls_rollout_run: no Φ loaded (sls_rollout_load first)");
  HIPCHK(ctx, hipSetDevice(L->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (st) {                                                    // the null stream cannot be captured
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(ctx, hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return fail(ctx, SLS_EUNSUPPORTED, "sls_rollout_run: the stream is being captured (ring slot and buffer parity are launch arguments)");
  }
  const RolloutParams& p = L->kp;
  const size_t sx = (size_t)p.Nx * p.nscen, su = (size_t)p.Nu * p.nscen, sw = (size_t)p.Nw * p.nscen;
  for (int64_t n = 0; n < steps; ++n) {
    const int s = (int)controller_slot(L->k, p.R), par = (int)(L->k & 1);
    HIPCHK(ctx, launch_rollout_step(L->scn, p, s, par, d_w ? d_w + n * sw : nullptr, d_x ? d_x + n * sx : nullptr,
                                    d_u && p.Nu > 0 ? d_u + n * su : nullptr, st));
    ++L->k;
  }
  return 0;
}

int sls_rollout_stats(sls_rollout* L, void* hip_stream, double* d_cost, double* d_peak_x, double* d_peak_u) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_stats: null rollout");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  return enqueue_stats(L, static_cast<hipStream_t>(hip_stream), d_cost, d_peak_x, d_peak_u);
}

int sls_rollout_fetch(sls_rollout* L, void* hip_stream, double* x_now, double* cost, double* peak_x, double* peak_u) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_fetch: null rollout");
  sls_ctx* ctx = L->ctx;
  HIPCHK(ctx, hipSetDevice(L->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const long long ns = L->kp.nscen;
  double* res = L->d_result;
  int rc = enqueue_stats(L, st, cost ? res : nullptr, peak_x ? res + ns : nullptr, peak_u ? res + 2 * ns : nullptr);
  if (rc) return rc;
  const size_t b = (size_t)ns * sizeof(double);
  if (cost) HIPCHK(ctx, hipMemcpyAsync(cost, res, b, hipMemcpyDeviceToHost, st));
  if (peak_x) HIPCHK(ctx, hipMemcpyAsync(peak_x, res + ns, b, hipMemcpyDeviceToHost, st));
  if (peak_u) HIPCHK(ctx, hipMemcpyAsync(peak_u, res + 2 * ns, b, hipMemcpyDeviceToHost, st));
  if (x_now) HIPCHK(ctx, hipMemcpyAsync(x_now, L->kp.x + (size_t)(L->k & 1) * L->kp.Nx * ns, (size_t)L->kp.Nx * b, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

int sls_rollout_info(const sls_rollout* L, int64_t* n_entries, int64_t* steps_done, int64_t* state_bytes, int64_t* plant_bytes) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_rollout_info: null rollout");
  if (n_entries) *n_entries = L->n_entries;
  if (steps_done) *steps_done = L->k;
  if (state_bytes) *state_bytes = (int64_t)L->state_bytes;
  if (plant_bytes) *plant_bytes = (int64_t)L->plant_bytes;
  return 0;
}

void sls_rollout_destroy(sls_rollout* L) {
  if (!L) return;
  (void)hipSetDevice(L->dev);
  if (L->arena) (void)hipFree(L->arena);
  delete L;
}

/* diagnostics (include/sls_mi355x_debug.h): the rollout's plan-time tables.  Needs no device. */
int sls_debug_rollout_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries,
                             int64_t* n_orphan, int32_t* A_ptr, int32_t* A_idx, int32_t* A_src, int32_t* B2_ptr, int32_t* B2_idx,
                             int32_t* B2_src, uint8_t* B2_owner, int32_t* orphan) {
  RolloutTables Tb;
  std::string msg;
  int rc = build_rollout_tables(dims, P, Sx, Su, Tb, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_rollout_tables: " + msg);
  const FirOperator& F = Tb.F;
  if (n_entries) *n_entries = (int64_t)F.hoff.size();
  if (n_orphan) *n_orphan = (int64_t)F.orphan.size();
  if (A_ptr) std::copy(F.A.ptr.begin(), F.A.ptr.end(), A_ptr);
  if (A_idx) std::copy(F.A.idx.begin(), F.A.idx.end(), A_idx);
  if (A_src) std::copy(Tb.A_src.begin(), Tb.A_src.end(), A_src);
  if (B2_ptr) std::copy(F.B2.ptr.begin(), F.B2.ptr.end(), B2_ptr);
  if (B2_idx) std::copy(F.B2.idx.begin(), F.B2.idx.end(), B2_idx);
  if (B2_src) std::copy(Tb.B2_src.begin(), Tb.B2_src.end(), B2_src);
  if (B2_owner) std::copy(Tb.b2_owner.begin(), Tb.b2_owner.end(), B2_owner);
  if (orphan) std::copy(F.orphan.begin(), F.orphan.end(), orphan);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of a whole rollout (csrc/sls_rollout.cpp).  Needs no device. */
int sls_debug_rollout_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                           int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario, const double* q,
                           const double* rr, const double* x0, const double* w, int64_t steps, const int64_t* chunks, int64_t nchunks,
                           const double* values2, int64_t switch_step, double* x, double* u, double* x_end, double* cost,
                           double* peak_x, double* peak_u) {
  RolloutTables Tb;
  std::string msg;
  int rc = build_rollout_tables(dims, P, Sx, Su, Tb, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_rollout_host: " + msg);
  if (steps < 0 || nchunks < 0 || (nchunks > 0 && !chunks)) return fail(nullptr, SLS_EINVAL, "sls_debug_rollout_host: bad steps or chunks");
  if (!values && !Tb.F.hoff.empty()) return fail(nullptr, SLS_EINVAL, "sls_debug_rollout_host: null values");
  RolloutHost H;
  rc = H.init(Tb, nscen, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_rollout_host: " + msg);
  H.load(values);
  H.set_plant(A_nzval, B2_nzval, per_scenario != 0);
  H.set_weights(q, rr);
  H.reset(x0);
  // the chunk boundaries: the caller's, plus the step at which values2 is loaded
  std::vector<int64_t> cuts;
  int64_t sum = 0;
  for (int64_t c = 0; c < nchunks; ++c) {
    if (chunks[c] < 0) return fail(nullptr, SLS_EINVAL, "sls_debug_rollout_host: negative chunk");
    sum += chunks[c];
    cuts.push_back(sum);
  }
  if (nchunks > 0 && sum != steps) return fail(nullptr, SLS_EINVAL, "sls_debug_rollout_host: chunks must add up to steps");
  if (nchunks == 0) cuts.push_back(steps);
  const int64_t Nx = Tb.F.Nx, Nu = Tb.F.Nu, Nw = Tb.F.Nw;
  int64_t done = 0;
  auto advance = [&](int64_t to) {
    if (to <= done) return 0;
    int r2 = H.run(w ? w + done * Nw * nscen : nullptr, to - done, x ? x + done * Nx * nscen : nullptr, u ? u + done * Nu * nscen : nullptr, msg);
    done = to;
    return r2;
  };
  for (int64_t cut : cuts) {
    if (values2 && switch_step >= done && switch_step < cut) {
      if ((rc = advance(switch_step))) break;
      H.load(values2);
      values2 = nullptr;
    }
    if ((rc = advance(cut))) break;
  }
  if (rc) return fail(nullptr, rc, "sls_debug_rollout_host: " + msg);
  if (x_end) std::copy(H.state(), H.state() + Nx * nscen, x_end);
  H.stats(cost, peak_x, peak_u);
  return 0;
}

}  // extern "C"
