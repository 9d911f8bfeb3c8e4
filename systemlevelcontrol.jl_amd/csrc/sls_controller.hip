// sls_controller.hip — the stand-alone SLS controller on the device: sls_controller_* of include/sls_mi355x.h.
//
// Semantics, the mirrored history ring and the β double buffer: sls_controller.h.  One step is ONE kernel launch: one wave per
// operator row and scenario chunk — the Nx β rows (row i also stores ŵ_k[i], twice in the ring and once for the caller) and
// the Nu u rows, each by its own wave; no plant and no B₂ are involved, so no row depends on another inside a step.  A row is
// evaluated by the simulator's `fir` routine (closed_loop_step_kernel, sls_closed_loop.hip) restated: the same entries on the
// same lanes in the same order — lanes = (entry slot le, scenario slot ls), lane = le·SCN + ls, four entries in flight per lane,
// (a0 + a1) + (a2 + a3), then the xor-shuffle sum over the entry slots — so that u is bit for bit what the simulator computes
// from the same x.  The only difference is where ŵ comes from: the ring window instead of an all-times array, and x_k − β_k for
// the entries of lag 1.  A step reads 12 B per stored Φ entry (value + hoff); x, β and ŵ stay in L2.
//
// The step counter lives on the host and advances at enqueue; the ring slot and the β parity are launch arguments, which is
// why a step refuses a capturing stream (a graph would freeze them).  load, reset and step allocate nothing and never wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "../../include/sls_mi355x_debug.h"
#include "sls_controller.h"
#include "sls_internal.h"
#include "sls_object.h"
#include "sls_symbolic.h"
#include "sls_wave_util.h"

namespace {

using sls::ControllerParams;

constexpr int kWavesPerBlock = 4;

// s: ring slot of this step, par: which β copy holds β_k.  x [Nx][nscen], u [Nu][nscen], what_out [Nx][nscen] or NULL.
template <int SCN>
__global__ void __launch_bounds__(64 * kWavesPerBlock)
controller_step_kernel(ControllerParams p, int s, int par, const double* __restrict__ x, double* __restrict__ u,
                       double* __restrict__ what_out) {
  constexpr int NE = 64 / SCN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ls = lane % SCN, le = lane / SCN;
  const int row = blockIdx.x * kWavesPerBlock + wave;
  const long long scen = (long long)blockIdx.y * SCN + ls;
  if (row >= p.Nx + p.Nu) return;
  const bool live = scen < p.nscen;
  const long long sc = live ? scen : 0;                       // dead lanes read scenario 0 and never write
  const long long ns = p.nscen;
  const long long Nx = p.Nx;
  const double* hist = p.hist + sls::controller_window_end(s, p.R, Nx) * ns + sc;
  const double* __restrict__ xs = x + sc;
  const double* bk = p.beta + (long long)par * Nx * ns + sc;
  // ŵ_{k+1−τ}[c] for hoff = τ·Nx − c: lag 1 (hoff ≤ Nx) is x_k[c] − β_k[c], not in the ring yet; older lags from the window
  auto rd = [&](long long h) { return h <= Nx ? xs[(Nx - h) * ns] - bk[(Nx - h) * ns] : hist[-h * ns]; };
  const int beg = p.row_ptr[row], end = p.row_ptr[row + 1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;               // four entries in flight per lane: the row is a latency chain otherwise
  int e = beg + le;
  for (; e + 3 * NE < end; e += 4 * NE) {
    const double v0 = p.vals[e], v1 = p.vals[e + NE], v2 = p.vals[e + 2 * NE], v3 = p.vals[e + 3 * NE];
    const long long h0 = p.hoff[e], h1 = p.hoff[e + NE], h2 = p.hoff[e + 2 * NE], h3 = p.hoff[e + 3 * NE];
    a0 = fma(v0, rd(h0), a0);
    a1 = fma(v1, rd(h1), a1);
    a2 = fma(v2, rd(h2), a2);
    a3 = fma(v3, rd(h3), a3);
  }
  for (; e < end; e += NE) a0 = fma(p.vals[e], rd(p.hoff[e]), a0);
  const double sum = sls::lane_group_sum<SCN>((a0 + a1) + (a2 + a3));
  if (le != 0 || !live) return;
  if (row >= p.Nx) {                                           // u row
    u[(long long)(row - p.Nx) * ns + scen] = sum;
    return;
  }
  const long long at = (long long)row * ns + scen;             // β row i: β_{k+1}[i], and ŵ_k[i] into both copies of slot s
  p.beta[(long long)(par ^ 1) * Nx * ns + at] = sum;
  const double w = x[at] - p.beta[(long long)par * Nx * ns + at];
  p.hist[(long long)s * Nx * ns + at] = w;
  p.hist[(long long)(s + p.R) * Nx * ns + at] = w;
  if (what_out) what_out[at] = w;
}

template <int SCN>
hipError_t launch_step(const ControllerParams& p, int s, int par, const double* x, double* u, double* what_out, hipStream_t st) {
  const int rows = p.Nx + p.Nu;
  dim3 grid((rows + kWavesPerBlock - 1) / kWavesPerBlock, (unsigned)((p.nscen + SCN - 1) / SCN));
  hipLaunchKernelGGL(controller_step_kernel<SCN>, grid, dim3(64 * kWavesPerBlock), 0, st, p, s, par, x, u, what_out);
  return hipGetLastError();
}

hipError_t launch_controller_step(int scn, const ControllerParams& p, int s, int par, const double* x, double* u, double* what_out,
                                  hipStream_t st) {
  switch (scn) {
    case 1: return launch_step<1>(p, s, par, x, u, what_out, st);
    case 2: return launch_step<2>(p, s, par, x, u, what_out, st);
    case 4: return launch_step<4>(p, s, par, x, u, what_out, st);
    case 8: return launch_step<8>(p, s, par, x, u, what_out, st);
    case 16: return launch_step<16>(p, s, par, x, u, what_out, st);
    case 32: return launch_step<32>(p, s, par, x, u, what_out, st);
    default: return launch_step<64>(p, s, par, x, u, what_out, st);
  }
}

}  // namespace

struct sls_controller {
  sls_ctx* ctx = nullptr;
  int dev = 0;
  int64_t n_entries = 0;
  void* arena = nullptr;               // row_ptr, hoff, perm, Φ in row order, β (two copies), history ring
  const int32_t* d_perm = nullptr;
  double* d_vals = nullptr;
  ControllerParams kp{};
  int scn = 1;                         // scenario slots per wave: smallest power of two ≥ nscen, at most 64
  size_t state_off = 0, state_bytes = 0;   // β and the history are one contiguous range: what reset clears
  int64_t k = 0;                       // steps enqueued since the last reset
  bool loaded = false;
};

using namespace sls;

extern "C" {

int sls_controller_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                        int64_t nscen, sls_controller** out) {
  int rc = check_plan_args(ctx, "sls_controller_plan", out, dims && Sx && Su, dev_slot, nscen);
  if (rc) return rc;
  FirOperator F;
  std::string msg;
  rc = build_controller_operator(dims, Sx, Su, F, msg);
  if (rc) return fail(ctx, rc, "sls_controller_plan: " + msg);
  if (F.Nx + F.Nu > 0x7ffffff0LL) return fail(ctx, SLS_EUNSUPPORTED, "sls_controller_plan: Nx + Nu exceeds int32");
  sls_controller* L = new (std::nothrow) sls_controller();
  if (!L) return fail(ctx, SLS_ENOMEM, "sls_controller_plan: out of memory");
  L->ctx = ctx; L->dev = ctx->devs[dev_slot];
  L->n_entries = (int64_t)F.hoff.size();
  std::vector<int32_t> row_ptr(F.beta_ptr);                   // β rows, then u rows: u_ptr[0] == beta_ptr[Nx]
  row_ptr.insert(row_ptr.end(), F.u_ptr.begin() + 1, F.u_ptr.end());
  hipError_t e = hipSetDevice(L->dev);
  if (e != hipSuccess) { delete L; return hipfail(ctx, e, "hipSetDevice"); }
  Arena ar;
  ControllerParams& kp = L->kp;
  ar.table(row_ptr, &kp.row_ptr); ar.table(F.hoff, &kp.hoff); ar.table(F.perm, &L->d_perm);
  ar.buffer((size_t)L->n_entries, &L->d_vals);
  L->state_off = ar.bytes();
  ar.buffer((size_t)controller_beta_doubles(F.Nx, nscen), &kp.beta);
  ar.buffer((size_t)controller_hist_doubles(F.Nx, F.T, nscen), &kp.hist);
  L->state_bytes = ar.bytes() - L->state_off;
  rc = ar.commit(ctx, &L->arena, "hipMalloc (controller)", "sls_controller_plan: upload");
  if (rc) { delete L; return rc; }
  kp.vals = L->d_vals;
  kp.Nx = (int32_t)F.Nx; kp.Nu = (int32_t)F.Nu; kp.T = (int32_t)F.T; kp.R = (int32_t)controller_ring_slots(F.T);
  kp.nscen = nscen;
  L->scn = scenario_slots(nscen);
  e = hipMemset(static_cast<unsigned char*>(L->arena) + L->state_off, 0, L->state_bytes);   // the state after a reset
  if (e == hipSuccess) e = hipDeviceSynchronize();                                          // plan time may wait; the calls below never do
  if (e != hipSuccess) { (void)hipFree(L->arena); delete L; return hipfail(ctx, e, "sls_controller_plan: upload"); }
  *out = L;
  return 0;
}

int sls_controller_load(sls_controller* L, void* hip_stream, const double* d_values) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_controller_load: null controller");
  if (!d_values && L->n_entries > 0) return fail(L->ctx, SLS_EINVAL, "sls_controller_load: null device pointer");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  // Φ: mask order → row order
  if (int rc = launch_gather_phi(L->ctx, d_values, L->d_perm, L->n_entries, L->d_vals, static_cast<hipStream_t>(hip_stream))) return rc;
  L->loaded = true;
  return 0;
}

int sls_controller_reset(sls_controller* L, void* hip_stream) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_controller_reset: null controller");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  HIPCHK(L->ctx, hipMemsetAsync(static_cast<unsigned char*>(L->arena) + L->state_off, 0, L->state_bytes, static_cast<hipStream_t>(hip_stream)));
  L->k = 0;
  return 0;
}

int sls_controller_step(sls_controller* L, void* hip_stream, const double* d_x, double* d_u, double* d_what) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_controller_step: null controller");
  sls_ctx* ctx = L->ctx;
  if (!L->loaded) return fail(ctx, SLS_EINVAL, "sls_controller_step: no Φ loaded (sls_controller_load first)");
  if (!d_x || (!d_u && L->kp.Nu > 0)) return fail(ctx, SLS_EINVAL, "sls_controller_step: null device pointer");
  HIPCHK(ctx, hipSetDevice(L->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (st) {                                                    // the null stream cannot be captured
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(ctx, hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return fail(ctx, SLS_EUNSUPPORTED, "sls_controller_step: the stream is being captured (ring slot and β parity are launch arguments)");
  }
  const int s = (int)controller_slot(L->k, L->kp.R), par = (int)(L->k & 1);
  HIPCHK(ctx, launch_controller_step(L->scn, L->kp, s, par, d_x, d_u, d_what, st));
  ++L->k;
  return 0;
}

int sls_controller_info(const sls_controller* L, int64_t* n_entries, int64_t* steps_done, int64_t* state_bytes) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_controller_info: null controller");
  if (n_entries) *n_entries = L->n_entries;
  if (steps_done) *steps_done = L->k;
  if (state_bytes) *state_bytes = (int64_t)L->state_bytes;
  return 0;
}

void sls_controller_destroy(sls_controller* L) {
  if (!L) return;
  (void)hipSetDevice(L->dev);
  if (L->arena) (void)hipFree(L->arena);
  delete L;
}

/* diagnostics (include/sls_mi355x_debug.h): the controller's tables from the masks.  Needs no device. */
int sls_debug_controller_tables(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries,
                                int32_t* row_ptr, int32_t* lag, int32_t* col, int32_t* perm) {
  FirOperator F;
  std::string msg;
  int rc = build_controller_operator(dims, Sx, Su, F, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_controller_tables: " + msg);
  const int64_t n = (int64_t)F.hoff.size();
  if (n_entries) *n_entries = n;
  if (row_ptr) {
    std::copy(F.beta_ptr.begin(), F.beta_ptr.end(), row_ptr);
    std::copy(F.u_ptr.begin() + 1, F.u_ptr.end(), row_ptr + F.Nx + 1);
  }
  for (int64_t e = 0; e < n; ++e) {
    if (lag) lag[e] = (int32_t)controller_lag(F.hoff[e], F.Nx);
    if (col) col[e] = (int32_t)controller_col(F.hoff[e], F.Nx);
    if (perm) perm[e] = F.perm[e];
  }
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of `steps` controller steps from a reset state (csrc/sls_controller.cpp).
   Needs no device. */
int sls_debug_controller_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                              int64_t nscen, int64_t steps, const double* x, double* u, double* what) {
  FirOperator F;
  std::string msg;
  int rc = build_controller_operator(dims, Sx, Su, F, msg);
  if (!rc) rc = controller_host(F, values, nscen, steps, x, u, what, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_controller_host: " + msg);
  return 0;
}

}  // extern "C"
