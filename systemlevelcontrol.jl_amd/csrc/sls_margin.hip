// sls_margin.hip — robust-stability margins of a resident Φ for an ensemble of plants: sls_margin_* of include/sls_mi355x.h.
//
// Semantics, the defect pattern, the value of an entry, the summation order and the memory: sls_margin.h.  A run is three
// launches on the caller's stream:
//   margin_defect_kernel<SCN>  the pattern entries are independent of each other, so the pass is flat over them: lanes = (entry
//                              slot le, scenario slot ls), lane = le·SCN + ls as in the rollout, SCN ∈ {1, 2, 4, …, 64}; a wave
//                              takes NE = 64/SCN consecutive entries for a chunk of SCN scenarios.  A lane evaluates
//                              margin_entry — the Φ factors by binary search inside the (j, τ) segment, the plant values at
//                              [e][scen], contiguous along the scenario lanes — and stores |D| once to the scratch
//                              [n_defect][nscen].  (One wave per column left 59 waves on the README chain.)
//   margin_sums_kernel         one wave per (list, chunk of 8 scenarios): the Nx row lists (through row_perm) and the Nx column
//                              lists in margin_slot_sum's order, 8 entry slots closed by the xor-shuffle tree.  The shape does
//                              not depend on nscen and the lane layout of the first kernel never enters a sum, which is what
//                              makes scenario s independent of nscen.
//   margin_totals_kernel       one wave per chunk of 8 scenarios: the two maxima.
// load and the device path of set_plant are one gather launch each.  load, set_plant (device path), run allocate nothing and
// never wait.  The worst case over a box of plants (sls_margin_set_radius, sls_margin_box_*; semantics in sls_margin_box.h, kernels
// in sls_margin_box.hip) lives on the same object: set_radius is a setup call, box_run enqueues two launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_internal.h"
#include "sls_margin.h"
#include "sls_margin_box.h"

namespace {

using sls::MarginParams;

constexpr int kWavesPerBlock = 4;

__global__ void margin_gather_phi_kernel(const double* __restrict__ values, const int32_t* __restrict__ perm, long long n,
                                         double* __restrict__ vals) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) vals[k] = values[perm[k]];
}

// dst[e][s] = src[from[e]][s] (per_scenario) or src[from[e]] (broadcast): CSC → CSR, scenario innermost; n = nnz·nscen
__global__ void margin_gather_plant_kernel(const double* __restrict__ src, const int32_t* __restrict__ from, long long n, long long ns,
                                           int per_scenario, double* __restrict__ dst) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long long e = k / ns, s = k - e * ns;
  dst[k] = per_scenario ? src[(long long)from[e] * ns + s] : src[from[e]];
}

// lanes = (entry slot le, scenario slot ls), lane = le·SCN + ls; the wave evaluates NE = 64/SCN consecutive pattern entries
template <int SCN>
__global__ void __launch_bounds__(64 * kWavesPerBlock) margin_defect_kernel(MarginParams p) {
  constexpr int NE = 64 / SCN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ls = lane % SCN, le = lane / SCN;
  const long long d = ((long long)blockIdx.x * kWavesPerBlock + wave) * NE + le;
  const long long scen = (long long)blockIdx.y * SCN + ls;
  if (d >= p.n_defect || scen >= p.v.nscen) return;
  p.scratch[d * p.v.nscen + scen] = sls::margin_entry(p.v, p.def_col[d], p.def_key[d], p.def_start[d], scen);
}

template <int SCN>
hipError_t launch_defect(const MarginParams& p, hipStream_t st) {
  constexpr long long per_block = (long long)kWavesPerBlock * (64 / SCN);
  dim3 grid((unsigned)((p.n_defect + per_block - 1) / per_block), (unsigned)((p.v.nscen + SCN - 1) / SCN));
  hipLaunchKernelGGL(margin_defect_kernel<SCN>, grid, dim3(64 * kWavesPerBlock), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_margin_defect(int scn, const MarginParams& p, hipStream_t st) {
  switch (scn) {
    case 1: return launch_defect<1>(p, st);
    case 2: return launch_defect<2>(p, st);
    case 4: return launch_defect<4>(p, st);
    case 8: return launch_defect<8>(p, st);
    case 16: return launch_defect<16>(p, st);
    case 32: return launch_defect<32>(p, st);
    default: return launch_defect<64>(p, st);
  }
}

// One wave per (list, chunk of kMarginSumScen scenarios), whatever nscen is: lanes = (entry slot q, scenario slot ls), lane =
// q·kMarginSumScen + ls.  Lists 0 … Nx−1 are the rows (through row_perm), Nx … 2·Nx−1 the columns.  margin_slot_sum's order: slot
// q adds the list positions q, q + 8, … ascending, then the xor tree over the slots.
__global__ void __launch_bounds__(64 * kWavesPerBlock) margin_sums_kernel(MarginParams p, long long nchunk, double* __restrict__ row_l1,
                                                                         double* __restrict__ col_l1) {
  constexpr int SS = sls::kMarginSumScen, SQ = sls::kMarginSumSlots;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ls = lane % SS, q = lane / SS;
  const long long w = (long long)blockIdx.x * kWavesPerBlock + wave;
  const long long ns = p.v.nscen;
  if (w >= 2LL * p.v.Nx * nchunk) return;
  const int list = (int)(w / nchunk);
  const long long scen = (w - (long long)list * nchunk) * SS + ls;
  const bool live = scen < ns;
  const double* __restrict__ sv = p.scratch + (live ? scen : 0);   // dead lanes read scenario 0 and never write
  double sum;
  if (list < p.v.Nx) {
    const int32_t* __restrict__ perm = p.row_perm + p.row_ptr[list];
    sum = sls::margin_slot_sum(p.row_ptr[list + 1] - p.row_ptr[list], q, [&](int32_t k) { return sv[(long long)perm[k] * ns]; });
  } else {
    const long long beg = p.def_ptr[list - p.v.Nx];
    sum = sls::margin_slot_sum(p.def_ptr[list - p.v.Nx + 1] - p.def_ptr[list - p.v.Nx], q, [&](int32_t k) { return sv[(beg + k) * ns]; });
  }
#pragma unroll
  for (int off = 32; off >= SS; off >>= 1) sum += __shfl_xor(sum, off, 64);
  static_assert(SS * SQ == 64, "one wave");
  if (q == 0 && live) (list < p.v.Nx ? row_l1 : col_l1)[(long long)(list < p.v.Nx ? list : list - p.v.Nx) * ns + scen] = sls::margin_report(sum);
}

// One wave per chunk of kMarginSumScen scenarios; fmax of non-negative numbers is exact in any order
__global__ void __launch_bounds__(64) margin_totals_kernel(const double* __restrict__ row_l1, const double* __restrict__ col_l1, int Nx,
                                                           long long ns, double* __restrict__ totals) {
  constexpr int SS = sls::kMarginSumScen, SQ = sls::kMarginSumSlots;
  const int ls = threadIdx.x % SS, q = threadIdx.x / SS;
  const long long scen = (long long)blockIdx.x * SS + ls;
  const bool live = scen < ns;
  const long long s = live ? scen : 0;
  double l1 = 0.0, e1 = 0.0;
  for (int i = q; i < Nx; i += SQ) {
    l1 = fmax(l1, row_l1[(long long)i * ns + s]);
    e1 = fmax(e1, col_l1[(long long)i * ns + s]);
  }
#pragma unroll
  for (int off = 32; off >= SS; off >>= 1) {
    l1 = fmax(l1, __shfl_xor(l1, off, 64));
    e1 = fmax(e1, __shfl_xor(e1, off, 64));
  }
  if (q == 0 && live) { totals[scen] = l1; totals[ns + scen] = e1; }
}

}  // namespace

struct sls_margin {
  sls_ctx* ctx = nullptr;
  int dev = 0;
  int64_t n_entries = 0, n_defect = 0, nnzA = 0, nnzB = 0;
  void* arena = nullptr;               // tables, Φ by columns, plant values, staging, scratch, results
  const int32_t *d_perm = nullptr, *d_A_src = nullptr, *d_B2_src = nullptr;
  double *d_phi = nullptr, *d_A_val = nullptr, *d_B2_val = nullptr;
  double* d_stage = nullptr;           // max(nnz(A), nnz(B₂))·nscen doubles: where the host path of set_plant lands
  double* d_result = nullptr;          // row_l1 [Nx][nscen], col_l1 [Nx][nscen], totals [2][nscen]
  MarginParams kp{};
  int scn = 1;                         // scenario slots per wave: smallest power of two ≥ nscen, at most 64
  size_t device_bytes = 0, plant_bytes = 0;
  bool loaded = false;
  // the box of sls_margin_set_radius (sls_margin_box.h): the plant by rows stays on the host for the active lists and the worst
  // plant; the second arena (active lists, radii, results) is allocated by the first set_radius
  std::vector<int32_t> h_A_ptr, h_A_src, h_B2_ptr, h_B2_src;
  sls::MarginBoxLists box;
  sls::MarginBoxView bview{};
  void* box_arena = nullptr;
  double *d_box_wc = nullptr, *d_box_tot = nullptr;
  long long* d_box_vertex = nullptr;
  size_t box_bytes = 0;
  bool has_radius = false;
};

using namespace sls;

namespace {

int enqueue_plant_gather(sls_margin* M, hipStream_t st, const double* d_src, const int32_t* d_from, int64_t nnz, int per_scenario,
                         double* d_dst) {
  const long long n = (long long)nnz * M->kp.v.nscen;
  if (n == 0) return 0;
  const int bs = 256;
  hipLaunchKernelGGL(margin_gather_plant_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, st, d_src, d_from, n, M->kp.v.nscen,
                     per_scenario, d_dst);
  HIPCHK(M->ctx, hipGetLastError());
  return 0;
}

// the three passes; every destination is a device pointer and not NULL
int enqueue_run(sls_margin* M, hipStream_t st, double* d_row, double* d_col, double* d_tot) {
  const MarginParams& p = M->kp;
  const long long ns = p.v.nscen;
  if (M->n_defect > 0) HIPCHK(M->ctx, launch_margin_defect(M->scn, p, st));
  const long long nchunk = (ns + kMarginSumScen - 1) / kMarginSumScen, nwave = 2LL * p.v.Nx * nchunk;
  hipLaunchKernelGGL(margin_sums_kernel, dim3((unsigned)((nwave + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, p,
                     nchunk, d_row, d_col);
  HIPCHK(M->ctx, hipGetLastError());
  hipLaunchKernelGGL(margin_totals_kernel, dim3((unsigned)nchunk), dim3(64), 0, st, d_row, d_col, p.v.Nx, ns, d_tot);
  HIPCHK(M->ctx, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int sls_margin_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                    int64_t nscen, sls_margin** out) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "sls_margin_plan: null context");
  if (!out || !dims || !P || !Sx || !Su) return fail(ctx, SLS_EINVAL, "sls_margin_plan: null argument");
  *out = nullptr;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "sls_margin_plan: dev_slot out of range");
  if (nscen < 1) return fail(ctx, SLS_EINVAL, "sls_margin_plan: nscen must be >= 1");
  if (nscen > 65535LL * 64) return fail(ctx, SLS_EUNSUPPORTED, "sls_margin_plan: nscen exceeds 65535 chunks of 64 scenarios");
  MarginTables Tb;
  std::string msg;
  int rc = build_margin_tables(dims, P, Sx, Su, Tb, msg);
  if (rc) return fail(ctx, rc, "sls_margin_plan: " + msg);
  const FirOperator& F = Tb.R.F;
  const int64_t Nx = Tb.Nx;
  const int64_t n_gather = (int64_t)std::max(F.A.val.size(), F.B2.val.size()) * nscen;
  if (n_gather / 256 + 1 > 0x7fffffffLL) return fail(ctx, SLS_EUNSUPPORTED, "sls_margin_plan: nnz·nscen exceeds the gather's grid");
  if (2 * Nx * (nscen / kMarginSumScen + 1) / 4 + 1 > 0x7fffffffLL) return fail(ctx, SLS_EUNSUPPORTED, "sls_margin_plan: Nx·nscen exceeds the sum pass's grid");
  sls_margin* M = new (std::nothrow) sls_margin();
  if (!M) return fail(ctx, SLS_ENOMEM, "sls_margin_plan: out of memory");
  M->ctx = ctx; M->dev = ctx->devs[dev_slot];
  M->n_entries = (int64_t)Tb.phi_perm.size(); M->n_defect = (int64_t)Tb.def_key.size();
  M->nnzA = (int64_t)F.A.val.size(); M->nnzB = (int64_t)F.B2.val.size();
  M->h_A_ptr = F.A.ptr; M->h_A_src = Tb.R.A_src; M->h_B2_ptr = F.B2.ptr; M->h_B2_src = Tb.R.B2_src;
  hipError_t e = hipSetDevice(M->dev);
  if (e != hipSuccess) { delete M; return hipfail(ctx, e, "hipSetDevice"); }
  // one arena: uploaded tables first, then the buffers the object owns
  struct Req { const void* src; size_t bytes; const void** out; };
  std::vector<Req> reqs;
  auto add = [&](const auto& v, const auto** o) { reqs.push_back({v.data(), v.size() * sizeof(v[0]), reinterpret_cast<const void**>(o)}); };
  MarginParams& kp = M->kp;
  add(Tb.phi_seg, &kp.v.phi_seg); add(Tb.phi_row, &kp.v.phi_row); add(Tb.phi_perm, &M->d_perm);
  add(F.A.ptr, &kp.v.A_ptr); add(F.A.idx, &kp.v.A_idx); add(F.B2.ptr, &kp.v.B2_ptr); add(F.B2.idx, &kp.v.B2_idx);
  add(Tb.R.A_src, &M->d_A_src); add(Tb.R.B2_src, &M->d_B2_src);
  add(Tb.def_ptr, &kp.def_ptr); add(Tb.def_col, &kp.def_col); add(Tb.def_key, &kp.def_key); add(Tb.def_start, &kp.def_start);
  add(Tb.row_ptr, &kp.row_ptr); add(Tb.row_perm, &kp.row_perm);
  auto al = [](size_t b) { return (std::max<size_t>(b, 16) + 255) / 256 * 256; };
  size_t total = 0;
  for (auto& r : reqs) total += al(r.bytes);
  const size_t D = sizeof(double);
  const size_t b_phi = al((size_t)M->n_entries * D), b_A = al((size_t)(M->nnzA * nscen) * D), b_B = al((size_t)(M->nnzB * nscen) * D);
  const size_t b_stage = al((size_t)n_gather * D), b_scr = al((size_t)(M->n_defect * nscen) * D), b_res = al((size_t)((2 * Nx + 2) * nscen) * D);
  const size_t off_phi = total, off_A = off_phi + b_phi, off_B = off_A + b_A, off_stage = off_B + b_B, off_scr = off_stage + b_stage;
  const size_t off_res = off_scr + b_scr;
  M->device_bytes = off_res + b_res;
  M->plant_bytes = b_A + b_B;
  e = hipMalloc(&M->arena, M->device_bytes);
  if (e != hipSuccess) { delete M; return hipfail(ctx, e, "hipMalloc (margin)"); }
  unsigned char* base = static_cast<unsigned char*>(M->arena);
  size_t off = 0;
  for (auto& r : reqs) {
    if (r.bytes) {
      e = hipMemcpy(base + off, r.src, r.bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) { (void)hipFree(M->arena); delete M; return hipfail(ctx, e, "hipMemcpy H2D (margin tables)"); }
    }
    *r.out = base + off;
    off += al(r.bytes);
  }
  M->d_phi = reinterpret_cast<double*>(base + off_phi); kp.v.phi_val = M->d_phi;
  M->d_A_val = reinterpret_cast<double*>(base + off_A); kp.v.A_val = M->d_A_val;
  M->d_B2_val = reinterpret_cast<double*>(base + off_B); kp.v.B2_val = M->d_B2_val;
  M->d_stage = reinterpret_cast<double*>(base + off_stage);
  kp.scratch = reinterpret_cast<double*>(base + off_scr);
  M->d_result = reinterpret_cast<double*>(base + off_res);
  kp.n_defect = M->n_defect;
  kp.v.Nx = (int32_t)Nx; kp.v.Nu = (int32_t)Tb.Nu; kp.v.T = (int32_t)Tb.T; kp.v.nscen = nscen;
  while (M->scn < 64 && M->scn < nscen) M->scn <<= 1;
  // every scenario starts from P's values: the broadcast gather from the CSC arrays, staged like a host-path set_plant
  rc = 0;
  const double* init[2] = {P->A->nzval, P->B2->nzval};
  const int64_t nnz[2] = {M->nnzA, M->nnzB};
  const int32_t* from[2] = {M->d_A_src, M->d_B2_src};
  double* dst[2] = {M->d_A_val, M->d_B2_val};
  for (int m = 0; m < 2 && e == hipSuccess && !rc; ++m) {
    if (!nnz[m]) continue;
    if (init[m]) e = hipMemcpy(M->d_stage, init[m], (size_t)nnz[m] * D, hipMemcpyHostToDevice);
    else { std::vector<double> one((size_t)nnz[m], 1.0); e = hipMemcpy(M->d_stage, one.data(), (size_t)nnz[m] * D, hipMemcpyHostToDevice); }
    if (e == hipSuccess) rc = enqueue_plant_gather(M, nullptr, M->d_stage, from[m], nnz[m], 0, dst[m]);
    if (e == hipSuccess && !rc) e = hipDeviceSynchronize();
  }
  if (e != hipSuccess || rc) { (void)hipFree(M->arena); delete M; return rc ? rc : hipfail(ctx, e, "sls_margin_plan: upload"); }
  *out = M;
  return 0;
}

int sls_margin_load(sls_margin* M, void* hip_stream, const double* d_values) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_load: null margin");
  if (!d_values && M->n_entries > 0) return fail(M->ctx, SLS_EINVAL, "sls_margin_load: null device pointer");
  HIPCHK(M->ctx, hipSetDevice(M->dev));
  if (M->n_entries > 0) {                                      // Φ: mask order → by columns
    const int bs = 256;
    hipLaunchKernelGGL(margin_gather_phi_kernel, dim3((unsigned)((M->n_entries + bs - 1) / bs)), dim3(bs), 0,
                       static_cast<hipStream_t>(hip_stream), d_values, M->d_perm, (long long)M->n_entries, M->d_phi);
    HIPCHK(M->ctx, hipGetLastError());
  }
  M->loaded = true;
  return 0;
}

int sls_margin_set_plant(sls_margin* M, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device, int per_scenario) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_set_plant: null margin");
  sls_ctx* ctx = M->ctx;
  HIPCHK(ctx, hipSetDevice(M->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const double* src[2] = {A_nzval, B2_nzval};
  const int64_t nnz[2] = {M->nnzA, M->nnzB};
  const int32_t* from[2] = {M->d_A_src, M->d_B2_src};
  double* dst[2] = {M->d_A_val, M->d_B2_val};
  for (int m = 0; m < 2; ++m) {
    if (!src[m] || !nnz[m]) continue;
    const double* d_src = src[m];
    if (!on_device) {                                          // host arrays land in the staging buffer; the caller's array is free on return
      const size_t bytes = (size_t)nnz[m] * (per_scenario ? (size_t)M->kp.v.nscen : 1) * sizeof(double);
      HIPCHK(ctx, hipMemcpyAsync(M->d_stage, src[m], bytes, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      d_src = M->d_stage;
    }
    int rc = enqueue_plant_gather(M, st, d_src, from[m], nnz[m], per_scenario ? 1 : 0, dst[m]);
    if (rc) return rc;
  }
  return 0;
}

int sls_margin_run(sls_margin* M, void* hip_stream, double* d_row_l1, double* d_col_l1, double* d_totals) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_run: null margin");
  if (!M->loaded) return fail(M->ctx, SLS_EINVAL, "sls_margin_run: no Φ loaded (sls_margin_load first)");
  HIPCHK(M->ctx, hipSetDevice(M->dev));
  const long long ns = M->kp.v.nscen, Nx = M->kp.v.Nx;
  double* res = M->d_result;                                   // a NULL output lands in the object's own buffer
  return enqueue_run(M, static_cast<hipStream_t>(hip_stream), d_row_l1 ? d_row_l1 : res, d_col_l1 ? d_col_l1 : res + Nx * ns,
                     d_totals ? d_totals : res + 2 * Nx * ns);
}

int sls_margin_fetch(sls_margin* M, void* hip_stream, double* row_l1, double* col_l1, double* totals) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_fetch: null margin");
  sls_ctx* ctx = M->ctx;
  if (!M->loaded) return fail(ctx, SLS_EINVAL, "sls_margin_fetch: no Φ loaded (sls_margin_load first)");
  HIPCHK(ctx, hipSetDevice(M->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const long long ns = M->kp.v.nscen, Nx = M->kp.v.Nx;
  double* res = M->d_result;
  int rc = enqueue_run(M, st, res, res + Nx * ns, res + 2 * Nx * ns);
  if (rc) return rc;
  const size_t b = (size_t)ns * sizeof(double);
  if (row_l1) HIPCHK(ctx, hipMemcpyAsync(row_l1, res, (size_t)Nx * b, hipMemcpyDeviceToHost, st));
  if (col_l1) HIPCHK(ctx, hipMemcpyAsync(col_l1, res + Nx * ns, (size_t)Nx * b, hipMemcpyDeviceToHost, st));
  if (totals) HIPCHK(ctx, hipMemcpyAsync(totals, res + 2 * Nx * ns, 2 * b, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

int sls_margin_info(const sls_margin* M, int64_t* n_entries, int64_t* n_defect, int64_t* device_bytes, int64_t* plant_bytes) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_info: null margin");
  if (n_entries) *n_entries = M->n_entries;
  if (n_defect) *n_defect = M->n_defect;
  if (device_bytes) *device_bytes = (int64_t)M->device_bytes;
  if (plant_bytes) *plant_bytes = (int64_t)M->plant_bytes;
  return 0;
}

/* ---- the worst case over a box of plants (sls_margin_box.h; kernels in sls_margin_box.hip) ---- */

int sls_margin_fetch_plant(sls_margin* M, void* hip_stream, double* A_nzval, double* B2_nzval) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_fetch_plant: null margin");
  sls_ctx* ctx = M->ctx;
  HIPCHK(ctx, hipSetDevice(M->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const size_t ns = (size_t)M->kp.v.nscen;
  double* out[2] = {A_nzval, B2_nzval};
  const double* d_val[2] = {M->d_A_val, M->d_B2_val};
  const std::vector<int32_t>* src[2] = {&M->h_A_src, &M->h_B2_src};
  std::vector<double> csr;
  for (int m = 0; m < 2; ++m) {
    if (!out[m] || src[m]->empty()) continue;
    csr.resize(src[m]->size() * ns);
    HIPCHK(ctx, hipMemcpyAsync(csr.data(), d_val[m], csr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (size_t e = 0; e < src[m]->size(); ++e) std::copy(csr.begin() + e * ns, csr.begin() + (e + 1) * ns, out[m] + (size_t)(*src[m])[e] * ns);
  }
  return 0;
}

int sls_margin_set_radius(sls_margin* M, const double* A_rad, const double* B2_rad, int per_scenario) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_set_radius: null margin");
  sls_ctx* ctx = M->ctx;
  const long long ns = M->kp.v.nscen, Nx = M->kp.v.Nx;
  if (Nx * ns > 0x7fffffffLL) return fail(ctx, SLS_EUNSUPPORTED, "sls_margin_set_radius: Nx·nscen exceeds the row pass's grid");
  MarginBoxLists L;
  std::string msg;
  int rc = build_margin_box_lists(M->h_A_ptr, M->h_A_src, M->h_B2_ptr, M->h_B2_src, ns, A_rad, B2_rad, per_scenario != 0, L, msg);
  if (rc) return fail(ctx, rc, "sls_margin_set_radius: " + msg);
  HIPCHK(ctx, hipSetDevice(M->dev));
  auto al = [](size_t b) { return (std::max<size_t>(b, 16) + 255) / 256 * 256; };
  const size_t b_ptr = al((size_t)(Nx + 1) * 4), b_ent = al((size_t)(M->nnzA + M->nnzB) * 4), b_ra = al((size_t)(M->nnzA * ns) * 8);
  const size_t b_rb = al((size_t)(M->nnzB * ns) * 8), b_rows = al((size_t)(Nx * ns) * 8), b_tot = al((size_t)ns * 8);
  if (!M->box_arena) {                                         // sizes depend on the plan alone: allocated once
    void* a = nullptr;
    const size_t total = b_ptr + b_ent + b_ra + b_rb + 2 * b_rows + b_tot;
    HIPCHK(ctx, hipMalloc(&a, total));
    M->box_arena = a; M->box_bytes = total;
    unsigned char* base = static_cast<unsigned char*>(a);
    M->bview.act_ptr = reinterpret_cast<const int32_t*>(base); base += b_ptr;
    M->bview.act_ent = reinterpret_cast<const int32_t*>(base); base += b_ent;
    M->bview.A_rad = reinterpret_cast<const double*>(base); base += b_ra;
    M->bview.B2_rad = reinterpret_cast<const double*>(base); base += b_rb;
    M->d_box_wc = reinterpret_cast<double*>(base); base += b_rows;
    M->d_box_vertex = reinterpret_cast<long long*>(base); base += b_rows;
    M->d_box_tot = reinterpret_cast<double*>(base);
    M->bview.nnzA = (int32_t)M->nnzA;
  }
  HIPCHK(ctx, hipDeviceSynchronize());                         // a run in flight still reads the lists
  struct Up { const void* dst; const void* src; size_t bytes; };
  const Up ups[4] = {{M->bview.act_ptr, L.act_ptr.data(), L.act_ptr.size() * 4}, {M->bview.act_ent, L.act_ent.data(), L.act_ent.size() * 4},
                     {M->bview.A_rad, L.A_rad.data(), L.A_rad.size() * 8}, {M->bview.B2_rad, L.B2_rad.data(), L.B2_rad.size() * 8}};
  for (const Up& u : ups)
    if (u.bytes) HIPCHK(ctx, hipMemcpy(const_cast<void*>(u.dst), u.src, u.bytes, hipMemcpyHostToDevice));
  M->box = std::move(L);
  M->has_radius = true;
  return 0;
}

namespace {
int box_ready(sls_margin* M, const char* who) {
  if (!M->loaded) return fail(M->ctx, SLS_EINVAL, std::string(who) + ": no Φ loaded (sls_margin_load first)");
  if (!M->has_radius) return fail(M->ctx, SLS_EINVAL, std::string(who) + ": no radii set (sls_margin_set_radius first)");
  return 0;
}
int enqueue_box(sls_margin* M, hipStream_t st, double* d_wc, long long* d_vertex, double* d_tot) {
  const MarginBoxParams bp{M->kp, M->bview};
  HIPCHK(M->ctx, launch_margin_box(bp, st, d_wc, d_vertex, d_tot));
  return 0;
}
}  // namespace

int sls_margin_box_run(sls_margin* M, void* hip_stream, double* d_row_wc, int64_t* d_row_vertex, double* d_totals) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_box_run: null margin");
  int rc = box_ready(M, "sls_margin_box_run");
  if (rc) return rc;
  HIPCHK(M->ctx, hipSetDevice(M->dev));
  static_assert(sizeof(long long) == sizeof(int64_t), "vertex codes are int64");
  return enqueue_box(M, static_cast<hipStream_t>(hip_stream), d_row_wc ? d_row_wc : M->d_box_wc,
                     d_row_vertex ? reinterpret_cast<long long*>(d_row_vertex) : M->d_box_vertex, d_totals ? d_totals : M->d_box_tot);
}

int sls_margin_box_fetch(sls_margin* M, void* hip_stream, double* row_wc, int64_t* row_vertex, uint8_t* row_exact, double* totals) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_box_fetch: null margin");
  sls_ctx* ctx = M->ctx;
  int rc = box_ready(M, "sls_margin_box_fetch");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(M->dev));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const size_t rows = (size_t)(M->kp.v.Nx * M->kp.v.nscen) * 8;
  if ((rc = enqueue_box(M, st, M->d_box_wc, M->d_box_vertex, M->d_box_tot))) return rc;
  if (row_wc && rows) HIPCHK(ctx, hipMemcpyAsync(row_wc, M->d_box_wc, rows, hipMemcpyDeviceToHost, st));
  if (row_vertex && rows) HIPCHK(ctx, hipMemcpyAsync(row_vertex, M->d_box_vertex, rows, hipMemcpyDeviceToHost, st));
  if (totals) HIPCHK(ctx, hipMemcpyAsync(totals, M->d_box_tot, (size_t)M->kp.v.nscen * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (row_exact) std::copy(M->box.exact.begin(), M->box.exact.end(), row_exact);
  return 0;
}

int sls_margin_box_worst_plant(sls_margin* M, void* hip_stream, double* A_nzval, double* B2_nzval) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_box_worst_plant: null margin");
  sls_ctx* ctx = M->ctx;
  const long long ns = M->kp.v.nscen, Nx = M->kp.v.Nx;
  std::vector<int64_t> vertex((size_t)(Nx * ns));
  int rc = sls_margin_box_fetch(M, hip_stream, nullptr, vertex.data(), nullptr, nullptr);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  std::vector<double> A_cen((size_t)(M->nnzA * ns)), B2_cen((size_t)(M->nnzB * ns));
  if (!A_cen.empty()) HIPCHK(ctx, hipMemcpyAsync(A_cen.data(), M->d_A_val, A_cen.size() * 8, hipMemcpyDeviceToHost, st));
  if (!B2_cen.empty()) HIPCHK(ctx, hipMemcpyAsync(B2_cen.data(), M->d_B2_val, B2_cen.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  margin_box_worst_plant(M->h_A_ptr, M->h_A_src, M->h_B2_ptr, M->h_B2_src, M->box, A_cen.data(), B2_cen.data(), vertex.data(), A_nzval, B2_nzval);
  return 0;
}

int sls_margin_box_info(const sls_margin* M, int64_t* max_bits, int64_t* n_inexact_rows, int64_t* n_vertex_sums, int64_t* device_bytes) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_box_info: null margin");
  if (!M->has_radius) return fail(M->ctx, SLS_EINVAL, "sls_margin_box_info: no radii set (sls_margin_set_radius first)");
  if (max_bits) *max_bits = M->box.max_bits;
  if (n_inexact_rows) *n_inexact_rows = M->box.n_inexact_rows;
  if (n_vertex_sums) *n_vertex_sums = M->box.n_vertex_sums;
  if (device_bytes) *device_bytes = (int64_t)M->box_bytes;
  return 0;
}

void sls_margin_destroy(sls_margin* M) {
  if (!M) return;
  (void)hipSetDevice(M->dev);
  if (M->arena) (void)hipFree(M->arena);
  if (M->box_arena) (void)hipFree(M->box_arena);
  delete M;
}

}  // extern "C"
