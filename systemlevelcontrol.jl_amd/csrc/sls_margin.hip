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
// load and set_plant are the shared gathers of sls_object.h.  load, set_plant (device path), run allocate nothing and never
// wait.  The worst case over a box of plants (sls_margin_set_radius, sls_margin_box_*; semantics in sls_margin_box.h, kernels
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
#include "sls_object.h"
#include "sls_wave_util.h"

namespace {

using sls::MarginParams;

constexpr int kWavesPerBlock = 4;

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
  sum = sls::lane_group_sum<SS>(sum);
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
  int64_t n_entries = 0, n_defect = 0;
  void* arena = nullptr;               // tables, Φ by columns, plant values, staging, scratch, results
  const int32_t* d_perm = nullptr;
  double* d_phi = nullptr;
  sls::PlantEnsemble plant;
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
  int rc = check_plan_args(ctx, "sls_margin_plan", out, dims && P && Sx && Su, dev_slot, nscen);
  if (rc) return rc;
  MarginTables Tb;
  std::string msg;
  rc = build_margin_tables(dims, P, Sx, Su, Tb, msg);
  if (rc) return fail(ctx, rc, "sls_margin_plan: " + msg);
  const FirOperator& F = Tb.R.F;
  const int64_t Nx = Tb.Nx;
  if ((rc = PlantEnsemble::check_size(ctx, "sls_margin_plan", F.A.val.size(), F.B2.val.size(), nscen))) return rc;
  if (2 * Nx * (nscen / kMarginSumScen + 1) / 4 + 1 > 0x7fffffffLL) return fail(ctx, SLS_EUNSUPPORTED, "sls_margin_plan: Nx·nscen exceeds the sum pass's grid");
  sls_margin* M = new (std::nothrow) sls_margin();
  if (!M) return fail(ctx, SLS_ENOMEM, "sls_margin_plan: out of memory");
  M->ctx = ctx; M->dev = ctx->devs[dev_slot];
  M->n_entries = (int64_t)Tb.phi_perm.size(); M->n_defect = (int64_t)Tb.def_key.size();
  M->h_A_ptr = F.A.ptr; M->h_A_src = Tb.R.A_src; M->h_B2_ptr = F.B2.ptr; M->h_B2_src = Tb.R.B2_src;
  hipError_t e = hipSetDevice(M->dev);
  if (e != hipSuccess) { delete M; return hipfail(ctx, e, "hipSetDevice"); }
  // one arena: uploaded tables first, then the buffers the object owns
  Arena ar;
  MarginParams& kp = M->kp;
  ar.table(Tb.phi_seg, &kp.v.phi_seg); ar.table(Tb.phi_row, &kp.v.phi_row); ar.table(Tb.phi_perm, &M->d_perm);
  ar.table(F.A.ptr, &kp.v.A_ptr); ar.table(F.A.idx, &kp.v.A_idx); ar.table(F.B2.ptr, &kp.v.B2_ptr); ar.table(F.B2.idx, &kp.v.B2_idx);
  M->plant.lay_out_tables(ar, Tb.R.A_src, Tb.R.B2_src);
  ar.table(Tb.def_ptr, &kp.def_ptr); ar.table(Tb.def_col, &kp.def_col); ar.table(Tb.def_key, &kp.def_key);
  ar.table(Tb.def_start, &kp.def_start); ar.table(Tb.row_ptr, &kp.row_ptr); ar.table(Tb.row_perm, &kp.row_perm);
  ar.buffer((size_t)M->n_entries, &M->d_phi);
  M->plant_bytes = M->plant.lay_out_values(ar, nscen);
  ar.buffer((size_t)(M->n_defect * nscen), &kp.scratch);
  ar.buffer((size_t)((2 * Nx + 2) * nscen), &M->d_result);
  M->device_bytes = ar.bytes();
  rc = ar.commit(ctx, &M->arena, "hipMalloc (margin)", "hipMemcpy H2D (margin tables)");
  if (rc) { delete M; return rc; }
  kp.v.phi_val = M->d_phi; kp.v.A_val = M->plant.d_A_val; kp.v.B2_val = M->plant.d_B2_val;
  kp.n_defect = M->n_defect;
  kp.v.Nx = (int32_t)Nx; kp.v.Nu = (int32_t)Tb.Nu; kp.v.T = (int32_t)Tb.T; kp.v.nscen = nscen;
  M->scn = scenario_slots(nscen);
  rc = M->plant.init_from(ctx, P, "sls_margin_plan: upload");
  if (rc) { (void)hipFree(M->arena); delete M; return rc; }
  *out = M;
  return 0;
}

int sls_margin_load(sls_margin* M, void* hip_stream, const double* d_values) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_load: null margin");
  if (!d_values && M->n_entries > 0) return fail(M->ctx, SLS_EINVAL, "sls_margin_load: null device pointer");
  HIPCHK(M->ctx, hipSetDevice(M->dev));
  // Φ: mask order → by columns
  if (int rc = launch_gather_phi(M->ctx, d_values, M->d_perm, M->n_entries, M->d_phi, static_cast<hipStream_t>(hip_stream))) return rc;
  M->loaded = true;
  return 0;
}

int sls_margin_set_plant(sls_margin* M, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device, int per_scenario) {
  if (!M) return fail(nullptr, SLS_EINVAL, "sls_margin_set_plant: null margin");
  HIPCHK(M->ctx, hipSetDevice(M->dev));
  return M->plant.set(M->ctx, static_cast<hipStream_t>(hip_stream), A_nzval, B2_nzval, on_device, per_scenario);
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
  const double* d_val[2] = {M->plant.d_A_val, M->plant.d_B2_val};
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
  if (!M->box_arena) {                                         // sizes depend on the plan alone: allocated once, filled below
    const size_t nnzA = (size_t)M->plant.nnzA, nnzB = (size_t)M->plant.nnzB;
    Arena ar;
    ar.buffer((size_t)(Nx + 1), &M->bview.act_ptr); ar.buffer(nnzA + nnzB, &M->bview.act_ent);
    ar.buffer(nnzA * ns, &M->bview.A_rad); ar.buffer(nnzB * ns, &M->bview.B2_rad);
    ar.buffer((size_t)(Nx * ns), &M->d_box_wc); ar.buffer((size_t)(Nx * ns), &M->d_box_vertex); ar.buffer((size_t)ns, &M->d_box_tot);
    if ((rc = ar.commit(ctx, &M->box_arena, "hipMalloc(&a, total)", ""))) return rc;   // what: the call text a HIPCHK reports here
    M->box_bytes = ar.bytes();
    M->bview.nnzA = (int32_t)nnzA;
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
  std::vector<double> A_cen((size_t)(M->plant.nnzA * ns)), B2_cen((size_t)(M->plant.nnzB * ns));
  if (!A_cen.empty()) HIPCHK(ctx, hipMemcpyAsync(A_cen.data(), M->plant.d_A_val, A_cen.size() * 8, hipMemcpyDeviceToHost, st));
  if (!B2_cen.empty()) HIPCHK(ctx, hipMemcpyAsync(B2_cen.data(), M->plant.d_B2_val, B2_cen.size() * 8, hipMemcpyDeviceToHost, st));
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
