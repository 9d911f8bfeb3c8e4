// sls_object.hip — the arena, the Φ gather and the plant ensemble of the objects that evaluate a resident Φ (sls_object.h).
#include "sls_object.h"

#include <cstring>

namespace {

__global__ void gather_phi_kernel(const double* __restrict__ values, const int32_t* __restrict__ perm, long long n,
                                  double* __restrict__ vals) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) vals[k] = values[perm[k]];
}

// dst[e][s] = src[from[e]][s] (per_scenario) or src[from[e]] (broadcast): CSC → CSR, scenario innermost; n = nnz·nscen
__global__ void gather_plant_kernel(const double* __restrict__ src, const int32_t* __restrict__ from, long long n, long long ns,
                                    int per_scenario, double* __restrict__ dst) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long long e = k / ns, s = k - e * ns;
  dst[k] = per_scenario ? src[(long long)from[e] * ns + s] : src[from[e]];
}

constexpr int kGatherBlock = 256;

int enqueue_plant_gather(sls_ctx* ctx, hipStream_t st, const double* d_src, const int32_t* d_from, int64_t nnz, int64_t nscen,
                         int per_scenario, double* d_dst) {
  const long long n = (long long)nnz * nscen;
  if (n == 0) return 0;
  hipLaunchKernelGGL(gather_plant_kernel, dim3((unsigned)((n + kGatherBlock - 1) / kGatherBlock)), dim3(kGatherBlock), 0, st, d_src,
                     d_from, n, (long long)nscen, per_scenario, d_dst);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // namespace

namespace sls {

int Arena::commit(sls_ctx* ctx, void** arena, const char* what_malloc, const char* what_upload) {
  *arena = nullptr;
  void* a = nullptr;
  hipError_t e = hipMalloc(&a, total_);
  if (e != hipSuccess) return hipfail(ctx, e, what_malloc);
  unsigned char* base = static_cast<unsigned char*>(a);
  size_t off = 0;
  for (const Req& r : reqs_) {
    if (r.src && r.bytes) {
      e = hipMemcpy(base + off, r.src, r.bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) { (void)hipFree(a); return hipfail(ctx, e, what_upload); }
    }
    *r.out = base + off;
    off += al(r.bytes);
  }
  *arena = a;
  return 0;
}

int Arena::commit_in(sls_ctx* ctx, void* base, const Layout& lay, unsigned char* stage, const char* what_upload) {
  unsigned char* b = static_cast<unsigned char*>(base);
  std::vector<unsigned char> stage_v;
  if (!stage) { stage_v.resize(lay.staged_end); stage = stage_v.data(); }
  for (size_t i = 0; i < reqs_.size(); ++i) {
    *reqs_[i].out = b + lay.off[i];
    if (reqs_[i].src && lay.off[i] < lay.staged_end) std::memcpy(stage + lay.off[i], reqs_[i].src, reqs_[i].bytes);
  }
  hipError_t e = lay.staged_end ? hipMemcpy(b, stage, lay.staged_end, hipMemcpyHostToDevice) : hipSuccess;
  for (size_t i = 0; i < reqs_.size() && e == hipSuccess; ++i)
    if (reqs_[i].src && lay.off[i] >= lay.staged_end) e = hipMemcpy(b + lay.off[i], reqs_[i].src, reqs_[i].bytes, hipMemcpyHostToDevice);
  return e == hipSuccess ? 0 : hipfail(ctx, e, what_upload);
}

int Arena::clear(sls_ctx* ctx, void* base, const Layout& lay, hipStream_t stream, const char* what) const {
  unsigned char* b = static_cast<unsigned char*>(base);
  hipError_t e = hipSuccess;
  if (lay.clear_hull) {
    if (lay.clear_end > lay.clear_begin) e = hipMemsetAsync(b + lay.clear_begin, 0, lay.clear_end - lay.clear_begin, stream);
  } else {
    for (size_t i = 0; i < reqs_.size() && e == hipSuccess; ++i)
      if (reqs_[i].own && reqs_[i].bytes <= kClearUpTo) e = hipMemsetAsync(b + lay.off[i], 0, reqs_[i].bytes, stream);
  }
  return e == hipSuccess ? 0 : hipfail(ctx, e, what);
}

int launch_gather_phi(sls_ctx* ctx, const double* d_values, const int32_t* d_perm, int64_t n, double* d_vals, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(gather_phi_kernel, dim3((unsigned)((n + kGatherBlock - 1) / kGatherBlock)), dim3(kGatherBlock), 0, stream, d_values,
                     d_perm, (long long)n, d_vals);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int PlantEnsemble::check_size(sls_ctx* ctx, const std::string& who, size_t nnzA, size_t nnzB, int64_t nscen) {
  const int64_t n_gather = (int64_t)std::max(nnzA, nnzB) * nscen;
  if (n_gather / kGatherBlock + 1 > 0x7fffffffLL) return fail(ctx, SLS_EUNSUPPORTED, who + ": nnz·nscen exceeds the gather's grid");
  return 0;
}

void PlantEnsemble::lay_out_tables(Arena& a, const std::vector<int32_t>& A_src, const std::vector<int32_t>& B2_src) {
  nnzA = (int64_t)A_src.size(); nnzB = (int64_t)B2_src.size();
  a.table(A_src, &d_A_src); a.table(B2_src, &d_B2_src);
}

size_t PlantEnsemble::lay_out_values(Arena& a, int64_t ns) {
  nscen = ns;
  const size_t before = a.bytes();
  a.buffer((size_t)(nnzA * ns), &d_A_val); a.buffer((size_t)(nnzB * ns), &d_B2_val);
  const size_t plant_bytes = a.bytes() - before;
  a.buffer((size_t)(std::max(nnzA, nnzB) * ns), &d_stage);
  return plant_bytes;
}

int PlantEnsemble::init_from(sls_ctx* ctx, const sls_plant* P, const char* what) {
  const double* init[2] = {P->A->nzval, P->B2->nzval};
  const int64_t nnz[2] = {nnzA, nnzB};
  const int32_t* from[2] = {d_A_src, d_B2_src};
  double* dst[2] = {d_A_val, d_B2_val};
  for (int m = 0; m < 2; ++m) {
    if (!nnz[m]) continue;
    std::vector<double> one;
    if (!init[m]) one.assign((size_t)nnz[m], 1.0);
    hipError_t e = hipMemcpy(d_stage, init[m] ? init[m] : one.data(), (size_t)nnz[m] * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipfail(ctx, e, what);
    if (int rc = enqueue_plant_gather(ctx, nullptr, d_stage, from[m], nnz[m], nscen, 0, dst[m])) return rc;
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return hipfail(ctx, e, what);
  }
  return 0;
}

int PlantEnsemble::set(sls_ctx* ctx, hipStream_t st, const double* A_nzval, const double* B2_nzval, int on_device, int per_scenario) {
  const double* src[2] = {A_nzval, B2_nzval};
  const int64_t nnz[2] = {nnzA, nnzB};
  const int32_t* from[2] = {d_A_src, d_B2_src};
  double* dst[2] = {d_A_val, d_B2_val};
  for (int m = 0; m < 2; ++m) {
    if (!src[m] || !nnz[m]) continue;
    const double* d_src = src[m];
    if (!on_device) {                                          // host arrays land in the staging buffer; the caller's array is free on return
      const size_t bytes = (size_t)nnz[m] * (per_scenario ? (size_t)nscen : 1) * sizeof(double);
      HIPCHK(ctx, hipMemcpyAsync(d_stage, src[m], bytes, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      d_src = d_stage;
    }
    if (int rc = enqueue_plant_gather(ctx, st, d_src, from[m], nnz[m], nscen, per_scenario ? 1 : 0, dst[m])) return rc;
  }
  return 0;
}

}  // namespace sls
