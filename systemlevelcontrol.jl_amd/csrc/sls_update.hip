// sls_update.hip — new values of A / B2 for a resident plan (sls_plan_update_plant).
//
// A plan keeps the operator four times (A, Aᵀ, B2, B2ᵀ as CSR value arrays next to index arrays that depend on the pattern only).
// operator_update_kernel rewrites the value arrays in one grid-stride pass over the nnz(A) + nnz(B2) entries of the caller's CSC
// nzval arrays: a coalesced load of the new value, the finite rule and the zero rule, a coalesced store into the
// transpose's array — which is the CSC order itself — and a scattered store through the value map into the row-ordered array.
// An entry that breaks a rule is left as it was and counted (one ordinary global atomic per thread that saw any).  Not measured on
// its own: a few thousand entries, launch-bound at every shape the project benchmarks.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sls_device.h"

namespace sls {

namespace {

constexpr int kUpdBlock = 256;

__global__ __launch_bounds__(kUpdBlock) void operator_update_kernel(const OperatorUpdateParams p) {
  const int64_t n = p.nnzA + p.nnzB;
  const int64_t stride = (int64_t)gridDim.x * kUpdBlock;
  unsigned long long refused = 0;
  for (int64_t k = (int64_t)blockIdx.x * kUpdBlock + threadIdx.x; k < n; k += stride) {
    const bool isA = k < p.nnzA;
    const double* src = isA ? p.newA : p.newB;
    if (!src) continue;
    const int64_t j = isA ? k : k - p.nnzA;
    const double v = src[j];
    // finite: |v| ≤ DBL_MAX is false for ±inf and for a NaN
    const bool finite = (v < 0.0 ? -v : v) <= 1.7976931348623157e308;
    if (!finite || (p.zero[k] && v != 0.0)) { ++refused; continue; }
    (isA ? p.At_val : p.Bt_val)[j] = v;
    (isA ? p.A_val : p.B_val)[p.row_pos[k]] = v;
  }
  if (refused) atomicAdd(p.rejected, refused);
}

}  // namespace

hipError_t launch_operator_update(const OperatorUpdateParams& p, hipStream_t st) {
  const int64_t n = p.nnzA + p.nnzB;
  if (n <= 0) return hipSuccess;
  const int grid = (int)std::min<int64_t>((n + kUpdBlock - 1) / kUpdBlock, 1024);
  hipLaunchKernelGGL(operator_update_kernel, dim3(grid), dim3(kUpdBlock), 0, st, p);
  return hipGetLastError();
}

}  // namespace sls
