// sls_update.hip — new values of A / B2 for a resident plan (sls_plan_update_plant).
//
// A plan keeps the operator four times (A, Aᵀ, B2, B2ᵀ as CSR value arrays next to index arrays that depend on the pattern only).
// operator_update_kernel rewrites the value arrays in one grid-stride pass over the nnz(A) + nnz(B2) entries of the caller's CSC
// nzval arrays: a coalesced load of the new value, the finite rule and the zero rule, a coalesced store into the
// transpose's array — which is the CSC order itself — and a scattered store through the value map into the row-ordered array.
// An entry that breaks a rule is left as it was and counted (one ordinary global atomic per thread that saw any).  Not measured on
// its own: a few thousand entries, launch-bound at every shape the project benchmarks.
//
// weights_update_kernel (sls_plan_update_weights) sits beside it: new diagonals of C1 / D12 for a plan built with
// SLS_PLAN_WEIGHTS_UPDATABLE.  Part one, one wave per subproblem with a record: the lanes stride over the ñx + ñu local
// variables, read the variable's global index and its new value, and store hinv = 1 / (b²·v² + ridge) — weight_record of
// sls_weights.h, uncontracted, the bits fill_range gives — into the record; a lane whose store changes bits marks the subproblem
// dirty when tracking is on.  Part two, grid-stride over the Nx + Nu values: coalesced stores into the plan's current
// diagonals, and the count of refused values (one ordinary global atomic per thread that saw any).  Both parts decide with
// weight_value_ok, so a refused value is written nowhere.  Launch-bound like the operator update.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sls_device.h"
#include "sls_weights.h"

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

__global__ __launch_bounds__(kUpdBlock) void weights_update_kernel(const WeightsUpdateParams p) {
  constexpr int kWaves = kUpdBlock / 64;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  for (int64_t q = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); q < p.nsub; q += nwaves) {
    const SubDesc sd = p.subs[q];
    if (sd.has_w != 1) continue;
    const double b2 = p.b2[sd.out_index];
    bool changed = false;
    for (int32_t i = lane; i < sd.n + sd.m; i += 64) {
      const bool isx = i < sd.n;
      const double* src = isx ? p.new_c1 : p.new_d12;
      if (!src) continue;
      const int64_t loc = isx ? p.idx_pool[sd.off_sx + i] : p.idx_pool[sd.off_su + (i - sd.n)];
      const int64_t g = isx ? loc : p.Nx + loc;
      const double v = src[loc];
      const double r = p.ridge ? p.ridge[g] : 0.0;
      if (!weight_value_ok(v, p.owner[g], r)) continue;
      const double h = weight_record(b2, v, r);
      double* dst = p.w_pool + sd.off_w + i;
      if (__double_as_longlong(*dst) != __double_as_longlong(h)) { *dst = h; changed = true; }
    }
    if (changed && p.dirty) p.dirty[sd.out_index] = 1;
  }
  const int64_t n = p.Nx + p.Nu;
  const int64_t stride = (int64_t)gridDim.x * kUpdBlock;
  unsigned long long refused = 0;
  for (int64_t k = (int64_t)blockIdx.x * kUpdBlock + threadIdx.x; k < n; k += stride) {
    const bool isx = k < p.Nx;
    const double* src = isx ? p.new_c1 : p.new_d12;
    if (!src) continue;
    const double v = src[isx ? k : k - p.Nx];
    if (!weight_value_ok(v, p.owner[k], p.ridge ? p.ridge[k] : 0.0)) { ++refused; continue; }
    p.diag[k] = v;
  }
  if (refused) atomicAdd(p.rejected, refused);
}

}  // namespace

hipError_t launch_weights_update(const WeightsUpdateParams& p, hipStream_t st) {
  if (p.nsub <= 0 && p.Nx + p.Nu <= 0) return hipSuccess;
  const int64_t by_sub = ((int64_t)p.nsub + kUpdBlock / 64 - 1) / (kUpdBlock / 64), by_val = (p.Nx + p.Nu + kUpdBlock - 1) / kUpdBlock;
  const int grid = (int)std::min<int64_t>(std::max<int64_t>(std::max(by_sub, by_val), 1), 1024);
  hipLaunchKernelGGL(weights_update_kernel, dim3(grid), dim3(kUpdBlock), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_operator_update(const OperatorUpdateParams& p, hipStream_t st) {
  const int64_t n = p.nnzA + p.nnzB;
  if (n <= 0) return hipSuccess;
  const int grid = (int)std::min<int64_t>((n + kUpdBlock - 1) / kUpdBlock, 1024);
  hipLaunchKernelGGL(operator_update_kernel, dim3(grid), dim3(kUpdBlock), 0, st, p);
  return hipGetLastError();
}

}  // namespace sls
