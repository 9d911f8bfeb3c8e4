// sls_gradient.hip — gradient of the 𝓗₂ cost in the stored entries of A and B2 and in the LQR diagonals, on the device, from the
// multipliers the one-wave kernel left in the plan's buffer and the written Φ (formulas and tables: sls_gradient.h).
//
// A pass of its own behind the execute.  Two kernels:
//   gradient_column_kernel   one 64-lane wave per subproblem.  λ (compact: (T+1)·ñx) and the column's z = (x, u) (T·(ñx+ñu), read
//                            through the mask and the destination table of the caller's layout, as objective_diag_kernel reads
//                            them) are staged in LDS when both fit, read through L2 when not — the same values in the same
//                            order either way.  A lane takes one listed entry at a time and runs ONE fma chain over k = 1 … T,
//                            scales by the column's factor and weight and stores to the entry's own contribution slot.  With
//                            weight derivatives asked for, the same wave forms Σ_t z² per variable into the weight slots.
//   gradient_owner_kernel    one thread per stored entry (and per weight): the sum of its slots in ascending subproblem order.
// No atomics: every slot has one writer and every owner one fixed order, so the result is bit-identical from call to call,
// between the two layouts and for multipliers of a full or a partial execute.
#include <hip/hip_runtime.h>

#include "../../include/sls_mi355x.h"
#include "sls_gradient.h"

namespace sls {

namespace {

constexpr int kGradOwnerBlock = 256;

__global__ __launch_bounds__(64) void gradient_column_kernel(GradientParams p, int lds_doubles) {
  extern __shared__ double gsh[];
  const int lane = threadIdx.x;
  const int q = blockIdx.x;                                               // subs is indexed by out_index
  const SubDesc sd = p.subs[q];
  const int n = sd.n, nm = sd.n + sd.m, T = p.T;
  const int64_t e0 = p.ent_ptr[q], e1 = p.ent_ptr[q + 1];
  const int st = p.status[q];
  const bool live = (st == SLS_COL_OK || st == SLS_COL_TRIVIAL) && !p.b_zero[q] && sd.has_w <= 1;
  double* wc = p.wcontrib ? p.wcontrib + p.w_base[q] : nullptr;
  if (!live) {                                                            // contributes 0 (its multipliers may be anything)
    for (int64_t e = e0 + lane; e < e1; e += 64) p.contrib[e] = 0.0;
    if (wc) for (int i = lane; i < nm; i += 64) wc[i] = 0.0;
    return;
  }
  const double cw = p.col_weight ? p.col_weight[q] : 1.0;
  const double fac = cw * column_factor(sd.has_w, p.obj_pool[2 * q]);
  const uint8_t* __restrict__ mk = p.mask_pool + sd.off_mask;
  const int32_t* __restrict__ ds = p.dest + sd.off_dest;
  const double* __restrict__ vals = p.values;
  const double* __restrict__ muq = p.mu + (int64_t)q * mu_slot_doubles(T);
  auto zglobal = [&](int s) -> double {                                  // s = t·(ñx+ñu) + i
    const uint8_t on = mk[s];
    const int32_t d = ds[s];
    return (on && d >= 0) ? vals[d] : 0.0;
  };
  const int nlam = (T + 1) * n, nz = T * nm;
  const bool staged = nlam + nz <= lds_doubles;                           // wave-uniform
  double* lam_s = gsh;
  double* z_s = gsh + nlam;
  if (staged) {
    for (int idx = lane; idx < nlam; idx += 64) { const int k = idx / n; lam_s[idx] = muq[k * kMuLd + (idx - k * n)]; }
    for (int idx = lane; idx < nz; idx += 64) z_s[idx] = zglobal(idx);
    __syncthreads();
  }
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t pos = p.ent[3 * e], a = p.ent[3 * e + 1], b = p.ent[3 * e + 2];
    const int i = pos < p.nnzA ? b : n + b;
    double acc = 0.0;
    if (staged) {
      for (int k = 1; k <= T; ++k) acc = __builtin_fma(lam_s[k * n + a], z_s[(k - 1) * nm + i], acc);
    } else {
      for (int k = 1; k <= T; ++k) acc = __builtin_fma(muq[k * kMuLd + a], zglobal((k - 1) * nm + i), acc);
    }
    p.contrib[e] = fac * acc;
  }
  if (wc) {
    const double wf = cw * p.b2[q];
    for (int i = lane; i < nm; i += 64) {
      double acc = 0.0;
      for (int t = 0; t < T; ++t) { const double z = staged ? z_s[t * nm + i] : zglobal(t * nm + i); acc = __builtin_fma(z, z, acc); }
      wc[i] = wf * acc;
    }
  }
}

// out[o] = scale_o · Σ slots, o < n0 + n1; owners below n0 go to out0, the others to out1 (either may be NULL); diag != NULL:
// scale_o = 2·diag[o] (the weight derivatives), else 1
__global__ __launch_bounds__(kGradOwnerBlock) void gradient_owner_kernel(const int64_t* __restrict__ ptr, const int64_t* __restrict__ slot,
                                                                        const double* __restrict__ contrib, const double* __restrict__ diag,
                                                                        int64_t n0, int64_t n1, double* __restrict__ out0,
                                                                        double* __restrict__ out1) {
  const int64_t o = (int64_t)blockIdx.x * kGradOwnerBlock + threadIdx.x;
  if (o >= n0 + n1) return;
  double* out = o < n0 ? out0 : out1;
  if (!out) return;
  double s = 0.0;
  for (int64_t w = ptr[o]; w < ptr[o + 1]; ++w) s += contrib[slot[w]];
  if (diag) s = 2.0 * diag[o] * s;
  out[o < n0 ? o : o - n0] = s;
}

}  // namespace

hipError_t launch_gradient(const GradientParams& p, int lds_doubles, hipStream_t stream) {
  if (p.nsub <= 0) return hipSuccess;
  hipLaunchKernelGGL(gradient_column_kernel, dim3(p.nsub), dim3(64), (size_t)lds_doubles * sizeof(double), stream, p, lds_doubles);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t nent = p.nnzA + p.nnzB;
  if (nent > 0 && (p.gA || p.gB2)) {
    hipLaunchKernelGGL(gradient_owner_kernel, dim3((unsigned)((nent + kGradOwnerBlock - 1) / kGradOwnerBlock)), dim3(kGradOwnerBlock), 0, stream,
                       p.inv_ptr, p.inv_slot, p.contrib, (const double*)nullptr, p.nnzA, p.nnzB, p.gA, p.gB2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int64_t nvar = p.Nx + p.Nu;
  if (p.wcontrib && nvar > 0) {
    hipLaunchKernelGGL(gradient_owner_kernel, dim3((unsigned)((nvar + kGradOwnerBlock - 1) / kGradOwnerBlock)), dim3(kGradOwnerBlock), 0, stream,
                       p.winv_ptr, p.winv_slot, p.wcontrib, p.diag, p.Nx, p.Nu, p.gc1, p.gd12);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sls
