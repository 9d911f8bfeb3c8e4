// sls_column_ops.h — what the column kernels of ñx ≤ 32 … 64 states do around their factorisations, where it can exist once: the
// one-wave and two-wave kernels (sls_wave_kernel.hip) and the four-wave kernel's plan-time prepare kernel
// (sls_twisted4_kernel.hip) gather the same per-lane lists of Ã and B̃ and scale the same Tikhonov shift, and the first two
// multiply by a column-layout block the same way.  Everything is forced inline and takes plain pointers and integers.  A kernel
// uses a piece only where its register, AGPR and scratch counts stay what they were with the text written out in its body
// (profiles/column_ops_resources.txt); DESIGN §5 says what stays a copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sls_device.h"
#include "sls_wave_util.h"

namespace sls {

// Row g of a CSR matrix → this lane's list: the stored non-zeros whose column lies in the index set `set` (ascending, ns long),
// as (local index, value) at [entry·stride + lane], in CSR order, at most cap of them.  DENSE: the values also go to
// dense[local index] (the lane's row of B̃'s image).  Returns the count; the maximum over the wave is the caller's.
template <bool DENSE = false>
__device__ __forceinline__ int gather_list(const int32_t* rowptr, const int32_t* colidx, const double* val, int g, const int32_t* set,
                                           int ns, int cap, int stride, int lane, int32_t* out_c, double* out_v, double* dense = nullptr) {
  int cnt = 0;
  for (int e = rowptr[g]; e < rowptr[g + 1]; ++e) {
    const double v = val[e];
    const int loc = (v != 0.0) ? wbsearch(set, ns, colidx[e]) : -1;
    if (loc >= 0 && cnt < cap) {
      out_c[cnt * stride + lane] = loc; out_v[cnt * stride + lane] = v;
      if constexpr (DENSE) dense[loc] = v;
      ++cnt;
    }
  }
  return cnt;
}

// Tikhonov shift, the lane's share: the largest possible Schur diagonal of row `lane`, hx_i + Σ v²·h over its rows of Ã and B̃.
// δ = delta_rel · (maximum over the wave) — the reduction and the product are the caller's.
template <int NPL>
__device__ __forceinline__ double tikhonov_scale(int lane, int n, const double* hx, const double* hu, const int32_t* arow_c,
                                                 const double* arow_v, int nzA, const int32_t* brow_c, const double* brow_v, int nzB) {
  double sc = 0.0;
  if (lane < n) {
    sc = hx[lane];
    for (int e = 0; e < nzA; ++e) { const double v = arow_v[e * NPL + lane]; sc = __builtin_fma(v * v, hx[arow_c[e * NPL + lane]], sc); }
    for (int e = 0; e < nzB; ++e) { const double v = brow_v[e * NPL + lane]; sc = __builtin_fma(v * v, hu[brow_c[e * NPL + lane]], sc); }
  }
  return sc;
}

// Pᵀ·y for a block in the column layout (lane (h, j) holds rows HS·r + h of column j), y read from LDS: four accumulators,
// then the sum over the row groups.  Entry j of the product, in every lane of column j.
template <int NPL, int RPL>
__device__ __forceinline__ double matvec_columns(const double (&Pk)[RPL], const double* y, int h) {
  constexpr int HS = 64 / NPL;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const double yr = y[HS * r + h];
    if ((r & 3) == 0) a0 = __builtin_fma(Pk[r], yr, a0);
    else if ((r & 3) == 1) a1 = __builtin_fma(Pk[r], yr, a1);
    else if ((r & 3) == 2) a2 = __builtin_fma(Pk[r], yr, a2);
    else a3 = __builtin_fma(Pk[r], yr, a3);
  }
  double part = (a0 + a1) + (a2 + a3);
  if (HS >= 2) part = xsum32(part);
  if (HS >= 4) part = xsum16(part);
  return part;
}

}  // namespace sls
