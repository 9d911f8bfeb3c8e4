// sls_residual.hip — achievability residual of every column against the full plant, evaluated on the device from the written Φ
// (definition and conventions: sls_residual.h).
//
// A read-only pass of its own beside sls_objective.hip: no solve kernel is touched.  Two kernels:
//   residual_kernel         one 64-lane wave per subproblem, four independent waves per 256-thread block, no barrier, no LDS.
//                           A lane owns rows of s_x ∪ H(q) (position i < ñx: row s_x[i]; beyond: the halo list), i striding over
//                           the lanes, with the loop over t = 0 … T inside.  For its row it gathers along the row of A_csr, then
//                           of B_csr, in ascending CSR position with fma; a global column index becomes a position in the
//                           ascending s_x / s_u list by binary search, and a stored column outside the set contributes nothing.
//                           The searches do not depend on t: the first eight entries of a row that survive them stay in
//                           registers (slot and value), so a time step is a handful of independent mask / destination / value
//                           loads; longer rows search again for the rest.  No row is owned by two lanes and nothing is
//                           scattered; every operand is re-read through L2.
//   residual_total_kernel   one workgroup takes the two maxima over the subproblems.
// Every lane accumulates in a fixed order (its rows ascending, t inside) and the wave reduces with a fixed tree (no floating-point atomics), and the
// packed and mask-order tables name the same values in the same positions: the results are bit-identical from call to call and
// between the two layouts.
#include <hip/hip_runtime.h>

#include "sls_residual.h"
#include "sls_wave_util.h"

namespace sls {

namespace {

constexpr int kResBlock = 256;
constexpr int kResCache = 8;         // entries of a row kept in registers across the time steps

// maximum of non-negative values (a NaN has already become +inf: resid_max); not wave_max_f64 of sls_wave_util.h, which is fmax
__device__ __forceinline__ double wave_resid_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = resid_max(v, __shfl_xor(v, off));
  return v;
}

// position of `key` in the ascending list s[0 .. n), or -1
__device__ __forceinline__ int find_sorted(const int32_t* __restrict__ s, int n, int32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && s[lo] == key) ? lo : -1;
}

__global__ __launch_bounds__(kResBlock) void residual_kernel(ResidualParams p) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (kResBlock / 64) + (threadIdx.x >> 6);      // wave-uniform
  if (q >= p.nsub) return;
  const SubDesc sd = p.subs[q];
  const int n = sd.n, m = sd.m, nm = n + m, T = p.T;
  const int32_t* __restrict__ sx = p.idx_pool + sd.off_sx;
  const int32_t* __restrict__ su = p.idx_pool + sd.off_su;
  const uint8_t* __restrict__ mk = p.mask_pool + sd.off_mask;
  const int32_t* __restrict__ ds = p.dest + sd.off_dest;
  const double* __restrict__ vals = p.values;
  const int32_t c = p.sub_col[sd.out_index];
  const int64_t hb = p.halo_ptr[q];
  const int nh = (int)(p.halo_ptr[q + 1] - hb);
  const int32_t* __restrict__ hr = p.halo_rows + hb;
  // one slot of the column: a stored-false mask entry or a destination < 0 reads as 0.0
  auto zat = [&](int t, int i) -> double {
    const int64_t e = (int64_t)t * nm + i;
    const uint8_t on = mk[e];
    const int32_t d = ds[e];
    return (on && d >= 0) ? vals[d] : 0.0;
  };
  double mx = 0.0, hmx = 0.0, l1 = 0.0;
  for (int i = lane; i < n + nh; i += 64) {
    const bool local = i < n;
    const int32_t r = local ? sx[i] : hr[i - n];
    const int a0 = p.A_rowptr[r], a1 = p.A_rowptr[r + 1], b0 = p.B_rowptr[r], b1 = p.B_rowptr[r + 1];
    // The row's products do not depend on t: its first kResCache stored entries whose column lies in the set (A's in CSR order,
    // then B2's) keep their slot of the column and their value in registers; a longer row walks the rest from [ra, a1) and
    // [rb, b1) at every step, in the same order.
    int ek[kResCache];
    double ev[kResCache];
    int ne = 0, ra = a1, rb = b1;
    auto keep = [&](int k, double v) {
#pragma unroll
      for (int j = 0; j < kResCache; ++j)
        if (j == ne) { ek[j] = k; ev[j] = v; }
      ++ne;
    };
    for (int e = a0; e < a1; ++e) {
      const int k = find_sorted(sx, n, p.A_colidx[e]);
      if (k < 0) continue;
      if (ne == kResCache) { ra = e; rb = b0; break; }
      keep(k, p.A_val[e]);
    }
    if (ra == a1)
      for (int e = b0; e < b1; ++e) {
        const int k = find_sorted(su, m, p.B_colidx[e]);
        if (k < 0) continue;
        if (ne == kResCache) { rb = e; break; }
        keep(n + k, p.B_val[e]);
      }
    for (int t = 0; t <= T; ++t) {
      const double lhs = (local && t < T) ? zat(t, i) : 0.0;
      double rhs;
      if (t == 0) {
        rhs = (r == c) ? 1.0 : 0.0;
      } else {
        double z[kResCache];
#pragma unroll
        for (int j = 0; j < kResCache; ++j) z[j] = (j < ne) ? zat(t - 1, ek[j]) : 0.0;     // independent loads, all in flight
        rhs = 0.0;
#pragma unroll
        for (int j = 0; j < kResCache; ++j)
          if (j < ne) rhs = __builtin_fma(ev[j], z[j], rhs);
        for (int e = ra; e < a1; ++e) {
          const int k = find_sorted(sx, n, p.A_colidx[e]);
          if (k >= 0) rhs = __builtin_fma(p.A_val[e], zat(t - 1, k), rhs);
        }
        for (int e = rb; e < b1; ++e) {
          const int k = find_sorted(su, m, p.B_colidx[e]);
          if (k >= 0) rhs = __builtin_fma(p.B_val[e], zat(t - 1, n + k), rhs);
        }
      }
      const double d = lhs - rhs;
      mx = resid_max(mx, d);
      if (!local) hmx = resid_max(hmx, d);
      l1 += fabs(d);
    }
  }
  mx = wave_resid_max(mx);
  hmx = wave_resid_max(hmx);
  l1 = lane_group_sum<1>(l1);
  if (lane == 0) {
    p.res_inf[sd.out_index] = mx;
    p.halo_inf[sd.out_index] = hmx;
    p.res_l1[sd.out_index] = l1;
  }
}

// totals[0] = max res_inf, totals[1] = max res_l1 (a NaN sum counts as +inf)
__global__ __launch_bounds__(kResBlock) void residual_total_kernel(const double* __restrict__ res_inf, const double* __restrict__ res_l1,
                                                                   int n, double* __restrict__ totals) {
  __shared__ double red[2][kResBlock];
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = tid; i < n; i += kResBlock) { a = resid_max(a, res_inf[i]); b = resid_max(b, res_l1[i]); }
  red[0][tid] = a; red[1][tid] = b;
  __syncthreads();
#pragma unroll
  for (int s = kResBlock / 2; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] = resid_max(red[0][tid], red[0][tid + s]); red[1][tid] = resid_max(red[1][tid], red[1][tid + s]); }
    __syncthreads();
  }
  if (tid == 0) { totals[0] = red[0][0]; totals[1] = red[1][0]; }
}

}  // namespace

hipError_t launch_residual(const ResidualParams& p, double* d_totals, hipStream_t stream) {
  if (p.nsub <= 0) return hipSuccess;
  const int grid = (p.nsub + kResBlock / 64 - 1) / (kResBlock / 64);
  hipLaunchKernelGGL(residual_kernel, dim3(grid), dim3(kResBlock), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (d_totals) {
    hipLaunchKernelGGL(residual_total_kernel, dim3(1), dim3(kResBlock), 0, stream, p.res_inf, p.res_l1, p.nsub, d_totals);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sls
