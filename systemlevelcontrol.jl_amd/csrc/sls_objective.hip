// sls_objective.hip — objective value of every column, evaluated on the device from the written Φ (formulas: sls_objective.h).
//
// A pass of its own over the value array, after whatever kernels wrote it (the attached refinement included): the solve kernels
// are not touched.  Three kernels:
//   objective_diag_kernel     has_w = 0 / 1, both objectives.  One 64-lane wave per subproblem, four independent waves per
//                             256-thread block, no barrier.  Lanes stride over i < ñx+ñu inside a loop over t: mask byte, int32
//                             destination (the table of the caller's layout), gathered value — destinations of one column and
//                             one t ascend in the mask's CSC order, so the gathers coalesce.  1/hinv and 2g sit in registers
//                             while ñx+ñu ≤ 64·kObjRegs, else they are re-read (L2-resident).
//   objective_general_kernel  has_w = 2 (dense Hessian) and 3 (coupled group, up to 64 columns): one 256-thread workgroup per
//                             work item; z_t of every column staged in LDS when nc·(ñx+ñu) fits, read through L2 when not.
//   objective_total_kernel    one workgroup sums col_objective in a fixed order.
// Every partial is accumulated in a fixed (t, i) order and reduced with a fixed tree (no floating-point atomics), and the
// packed and mask-order tables name the same values in the same positions: the results are bit-identical from call to call
// and between the two layouts.
#include <hip/hip_runtime.h>

#include "sls_objective.h"
#include "sls_wave_util.h"

namespace sls {

namespace {

constexpr int kObjRegs = 4;          // weight registers per lane of the diagonal build
constexpr int kObjBlock = 256;

// sum over the 256 threads of a workgroup, fixed tree; result in every thread
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kObjBlock / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

template <bool SON>
__global__ __launch_bounds__(kObjBlock) void objective_diag_kernel(ObjectiveParams p) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (kObjBlock / 64) + (threadIdx.x >> 6);      // wave-uniform
  if (q >= p.nsub) return;
  const SubDesc sd = p.subs[q];
  if (sd.has_w == 2 || sd.has_w == 3) return;                            // the general build's
  const int64_t oi = sd.out_index;
  if (sd.has_w == 4) {                                                    // member of a coupled group: its first column carries the value
    if (lane == 0) p.col_objective[oi] = 0.0;
    return;
  }
  const int nm = sd.n + sd.m, T = p.T;
  const double scale = p.obj_pool[2 * oi], c0 = p.obj_pool[2 * oi + 1];
  const uint8_t* __restrict__ mk = p.mask_pool + sd.off_mask;
  const int32_t* __restrict__ ds = p.dest + sd.off_dest;
  const double* __restrict__ vals = p.values;
  const bool hw = sd.has_w == 1;
  const double* hinv = p.w_pool + sd.off_w;
  const double* g = hinv + nm;
  double acc = 0.0;
  // one slot of the column: mask and destination are read unconditionally (independent loads), the value only where free
  auto slot = [&](int t, int i, double w, double g2, double& into) {
    const int64_t e = (int64_t)t * nm + i;
    const uint8_t on = mk[e];
    const int32_t d = ds[e];
    const double z = (on && d >= 0) ? vals[d] : 0.0;
    into = __builtin_fma(w, z * z, into);
    if (!SON) into = __builtin_fma(g2, z, into);
  };
  // one time step of the column; the sum of norms needs the wave's sum per step (a cross-lane operation: no unrolling across it)
  auto norm_of = [&](double qt) { qt = lane_group_sum<1>(qt); return sqrt(hw ? qt : scale * qt); };
  if (nm <= 64 * kObjRegs) {
    double wr[kObjRegs], gr[kObjRegs];
#pragma unroll
    for (int j = 0; j < kObjRegs; ++j) {
      const int i = lane + 64 * j;
      wr[j] = (hw && i < nm) ? 1.0 / hinv[i] : 1.0;
      gr[j] = (hw && i < nm) ? 2.0 * g[i] : 0.0;
    }
    auto step = [&](int t, double& into) {
#pragma unroll
      for (int j = 0; j < kObjRegs; ++j) {
        const int i = lane + 64 * j;
        if (i < nm) slot(t, i, wr[j], gr[j], into);
      }
    };
    if constexpr (SON) {
      for (int t = 0; t < T; ++t) { double qt = 0.0; step(t, qt); acc += norm_of(qt); }
    } else {
#pragma unroll 4
      for (int t = 0; t < T; ++t) step(t, acc);          // the loads of four steps in flight, the adds in (t, i) order
    }
  } else {
    for (int t = 0; t < T; ++t) {
      double qt = 0.0;
      for (int i = lane; i < nm; i += 64) slot(t, i, hw ? 1.0 / hinv[i] : 1.0, hw ? 2.0 * g[i] : 0.0, SON ? qt : acc);
      if constexpr (SON) acc += norm_of(qt);
    }
  }
  double val;
  if (SON) val = acc + c0;                                               // the same bits in every lane already
  else { acc = lane_group_sum<1>(acc); val = hw ? acc + c0 : scale * acc + c0; }
  if (lane == 0) p.col_objective[oi] = val;
}

__global__ __launch_bounds__(kObjBlock) void objective_general_kernel(ObjectiveParams p, int lds_doubles) {
  extern __shared__ double zs[];                                         // z_t of the work item's columns: [nc][nm], when it fits
  __shared__ double red[kObjBlock];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = p.gen_list[blockIdx.x];
  const SubDesc sd = p.subs[q];
  const int nm = sd.n + sd.m, T = p.T;
  const GeneralRecord R = parse_general_record(p.w_pool + sd.off_w, nm, sd.has_w == 3);
  const int nc = R.nc;
  const int ntot = nc * nm;                                              // ≤ 64 · (ñx + ñu): far below 2^31
  const bool staged = ntot <= lds_doubles;
  const double* __restrict__ vals = p.values;
  auto zglobal = [&](int c, int t, int i) -> double {
    const int64_t e = p.subs[q + c].off_mask + (int64_t)t * nm + i;      // off_dest == off_mask
    const uint8_t on = p.mask_pool[e];
    const int32_t d = p.dest[e];
    return (on && d >= 0) ? vals[d] : 0.0;
  };
  double acc = 0.0;
  for (int t = 0; t < T; ++t) {
    if (staged) {
      for (int idx = tid; idx < ntot; idx += kObjBlock) { const int c = idx / nm; zs[idx] = zglobal(c, t, idx - c * nm); }
      __syncthreads();
    }
    auto zget = [&](int c, int i) -> double { return staged ? zs[c * nm + i] : zglobal(c, t, i); };
    if (nc == 1) {
      // single dense column (M = 1): a z-row of b·W per thread
      for (int zr = tid; zr < R.nz; zr += kObjBlock) {
        double y = 0.0;
        for (int e = (int)R.rp[zr]; e < (int)R.rp[zr + 1]; ++e) y = __builtin_fma(R.rv[e], zget(0, (int)R.ri[e]), y);
        acc = __builtin_fma(y, y, acc);
      }
    } else {
      // coupled group: a z-row per wave, lane c holds (W z_c)[row]; yᵀ M y through the wave (nc ≤ 64)
      for (int zr = wave; zr < R.nz; zr += kObjBlock / 64) {
        double y = 0.0;
        if (lane < nc)
          for (int e = (int)R.rp[zr]; e < (int)R.rp[zr + 1]; ++e) y = __builtin_fma(R.rv[e], zget(lane, (int)R.ri[e]), y);
        double r = 0.0;
        for (int c2 = 0; c2 < nc; ++c2) {
          const double y2 = __shfl(y, c2);
          const double mcc = lane < nc ? R.M[lane * nc + c2] : 0.0;
          r = __builtin_fma(mcc, y2, r);
        }
        acc = __builtin_fma(y, r, acc);
      }
    }
    for (int idx = tid; idx < ntot; idx += kObjBlock) {
      const int c = idx / nm, i = idx - c * nm;
      const double z = zget(c, i);
      const double g = p.w_pool[p.subs[q + c].off_w + nm + i];
      acc += 2.0 * g * z + R.ridge[i] * (z * z);
    }
    if (staged) __syncthreads();                                         // everyone done with zs before the next t overwrites it
  }
  const double s = block_sum_f64(acc, red);
  if (tid == 0) p.col_objective[sd.out_index] = s + p.obj_pool[2 * sd.out_index + 1];
}

__global__ __launch_bounds__(kObjBlock) void objective_total_kernel(const double* __restrict__ col, int n, double* __restrict__ total) {
  __shared__ double red[kObjBlock];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += kObjBlock) a += col[i];
  const double s = block_sum_f64(a, red);
  if (threadIdx.x == 0) *total = s;
}

}  // namespace

hipError_t launch_objective(const ObjectiveParams& p, int lds_doubles, double* d_total, hipStream_t stream) {
  if (p.nsub <= 0) return hipSuccess;
  const int grid = (p.nsub + kObjBlock / 64 - 1) / (kObjBlock / 64);
  if (p.objective == 1) hipLaunchKernelGGL(objective_diag_kernel<true>, dim3(grid), dim3(kObjBlock), 0, stream, p);
  else hipLaunchKernelGGL(objective_diag_kernel<false>, dim3(grid), dim3(kObjBlock), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (p.ngen > 0) {
    hipLaunchKernelGGL(objective_general_kernel, dim3(p.ngen), dim3(kObjBlock), (size_t)lds_doubles * sizeof(double), stream, p, lds_doubles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (d_total) {
    hipLaunchKernelGGL(objective_total_kernel, dim3(1), dim3(kObjBlock), 0, stream, p.col_objective, p.nsub, d_total);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sls
