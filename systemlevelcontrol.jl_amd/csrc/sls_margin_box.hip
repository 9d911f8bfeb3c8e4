// sls_margin_box.hip — worst-case 𝓛₁ margin of a resident Φ over a box of plants: the device pass behind sls_margin_box_run.
//
// Semantics, the active lists, the value of a vertex and the summation order: sls_margin_box.h.  Two launches:
//   margin_box_rows_kernel    one wave (one block of 64) per (row i, scenario s), a shape that depends on neither nscen nor the
//                             other scenarios.  An exact row (b ≤ kMarginBoxMaxBits active coefficients) goes through its list
//                             in chunks of 64 entries:
//                               phase A  lane l takes entry 64·c + l, evaluates d⁰ (margin_entry_signed) and the b factors φ_b —
//                                        the binary searches, once per entry and not once per vertex — and parks them in LDS,
//                                        11 doubles per entry (stride 22 banks: neither the writes nor the reads below conflict);
//                               phase B  lanes = (slot q, vertex lane vl), lane = 8·q + vl as in margin_sums_kernel.  A lane
//                                        owns R = 1, 2, 4 or 8 vertices (2^b ≤ 8·R; 64 vertices a pass at most), walks the chunk's
//                                        entries q, q + 8, … — eight distinct LDS addresses per read, broadcast to the vertex
//                                        lanes — and keeps one running sum per vertex in registers.
//                             After the last chunk the xor tree over q closes the eight slots of every vertex (margin_slot_sum's
//                             order), margin_report maps NaN to +inf, and the largest sum with the lowest code wins: over the
//                             lane's registers, over the vertex lanes, over the passes.  Rows with more than 64 vertices take
//                             2^b / 64 passes and repeat phase A in each (b = 10: 16 passes).
//                             A bound row (b > kMarginBoxMaxBits) needs no LDS: lanes = (slot q, column lane), column 0 is
//                             Σ|d⁰| and column 1 + b is Σ|φ_b|, eight columns a pass, each closed by the same tree; then
//                             acc = fma(ρ_b, Σ|φ_b|, acc) in ascending b.
//   margin_box_totals_kernel  one wave per chunk of 8 scenarios: the maximum over the rows.
// Nothing is allocated, nothing waits, no floating-point atomics.
#include <hip/hip_runtime.h>

#include "sls_margin_box.h"
#include "sls_wave_util.h"

namespace {

using sls::MarginBoxParams;

constexpr int kChunk = 64;                                  // entries parked at a time
constexpr int kStride = sls::kMarginBoxMaxBits + 1;         // doubles per parked entry: d⁰, φ_0 … φ_9

// the exact path of one (row, scenario); R vertices per lane.  perm: the row's list, n entries; ent: its nb active coefficients
template <int R>
__device__ __forceinline__ void box_exact_row(const MarginBoxParams& bp, const int32_t* __restrict__ perm, int32_t n,
                                              const int32_t* __restrict__ ent, int nb, long long sc, double* park, const double* rho,
                                              double& best, int& best_code) {
  constexpr int SQ = sls::kMarginSumSlots;
  const sls::MarginParams& p = bp.p;
  const int lane = threadIdx.x, q = lane / SQ, vl = lane % SQ;
  const int npass = R < 8 ? 1 : ((1 << nb) + 63) >> 6;         // R < 8: the row's 2^nb ≤ 8·R vertices fit one pass
  best = -1.0; best_code = 0;
  for (int pass = 0; pass < npass; ++pass) {
    double s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = 0.0;
    for (int32_t base = 0; base < n; base += kChunk) {
      __syncthreads();                                        // the previous chunk has been read
      if (base + lane < n) {                                  // phase A
        const int32_t d = perm[base + lane];
        const int32_t j = p.def_col[d], key = p.def_key[d];
        double* mine = park + lane * kStride;
        mine[0] = sls::margin_entry_signed(p.v, j, key, p.def_start[d], sc);
        for (int b = 0; b < nb; ++b) {
          double phi;
          mine[1 + b] = sls::margin_box_factor(p.v, bp.b.nnzA, ent[b], j, key, phi) ? phi : 0.0;
        }
      }
      __syncthreads();
      const int cnt = min(kChunk, n - base);                  // phase B
      for (int e = q; e < cnt; e += SQ) {
        const double* at = park + e * kStride;
        double v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = at[0];
        for (int b = 0; b < nb; ++b) {
          const double ph = at[1 + b], rb = rho[b];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int code = pass * (8 * R) + r * 8 + vl;
            v[r] = fma((code >> b) & 1 ? -rb : rb, ph, v[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += fabs(v[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {                             // the slots of every vertex, then the lane's best in ascending code
      s[r] = sls::lane_group_sum<SQ>(s[r]);
      const double val = sls::margin_report(s[r]);
      if (val > best) { best = val; best_code = pass * (8 * R) + r * 8 + vl; }
    }
  }
#pragma unroll
  for (int off = 1; off < SQ; off <<= 1) {                    // over the vertex lanes: the larger sum, the lower code on a tie
    const double ov = __shfl_xor(best, off, 64);
    const int oc = __shfl_xor(best_code, off, 64);
    if (ov > best || (ov == best && oc < best_code)) { best = ov; best_code = oc; }
  }
}

__global__ void __launch_bounds__(64) margin_box_rows_kernel(MarginBoxParams bp, double* __restrict__ row_wc,
                                                             long long* __restrict__ row_vertex) {
  constexpr int SQ = sls::kMarginSumSlots, MB = sls::kMarginBoxMaxBits;
  __shared__ double park[kChunk * kStride];
  __shared__ double rho[MB];
  const sls::MarginParams& p = bp.p;
  const long long ns = p.v.nscen;
  const long long w = blockIdx.x;                             // grid = Nx·nscen exactly
  const int row = (int)(w / ns);
  const long long sc = w - (long long)row * ns;
  const int lane = threadIdx.x, q = lane / SQ, vl = lane % SQ;
  const int32_t* __restrict__ perm = p.row_perm + p.row_ptr[row];
  const int32_t n = p.row_ptr[row + 1] - p.row_ptr[row];
  const int32_t* __restrict__ ent = bp.b.act_ent + bp.b.act_ptr[row];
  const int nb = bp.b.act_ptr[row + 1] - bp.b.act_ptr[row];
  double out;
  long long code;
  if (nb <= MB) {
    if (lane < nb) rho[lane] = sls::margin_box_radius(bp.b, ent[lane], ns, sc);
    double best; int bc;                                      // the first barrier of the chunk loop orders rho; a row without
    if (nb <= 3) box_exact_row<1>(bp, perm, n, ent, nb, sc, park, rho, best, bc);   // entries never reads it
    else if (nb == 4) box_exact_row<2>(bp, perm, n, ent, nb, sc, park, rho, best, bc);
    else if (nb == 5) box_exact_row<4>(bp, perm, n, ent, nb, sc, park, rho, best, bc);
    else box_exact_row<8>(bp, perm, n, ent, nb, sc, park, rho, best, bc);
    out = best; code = bc & ((1 << nb) - 1);                  // codes beyond 2^nb repeat the lower ones and never win a tie
  } else {
    double acc = 0.0;
    for (int c0 = 0; c0 <= nb; c0 += SQ) {                    // column 0: Σ|d⁰|; column 1 + b: Σ|φ_b|
      const int c = c0 + vl;
      double s = 0.0;
      if (c <= nb)
        for (int32_t e = q; e < n; e += SQ) {
          const int32_t d = perm[e];
          double val = 0.0;
          if (c == 0) val = fabs(sls::margin_entry_signed(p.v, p.def_col[d], p.def_key[d], p.def_start[d], sc));
          else { double phi; if (sls::margin_box_factor(p.v, bp.b.nnzA, ent[c - 1], p.def_col[d], p.def_key[d], phi)) val = fabs(phi); }
          s += val;
        }
      s = sls::lane_group_sum<SQ>(s);
      for (int k = 0; k < SQ; ++k) {                          // lanes 0 … 7 hold the eight columns of this pass
        const double col = __shfl(s, k, 64);
        const int cc = c0 + k;
        if (cc == 0) acc = col;
        else if (cc <= nb) acc = fma(sls::margin_box_radius(bp.b, ent[cc - 1], ns, sc), col, acc);
      }
    }
    out = sls::margin_report(acc); code = -1;
  }
  if (lane == 0) { row_wc[(long long)row * ns + sc] = out; row_vertex[(long long)row * ns + sc] = code; }
}

// One wave per chunk of kMarginSumScen scenarios; fmax of non-negative numbers is exact in any order
__global__ void __launch_bounds__(64) margin_box_totals_kernel(const double* __restrict__ row_wc, int Nx, long long ns,
                                                               double* __restrict__ totals) {
  constexpr int SS = sls::kMarginSumScen, SQ = sls::kMarginSumSlots;
  const int ls = threadIdx.x % SS, q = threadIdx.x / SS;
  const long long scen = (long long)blockIdx.x * SS + ls;
  const bool live = scen < ns;
  const long long s = live ? scen : 0;
  double l1 = 0.0;
  for (int i = q; i < Nx; i += SQ) l1 = fmax(l1, row_wc[(long long)i * ns + s]);
#pragma unroll
  for (int off = 32; off >= SS; off >>= 1) l1 = fmax(l1, __shfl_xor(l1, off, 64));
  if (q == 0 && live) totals[scen] = l1;
}

}  // namespace

namespace sls {

hipError_t launch_margin_box(const MarginBoxParams& bp, hipStream_t st, double* d_row_wc, long long* d_row_vertex, double* d_totals) {
  const long long ns = bp.p.v.nscen, nwave = (long long)bp.p.v.Nx * ns;
  if (nwave > 0) {
    hipLaunchKernelGGL(margin_box_rows_kernel, dim3((unsigned)nwave), dim3(64), 0, st, bp, d_row_wc, d_row_vertex);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(margin_box_totals_kernel, dim3((unsigned)((ns + kMarginSumScen - 1) / kMarginSumScen)), dim3(64), 0, st, d_row_wc,
                     bp.p.v.Nx, ns, d_totals);
  return hipGetLastError();
}

}  // namespace sls
