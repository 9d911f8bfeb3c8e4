// sls_norms.hip — closed-loop 𝓛₁ and 𝓗∞ norms of a resident Φ on the device: sls_norms_* of include/sls_mi355x.h.
//
// Operator, iteration and the per-entry arithmetic: sls_norms.h.  Frequencies play the part scenarios play in the controller
// (sls_controller.hip): one wave per line — a row of the row table in the forward pass, a column of the column table in the
// adjoint — and chunk of SCN frequencies, lanes = (entry slot le, frequency slot ls), lane = le·SCN + ls.  A pass reads 12 B per
// entry (value + key); x, the output and the twiddles stay in L2.
//
// Summation order.  SCN follows the number of frequencies of the CALL, and the sigma of a frequency must not depend on the call
// it sat in, so the order is the one of SCN = 1 whatever SCN is: 64 VIRTUAL entry slots, slot s sums the entries beg + s,
// beg + s + 64, … with four in flight, (a0 + a1) + (a2 + a3); the 64 slot sums are added by the xor butterfly 32, 16, … 1.  A lane
// owns the SCN slots le + k·NE (NE = 64/SCN): it runs them one after the other and adds them in the butterfly's order for the
// offsets ≥ NE (a binary counter over a stack of log₂SCN partial sums, held in registers), then the shuffles finish the offsets
// below NE.  a + b is commutative bit for bit, so every lane of a butterfly holds the same double and the result is the same
// for every SCN.  The 𝓛₁ pass is the SCN = 1 traversal with fabs.
//
// ‖·‖² per frequency: each wave leaves |out|² of its line, norms_norm2_kernel adds them over the lines in a fixed order (one
// block per frequency) and leaves 1/‖·‖ for the next forward pass to read, or sigma.  No floating-point atomics; no launch
// argument depends on device data; load, l1 and hinf allocate nothing, and only the fetch calls wait.
//
// 𝓗₂ shares and covariance (sls_norms.h): norms_h2_kernel is the 𝓛₁ traversal with fma(v, v, ·); norms_cov_kernel intersects the
// sorted row lists of a pair, one wave per pair, over a pattern the caller sets once (sls_norms_cov_pattern — the only call
// here besides the plan that allocates and waits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "../../include/sls_mi355x_debug.h"
#include "sls_internal.h"
#include "sls_norms.h"
#include "sls_object.h"
#include "sls_symbolic.h"
#include "sls_wave_util.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = 64 * kWavesPerBlock;

// both value orders in one launch: vals[k] = Φ[perm[k]]·w[k], k < 2·n (row order, then column order); w NULL = no weights
__global__ void norms_gather_kernel(const double* __restrict__ values, const int32_t* __restrict__ perm, const double* __restrict__ w,
                                    long long n2, double* __restrict__ vals) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n2) return;
  const double v = values[perm[k]];
  vals[k] = w ? v * w[k] : v;
}

struct L1Params {
  const int32_t* row_ptr; const int32_t* col_ptr;
  const double* vals;          // row order [n], then column order [n]
  long long n;
  int N, Nx;
  double* res;                 // plan-owned: row_l1 [N], col_l1 [Nx]
  double* row_out; double* col_out;   // the caller's, each may be NULL
};

// lines 0 … N−1: rows, N … N+Nx−1: columns
__global__ void __launch_bounds__(kBlock) norms_l1_kernel(L1Params p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int line = blockIdx.x * kWavesPerBlock + wave;
  if (line >= p.N + p.Nx) return;
  const bool col = line >= p.N;
  const int i = col ? line - p.N : line;
  const int32_t* ptr = col ? p.col_ptr : p.row_ptr;
  const double* vals = col ? p.vals + p.n : p.vals;
  const int beg = ptr[i], end = ptr[i + 1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int e = beg + lane;
  for (; e + 192 < end; e += 256) {
    a0 += fabs(vals[e]); a1 += fabs(vals[e + 64]); a2 += fabs(vals[e + 128]); a3 += fabs(vals[e + 192]);
  }
  for (; e < end; e += 64) a0 += fabs(vals[e]);
  const double s = sls::norms_l1_report(sls::lane_group_sum<1>((a0 + a1) + (a2 + a3)));
  if (lane != 0) return;
  p.res[line] = s;
  double* out = col ? p.col_out : p.row_out;
  if (out) out[i] = s;
}

// max over a [n] by one block; every thread returns it
__device__ double block_max(const double* a, int n, double* lds) {
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) m = fmax(m, a[i]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
}

// totals[0] = max row_l1, totals[1] = max col_l1 (the entries are ≥ 0 or +inf, never NaN)
__global__ void __launch_bounds__(kBlock) norms_l1_totals_kernel(const double* __restrict__ res, int N, int Nx, double* res_totals,
                                                                 double* out) {
  __shared__ double lds[kWavesPerBlock];
  const double m0 = block_max(res, N, lds), m1 = block_max(res + N, Nx, lds);
  if (threadIdx.x != 0) return;
  res_totals[0] = m0; res_totals[1] = m1;
  if (out) { out[0] = m0; out[1] = m1; }
}

// the 𝓛₁ pass with fma(v, v, ·) per entry: row_h2 [N], col_h2 [Nx] (sls_norms.h).  The lines, the slots and the order are
// those of norms_l1_kernel; the results take the 𝓛₁ slots of the plan-owned buffer (a fetch runs its own pass first).
__global__ void __launch_bounds__(kBlock) norms_h2_kernel(L1Params p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int line = blockIdx.x * kWavesPerBlock + wave;
  if (line >= p.N + p.Nx) return;
  const bool col = line >= p.N;
  const int i = col ? line - p.N : line;
  const int32_t* ptr = col ? p.col_ptr : p.row_ptr;
  const double* vals = col ? p.vals + p.n : p.vals;
  const int beg = ptr[i], end = ptr[i + 1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int e = beg + lane;
  for (; e + 192 < end; e += 256) {
    const double v0 = vals[e], v1 = vals[e + 64], v2 = vals[e + 128], v3 = vals[e + 192];
    a0 = fma(v0, v0, a0); a1 = fma(v1, v1, a1); a2 = fma(v2, v2, a2); a3 = fma(v3, v3, a3);
  }
  for (; e < end; e += 64) { const double v = vals[e]; a0 = fma(v, v, a0); }
  const double s = sls::norms_l1_report(sls::lane_group_sum<1>((a0 + a1) + (a2 + a3)));
  if (lane != 0) return;
  p.res[line] = s;
  double* out = col ? p.col_out : p.row_out;
  if (out) out[i] = s;
}

// totals[0] = Σ_i row_h2[i] — thread k adds the rows k, k + 256, … in turn, then the butterfly, then the four waves as
// (w0 + w1) + (w2 + w3) — and totals[1] = max_i row_h2 (the entries are ≥ 0 or +inf, never NaN)
__global__ void __launch_bounds__(kBlock) norms_h2_totals_kernel(const double* __restrict__ res, int N, double* res_totals, double* out) {
  __shared__ double lds[2 * kWavesPerBlock];
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += kBlock) s += res[i];
  s = sls::lane_group_sum<1>(s);
  if ((threadIdx.x & 63) == 0) lds[kWavesPerBlock + (threadIdx.x >> 6)] = s;
  const double m = block_max(res, N, lds);                      // its barriers publish the sums as well
  if (threadIdx.x != 0) return;
  const double t = (lds[4] + lds[5]) + (lds[6] + lds[7]);
  res_totals[0] = t; res_totals[1] = m;
  if (out) { out[0] = t; out[1] = m; }
}

struct CovParams {
  const int32_t* row_ptr; const int32_t* row_key; const double* vals;   // the row table, values in row order
  const int32_t* pair;         // [npairs][2]: (i, j), 0-based
  int npairs;
  double* res;                 // [npairs], owned by the pattern
  double* out;                 // the caller's, or NULL
};

// first index of key[lo, lo + n) whose key is ≥ k, lo + n when there is none.  The trip count depends on n alone: lanes that
// search the same window for different keys stay together.  Reads inside [lo, lo + n) only.
__device__ __forceinline__ int cov_lower_bound(const int32_t* __restrict__ key, int lo, int n, int32_t k) {
  while (n > 1) {
    const int half = n >> 1;
    lo = key[lo + half - 1] < k ? lo + half : lo;
    n -= half;
  }
  return (n == 1 && key[lo] < k) ? lo + 1 : lo;
}

// One wave per pair: cov = Σ over the keys rows i and j share of v_i·v_j.  a = the shorter list (norms_cov_swap), walked in
// chunks of 64, one entry per lane; the chunk's first and last key (read by every lane from the same address — a partly filled
// chunk has no lane 63 to broadcast from) cut b down to the window [lo, hi) that can hold a partner, and lo only moves up
// from chunk to chunk.  A lane looks its key up in the window and adds fma(va, vb, acc) on a hit: per lane the chunks
// ascend, then the xor butterfly — an order that depends on the two rows alone, not on the pair's place in the list or on the
// grid (the pairs of a wave are q, q + waves of the grid, …).  No LDS, no atomics; every cross-lane operation sits in
// wave-uniform control flow.
__global__ void __launch_bounds__(kBlock) norms_cov_kernel(CovParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t* __restrict__ key = p.row_key;
  const double* __restrict__ vals = p.vals;
  for (long long q = (long long)blockIdx.x * kWavesPerBlock + wave; q < p.npairs; q += (long long)gridDim.x * kWavesPerBlock) {
    const int i = __builtin_amdgcn_readfirstlane(p.pair[2 * q]), j = __builtin_amdgcn_readfirstlane(p.pair[2 * q + 1]);
    const int ib = p.row_ptr[i], ie = p.row_ptr[i + 1], jb = p.row_ptr[j], je = p.row_ptr[j + 1];
    const bool swap = sls::norms_cov_swap(i, ie - ib, j, je - jb);
    const int a_end = swap ? je : ie, b_end = swap ? ie : je;
    int lo = swap ? ib : jb;                                      // b below lo lies below every key of the chunks still to come
    double acc = 0.0;
    for (int c = swap ? jb : ib; c < a_end && lo < b_end; c += 64) {
      const int32_t k_first = key[c], k_last = key[min(c + 63, a_end - 1)];
      lo = cov_lower_bound(key, lo, b_end - lo, k_first);
      int hi = cov_lower_bound(key, lo, b_end - lo, k_last);
      if (hi < b_end && key[hi] == k_last) ++hi;                  // keys ascend strictly: at most one equal
      const int e = c + lane;
      if (e < a_end && lo < hi) {
        const int32_t k = key[e];
        const int at = cov_lower_bound(key, lo, hi - lo, k);
        if (at < hi && key[at] == k) acc = fma(vals[e], vals[at], acc);
      }
      lo = hi;
    }
    acc = sls::lane_group_sum<1>(acc);
    if (lane == 0) {
      p.res[q] = acc;
      if (p.out) p.out[q] = acc;
    }
  }
}

// v[j][f] = norms_v0(j) and its square for the norm kernel
__global__ void norms_init_kernel(int Nx, int F, double2* __restrict__ v, double* __restrict__ part) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (long long)Nx * F) return;
  const double x = sls::norms_v0(k / F);
  v[k] = make_double2(x, 0.0);
  part[k] = fma(x, x, 0.0 * 0.0);
}

struct PassParams {
  const int32_t* ptr; const int32_t* key; const double* vals;
  int nlines;                  // N (forward) or Nx (adjoint)
  int kdiv; double inv_kdiv;   // key = t·kdiv + other: Nx (forward) or N (adjoint)
  int F;                       // frequencies of this call: the stride of in, out, part, tw
  double sgn;                  // −1: forward, e^{−iωt}; +1: adjoint, the conjugate
  const double2* tw;           // [T][F]: (cos ω_f t, sin ω_f t)
  const double2* in;           // [kdiv][F]
  const double* scale;         // [F] or NULL: multiplies every line's sum
  double2* out;                // [nlines][F]
  double* part;                // [nlines][F]: |out|², or NULL
};

struct Acc { double re, im; };

// acc += (val·tw)·x (sls_norms.h)
__device__ __forceinline__ void cmla(Acc& a, double val, int32_t key, const PassParams& p, const double2* __restrict__ tw,
                                     const double2* __restrict__ in) {
  int32_t t, o;
  sls::norms_split_key(key, p.kdiv, p.inv_kdiv, t, o);
  const double2 w = tw[(long long)t * p.F], x = in[(long long)o * p.F];
  const double wr = val * w.x, wi = val * (p.sgn * w.y);
  a.re = fma(wr, x.x, a.re); a.re = fma(-wi, x.y, a.re);
  a.im = fma(wr, x.y, a.im); a.im = fma(wi, x.x, a.im);
}

template <int SCN>
__global__ void __launch_bounds__(kBlock) norms_pass_kernel(PassParams p) {
  constexpr int NE = 64 / SCN;
  constexpr int LOG = SCN == 1 ? 0 : SCN == 2 ? 1 : SCN == 4 ? 2 : SCN == 8 ? 3 : SCN == 16 ? 4 : SCN == 32 ? 5 : 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ls = lane % SCN, le = lane / SCN;
  const int line = blockIdx.x * kWavesPerBlock + wave;
  if (line >= p.nlines) return;
  const int f = blockIdx.y * SCN + ls;
  const bool live = f < p.F;
  const int fc = live ? f : 0;                                  // dead lanes read frequency 0 and never write
  const double2* __restrict__ tw = p.tw + fc;
  const double2* __restrict__ in = p.in + fc;
  const int beg = p.ptr[line], end = p.ptr[line + 1];
  double sr[LOG + 1], si[LOG + 1];                              // the binary counter's partial sums (static indices only)
  Acc tot{0.0, 0.0};
#pragma unroll 1
  for (int n = 0; n < SCN; ++n) {
    // virtual slot le + k·NE; k runs in bit-reversed order, so that slots 32 apart meet first and slots NE apart last
    const int k = LOG == 0 ? 0 : (int)(__brev((unsigned)n) >> (32 - (LOG == 0 ? 1 : LOG)));
    Acc a0{0.0, 0.0}, a1{0.0, 0.0}, a2{0.0, 0.0}, a3{0.0, 0.0};   // four entries in flight: the slot is a latency chain otherwise
    int e = beg + le + k * NE;
    for (; e + 192 < end; e += 256) {
      const double v0 = p.vals[e], v1 = p.vals[e + 64], v2 = p.vals[e + 128], v3 = p.vals[e + 192];
      const int32_t k0 = p.key[e], k1 = p.key[e + 64], k2 = p.key[e + 128], k3 = p.key[e + 192];
      cmla(a0, v0, k0, p, tw, in);
      cmla(a1, v1, k1, p, tw, in);
      cmla(a2, v2, k2, p, tw, in);
      cmla(a3, v3, k3, p, tw, in);
    }
    for (; e < end; e += 64) cmla(a0, p.vals[e], p.key[e], p, tw, in);
    Acc c{(a0.re + a1.re) + (a2.re + a3.re), (a0.im + a1.im) + (a2.im + a3.im)};
    bool placed = false;
#pragma unroll
    for (int L = 0; L < LOG; ++L) {
      if (placed) continue;
      if ((n >> L) & 1) { c.re = sr[L] + c.re; c.im = si[L] + c.im; }
      else { sr[L] = c.re; si[L] = c.im; placed = true; }
    }
    if (!placed) tot = c;                                       // n = SCN − 1: every level merged
  }
#pragma unroll
  for (int off = 32; off >= SCN; off >>= 1) {                   // the butterfly's offsets below NE, over the entry lanes
    tot.re += __shfl_xor(tot.re, off, 64);
    tot.im += __shfl_xor(tot.im, off, 64);
  }
  if (le != 0 || !live) return;
  if (p.scale) { const double s = p.scale[f]; tot.re *= s; tot.im *= s; }
  const long long at = (long long)line * p.F + f;
  p.out[at] = make_double2(tot.re, tot.im);
  if (p.part) p.part[at] = fma(tot.re, tot.re, tot.im * tot.im);
}

template <int SCN>
hipError_t launch_pass_scn(const PassParams& p, hipStream_t st) {
  dim3 grid((p.nlines + kWavesPerBlock - 1) / kWavesPerBlock, (unsigned)((p.F + SCN - 1) / SCN));
  hipLaunchKernelGGL(norms_pass_kernel<SCN>, grid, dim3(kBlock), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_pass(int scn, const PassParams& p, hipStream_t st) {
  switch (scn) {
    case 1: return launch_pass_scn<1>(p, st);
    case 2: return launch_pass_scn<2>(p, st);
    case 4: return launch_pass_scn<4>(p, st);
    case 8: return launch_pass_scn<8>(p, st);
    case 16: return launch_pass_scn<16>(p, st);
    case 32: return launch_pass_scn<32>(p, st);
    default: return launch_pass_scn<64>(p, st);
  }
}

// one block per frequency: n2 = Σ_i part[i][f] — thread k adds the lines k, k + 256, … in turn, then the butterfly, then the
// four waves as (w0 + w1) + (w2 + w3).  scale[f] = 1/√n2 (0 for n2 = 0), or with `sigma` set: sigma[f] = √n2 (and the caller's).
__global__ void __launch_bounds__(kBlock) norms_norm2_kernel(const double* __restrict__ part, int nlines, int F, double* scale,
                                                             double* sigma, double* sigma_out) {
  __shared__ double lds[kWavesPerBlock];
  const int f = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nlines; i += kBlock) s += part[(long long)i * F + f];
  s = sls::lane_group_sum<1>(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n2 = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  if (sigma) {
    const double sg = sqrt(n2);
    sigma[f] = sg;
    if (sigma_out) sigma_out[f] = sg;
  } else {
    scale[f] = sls::norms_scale(n2);
  }
}

// peak[0] = max_f sigma[f], peak[1] = the first f that attains it: one wave
__global__ void __launch_bounds__(64) norms_peak_kernel(const double* __restrict__ sigma, int F, double* res_peak, double* out) {
  const int lane = threadIdx.x;
  double best = sigma[lane < F ? lane : 0];
  int arg = lane < F ? lane : 0;
  for (int f = lane + 64; f < F; f += 64) if (sigma[f] > best) { best = sigma[f]; arg = f; }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off, 64);
    const int oa = __shfl_xor(arg, off, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (lane != 0) return;
  res_peak[0] = best; res_peak[1] = (double)arg;
  if (out) { out[0] = best; out[1] = (double)arg; }
}

}  // namespace

struct sls_norms {
  sls_ctx* ctx = nullptr;
  int dev = 0, slot = 0;
  int64_t n_entries = 0, max_freq = 0, Nx = 0, Nu = 0, T = 0;
  void* arena = nullptr;               // tables, weights, both value orders, work vectors, result buffer
  size_t arena_bytes = 0;
  const int32_t *d_row_ptr = nullptr, *d_col_ptr = nullptr, *d_row_key = nullptr, *d_col_key = nullptr, *d_perm = nullptr;
  const double* d_w = nullptr;         // [2·n] or NULL (no weights)
  double* d_vals = nullptr;            // [2·n]
  double2 *d_v = nullptr, *d_y = nullptr, *d_tw = nullptr;   // [Nx][max_freq], [N][max_freq], [T][max_freq]
  double *d_part = nullptr, *d_scale = nullptr;             // [N][max_freq], [max_freq]
  double* d_res = nullptr;             // row_l1 [N], col_l1 [Nx], totals [2], sigma [max_freq], peak [2]; h2 takes the l1 slots
  bool loaded = false;
  // the covariance pattern (sls_norms_cov_pattern): its own allocation, absent until the first pattern is set
  int64_t index_base = 0, npairs = 0;
  void* cov_arena = nullptr;           // pairs [npairs][2] int32, then the result buffer [npairs]
  size_t cov_bytes = 0;
  const int32_t* d_pair = nullptr;
  double* d_cov = nullptr;
};

using namespace sls;

namespace {

int enqueue_l1(sls_norms* L, hipStream_t st, double* d_row, double* d_col, double* d_totals) {
  const int N = (int)(L->Nx + L->Nu), Nx = (int)L->Nx;
  L1Params p{L->d_row_ptr, L->d_col_ptr, L->d_vals, (long long)L->n_entries, N, Nx, L->d_res, d_row, d_col};
  hipLaunchKernelGGL(norms_l1_kernel, dim3((N + Nx + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, st, p);
  HIPCHK(L->ctx, hipGetLastError());
  hipLaunchKernelGGL(norms_l1_totals_kernel, dim3(1), dim3(kBlock), 0, st, L->d_res, N, Nx, L->d_res + N + Nx, d_totals);
  HIPCHK(L->ctx, hipGetLastError());
  return 0;
}

int enqueue_h2(sls_norms* L, hipStream_t st, double* d_row, double* d_col, double* d_totals) {
  const int N = (int)(L->Nx + L->Nu), Nx = (int)L->Nx;
  L1Params p{L->d_row_ptr, L->d_col_ptr, L->d_vals, (long long)L->n_entries, N, Nx, L->d_res, d_row, d_col};
  hipLaunchKernelGGL(norms_h2_kernel, dim3((N + Nx + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, st, p);
  HIPCHK(L->ctx, hipGetLastError());
  hipLaunchKernelGGL(norms_h2_totals_kernel, dim3(1), dim3(kBlock), 0, st, L->d_res, N, L->d_res + N + Nx, d_totals);
  HIPCHK(L->ctx, hipGetLastError());
  return 0;
}

// one wave per pair up to kCovMaxBlocks blocks; past that a wave takes several pairs (a launch stays below 2³² threads)
constexpr long long kCovMaxBlocks = 1LL << 22;

int enqueue_cov(sls_norms* L, hipStream_t st, double* d_out) {
  const long long blocks = std::min<long long>((L->npairs + kWavesPerBlock - 1) / kWavesPerBlock, kCovMaxBlocks);
  CovParams p{L->d_row_ptr, L->d_row_key, L->d_vals, L->d_pair, (int)L->npairs, L->d_cov, d_out};
  hipLaunchKernelGGL(norms_cov_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, p);
  HIPCHK(L->ctx, hipGetLastError());
  return 0;
}

// what every covariance pass needs: a Φ and a pattern
int cov_ready(sls_norms* L, const char* who) {
  if (!L) return fail(nullptr, SLS_EINVAL, std::string(who) + ": null object");
  if (!L->loaded) return fail(L->ctx, SLS_EINVAL, std::string(who) + ": no Φ loaded (sls_norms_load first)");
  if (L->npairs == 0) return fail(L->ctx, SLS_EINVAL, std::string(who) + ": no pattern set (sls_norms_cov_pattern first)");
  return 0;
}

int enqueue_hinf(sls_norms* L, hipStream_t st, const double* omega, int64_t nfreq, int64_t iters, double* d_sigma, double* d_peak) {
  sls_ctx* ctx = L->ctx;
  if (!omega) return fail(ctx, SLS_EINVAL, "sls_norms_hinf: null omega");
  if (nfreq < 1 || nfreq > L->max_freq) return fail(ctx, SLS_EINVAL, "sls_norms_hinf: nfreq must be 1 … max_freq");
  if (iters < 1) return fail(ctx, SLS_EINVAL, "sls_norms_hinf: iters must be >= 1");
  for (int64_t f = 0; f < nfreq; ++f)
    if (!std::isfinite(omega[f])) return fail(ctx, SLS_EINVAL, "sls_norms_hinf: omega[" + std::to_string(f) + "] is not finite");
  const int N = (int)(L->Nx + L->Nu), Nx = (int)L->Nx, T = (int)L->T, F = (int)nfreq;
  // twiddles [T][F] through the slot's pinned buffer when they fit; otherwise from a pageable array, waited for
  const size_t tw_bytes = (size_t)T * F * sizeof(double2);
  std::vector<double> pageable;
  double* tw = reinterpret_cast<double*>(slot_pinned(ctx, L->slot, tw_bytes));
  const bool pinned = tw != nullptr;
  if (!pinned) { pageable.resize((size_t)T * F * 2); tw = pageable.data(); }
  for (int t = 0; t < T; ++t)
    for (int f = 0; f < F; ++f) norms_twiddle(omega[f], t, tw[2 * ((size_t)t * F + f)], tw[2 * ((size_t)t * F + f) + 1]);
  HIPCHK(ctx, hipMemcpyAsync(L->d_tw, tw, tw_bytes, hipMemcpyHostToDevice, st));
  if (!pinned) HIPCHK(ctx, hipStreamSynchronize(st));
  else if (int rc = pinned_read_until(ctx, L->slot, st)) return rc;
  const int scn = scenario_slots(F);
  double* res_sigma = L->d_res + N + Nx + 2;
  const long long nv = (long long)Nx * F;
  hipLaunchKernelGGL(norms_init_kernel, dim3((unsigned)((nv + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, Nx, F, L->d_v, L->d_part);
  HIPCHK(ctx, hipGetLastError());
  auto norm2 = [&](int nlines, bool final) {
    hipLaunchKernelGGL(norms_norm2_kernel, dim3(F), dim3(kBlock), 0, st, L->d_part, nlines, F, L->d_scale,
                       final ? res_sigma : nullptr, final ? d_sigma : nullptr);
    return hipGetLastError();
  };
  HIPCHK(ctx, norm2(Nx, false));
  PassParams fw{L->d_row_ptr, L->d_row_key, L->d_vals, N, Nx, 1.0 / (double)Nx, F, -1.0, L->d_tw, L->d_v, L->d_scale, L->d_y, nullptr};
  PassParams ad{L->d_col_ptr, L->d_col_key, L->d_vals + L->n_entries, Nx, N, 1.0 / (double)N, F, 1.0, L->d_tw, L->d_y, nullptr, L->d_v, L->d_part};
  for (int64_t it = 0; it < iters; ++it) {
    HIPCHK(ctx, launch_pass(scn, fw, st));
    HIPCHK(ctx, launch_pass(scn, ad, st));
    HIPCHK(ctx, norm2(Nx, false));
  }
  fw.part = L->d_part;
  HIPCHK(ctx, launch_pass(scn, fw, st));
  HIPCHK(ctx, norm2(N, true));
  hipLaunchKernelGGL(norms_peak_kernel, dim3(1), dim3(64), 0, st, res_sigma, F, res_sigma + L->max_freq, d_peak);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// n doubles of an object-owned device buffer to the host, after waiting for `st`
int fetch_from(sls_norms* L, hipStream_t st, const double* d_src, size_t n, double* stage_out) {
  return fetch_to_host(L->ctx, L->slot, st, stage_out, d_src, n * sizeof(double));
}

// the plan-owned result buffer [off, off + n) to the host, after waiting for `st`
int fetch(sls_norms* L, hipStream_t st, size_t off, size_t n, double* stage_out) { return fetch_from(L, st, L->d_res + off, n, stage_out); }

}  // namespace

extern "C" {

int sls_norms_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* cz,
                   const double* b, int64_t max_freq, sls_norms** out) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "sls_norms_plan: null context");
  if (!out || !dims || !Sx || !Su) return fail(ctx, SLS_EINVAL, "sls_norms_plan: null argument");
  *out = nullptr;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "sls_norms_plan: dev_slot out of range");
  if (max_freq < 1) return fail(ctx, SLS_EINVAL, "sls_norms_plan: max_freq must be >= 1");
  if (max_freq > 65535LL * 64) return fail(ctx, SLS_EUNSUPPORTED, "sls_norms_plan: max_freq exceeds 65535 chunks of 64 frequencies");
  NormsOperator Op;
  std::string msg;
  int rc = build_norms_operator(dims, Sx, Su, Op, msg);
  if (rc) return fail(ctx, rc, "sls_norms_plan: " + msg);
  std::vector<double> w_row, w_col;
  if ((rc = norms_entry_weights(Op, cz, b, w_row, w_col, msg))) return fail(ctx, rc, "sls_norms_plan: " + msg);
  const bool weighted = cz || b;
  const int64_t Nx = Op.Nx, N = Op.Nx + Op.Nu, T = Op.T, n = Op.row_ptr[N];
  if (N + Nx > 0x7ffffff0LL) return fail(ctx, SLS_EUNSUPPORTED, "sls_norms_plan: 2·Nx + Nu exceeds int32");
  sls_norms* L = new (std::nothrow) sls_norms();
  if (!L) return fail(ctx, SLS_ENOMEM, "sls_norms_plan: out of memory");
  L->ctx = ctx; L->dev = ctx->devs[dev_slot]; L->slot = dev_slot;
  L->n_entries = n; L->max_freq = max_freq; L->Nx = Nx; L->Nu = Op.Nu; L->T = T; L->index_base = dims->index_base;
  hipError_t e = hipSetDevice(L->dev);
  if (e != hipSuccess) { delete L; return hipfail(ctx, e, "hipSetDevice"); }
  // the two permutations share a block, row order then column order, and so do the two weight arrays; no weights, no block
  std::vector<int32_t> perm(Op.row_perm);
  perm.insert(perm.end(), Op.col_perm.begin(), Op.col_perm.end());
  std::vector<double> w(w_row);
  w.insert(w.end(), w_col.begin(), w_col.end());
  Arena ar;
  ar.table(Op.row_ptr, &L->d_row_ptr); ar.table(Op.col_ptr, &L->d_col_ptr); ar.table(Op.row_key, &L->d_row_key);
  ar.table(Op.col_key, &L->d_col_key); ar.table(perm, &L->d_perm);
  if (weighted) ar.table(w, &L->d_w);
  ar.buffer(2 * (size_t)n, &L->d_vals);
  ar.buffer((size_t)(Nx * max_freq), &L->d_v); ar.buffer((size_t)(N * max_freq), &L->d_y); ar.buffer((size_t)(T * max_freq), &L->d_tw);
  ar.buffer((size_t)(N * max_freq), &L->d_part); ar.buffer((size_t)max_freq, &L->d_scale);
  const size_t n_res = (size_t)(N + Nx + 2 + max_freq + 2);
  ar.buffer(n_res, &L->d_res);
  L->arena_bytes = ar.bytes();
  rc = ar.commit(ctx, &L->arena, "hipMalloc (norms)", "sls_norms_plan: upload");
  if (rc) { delete L; return rc; }
  e = hipMemset(L->d_res, 0, Arena::al(n_res * 8));
  if (e == hipSuccess) e = hipDeviceSynchronize();              // plan time may wait; load, l1 and hinf never do
  if (e != hipSuccess) { (void)hipFree(L->arena); delete L; return hipfail(ctx, e, "sls_norms_plan: upload"); }
  *out = L;
  return 0;
}

int sls_norms_load(sls_norms* L, void* hip_stream, const double* d_values) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_norms_load: null object");
  if (!d_values && L->n_entries > 0) return fail(L->ctx, SLS_EINVAL, "sls_norms_load: null device pointer");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  if (L->n_entries > 0) {                                       // Φ: mask order → row order and column order, weights folded in
    const long long n2 = 2 * (long long)L->n_entries;
    hipLaunchKernelGGL(norms_gather_kernel, dim3((unsigned)((n2 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(hip_stream), d_values, L->d_perm, L->d_w, n2, L->d_vals);
    HIPCHK(L->ctx, hipGetLastError());
  }
  L->loaded = true;
  return 0;
}

int sls_norms_l1(sls_norms* L, void* hip_stream, double* d_row_l1, double* d_col_l1, double* d_totals) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_norms_l1: null object");
  if (!L->loaded) return fail(L->ctx, SLS_EINVAL, "sls_norms_l1: no Φ loaded (sls_norms_load first)");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  return enqueue_l1(L, static_cast<hipStream_t>(hip_stream), d_row_l1, d_col_l1, d_totals);
}

int sls_norms_hinf(sls_norms* L, void* hip_stream, const double* omega, int64_t nfreq, int64_t iters, double* d_sigma, double* d_peak) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_norms_hinf: null object");
  if (!L->loaded) return fail(L->ctx, SLS_EINVAL, "sls_norms_hinf: no Φ loaded (sls_norms_load first)");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  return enqueue_hinf(L, static_cast<hipStream_t>(hip_stream), omega, nfreq, iters, d_sigma, d_peak);
}

int sls_norms_fetch_l1(sls_norms* L, void* hip_stream, double* row_l1, double* col_l1, double* totals) {
  if (int rc = sls_norms_l1(L, hip_stream, nullptr, nullptr, nullptr)) return rc;
  const size_t N = (size_t)(L->Nx + L->Nu), Nx = (size_t)L->Nx;
  std::vector<double> h(N + Nx + 2);
  if (int rc = fetch(L, static_cast<hipStream_t>(hip_stream), 0, h.size(), h.data())) return rc;
  if (row_l1) std::memcpy(row_l1, h.data(), N * sizeof(double));
  if (col_l1) std::memcpy(col_l1, h.data() + N, Nx * sizeof(double));
  if (totals) std::memcpy(totals, h.data() + N + Nx, 2 * sizeof(double));
  return 0;
}

int sls_norms_fetch_hinf(sls_norms* L, void* hip_stream, const double* omega, int64_t nfreq, int64_t iters, double* sigma, double* peak) {
  if (int rc = sls_norms_hinf(L, hip_stream, omega, nfreq, iters, nullptr, nullptr)) return rc;
  const size_t off = (size_t)(L->Nx + L->Nu + L->Nx + 2);
  std::vector<double> h((size_t)L->max_freq + 2);
  if (int rc = fetch(L, static_cast<hipStream_t>(hip_stream), off, h.size(), h.data())) return rc;
  if (sigma) std::memcpy(sigma, h.data(), (size_t)nfreq * sizeof(double));
  if (peak) std::memcpy(peak, h.data() + L->max_freq, 2 * sizeof(double));
  return 0;
}

int sls_norms_h2(sls_norms* L, void* hip_stream, double* d_row_h2, double* d_col_h2, double* d_totals) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_norms_h2: null object");
  if (!L->loaded) return fail(L->ctx, SLS_EINVAL, "sls_norms_h2: no Φ loaded (sls_norms_load first)");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  return enqueue_h2(L, static_cast<hipStream_t>(hip_stream), d_row_h2, d_col_h2, d_totals);
}

int sls_norms_fetch_h2(sls_norms* L, void* hip_stream, double* row_h2, double* col_h2, double* totals) {
  if (int rc = sls_norms_h2(L, hip_stream, nullptr, nullptr, nullptr)) return rc;
  const size_t N = (size_t)(L->Nx + L->Nu), Nx = (size_t)L->Nx;
  std::vector<double> h(N + Nx + 2);
  if (int rc = fetch(L, static_cast<hipStream_t>(hip_stream), 0, h.size(), h.data())) return rc;
  if (row_h2) std::memcpy(row_h2, h.data(), N * sizeof(double));
  if (col_h2) std::memcpy(col_h2, h.data() + N, Nx * sizeof(double));
  if (totals) std::memcpy(totals, h.data() + N + Nx, 2 * sizeof(double));
  return 0;
}

int sls_norms_cov_pattern(sls_norms* L, int64_t npairs, const int64_t* pair_i, const int64_t* pair_j) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_norms_cov_pattern: null object");
  if (npairs > 0x7fffffffLL) return fail(L->ctx, SLS_EUNSUPPORTED, "sls_norms_cov_pattern: npairs exceeds int32");
  std::string msg;
  if (int rc = norms_cov_check(L->Nx + L->Nu, L->index_base, npairs, pair_i, pair_j, msg)) return fail(L->ctx, rc, "sls_norms_cov_pattern: " + msg);
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  void* arena = nullptr;
  size_t bytes = 0;
  const int32_t* d_pair = nullptr;
  double* d_cov = nullptr;
  if (npairs > 0) {
    std::vector<int32_t> pr;
    try { pr.resize(2 * (size_t)npairs); } catch (const std::bad_alloc&) { return fail(L->ctx, SLS_ENOMEM, "sls_norms_cov_pattern: out of memory"); }
    for (int64_t p = 0; p < npairs; ++p) {
      pr[2 * (size_t)p] = (int32_t)(pair_i[p] - L->index_base);
      pr[2 * (size_t)p + 1] = (int32_t)(pair_j[p] - L->index_base);
    }
    Arena ar;
    ar.table(pr, &d_pair);
    ar.buffer((size_t)npairs, &d_cov);
    bytes = ar.bytes();
    if (int rc = ar.commit(L->ctx, &arena, "hipMalloc (covariance pattern)", "sls_norms_cov_pattern: upload")) return rc;
    const hipError_t e = hipMemset(d_cov, 0, Arena::al((size_t)npairs * 8));
    if (e != hipSuccess) { (void)hipFree(arena); return hipfail(L->ctx, e, "sls_norms_cov_pattern: upload"); }
  }
  const hipError_t idle = hipDeviceSynchronize();                 // the new list is up, and no pass reads the old buffers any more
  if (idle != hipSuccess) { if (arena) (void)hipFree(arena); return hipfail(L->ctx, idle, "sls_norms_cov_pattern: hipDeviceSynchronize"); }
  if (L->cov_arena) (void)hipFree(L->cov_arena);
  L->cov_arena = arena; L->cov_bytes = bytes; L->npairs = npairs;
  L->d_pair = d_pair; L->d_cov = d_cov;
  return 0;
}

int sls_norms_cov(sls_norms* L, void* hip_stream, double* d_cov) {
  if (int rc = cov_ready(L, "sls_norms_cov")) return rc;
  if (!d_cov) return fail(L->ctx, SLS_EINVAL, "sls_norms_cov: null output");
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  return enqueue_cov(L, static_cast<hipStream_t>(hip_stream), d_cov);
}

int sls_norms_fetch_cov(sls_norms* L, void* hip_stream, double* cov) {
  if (int rc = cov_ready(L, "sls_norms_fetch_cov")) return rc;
  HIPCHK(L->ctx, hipSetDevice(L->dev));
  if (int rc = enqueue_cov(L, static_cast<hipStream_t>(hip_stream), nullptr)) return rc;
  if (cov) return fetch_from(L, static_cast<hipStream_t>(hip_stream), L->d_cov, (size_t)L->npairs, cov);
  HIPCHK(L->ctx, hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int sls_norms_info(const sls_norms* L, int64_t* n_entries, int64_t* device_bytes, int64_t* max_freq) {
  if (!L) return fail(nullptr, SLS_EINVAL, "sls_norms_info: null object");
  if (n_entries) *n_entries = L->n_entries;
  if (device_bytes) *device_bytes = (int64_t)(L->arena_bytes + L->cov_bytes);
  if (max_freq) *max_freq = L->max_freq;
  return 0;
}

void sls_norms_destroy(sls_norms* L) {
  if (!L) return;
  (void)hipSetDevice(L->dev);
  if (L->arena) (void)hipFree(L->arena);
  if (L->cov_arena) (void)hipFree(L->cov_arena);
  delete L;
}

/* diagnostics (include/sls_mi355x_debug.h): both tables of the norm passes from the masks.  Needs no device. */
int sls_debug_norms_tables(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries, int32_t* row_ptr,
                           int32_t* row_key, int32_t* row_perm, int32_t* col_ptr, int32_t* col_key, int32_t* col_perm) {
  NormsOperator Op;
  std::string msg;
  int rc = build_norms_operator(dims, Sx, Su, Op, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_norms_tables: " + msg);
  if (n_entries) *n_entries = (int64_t)Op.row_key.size();
  auto put = [](const std::vector<int32_t>& v, int32_t* dst) { if (dst) std::copy(v.begin(), v.end(), dst); };
  put(Op.row_ptr, row_ptr); put(Op.row_key, row_key); put(Op.row_perm, row_perm);
  put(Op.col_ptr, col_ptr); put(Op.col_key, col_key); put(Op.col_perm, col_perm);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of load + l1 + hinf (csrc/sls_norms.cpp).  Needs no device. */
int sls_debug_norms_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values, const double* cz,
                         const double* b, const double* omega, int64_t nfreq, int64_t iters, double* row_l1, double* col_l1,
                         double* totals, double* sigma, double* peak) {
  NormsOperator Op;
  std::string msg;
  int rc = build_norms_operator(dims, Sx, Su, Op, msg);
  if (!rc) rc = norms_host(Op, values, cz, b, omega, nfreq, iters, row_l1, col_l1, totals, sigma, peak, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_norms_host: " + msg);
  return 0;
}

}  // extern "C"
