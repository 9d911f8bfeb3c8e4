// sls_norms.h — closed-loop 𝓛₁ and 𝓗∞ norms of a resident Φ (pure C++, no HIP).
//
// The operator.  Rows are the Nx state rows followed by the Nu input rows, N = Nx + Nu; for t = 0 … T−1 (0-based)
//     G[t] = diag(cz) · [Φx[t]; Φu[t]] · diag(b)        N × Nx, real          G(ω) = Σ_t G[t] · e^{−iωt}
// with cz [N] and b [Nx] (NULL = ones) folded into the stored entries at load time: cz[row]·b[col] is one double per entry,
// the stored value is Φ times it.  Φx[0] IS part of the operator (the identity block of the closed-loop response); a
// stored-false mask entry is not, and is never read.  The tables are NormsOperator (sls_symbolic.h): every entry twice, by rows
// (key = t·Nx + col) and by columns (key = t·N + row).
//
// 𝓛₁.  row_l1[i] = Σ_t Σ_j |G[t][i,j]|, col_l1[j] = Σ_t Σ_i |G[t][i,j]|; totals[0] = max_i row_l1 (the 𝓛₁ norm, induced
// ℓ∞ → ℓ∞), totals[1] = max_j col_l1 (the 𝓔₁ norm).  A sum that comes out NaN is reported as +inf.
//
// 𝓗∞ on a grid.  For every frequency f of the caller's list, independently (the twiddles cos(ω_f·t), sin(ω_f·t) are made on
// the host, norms_twiddle below, so that the twin and the device use the same numbers):
//     v[j]  = 1 + (uint32)(j·2654435761u)·2⁻³²                                (norms_v0: exact in double)
//     s     = 1/‖v‖₂                                                          (0 when ‖v‖₂ = 0)
//     repeat iters times:   y = s·(G(ω_f)·v) ;   v = G(ω_f)ᴴ·y ;   s = 1/‖v‖₂
//     sigma[f] = ‖s·(G(ω_f)·v)‖₂
// v is kept un-normalised; its scale s is a number the next forward pass reads from memory and applies to each row's sum.
// sigma[f] is a lower bound of σ_max(G(ω_f)) that does not decrease with iters; peak[0] = max_f sigma[f], peak[1] the index of
// the first frequency that attains it.  The peak bounds the 𝓗∞ norm from below ON THE CALLER'S GRID only.
// One entry of a pass is one complex multiply-add acc += (val·tw)·x: w = (val·c, val·(∓s)) — minus in the forward pass,
// e^{−iωt}, plus in the adjoint — then four FMAs, re: fma(w.re, x.re, ·), fma(−w.im, x.im, ·); im: fma(w.re, x.im, ·),
// fma(w.im, x.re, ·).  ‖·‖² is Σ fma(re, re, im·im) over the rows.
//
//
// 𝓗₂ shares and covariance.  Under unit white w the steady-state covariance of z is Σ = Σ_{t<T} G[t]·G[t]ᵀ (exact for the FIR
// closed loop from step T on: z[k] = Σ_{t<T} G[t]·w[k−t] is a finite sum of independent terms).  row_h2[i] = Σ_t Σ_j G[t][i,j]²
// is its diagonal — the variance of z_i — and col_h2[j] = Σ_t Σ_i G[t][i,j]² the share of disturbance j; totals[0] = Σ_i row_h2
// (the squared 𝓗₂ norm, rows ascending), totals[1] = max_i row_h2.  One entry is fma(v, v, acc); a sum that comes out NaN is
// reported as +inf.  Σ[i,j] = Σ over the keys the row lists of i and j share of fma(v_i, v_j, acc): the lists are ascending in
// key = t·Nx + col, so the sum is a sparse dot product of two sorted lists.  The pair is canonicalised first (norms_cov_swap:
// the shorter list leads, the smaller row on equal lengths), so (i,j) and (j,i) run the same operations.
//
// The device passes are csrc/sls_norms.hip; this header holds what they share with the host twin (csrc/sls_norms.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "sls_symbolic.h"

#if defined(__HIPCC__)
#define SLS_NRM_HD __host__ __device__
#else
#define SLS_NRM_HD
#endif

namespace sls {

// start vector of the power iteration, entry j: 1 + u·2⁻³² with u < 2³² — 33 significant bits, exact in double
SLS_NRM_HD static inline double norms_v0(int64_t j) {
  return 1.0 + (double)(uint32_t)((uint32_t)j * 2654435761u) * (1.0 / 4294967296.0);
}
// (t, other index) of a key = t·d + other; inv_d = 1.0/d.  The quotient estimate is off by at most one for keys below 2³¹.
SLS_NRM_HD static inline void norms_split_key(int32_t key, int32_t d, double inv_d, int32_t& t, int32_t& other) {
  t = (int32_t)((double)key * inv_d);
  other = key - t * d;
  if (other < 0) { --t; other += d; }
  else if (other >= d) { ++t; other -= d; }
}
// cos(ω·t), sin(ω·t): the product and the functions in long double, rounded once
static inline void norms_twiddle(double omega, int64_t t, double& c, double& s) {
  const long double a = (long double)omega * (long double)t;
  c = (double)std::cos(a); s = (double)std::sin(a);
}
// 1/√n2, and 0 for a zero vector (an operator without entries): the iteration then reports sigma = 0
SLS_NRM_HD static inline double norms_scale(double n2) { return n2 > 0.0 ? 1.0 / sqrt(n2) : 0.0; }
// what a sum of absolute values reports: +inf when a NaN went in
SLS_NRM_HD static inline double norms_l1_report(double s) { return s != s ? (double)INFINITY : s; }

// a covariance pair in the order the passes walk it: true when row j leads (its list is the shorter one, or as long and j < i)
SLS_NRM_HD static inline bool norms_cov_swap(int32_t i, int32_t len_i, int32_t j, int32_t len_j) {
  return len_j < len_i || (len_j == len_i && j < i);
}

// per-entry weights cz[row]·b[col] in row order and in column order (either vector NULL = ones); non-finite weights refused
int norms_entry_weights(const NormsOperator& Op, const double* cz, const double* b, std::vector<double>& w_row,
                        std::vector<double>& w_col, std::string& msg);

// Host twin of sls_norms_load + sls_norms_l1 + sls_norms_hinf: the same tables, the same per-entry operations, plain loop order
// (rows and entries ascending), all in double.  values: Φ in mask order (Op.n_values doubles; only perm[] positions are read).
// Outputs, each nullable: row_l1 [N], col_l1 [Nx], totals [2]; sigma [nfreq], peak [2] (these two need omega, nfreq ≥ 1 and
// iters ≥ 1 when either is asked for).
int norms_host(const NormsOperator& Op, const double* values, const double* cz, const double* b, const double* omega, int64_t nfreq,
               int64_t iters, double* row_l1, double* col_l1, double* totals, double* sigma, double* peak, std::string& msg);

// Host twin of sls_norms_load + sls_norms_h2.  Outputs, each nullable: row_h2 [N], col_h2 [Nx], totals [2].
int norms_h2_host(const NormsOperator& Op, const double* values, const double* cz, const double* b, double* row_h2, double* col_h2,
                  double* totals, std::string& msg);

// Range check of a covariance pattern (shared with sls_norms_cov_pattern): pair_i[p], pair_j[p] − index_base in 0 … N−1.
// SLS_EINVAL names the first bad position p.
int norms_cov_check(int64_t N, int64_t index_base, int64_t npairs, const int64_t* pair_i, const int64_t* pair_j, std::string& msg);

// Host twin of sls_norms_load + sls_norms_cov: cov[p] over the pairs (pair_i[p], pair_j[p]) (index_base applied), a two-pointer
// merge of the two row lists in ascending key order.
int norms_cov_host(const NormsOperator& Op, const double* values, const double* cz, const double* b, int64_t index_base, int64_t npairs,
                   const int64_t* pair_i, const int64_t* pair_j, double* cov, std::string& msg);

}  // namespace sls
