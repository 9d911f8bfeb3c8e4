// sls_margin_box.h — worst-case 𝓛₁ margin of a resident Φ over a box of plants (pure C++, host and device).
//
// sls_margin.h certifies the plants one hands it.  Here every stored coefficient of row i of A and B₂ is known to ± a radius,
//     a_e = a⁰_e + δ_e,  |δ_e| ≤ ρ_e            (a⁰: what sls_margin_set_plant set; ρ: sls_margin_set_radius, per scenario),
// and the question is the largest ‖D‖_𝓛₁ over the whole box.  Row i of every D[τ] depends on row i of A and B₂ only, so the
// rows decouple, and the row sum
//     f_i(δ) = Σ_{(τ,j)} | d⁰[τ][i,j] − Σ_e δ_e·φ_e(τ,j) |
// (d⁰ the signed defect at the centre, φ_e the factor margin_entry multiplies a_e with) is convex in δ: its maximum over the
// box is attained at one of the 2^b sign patterns of the row's b uncertain coefficients.  Hence
//     max_plant ‖D‖_𝓛₁ = max_i max_σ f_i(σ)
// exactly, and the plant that takes every row's arg-max vertex attains every row's worst case at once.
//
// THE ACTIVE LIST of row i: the row's CSR entries of A, then of B₂, whose radius is > 0 in at least one scenario, in that order;
// coefficient c < nnz(A) is CSR entry c of A, c ≥ nnz(A) is CSR entry c − nnz(A) of B₂.  Bit b of a vertex code set means
// δ_b = +ρ_b, clear means −ρ_b.  In a scenario where ρ_b = 0 both settings give the same bits, so the numbers of scenario s do
// not depend on which other scenarios made a coefficient active — only the code does, and ties go to the lowest code.
//
// THE VALUE OF A VERTEX at a pattern entry (phase B of sls_margin_box.hip): v = d⁰ = margin_entry_signed (margin_entry's fma chain
// without the final fabs), then v = fma(∓ρ_b, φ_b, v) for b ascending (− where the bit is set), then |v|.  A factor that is
// not in the operator contributes no term; it may be handed in as 0.0, since fma(∓ρ, 0.0, v) = v for finite ρ.
//
// THE ROW SUM of a vertex uses the order of sls_margin.h: margin_slot_sum over the row's list in row_perm order, eight slots,
// the same xor tree, margin_report for NaN.  With every radius 0 it is sls_margin_run's row_l1 bit for bit.  The result of a row
// is the largest vertex sum, ties to the lowest code.
//
// A row with more than kMarginBoxMaxBits active coefficients reports the triangle bound
//     Σ|d⁰| + Σ_b ρ_b·Σ|φ_b|
// instead — Σ|d⁰| and every Σ|φ_b| in the same slot order, then acc = fma(ρ_b, Σ|φ_b|, acc) for b ascending — with exact = 0 and
// vertex −1.  It is an upper bound of the row's worst case, so a certificate built on it stays sound.
#pragma once
#include "sls_margin.h"

namespace sls {

constexpr int kMarginBoxMaxBits = 10;

// d⁰: margin_entry without the final fabs — the same walk and the same fma chain, fabs(margin_entry_signed) == margin_entry
SLS_MRG_HD static inline double margin_entry_signed(const MarginView& v, int32_t j, int32_t key, int32_t start, long long sc) {
  const int32_t tau = key / v.Nx, i = key - tau * v.Nx;
  const int32_t lo = v.phi_seg[(long long)j * v.T + tau], hi = v.phi_seg[(long long)j * v.T + tau + 1];
  double acc = start >= 0 ? v.phi_val[start] : 0.0;
  for (int32_t e = v.A_ptr[i]; e < v.A_ptr[i + 1]; ++e) {
    const int32_t k = v.A_idx[e];
    double phi = 1.0;                                          // Φx[0] := I
    if (tau == 0) {
      if (k != j) continue;
    } else {
      const int32_t p = margin_find(v.phi_row, lo, hi, k);
      if (p < 0) continue;
      phi = v.phi_val[p];
    }
    acc = fma(-v.A_val[(long long)e * v.nscen + sc], phi, acc);
  }
  for (int32_t e = v.B2_ptr[i]; e < v.B2_ptr[i + 1]; ++e) {
    const int32_t p = margin_find(v.phi_row, lo, hi, v.Nx + v.B2_idx[e]);
    if (p < 0) continue;
    acc = fma(-v.B2_val[(long long)e * v.nscen + sc], v.phi_val[p], acc);
  }
  return acc;
}

// The active lists and the radii by rows; host or device pointers.
struct MarginBoxView {
  const int32_t *act_ptr, *act_ent;           // [Nx + 1], [n_active]: coefficient codes, see above
  const double *A_rad, *B2_rad;               // [nnz][nscen] in the CSR order of the plant values
  int32_t nnzA;
};

// ρ of coefficient c in scenario sc
SLS_MRG_HD static inline double margin_box_radius(const MarginBoxView& b, int32_t c, long long ns, long long sc) {
  return c < b.nnzA ? b.A_rad[(long long)c * ns + sc] : b.B2_rad[(long long)(c - b.nnzA) * ns + sc];
}

// φ_c at the pattern entry (j, key): the factor margin_entry multiplies coefficient c with; false = not in the operator
SLS_MRG_HD static inline bool margin_box_factor(const MarginView& v, int32_t nnzA, int32_t c, int32_t j, int32_t key, double& phi) {
  const int32_t tau = key / v.Nx;
  int32_t r;
  if (c < nnzA) {
    r = v.A_idx[c];
    if (tau == 0) { phi = 1.0; return r == j; }                // Φx[0] := I
  } else {
    r = v.Nx + v.B2_idx[c - nnzA];
  }
  const int32_t p = margin_find(v.phi_row, v.phi_seg[(long long)j * v.T + tau], v.phi_seg[(long long)j * v.T + tau + 1], r);
  if (p < 0) return false;
  phi = v.phi_val[p];
  return true;
}

// What sls_margin_set_radius builds on the host.
struct MarginBoxLists {
  int64_t nscen = 0;
  std::vector<int32_t> act_ptr, act_ent;      // Nx + 1, n_active
  std::vector<double> A_rad, B2_rad;          // [nnz][nscen], CSR order
  std::vector<uint8_t> exact;                 // Nx: the row has at most kMarginBoxMaxBits active coefficients
  int64_t max_bits = 0;                       // the longest active list (of any row, exact or not)
  int64_t n_inexact_rows = 0;
  int64_t n_vertex_sums = 0;                  // Σ over the exact rows of 2^b_i: the row sums one scenario evaluates
};
// A_ptr / B2_ptr: the plant by rows; A_src / B2_src: the CSC position of each CSR entry (RolloutTables).  A_rad / B2_rad: the
// caller's CSC nzval order, NULL = zeros, [nnz] or [nnz][nscen] by per_scenario.  SLS_EINVAL (and `out` untouched) for a
// radius that is not finite or is negative.
int build_margin_box_lists(const std::vector<int32_t>& A_ptr, const std::vector<int32_t>& A_src, const std::vector<int32_t>& B2_ptr,
                           const std::vector<int32_t>& B2_src, int64_t nscen, const double* A_rad, const double* B2_rad, bool per_scenario,
                           MarginBoxLists& out, std::string& msg);

// The plant that takes every row's vertex: centre + ρ where the bit is set, centre − ρ where it is clear, every coefficient
// + ρ in a row whose vertex is −1.  A_cen / B2_cen: [nnz][nscen] in CSR order; row_vertex [Nx][nscen]; A_out / B2_out (each
// nullable): [nnz][nscen] in the CSC nzval order.
void margin_box_worst_plant(const std::vector<int32_t>& A_ptr, const std::vector<int32_t>& A_src, const std::vector<int32_t>& B2_ptr,
                            const std::vector<int32_t>& B2_src, const MarginBoxLists& L, const double* A_cen, const double* B2_cen,
                            const int64_t* row_vertex, double* A_out, double* B2_out);

// Host twin of plan → load → set_plant → set_radius → box_run: the same tables and active lists, d⁰ by margin_entry_signed, every
// vertex of an exact row in long double (rounded once), the triangle bound of the other rows in long double.  Plant values and
// radii as in margin_host / build_margin_box_lists.  Outputs, each nullable: row_wc [Nx][nscen], row_vertex [Nx][nscen],
// row_exact [Nx], totals [nscen] (the maxima of row_wc), the worst plant A_worst / B2_worst [nnz][nscen] (CSC order), and the
// error model of row_wc (DESIGN §3.9's rule): row_n [Nx] counts the terms of the row — per entry the start value, when
// stored, every centre product and every ρ·φ product — and row_s [Nx][nscen] adds up their absolute values (|Φx[τ+1]|, |a⁰|·|φ|,
// ρ·|φ|); a double evaluation of any vertex sum, or of the triangle bound, is within 2·N·2⁻⁵³·S of its exact value.
int margin_box_host(const MarginTables& Tb, const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval,
                    bool per_scenario, const double* A_rad, const double* B2_rad, bool rad_per_scenario, double* row_wc,
                    int64_t* row_vertex, uint8_t* row_exact, double* totals, int64_t* row_n, double* row_s, double* A_worst,
                    double* B2_worst, std::string& msg);

// fabs(margin_entry_signed) against margin_entry on every pattern entry and scenario: the entries compared, those whose bits
// differ, those whose signed value is negative
int margin_entry_signed_check(const MarginTables& Tb, const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval,
                              bool per_scenario, int64_t* n_entries, int64_t* n_mismatch, int64_t* n_negative, std::string& msg);

// What the device pass (sls_margin_box.hip) reads; every pointer is a device pointer.
struct MarginBoxParams {
  MarginParams p;                             // the tables, Φ by columns and the centres of the owner (p.scratch is not used)
  MarginBoxView b;
};

}  // namespace sls

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace sls {
// d_row_wc [Nx][nscen], d_row_vertex [Nx][nscen] (−1 for a bound row), d_totals [nscen]; two launches, nothing waits
hipError_t launch_margin_box(const MarginBoxParams& bp, hipStream_t st, double* d_row_wc, long long* d_row_vertex, double* d_totals);
}  // namespace sls
#endif
