// sls_margin.h — robust-stability margins of a resident Φ for an ensemble of plants (pure C++, no HIP).
//
// The controller of sls_controller.h (ŵ_k = x_k − β_k; Φx[0] taken as I and never read) on plant s,
//     x_{k+1} = A⁽ˢ⁾·x_k + B₂⁽ˢ⁾·u_k + w̃_k,
// reconstructs a disturbance that obeys exactly
//     ŵ_{k+1} = w̃_k − Σ_{τ=0..T−1} D⁽ˢ⁾[τ]·ŵ_{k−τ}
//     D⁽ˢ⁾[τ] = Φx[τ+1] − A⁽ˢ⁾·Φx[τ] − B₂⁽ˢ⁾·Φu[τ]            (0-based slices; Φx[0] := I, Φx[T] := 0)
// with x = Φx ∗ ŵ and u = Φu ∗ ŵ (substitute x_k = ŵ_k + β_k, β_{k+1} = Σ_{τ≥0} Φx[τ+1]·ŵ_{k−τ} and u_k = Σ_{τ≥0} Φu[τ]·ŵ_{k−τ}
// into ŵ_{k+1} = x_{k+1} − β_{k+1}).  The loop on plant s is internally stable when ‖D⁽ˢ⁾‖ < 1 in an induced norm,
//     ‖D‖_𝓛₁ = max_i Σ_τ Σ_j |D[τ][i,j]|        ‖D‖_𝓔₁ = max_j Σ_τ Σ_i |D[τ][i,j]|,
// and then ‖ŵ‖∞ ≤ ‖w̃‖∞ / (1 − ‖D‖_𝓛₁): every 𝓛₁ bound of sls_norms_l1 degrades by at most that factor.
//
// READING RULES.  A stored-false mask entry is 0 and is never read; no value of Sx[0] is ever read.
//
// THE DEFECT PATTERN depends on the non-zero patterns only, never on values.  Entry (τ, i, j) belongs to it when
//     Φx[τ+1][i,j] is stored-true (τ+1 ≤ T−1),  or
//     some stored A[i,k] meets a stored-true Φx[τ][k,j] (for τ = 0: k = j),  or
//     some stored B₂[i,m] meets a stored-true Φu[τ][m,j].
// Outside the pattern D is identically 0.
//
// THE VALUE OF AN ENTRY (margin_entry below, the one statement the kernel and the host twin share): start from Φx[τ+1][i,j], or
// 0.0 where that is not stored-true; then acc = fma(−a, φ, acc) over CSR row i of A⁽ˢ⁾ in ascending position, then over CSR row
// i of B₂⁽ˢ⁾, skipping the terms whose Φ factor is not in the operator (for τ = 0 the factor of A[i,j] is 1.0).  A factor is
// looked up by binary search inside the (j, τ) segment of the by-column list of Φ.
//
// THE SUMS.  |D| of every pattern entry is stored once in a scratch [n_defect][nscen] (column order); the entries are independent
// of each other, so that pass is parallel over (entry, scenario).  row_l1[i][s] and col_l1[j][s] are sums of the scratch over the
// entry's list — column j's entries in ascending (τ, i), row i's in ascending (j, τ) through the plan-time permutation — in ONE
// order whatever nscen is (margin_slot_sum below): kMarginSumSlots = 8 running sums, slot q over the list positions q, q + 8, …
// ascending, closed by the xor-shuffle tree ((q0 + q4) + (q2 + q6)) + ((q1 + q5) + (q3 + q7)).  One wave owns one (list, chunk of
// 8 scenarios) — a shape that does not depend on nscen; no floating-point atomics.  Hence the numbers of scenario s are
// bit-identical from call to call and do not depend on nscen, on the scenario's position, on the other scenarios or on how the
// plant values arrived.  A list without entries reports exactly 0.0; a sum that comes out NaN is reported as +inf.
// totals[0][s] = max_i row_l1[i][s] (‖D⁽ˢ⁾‖_𝓛₁), totals[1][s] = max_j col_l1[j][s] (‖D⁽ˢ⁾‖_𝓔₁); a maximum of non-negative numbers
// is exact in any order.
//
// Memory of one object (all allocated at plan time): Φ by columns (12 B per entry + the segment pointers 4·(Nx·T + 1) B), the
// defect lists (16 B per entry by columns, 4 B by rows), the plant values [nnz][nscen], the staging buffer of set_plant, the
// scratch 8·n_defect·nscen B and the results 8·(2·Nx + 2)·nscen B.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "sls_rollout.h"
#include "sls_symbolic.h"

#if defined(__HIPCC__)
#define SLS_MRG_HD __host__ __device__
#else
#define SLS_MRG_HD
#endif

namespace sls {

// What sls_margin_plan builds on the host.
struct MarginTables {
  RolloutTables R;                       // the plant by rows (R.F.A, R.F.B2) and where set_plant's gather finds each CSR entry
  int64_t Nx = 0, Nu = 0, T = 0, n_values = 0;
  // Φ by columns without Sx[0]: column j, slice τ is the segment [phi_seg[j·T + τ], phi_seg[j·T + τ + 1]); inside a segment the
  // rows ascend (state rows 0 … Nx−1, then input row m as Nx + m)
  std::vector<int32_t> phi_seg;          // Nx·T + 1
  std::vector<int32_t> phi_row, phi_perm;   // n_entries: row, index in the mask-order value array
  // the defect pattern by columns: key = τ·Nx + i ascending inside a column; start = position of Φx[τ+1][i,j] in the Φ list or −1
  std::vector<int32_t> def_ptr;          // Nx + 1
  std::vector<int32_t> def_col, def_key, def_start;   // n_defect (def_col: the column j of the entry, what def_ptr says)
  // the same entries grouped by row i: positions in the column order, ascending (so ascending in (j, τ))
  std::vector<int32_t> row_ptr;          // Nx + 1
  std::vector<int32_t> row_perm;         // n_defect
};
// dims, P->A, P->B1, P->B2 and the masks are read.  Errors and limits: build_rollout_tables', plus SLS_EUNSUPPORTED when the
// defect pattern exceeds int32.
int build_margin_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, MarginTables& out,
                        std::string& msg);

// What an entry reads; host or device pointers.
struct MarginView {
  const int32_t *phi_seg, *phi_row;
  const double* phi_val;                      // Φ by columns (sls_margin_load)
  const int32_t *A_ptr, *A_idx, *B2_ptr, *B2_idx;
  const double *A_val, *B2_val;               // [nnz][nscen]
  int32_t Nx, Nu, T;
  long long nscen;
};

// position of row r in the ascending list phi_row[lo … hi), or −1
SLS_MRG_HD static inline int32_t margin_find(const int32_t* phi_row, int32_t lo, int32_t hi, int32_t r) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    const int32_t v = phi_row[mid];
    if (v == r) return mid;
    if (v < r) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// |D⁽ˢᶜ⁾[τ][i,j]| of the pattern entry (j, key = τ·Nx + i, start)
SLS_MRG_HD static inline double margin_entry(const MarginView& v, int32_t j, int32_t key, int32_t start, long long sc) {
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
  return fabs(acc);
}

// The one summation order of a list of n scratch values, at(p) the p-th value of the list: slot q's running sum.  The device
// closes the kMarginSumSlots slots with the xor-shuffle tree (sls_margin.hip); a wave holds kMarginSumScen scenarios of a list.
constexpr int kMarginSumSlots = 8, kMarginSumScen = 8;
template <class At>
SLS_MRG_HD static inline double margin_slot_sum(int32_t n, int32_t q, At&& at) {
  double s = 0.0;
  for (int32_t p = q; p < n; p += kMarginSumSlots) s += at(p);
  return s;
}
// what a sum of absolute values reports: +inf when a NaN went in
SLS_MRG_HD static inline double margin_report(double s) { return s != s ? (double)INFINITY : s; }

// What the device passes (sls_margin.hip) read and write; every pointer is a device pointer.
struct MarginParams {
  MarginView v;
  const int32_t *def_ptr, *def_col, *def_key, *def_start, *row_ptr, *row_perm;
  long long n_defect;
  double* scratch;                            // [n_defect][nscen]
};

// Host twin of plan → load(values) → set_plant(A_nzval, B2_nzval, per_scenario) → run: the same tables, margin_entry for every
// entry, the sums in long double (rounded once).  values: Φ in mask order (only phi_perm[] positions are read).  A_nzval /
// B2_nzval: the caller's CSC nzval order, NULL = the values of the tables; per_scenario: [nnz][nscen] instead of [nnz].
// Outputs, each nullable: row_l1, col_l1 [Nx][nscen], totals [2][nscen].  The error model of every output (DESIGN §3.9's rule):
// row_n / col_n [Nx] count the terms that went into the sum — per entry the start value, when stored, and every product — and
// row_s / col_s [Nx][nscen] add up their absolute values (|Φx[τ+1]| and |a|·|φ|, in long double); a double evaluation of the
// output in any order is within 2·N·2⁻⁵³·S of the exact value.  tot_n [2] and tot_s [2][nscen] are the maxima over the rows
// and over the columns, which bound the error of the two maxima.
int margin_host(const MarginTables& Tb, const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval,
                bool per_scenario, double* row_l1, double* col_l1, double* totals, int64_t* row_n, int64_t* col_n, int64_t* tot_n,
                double* row_s, double* col_s, double* tot_s, std::string& msg);

}  // namespace sls
