// sls_residual.h — achievability residual of every column of a written Φ against the FULL plant (pure C++, no HIP).
//
// The solve reports ‖Ez − f‖∞ of the REDUCED problem (rows of s_x only).  This is the defect of the system-level identities
//   Φx[1] = I,   Φx[t+1] = A·Φx[t] + B2·Φu[t],   0 = A·Φx[T] + B2·Φu[T]
// on all rows of the plant, per subproblem q (global column c, index sets s_x, s_u, horizon T, 0-based t):
//   Δ[0]   = Φx[0][:,c] − e_c
//   Δ[t+1] = Φx[t+1][:,c] − A·Φx[t][:,c] − B2·Φu[t][:,c]        t = 0 … T−2
//   Δ[T]   =            − A·Φx[T−1][:,c] − B2·Φu[T−1][:,c]
// Φ is read through the subproblem's mask bytes and destination table, as sls_objective.hip reads it (a stored-false mask
// entry or a destination < 0 reads as 0.0), so Φ[:,c] lives on s_x / s_u and Δ can be non-zero on two kinds of rows only:
//   local  rows of s_x;
//   halo   H(q): rows r ∉ s_x with A[r,j] stored for some j ∈ s_x or B2[r,k] stored for some k ∈ s_u (by pattern, like the
//          index sets: build_halo_rows, sls_symbolic.h), and row c itself when c ∉ s_x.
// A SLS_COL_TRIVIAL column (c ∉ s_x, Φ = 0) therefore reports 1.0 in all three numbers: against the full system that is its defect.
// Per subproblem, in col_status order:
//   res_inf  = max_{t,r} |Δ[t][r]| over local and halo rows       halo_inf = the same over halo rows only (0.0: H(q) empty)
//   res_l1   = Σ_t Σ_r |Δ[t][r]|
// and two totals: max_q res_inf, and max_q res_l1 — the 𝓔₁ norm of Δ, which robust SLS needs below 1.  A NaN in Φ gives +inf
// (resid_max, sls_device.h).  A and B2 are the values the plan holds when the evaluation runs.  A coupled or multi-column group
// reports one value per column: each of its columns is a column of Φ.  Both objectives: the constraints are the same.
// A row's products are gathered along its row of A_csr, then of B_csr, in ascending CSR position with fma; a stored column
// outside the index set contributes nothing.  The device evaluation is csrc/sls_residual.hip; this unit is its host twin
// (the same formulas in one serial loop, accumulated in long double) and the reference of the GPU tests.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sls_symbolic.h"

namespace sls {

// What the device evaluation (sls_residual.hip: launch_residual) reads and writes; every pointer is a device pointer.
struct ResidualParams {
  const SubDesc* subs;        // indexed by out_index
  int32_t nsub, T;
  const int32_t* idx_pool;
  const uint8_t* mask_pool;
  const int32_t* dest;        // destinations in the layout of `values`: mask order or packed
  const int32_t* A_rowptr; const int32_t* A_colidx; const double* A_val;     // CSR of A
  const int32_t* B_rowptr; const int32_t* B_colidx; const double* B_val;     // CSR of B2
  const int32_t* sub_col;     // global column of each subproblem
  const int64_t* halo_ptr;    // nsub + 1
  const int32_t* halo_rows;   // ascending per subproblem
  const double* values;
  double* res_inf;            // nsub each, written
  double* halo_inf;
  double* res_l1;
};

// Residual of every subproblem of S from a value array in mask order (S.n_values doubles; S must hold the explicit tables:
// built with compact = false) against S.A_csr / S.B_csr.  Outputs, each nullable, indexed by out_index: res_inf, halo_inf,
// res_l1 [n_subs]; totals[2] = {max res_inf, max res_l1}.  What a summation-order bound (2·N·2⁻⁵³·S) needs: ent_terms / ent_abs
// — the largest number N of terms one entry Δ[t][r] of the column sums and the largest sum S of their absolute values (each
// maximum over the column's entries, so the pair bounds every entry, hence res_inf and halo_inf); l1_terms / l1_abs — the
// same two numbers for res_l1 (all terms of all entries).  halo_ptr / halo_rows (nullable): H(q), as build_halo_rows leaves it.
int residual_host(const Symbolic& S, const double* values, double* res_inf, double* halo_inf, double* res_l1, double* totals,
                  int64_t* ent_terms, double* ent_abs, int64_t* l1_terms, double* l1_abs, std::vector<int64_t>* halo_ptr,
                  std::vector<int32_t>* halo_rows, std::string& msg);

}  // namespace sls
