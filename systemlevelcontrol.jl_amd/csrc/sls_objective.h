// sls_objective.h — the objective value every column achieved, evaluated from the written Φ (pure C++, no HIP).
//
// The number is what the reference's JuMP model calls objective_value(problem) (src/synthesis.jl:52): per column the cost it
// minimised, at the point that was written; the sum over the columns is the squared 𝓗₂ norm of the closed loop.
//   has_w = 0            s·Σz² + c₀                                   (s = obj_scale, c₀ = obj_const: Symbolic::obj_pool)
//   has_w = 1            Σ z²/hinv + 2g·z + c₀                         (hinv holds the ridge term: the ridge is part of the value)
//   has_w = 2 / 3        Σₜ[ Σ_{c,c'} M_cc' (W z_c)·(W z_c') + 2Σ_c g_c·z_c + Σ_c r⊙z_c² ] + c₀     (M = 1 for one dense column)
//   has_w = 4            0.0 — a coupled group's joint value sits on its first column, so the array always sums to the total
//   sum of norms         Σₜ sqrt(Σᵢ z²_{t,i}/hinv_i), with has_w = 0: Σₜ sqrt(s·Σᵢ z²_{t,i})
// A b = 0 column (B1[c,c] = 0) has the constant c₀ as its true cost; what it minimised, and what is reported, is the norm of
// its minimum-norm point: 1·Σz² + c₀.  Columns that are not OK are evaluated like any other, at the point that was written.
// The device evaluation is csrc/sls_objective.hip; this unit is its host twin (same formulas, one serial loop) and the
// reference of the GPU tests.
#pragma once
#include <cstdint>
#include <string>

#include "sls_symbolic.h"

namespace sls {

// The weight record of a dense column (has_w = 2) or of a coupled group (has_w = 3, on its first column) taken apart: the
// layout fill_range (sls_symbolic.cpp) writes after hinv[nm], g[nm].  Integers are stored as doubles.
struct GeneralRecord {
  int nc = 1;                 // columns of the group (1: a single dense column)
  const double* M = nullptr;  // nc × nc, row-major (NULL: M = 1)
  int nz = 0, nnzw = 0;       // z-rows of W with an entry, entries of W
  const double* rp = nullptr; // CSR of W by z-row: ptr[nz+1], idx[nnzw] (local variable), val[nnzw]
  const double* ri = nullptr;
  const double* rv = nullptr;
  const double* ridge = nullptr;  // nm: ridge weight per variable (zeros when none)
};
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline GeneralRecord parse_general_record(const double* rec /* w_pool + off_w */, int nm, bool group) {
  GeneralRecord R;
  const double* p = rec + 2 * (int64_t)nm;
  if (group) { R.nc = (int)p[0]; R.M = p + 1; p += 1 + (int64_t)R.nc * R.nc; }
  R.nz = (int)p[0]; R.nnzw = (int)p[1];
  R.rp = p + 2; R.ri = R.rp + R.nz + 1; R.rv = R.ri + R.nnzw;
  const double* cp = R.rv + R.nnzw;                     // CSC half: ptr[nm+1], idx[nnzw], val[nnzw]
  R.ridge = cp + (nm + 1) + 2 * (int64_t)R.nnzw;
  return R;
}

// What the device evaluation (sls_objective.hip: launch_objective) reads and writes; every pointer is a device pointer.
struct ObjectiveParams {
  const SubDesc* subs;        // indexed by out_index
  int32_t nsub, T;
  int32_t objective;          // 0 = 𝓗₂, 1 = sum of norms
  int32_t ngen;               // work items of the general build
  const int32_t* gen_list;    // their subproblems (has_w = 2, or the first column of a coupled group: has_w = 3)
  const uint8_t* mask_pool;
  const int32_t* dest;        // destinations in the layout of `values`: mask order or packed
  const double* w_pool;
  const double* obj_pool;     // Symbolic::obj_pool
  const double* values;
  double* col_objective;      // nsub, written
};

// Objective of every subproblem of S from a value array in mask order (S.n_values doubles; S must hold the explicit tables:
// built with compact = false).  objective: 0 = 𝓗₂, 1 = sum of norms.  Outputs (each nullable): col_objective[n_subs] indexed by
// out_index, *total = their sum in index order; col_terms / col_abs: the number of products the column's value sums and the
// sum of their absolute values (the same formulas with |·| on every factor) — what a summation-order bound needs.
int objective_host(const Symbolic& S, int objective, const double* values, double* col_objective, double* total,
                   int64_t* col_terms, double* col_abs, std::string& msg);

}  // namespace sls
