// sls_gradient.h — gradient of the 𝓗₂ cost in the stored entries of A and B2 and in the LQR diagonals, from the multipliers a plan
// built with SLS_PLAN_MULTIPLIERS keeps (sls_plan_gradient).  Pure C++ declarations: the tables and the host twin
// are in sls_gradient.cpp (no HIP), the two kernels in sls_gradient.hip.
//
// The one-wave kernel solves  min ½ zᵀHz + gᵀz  s.t.  E z = f  with z = H⁻¹(Eᵀλ − g); the cost the plan reports is
//   has_w = 0:  J = s·Σz² + c₀   (H = I, g = 0, s = obj_scale)      ⇒  ∇J = 2s·z = Eᵀ(2s·λ)
//   has_w = 1:  J = zᵀHz + 2gᵀz + c₀                                ⇒  ∇J = 2(Hz + g) = Eᵀ(2λ)
// so μ = f_j·λ with f_j = 2s or 2 (column_factor).  Block row k ≥ 1 of E is x_k − Ãx_{k−1} − B̃u_{k−1}: an entry Ã[a,b] enters
// the Lagrangian J − μᵀ(Ez − f) as +μ_k[a]·x_{k−1}[b], which is the derivative of the optimal cost (envelope theorem).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sls_symbolic.h"

namespace sls {

// a multiplier slot: λ_k[a] at k·kMuLd + a (kMuLd: sls_device.h)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int64_t mu_slot_doubles(int T) { return (int64_t)(T + 1) * kMuLd; }

// μ = column_factor · λ
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline double column_factor(int has_w, double obj_scale) { return has_w ? 2.0 : 2.0 * obj_scale; }

// Per subproblem q (out_index order) the stored entries of A and B2 with both indices inside its index sets:
//   ent[3e .. 3e+3) for e in [ent_ptr[q], ent_ptr[q+1]) = (position, local row a, local column b).  The position is the CSC
//   position in the caller's nzval for A, nnzA + that for B2; b counts inside s_x for A, inside s_u for B2.  Entries of A first,
//   by ascending column then row; e is also the entry's contribution slot.
// The inverse map: stored entry p owns the slots inv_slot[inv_ptr[p] .. inv_ptr[p+1]), in ascending subproblem order (inv_sub).
// Weight slots: subproblem q's variable i < ñx+ñu has slot w_base[q] + i; global variable v (states, then inputs behind Nx) owns
// winv_slot[winv_ptr[v] .. winv_ptr[v+1]), in ascending subproblem order.
struct GradientTables {
  int64_t nnzA = 0, nnzB = 0, Nx = 0, Nu = 0;
  std::vector<int64_t> ent_ptr;
  std::vector<int32_t> ent;
  std::vector<int64_t> inv_ptr, inv_slot;
  std::vector<int32_t> inv_sub;
  std::vector<int64_t> w_base, winv_ptr, winv_slot;
};
// At / Bt: the CSC halves of the operator (At_csr, Bt_csr: row j is column j of A / B2; only ptr and idx are read)
void build_gradient_tables(const HostCsr& At, const HostCsr& Bt, const SubDesc* subs, int64_t nsub, const int32_t* idx_pool,
                           GradientTables& G);

// What the device pass (sls_gradient.hip: launch_gradient) reads and writes; every pointer is a device pointer.
struct GradientParams {
  const SubDesc* subs;  int32_t nsub, T;
  const uint8_t* mask_pool;
  const int32_t* dest;          // destinations in the layout of `values`
  const double* values;
  const double* mu;             // nsub slots of mu_slot_doubles(T): the kernel's λ
  const double* obj_pool;
  const uint8_t* b_zero;        // [nsub] 1: B1[c,c] = 0
  const int32_t* status;        // [nsub]
  const double* col_weight;     // [nsub] or NULL
  const int64_t* ent_ptr;  const int32_t* ent;
  const int64_t* inv_ptr;  const int64_t* inv_slot;
  double* contrib;              // one per listed entry
  int64_t nnzA, nnzB;
  double* gA;  double* gB2;     // each may be NULL
  // weight derivatives (all NULL / 0 unless asked for)
  const double* b2;  const double* diag;
  const int64_t* w_base;  const int64_t* winv_ptr;  const int64_t* winv_slot;
  double* wcontrib;
  int64_t Nx, Nu;
  double* gc1;  double* gd12;
};

// Host twin: the gradient from given multipliers and values, accumulated in long double in the device's order.  S needs the
// explicit mask / destination tables and idx_pool; mu: nsub slots of (T+1)·ñx doubles each, concatenated (mu_off[q] = Σ over
// earlier subproblems), already scaled (μ, not λ); values in mask order.  status / col_weight / b_zero nullable.  Outputs
// nullable: gA / gB2, and per entry abs_A / abs_B2 = Σ|terms| and terms_A / terms_B2 = the number of products.
int gradient_host(const Symbolic& S, const GradientTables& G, const double* mu, const double* values, const int32_t* status,
                  const double* col_weight, const uint8_t* b_zero, double* gA, double* gB2, double* abs_A, double* abs_B2,
                  int64_t* terms_A, int64_t* terms_B2, std::string& msg);

}  // namespace sls
