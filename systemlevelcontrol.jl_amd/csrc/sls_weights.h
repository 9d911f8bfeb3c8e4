// sls_weights.h — new LQR weights for a resident plan (sls_plan_update_weights): the host arithmetic, HIP-free.
//
// A plan built with SLS_PLAN_WEIGHTS_UPDATABLE has the LQR shape C1 = [diag(q); 0], D12 = [0; diag(r)] (either may be NULL =
// identity), no D11 on a selected row and no coupled group.  Then the only place a weight value lives in is the hinv half of a
// subproblem's weight record (SubDesc::off_w): hinv_i = 1 / (b²·v_i² + ridge_i) with b = B1[c, c] and v_i the diagonal value of
// variable i — what fill_range (sls_symbolic.cpp) computes, each operation rounded once.  weight_record below is that formula;
// weights_update_kernel (sls_update.hip) and weight_records_host use it, so both rewrite a record to the bits a fresh pass gives.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "sls_symbolic.h"

namespace sls {

#if defined(__HIP_DEVICE_COMPILE__) || defined(__clang__)
#define SLS_NO_CONTRACT_ATTR
#define SLS_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#else
#define SLS_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#define SLS_NO_CONTRACT_BODY
#endif

// hinv of one variable: v·v, then b²·(v·v), then + ridge, then 1 / …, none of them contracted into an fma (the library is built
// with -ffp-contract=fast)
SLS_NO_CONTRACT_ATTR __host__ __device__ inline double weight_record(double b2, double v, double ridge) {
  SLS_NO_CONTRACT_BODY
  const double hd = v * v;
  const double bh = b2 * hd;
  const double h = bh + ridge;
  return 1.0 / h;
}

// The value rule: finite, and the plan-time rule of fill_range (b²·v² + ridge > 0) with the smallest b² over the records that
// hold the variable (`owner`; the products are monotone in b², so the value then passes in every record).  owner < 0: no
// record holds the variable — any finite value is accepted and kept in the plan's current diagonals only.
SLS_NO_CONTRACT_ATTR __host__ __device__ inline bool weight_value_ok(double v, double owner, double ridge) {
  SLS_NO_CONTRACT_BODY
  const bool finite = (v < 0.0 ? -v : v) <= 1.7976931348623157e308;     // false for ±inf and for a NaN
  if (!finite) return false;
  if (owner < 0.0) return true;
  const double hd = v * v;
  const double bh = owner * hd;
  return bh + ridge > 0.0;
}

// Rule (a) of the flag, the part that needs no index set: C1 (Nz×Nx) and D12 (Nz×Nu) are each NULL or hold exactly one stored
// entry per column, column j of C1 on z-row j and column j of D12 on z-row Nx + j.  diag receives the Nx + Nu stored values (1.0
// for a NULL matrix).  0, or SLS_EUNSUPPORTED with the reason.  The matrices have passed validate_inputs.  (This function and the
// next two are inline: the symbolic pass calls them, and sls_symbolic.cpp links on its own in the host test programs.)
inline int weights_shape_check(const sls_dims* dims, const sls_plant* P, std::vector<double>& diag, std::string& msg) {
  const int base = dims->index_base;
  const int64_t Nx = dims->Nx, Nu = dims->Nu;
  diag.assign((size_t)(Nx + Nu), 1.0);
  const sls_csc_f64* mats[2] = {P->C1, P->D12};
  const char* name[2] = {"C1", "D12"};
  const int64_t ncs[2] = {Nx, Nu}, shift[2] = {0, Nx};
  for (int q = 0; q < 2; ++q) {
    const sls_csc_f64* m = mats[q];
    if (!m) continue;                                                   // NULL: identity
    for (int64_t c = 0; c < ncs[q]; ++c) {
      const int64_t k0 = m->colptr[c] - base, k1 = m->colptr[c + 1] - base;
      if (k1 - k0 != 1) {
        msg = std::string("SLS_PLAN_WEIGHTS_UPDATABLE: column ") + std::to_string(c) + " of " + name[q] + " stores " + std::to_string(k1 - k0) +
              " entries; an updatable plan needs exactly one entry per column (C1 = [diag(q); 0], D12 = [0; diag(r)])";
        return SLS_EUNSUPPORTED;
      }
      if (m->rowval[k0] - base != c + shift[q]) {
        msg = std::string("SLS_PLAN_WEIGHTS_UPDATABLE: column ") + std::to_string(c) + " of " + name[q] + " has its entry on z-row " +
              std::to_string(m->rowval[k0] - base) + ", not on its own z-row " + std::to_string(c + shift[q]) +
              " (C1 = [diag(q); 0], D12 = [0; diag(r)])";
        return SLS_EUNSUPPORTED;
      }
      diag[(size_t)(shift[q] + c)] = m->nzval ? m->nzval[k0] : 1.0;
    }
  }
  return 0;
}

// The per-group part, called where the group's index sets are known (map_x / map_u: local index of a global state / input, −1
// outside the set): no coupled group, and no non-zero of D11 on a selected z-row in any of the group's columns (0-based `cols`).
inline int weights_group_check(const sls_dims* dims, const sls_plant* P, const int64_t* cols, int64_t nc, const int32_t* map_x,
                        const int32_t* map_u, bool coupled, std::string& msg) {
  if (coupled) {
    msg = "SLS_PLAN_WEIGHTS_UPDATABLE: a coupled column group (non-diagonal B1[c_j, c_j]) is not updatable";
    return SLS_EUNSUPPORTED;
  }
  if (!P->D11) return 0;
  const int base = dims->index_base;
  const int64_t Nx = dims->Nx;
  for (int64_t q = 0; q < nc; ++q) {
    const int64_t c = cols[q];
    for (int64_t k = P->D11->colptr[c] - base; k < P->D11->colptr[c + 1] - base; ++k) {
      const int64_t z = P->D11->rowval[k] - base;
      const double v = P->D11->nzval ? P->D11->nzval[k] : 1.0;
      if (v != 0.0 && (z < Nx ? map_x[z] >= 0 : map_u[z - Nx] >= 0)) {
        msg = "SLS_PLAN_WEIGHTS_UPDATABLE: D11 has a non-zero on z-row " + std::to_string(z) + " of column " + std::to_string(c) +
              ", a row that column selects; an updatable plan needs D11 = 0 there";
        return SLS_EUNSUPPORTED;
      }
    }
  }
  return 0;
}

// S.wu.owner from S.subs, S.idx_pool and S.wu.b2 (after the pass, while the index sets are still on the host)
inline void weights_owner_scale(Symbolic& S) {
  std::vector<double>& own = S.wu.owner;
  own.assign((size_t)(S.Nx + S.Nu), -1.0);
  for (const SubDesc& sd : S.subs) {
    if (sd.has_w != 1) continue;
    const double b2 = S.wu.b2[(size_t)sd.out_index];
    for (int32_t i = 0; i < sd.n + sd.m; ++i) {
      const size_t g = i < sd.n ? (size_t)S.idx_pool[(size_t)sd.off_sx + i] : (size_t)S.Nx + (size_t)S.idx_pool[(size_t)sd.off_su + (i - sd.n)];
      own[g] = own[g] < 0.0 ? b2 : std::min(own[g], b2);
    }
  }
}

// The host path's check of sls_plan_update_weights: every given value against the value rule.  0, or SLS_EINVAL with a message
// that names the matrix and the 0-based position of the first offender.  c1_diag [Nx] / d12_diag [Nu], either may be NULL.
int check_weights_update(const Symbolic::UpdatableWeights& W, int64_t Nx, int64_t Nu, const double* c1_diag, const double* d12_diag,
                         std::string& msg);

// Host twin of weights_update_kernel: the same two parts in plain loops.  Needs S.subs, S.idx_pool and S.wu of a flagged pass.
// Part one rewrites, in w_pool (laid out like S.w_pool), the hinv half of every has_w = 1 record for the variables whose new
// value is accepted, and sets dirty[out_index] (nullable) where a written value differs in bits from the old one; part two
// stores the accepted values into diag [Nx + Nu] and counts the refused ones in *rejected.  NULL c1_diag / d12_diag: that half
// keeps its values.
int weight_records_host(const Symbolic& S, const double* c1_diag, const double* d12_diag, double* w_pool, double* diag, uint8_t* dirty,
                        int64_t* rejected, std::string& msg);

// The device-resident symbolic route's records, behind its fill pass (S as localized_layout left it, plus idx_pool and wu.diag): a
// has_w = 1 record at 2·idx_off[c] for every column with B1[c,c] ≠ 0, b², the value rule's scale; SLS_EUNSUPPORTED on a bad weight.
int localized_weight_records(const sls_dims* dims, const sls_csc_f64* B1, const LocalizedLayout& lay, Symbolic& S, std::string& msg);

}  // namespace sls
