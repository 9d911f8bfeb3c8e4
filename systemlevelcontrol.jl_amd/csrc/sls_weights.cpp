// sls_weights.cpp — host arithmetic of sls_plan_update_weights (sls_weights.h).  Plain C++, no HIP: the shape
// rule of SLS_PLAN_WEIGHTS_UPDATABLE, the value rule of the host path, and the host twin of weights_update_kernel.
#include "sls_weights.h"

#include <algorithm>
#include <cstring>

namespace sls {

int check_weights_update(const Symbolic::UpdatableWeights& W, int64_t Nx, int64_t Nu, const double* c1_diag, const double* d12_diag,
                         std::string& msg) {
  if ((int64_t)W.owner.size() != Nx + Nu || (!W.ridge.empty() && (int64_t)W.ridge.size() != Nx + Nu)) {
    msg = "weights update: the plan's weight tables do not belong to this plant";
    return SLS_EINVAL;
  }
  const double* src[2] = {c1_diag, d12_diag};
  const int64_t n[2] = {Nx, Nu}, first[2] = {0, Nx};
  const char* name[2] = {"C1", "D12"};
  for (int q = 0; q < 2; ++q) {
    if (!src[q]) continue;
    for (int64_t k = 0; k < n[q]; ++k) {
      const double v = src[q][k];
      const size_t g = (size_t)(first[q] + k);
      if (!std::isfinite(v)) {
        msg = std::string("weights update: ") + name[q] + " diagonal position " + std::to_string(k) + " is not finite";
        return SLS_EINVAL;
      }
      if (!weight_value_ok(v, W.owner[g], W.ridge.empty() ? 0.0 : W.ridge[g])) {
        msg = std::string("weights update: ") + name[q] + " diagonal position " + std::to_string(k) +
              " gives a zero cost weight (b²·v² + ridge is not positive: singular Hessian)";
        return SLS_EINVAL;
      }
    }
  }
  return 0;
}

int weight_records_host(const Symbolic& S, const double* c1_diag, const double* d12_diag, double* w_pool, double* diag, uint8_t* dirty,
                        int64_t* rejected, std::string& msg) {
  const Symbolic::UpdatableWeights& W = S.wu;
  const int64_t Nx = S.Nx, Nu = S.Nu;
  if (!W.updatable || W.b2.size() != S.subs.size() || (int64_t)W.owner.size() != Nx + Nu || (!W.ridge.empty() && (int64_t)W.ridge.size() != Nx + Nu)) {
    msg = "weights update: the symbolic pass was not made with SLS_PLAN_WEIGHTS_UPDATABLE";
    return SLS_EINVAL;
  }
  auto ridge = [&](size_t g) { return W.ridge.empty() ? 0.0 : W.ridge[g]; };
  // part one: the records
  for (const SubDesc& sd : S.subs) {
    if (sd.has_w != 1) continue;
    const double b2 = W.b2[(size_t)sd.out_index];
    bool changed = false;
    for (int32_t i = 0; i < sd.n + sd.m; ++i) {
      const bool isx = i < sd.n;
      const double* src = isx ? c1_diag : d12_diag;
      if (!src) continue;
      const int64_t loc = isx ? S.idx_pool[(size_t)sd.off_sx + i] : S.idx_pool[(size_t)sd.off_su + (i - sd.n)];
      const size_t g = (size_t)(isx ? loc : Nx + loc);
      const double v = src[loc];
      if (!weight_value_ok(v, W.owner[g], ridge(g))) continue;
      const double h = weight_record(b2, v, ridge(g));
      double* dst = w_pool + sd.off_w + i;
      if (std::memcmp(dst, &h, sizeof(double)) != 0) { *dst = h; changed = true; }
    }
    if (changed && dirty) dirty[sd.out_index] = 1;
  }
  // part two: the current diagonals and the count
  int64_t refused = 0;
  for (int64_t k = 0; k < Nx + Nu; ++k) {
    const double* src = k < Nx ? c1_diag : d12_diag;
    if (!src) continue;
    const double v = src[k < Nx ? k : k - Nx];
    if (!weight_value_ok(v, W.owner[(size_t)k], ridge((size_t)k))) { ++refused; continue; }
    if (diag) diag[k] = v;
  }
  if (rejected) *rejected = refused;
  return 0;
}

int localized_weight_records(const sls_dims* dims, const sls_csc_f64* B1, const LocalizedLayout& lay, Symbolic& S, std::string& msg) {
  const int64_t Nx = S.Nx, Nu = S.Nu;
  S.wu.b2.assign((size_t)Nx, 0.0);
  for (int64_t c = 0; c < Nx; ++c) {
    const double bd = b1_diagonal(B1, dims->index_base, c);
    if (bd == 0.0) continue;                                  // a b = 0 column keeps no record: its minimiser ignores the weights
    SubDesc& sd = S.subs[(size_t)c];
    sd.has_w = 1; sd.off_w = 2 * lay.idx_off[(size_t)c];
    S.wu.b2[(size_t)c] = bd * bd;
    S.obj_pool[2 * (size_t)c] = 1.0;                          // the scale belongs to has_w = 0 columns
  }
  weights_owner_scale(S);
  const double* dg = S.wu.diag.data();
  if (check_weights_update(S.wu, Nx, Nu, dg, dg + Nx, msg)) { msg += " (plan-time weights)"; return SLS_EUNSUPPORTED; }
  S.w_pool.assign((size_t)(2 * lay.idx_total), 0.0);
  return weight_records_host(S, dg, dg + Nx, S.w_pool.data(), nullptr, nullptr, nullptr, msg);
}

}  // namespace sls
