// sls_rollout.cpp — host side of the ensemble rollout (pure C++, no HIP): the plan-time tables (where the gather of
// sls_rollout_set_plant finds each CSR entry, the owner flags of the u accumulators) and the host twin of the device object —
// the same tables, mirrored ring, double buffers, owner flags and stats reduction as csrc/sls_rollout.hip, in serial loops.
// Reference of the non-GPU tests; the GPU tests hold the device to a long-double statement that shares no code with either.
#include "sls_rollout.h"

#include <algorithm>
#include <cmath>

namespace sls {

namespace {

// src[e] = the CSC position csc_to_csr (sls_symbolic.cpp) copied into CSR position e: columns ascending, a write cursor per row
void csr_sources(const sls_csc_f64* m, int base, const HostCsr& rows, std::vector<int32_t>& src) {
  src.assign(rows.idx.size(), 0);
  std::vector<int32_t> w(rows.ptr.begin(), rows.ptr.end() - 1);
  for (int64_t c = 0; c < m->ncols; ++c)
    for (int64_t k = m->colptr[c] - base; k < m->colptr[c + 1] - base; ++k) src[(size_t)w[m->rowval[k] - base]++] = (int32_t)k;
}

}  // namespace

int build_rollout_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, RolloutTables& out,
                         std::string& msg) {
  if (!dims || !P) { msg = "null argument"; return SLS_EINVAL; }
  out = RolloutTables();
  int rc = build_fir_operator(dims, P->A, P->B1, P->B2, Sx, Su, out.F, msg);
  if (rc) return rc;
  const FirOperator& F = out.F;
  if ((int64_t)F.A.idx.size() > 0x7fffffffLL || (int64_t)F.B2.idx.size() > 0x7fffffffLL) { msg = "nnz(A) or nnz(B2) exceeds int32"; return SLS_EUNSUPPORTED; }
  csr_sources(P->A, dims->index_base, F.A, out.A_src);
  csr_sources(P->B2, dims->index_base, F.B2, out.B2_src);
  // the first state row (ascending) that stores column j owns u_j: CSR entries are visited in exactly that order
  out.b2_owner.assign(F.B2.idx.size(), 0);
  std::vector<uint8_t> seen((size_t)F.Nu, 0);
  for (size_t e = 0; e < F.B2.idx.size(); ++e) {
    const int32_t j = F.B2.idx[e];
    if (!seen[(size_t)j]) { seen[(size_t)j] = 1; out.b2_owner[e] = 1; }
  }
  return 0;
}

int RolloutHost::init(const RolloutTables& tables, int64_t nscen, std::string& msg) {
  if (nscen < 1) { msg = "nscen must be >= 1"; return SLS_EINVAL; }
  T_ = tables;
  const FirOperator& F = T_.F;
  if ((int64_t)F.beta_ptr.size() != F.Nx + 1 || (int64_t)F.u_ptr.size() != F.Nu + 1) { msg = "operator tables missing"; return SLS_EINVAL; }
  ns_ = nscen; k_ = 0; loaded_ = false;
  R_ = controller_ring_slots(F.T);
  vals_.assign(F.hoff.size(), 0.0);
  A_val_.resize(F.A.val.size() * (size_t)ns_); B2_val_.resize(F.B2.val.size() * (size_t)ns_);
  for (size_t e = 0; e < F.A.val.size(); ++e) std::fill_n(A_val_.begin() + e * ns_, ns_, F.A.val[e]);
  for (size_t e = 0; e < F.B2.val.size(); ++e) std::fill_n(B2_val_.begin() + e * ns_, ns_, F.B2.val[e]);
  q_.assign((size_t)F.Nx, 1.0); r_.assign((size_t)F.Nu, 1.0);
  hist_.assign((size_t)controller_hist_doubles(F.Nx, F.T, ns_), 0.0);
  beta_.assign((size_t)controller_beta_doubles(F.Nx, ns_), 0.0);
  x_.assign((size_t)(2 * F.Nx * ns_), 0.0);
  acc_cost_.assign((size_t)((F.Nx + F.Nu) * ns_), 0.0); acc_peak_ = acc_cost_;
  return 0;
}

void RolloutHost::load(const double* values) {
  for (size_t e = 0; e < vals_.size(); ++e) vals_[e] = values[T_.F.perm[e]];
  loaded_ = true;
}

void RolloutHost::set_plant(const double* A_nzval, const double* B2_nzval, bool per_scenario) {
  auto gather = [&](const double* src, const std::vector<int32_t>& from, std::vector<double>& dst) {
    if (!src) return;
    for (size_t e = 0; e < from.size(); ++e)
      for (int64_t s = 0; s < ns_; ++s) dst[e * ns_ + s] = per_scenario ? src[(size_t)from[e] * ns_ + s] : src[from[e]];
  };
  gather(A_nzval, T_.A_src, A_val_);
  gather(B2_nzval, T_.B2_src, B2_val_);
}

void RolloutHost::set_weights(const double* q, const double* r) {
  if (q) std::copy(q, q + q_.size(), q_.begin());
  if (r) std::copy(r, r + r_.size(), r_.begin());
}

void RolloutHost::reset(const double* x0) {
  std::fill(hist_.begin(), hist_.end(), 0.0);
  std::fill(beta_.begin(), beta_.end(), 0.0);
  std::fill(x_.begin(), x_.end(), 0.0);
  std::fill(acc_cost_.begin(), acc_cost_.end(), 0.0);
  std::fill(acc_peak_.begin(), acc_peak_.end(), 0.0);
  if (x0) std::copy(x0, x0 + T_.F.Nx * ns_, x_.begin());
  k_ = 0;
}

int RolloutHost::run(const double* w, int64_t steps, double* x_rec, double* u_rec, std::string& msg) {
  if (steps < 0) { msg = "steps must be >= 0"; return SLS_EINVAL; }
  if (!loaded_ && steps > 0) { msg = "no Φ loaded"; return SLS_EINVAL; }
  const FirOperator& F = T_.F;
  const int64_t Nx = F.Nx, Nu = F.Nu, Nw = F.Nw, ns = ns_;
  for (int64_t n = 0; n < steps; ++n, ++k_) {
    const int64_t s = controller_slot(k_, R_), par = k_ & 1;
    const double* xk = x_.data() + par * Nx * ns;
    double* xn = x_.data() + (par ^ 1) * Nx * ns;
    const double* bk = beta_.data() + par * Nx * ns;
    double* bn = beta_.data() + (par ^ 1) * Nx * ns;
    const double* win = hist_.data() + controller_window_end(s, R_, Nx) * ns;
    const double* wk = w ? w + n * Nw * ns : nullptr;
    auto row = [&](int64_t beg, int64_t end, int64_t sc) {
      long double a = 0.0L;
      for (int64_t e = beg; e < end; ++e) {
        const int64_t h = F.hoff[e];
        const double v = h <= Nx ? xk[(Nx - h) * ns + sc] - bk[(Nx - h) * ns + sc] : win[-h * ns + sc];
        a += (long double)vals_[e] * (long double)v;
      }
      return (double)a;
    };
    auto count = [&](int64_t arow, double wgt, double v, int64_t sc) {
      const double t = (double)((long double)wgt * (long double)v);
      double& c = acc_cost_[(size_t)(arow * ns + sc)];
      c = (double)((long double)c + (long double)t * (long double)t);
      double& p = acc_peak_[(size_t)(arow * ns + sc)];
      p = std::fmax(p, std::fabs(v));
    };
    for (int64_t sc = 0; sc < ns; ++sc) {
      for (int64_t i = 0; i < Nx; ++i) {
        bn[i * ns + sc] = row(F.beta_ptr[i], F.beta_ptr[i + 1], sc);
        long double part = 0.0L;
        for (int32_t e = F.A.ptr[i]; e < F.A.ptr[i + 1]; ++e)
          part += (long double)A_val_[(size_t)e * ns + sc] * (long double)xk[(int64_t)F.A.idx[e] * ns + sc];
        if (wk)
          for (int32_t e = F.B1.ptr[i]; e < F.B1.ptr[i + 1]; ++e) part += (long double)F.B1.val[e] * (long double)wk[(int64_t)F.B1.idx[e] * ns + sc];
        double xi = (double)part;
        for (int32_t e = F.B2.ptr[i]; e < F.B2.ptr[i + 1]; ++e) {
          const int64_t j = F.B2.idx[e];
          const double uj = row(F.u_ptr[j], F.u_ptr[j + 1], sc);
          xi = (double)((long double)B2_val_[(size_t)e * ns + sc] * (long double)uj + (long double)xi);
          if (u_rec) u_rec[(n * Nu + j) * ns + sc] = uj;
          if (T_.b2_owner[e]) count(Nx + j, r_[(size_t)j], uj, sc);
        }
        xn[i * ns + sc] = xi;
        if (x_rec) x_rec[(n * Nx + i) * ns + sc] = xk[i * ns + sc];
        count(i, q_[(size_t)i], xk[i * ns + sc], sc);
      }
      for (int32_t j : F.orphan) {
        const double uj = row(F.u_ptr[j], F.u_ptr[j + 1], sc);
        if (u_rec) u_rec[(n * Nu + j) * ns + sc] = uj;
        count(Nx + j, r_[(size_t)j], uj, sc);
      }
    }
    // ŵ_k into both copies of its slot, after every row has read the window (the device writes s and s + R, which no row reads)
    for (int64_t i = 0; i < Nx * ns; ++i) {
      const double wv = xk[i] - bk[i];
      hist_[(size_t)(s * Nx * ns + i)] = wv;
      hist_[(size_t)((s + R_) * Nx * ns + i)] = wv;
    }
  }
  return 0;
}

void RolloutHost::stats(double* cost, double* peak_x, double* peak_u) const {
  const int64_t Nx = T_.F.Nx, Nu = T_.F.Nu, ns = ns_;
  for (int64_t sc = 0; sc < ns; ++sc) {
    double c = 0.0, px = 0.0, pu = 0.0;
    for (int64_t rr = 0; rr < Nx + Nu; ++rr) {
      c = c + acc_cost_[(size_t)(rr * ns + sc)];
      double& p = rr < Nx ? px : pu;
      p = std::fmax(p, acc_peak_[(size_t)(rr * ns + sc)]);
    }
    if (cost) cost[sc] = c;
    if (peak_x) peak_x[sc] = px;
    if (peak_u) peak_u[sc] = pu;
  }
}

}  // namespace sls
