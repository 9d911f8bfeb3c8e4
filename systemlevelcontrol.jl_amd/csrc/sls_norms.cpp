// sls_norms.cpp — host twin of the closed-loop norm passes (pure C++, no HIP): the same tables (NormsOperator), the same
// per-entry operations and the same twiddles (sls_norms.h) as csrc/sls_norms.hip, in a plain loop order.  Reference of the
// non-GPU tests; the GPU tests hold the device to a long-double statement that shares no code with either.
#include "sls_norms.h"

#include <algorithm>

namespace sls {

int norms_entry_weights(const NormsOperator& Op, const double* cz, const double* b, std::vector<double>& w_row,
                        std::vector<double>& w_col, std::string& msg) {
  const int64_t Nx = Op.Nx, N = Op.Nx + Op.Nu;
  if ((int64_t)Op.row_ptr.size() != N + 1 || (int64_t)Op.col_ptr.size() != Nx + 1) { msg = "operator tables missing"; return SLS_EINVAL; }
  for (int64_t i = 0; cz && i < N; ++i) if (!std::isfinite(cz[i])) { msg = "cz[" + std::to_string(i) + "] is not finite"; return SLS_EINVAL; }
  for (int64_t j = 0; b && j < Nx; ++j) if (!std::isfinite(b[j])) { msg = "b[" + std::to_string(j) + "] is not finite"; return SLS_EINVAL; }
  const int64_t n = Op.row_ptr[N];
  w_row.assign((size_t)n, 1.0); w_col.assign((size_t)n, 1.0);
  const double inv_x = 1.0 / (double)Nx, inv_n = 1.0 / (double)N;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t e = Op.row_ptr[i]; e < Op.row_ptr[i + 1]; ++e) {
      int32_t t, c; norms_split_key(Op.row_key[e], (int32_t)Nx, inv_x, t, c);
      w_row[(size_t)e] = (cz ? cz[i] : 1.0) * (b ? b[c] : 1.0);
    }
  for (int64_t j = 0; j < Nx; ++j)
    for (int64_t e = Op.col_ptr[j]; e < Op.col_ptr[j + 1]; ++e) {
      int32_t t, r; norms_split_key(Op.col_key[e], (int32_t)N, inv_n, t, r);
      w_col[(size_t)e] = (cz ? cz[r] : 1.0) * (b ? b[j] : 1.0);
    }
  return 0;
}

namespace {

struct Cx { double re, im; };

// out[line] = scale · Σ_e (val·tw)·in[other], one frequency; sgn = −1: forward (e^{−iωt}), +1: adjoint.  Returns Σ |out|².
double pass(const std::vector<int32_t>& ptr, const std::vector<int32_t>& key, const std::vector<double>& vals, int64_t nlines,
            int32_t kdiv, const std::vector<double>& tc, const std::vector<double>& ts, double sgn, const std::vector<Cx>& in,
            double scale, std::vector<Cx>& out) {
  const double inv = 1.0 / (double)kdiv;
  double n2 = 0.0;
  for (int64_t i = 0; i < nlines; ++i) {
    double ar = 0.0, ai = 0.0;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
      int32_t t, o; norms_split_key(key[e], kdiv, inv, t, o);
      const double wr = vals[(size_t)e] * tc[(size_t)t], wi = vals[(size_t)e] * (sgn * ts[(size_t)t]);
      const Cx x = in[(size_t)o];
      ar = std::fma(wr, x.re, ar); ar = std::fma(-wi, x.im, ar);
      ai = std::fma(wr, x.im, ai); ai = std::fma(wi, x.re, ai);
    }
    out[(size_t)i] = Cx{scale * ar, scale * ai};
    n2 += std::fma(out[(size_t)i].re, out[(size_t)i].re, out[(size_t)i].im * out[(size_t)i].im);
  }
  return n2;
}

}  // namespace

int norms_host(const NormsOperator& Op, const double* values, const double* cz, const double* b, const double* omega, int64_t nfreq,
               int64_t iters, double* row_l1, double* col_l1, double* totals, double* sigma, double* peak, std::string& msg) {
  const int64_t Nx = Op.Nx, N = Op.Nx + Op.Nu, T = Op.T;
  std::vector<double> w_row, w_col;
  if (int rc = norms_entry_weights(Op, cz, b, w_row, w_col, msg)) return rc;
  const int64_t n = Op.row_ptr[N];
  if (n > 0 && !values) { msg = "null values"; return SLS_EINVAL; }
  const bool want_hinf = sigma || peak;
  if (want_hinf) {
    if (!omega || nfreq < 1) { msg = "omega and nfreq >= 1 are needed for sigma / peak"; return SLS_EINVAL; }
    if (iters < 1) { msg = "iters must be >= 1"; return SLS_EINVAL; }
    for (int64_t f = 0; f < nfreq; ++f) if (!std::isfinite(omega[f])) { msg = "omega[" + std::to_string(f) + "] is not finite"; return SLS_EINVAL; }
  }
  std::vector<double> rv((size_t)n), cv((size_t)n);                    // the gather of sls_norms_load: both value orders
  for (int64_t e = 0; e < n; ++e) {
    rv[(size_t)e] = values[Op.row_perm[e]] * w_row[(size_t)e];
    cv[(size_t)e] = values[Op.col_perm[e]] * w_col[(size_t)e];
  }
  auto l1 = [](const std::vector<int32_t>& ptr, const std::vector<double>& vals, int64_t nlines, double* out) {
    double mx = 0.0;
    for (int64_t i = 0; i < nlines; ++i) {
      double s = 0.0;
      for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) s += std::fabs(vals[(size_t)e]);
      s = norms_l1_report(s);
      if (out) out[i] = s;
      mx = std::max(mx, s);
    }
    return mx;
  };
  if (row_l1 || col_l1 || totals) {
    const double m0 = l1(Op.row_ptr, rv, N, row_l1), m1 = l1(Op.col_ptr, cv, Nx, col_l1);
    if (totals) { totals[0] = m0; totals[1] = m1; }
  }
  if (!want_hinf) return 0;
  std::vector<double> tc((size_t)T), ts((size_t)T);
  std::vector<Cx> v((size_t)Nx), y((size_t)N);
  double best = 0.0; int64_t arg = 0;
  for (int64_t f = 0; f < nfreq; ++f) {
    for (int64_t t = 0; t < T; ++t) norms_twiddle(omega[f], t, tc[(size_t)t], ts[(size_t)t]);
    double n2 = 0.0;
    for (int64_t j = 0; j < Nx; ++j) { v[(size_t)j] = Cx{norms_v0(j), 0.0}; n2 += std::fma(v[(size_t)j].re, v[(size_t)j].re, 0.0 * 0.0); }
    double s = norms_scale(n2);
    for (int64_t it = 0; it < iters; ++it) {
      (void)pass(Op.row_ptr, Op.row_key, rv, N, (int32_t)Nx, tc, ts, -1.0, v, s, y);
      n2 = pass(Op.col_ptr, Op.col_key, cv, Nx, (int32_t)N, tc, ts, 1.0, y, 1.0, v);
      s = norms_scale(n2);
    }
    const double sg = sqrt(pass(Op.row_ptr, Op.row_key, rv, N, (int32_t)Nx, tc, ts, -1.0, v, s, y));
    if (sigma) sigma[f] = sg;
    if (f == 0 || sg > best) { best = sg; arg = f; }
  }
  if (peak) { peak[0] = best; peak[1] = (double)arg; }
  return 0;
}

int norms_h2_host(const NormsOperator& Op, const double* values, const double* cz, const double* b, double* row_h2, double* col_h2,
                  double* totals, std::string& msg) {
  const int64_t Nx = Op.Nx, N = Op.Nx + Op.Nu;
  std::vector<double> w_row, w_col;
  if (int rc = norms_entry_weights(Op, cz, b, w_row, w_col, msg)) return rc;
  const int64_t n = Op.row_ptr[N];
  if (n > 0 && !values) { msg = "null values"; return SLS_EINVAL; }
  auto h2 = [&](const std::vector<int32_t>& ptr, const std::vector<int32_t>& perm, const std::vector<double>& w, int64_t nlines,
                double* out, double* tot) {
    double sum = 0.0, mx = 0.0;
    for (int64_t i = 0; i < nlines; ++i) {
      double s = 0.0;
      for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) { const double v = values[perm[e]] * w[(size_t)e]; s = std::fma(v, v, s); }
      s = norms_l1_report(s);
      if (out) out[i] = s;
      sum += s; mx = std::max(mx, s);
    }
    if (tot) { tot[0] = sum; tot[1] = mx; }
  };
  if (row_h2 || totals) h2(Op.row_ptr, Op.row_perm, w_row, N, row_h2, totals);
  if (col_h2) h2(Op.col_ptr, Op.col_perm, w_col, Nx, col_h2, nullptr);
  return 0;
}

int norms_cov_check(int64_t N, int64_t index_base, int64_t npairs, const int64_t* pair_i, const int64_t* pair_j, std::string& msg) {
  if (npairs < 0) { msg = "npairs must be >= 0"; return SLS_EINVAL; }
  if (npairs > 0 && (!pair_i || !pair_j)) { msg = "null pair list"; return SLS_EINVAL; }
  for (int64_t p = 0; p < npairs; ++p) {
    const int64_t i = pair_i[p] - index_base, j = pair_j[p] - index_base;
    if (i < 0 || i >= N || j < 0 || j >= N) {
      msg = "pair " + std::to_string(p) + " (" + std::to_string(pair_i[p]) + ", " + std::to_string(pair_j[p]) + ") is outside the " +
            std::to_string(N) + " rows";
      return SLS_EINVAL;
    }
  }
  return 0;
}

int norms_cov_host(const NormsOperator& Op, const double* values, const double* cz, const double* b, int64_t index_base, int64_t npairs,
                   const int64_t* pair_i, const int64_t* pair_j, double* cov, std::string& msg) {
  const int64_t N = Op.Nx + Op.Nu;
  std::vector<double> w_row, w_col;
  if (int rc = norms_entry_weights(Op, cz, b, w_row, w_col, msg)) return rc;
  if (int rc = norms_cov_check(N, index_base, npairs, pair_i, pair_j, msg)) return rc;
  const int64_t n = Op.row_ptr[N];
  if (n > 0 && !values) { msg = "null values"; return SLS_EINVAL; }
  if (npairs > 0 && !cov) { msg = "null output"; return SLS_EINVAL; }
  std::vector<double> rv((size_t)n);                                   // the gather of sls_norms_load, row order
  for (int64_t e = 0; e < n; ++e) rv[(size_t)e] = values[Op.row_perm[e]] * w_row[(size_t)e];
  for (int64_t p = 0; p < npairs; ++p) {
    int32_t i = (int32_t)(pair_i[p] - index_base), j = (int32_t)(pair_j[p] - index_base);
    if (norms_cov_swap(i, Op.row_ptr[i + 1] - Op.row_ptr[i], j, Op.row_ptr[j + 1] - Op.row_ptr[j])) std::swap(i, j);
    int32_t ea = Op.row_ptr[i], eb = Op.row_ptr[j];
    const int32_t a_end = Op.row_ptr[i + 1], b_end = Op.row_ptr[j + 1];
    double s = 0.0;
    while (ea < a_end && eb < b_end) {
      const int32_t ka = Op.row_key[ea], kb = Op.row_key[eb];
      if (ka == kb) s = std::fma(rv[(size_t)ea], rv[(size_t)eb], s);
      ea += ka <= kb; eb += kb <= ka;
    }
    cov[p] = s;
  }
  return 0;
}

}  // namespace sls
