// sls_margin.cpp — host side of the robust-stability margins (pure C++, no HIP): the plan-time tables (Φ by columns with a
// segment per (column, τ), the defect pattern by columns and its by-row grouping) and the host twin of the device passes — the
// same tables and margin_entry (sls_margin.h) for every entry, the sums in long double, plus the term counts and absolute sums
// the tests derive their bounds from.  The GPU tests hold the device to this twin; the non-GPU tests hold the twin to a dense
// long-double statement of the definition that shares no code with it.
#include "sls_margin.h"

#include <algorithm>
#include <cmath>

namespace sls {

int build_margin_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, MarginTables& out,
                        std::string& msg) {
  out = MarginTables();
  int rc = build_rollout_tables(dims, P, Sx, Su, out.R, msg);
  if (rc) return rc;
  NormsOperator Op;
  if ((rc = build_norms_operator(dims, Sx, Su, Op, msg))) return rc;
  const int64_t Nx = dims->Nx, Nu = dims->Nu, T = dims->T, N = Nx + Nu;
  const int base = dims->index_base;
  out.Nx = Nx; out.Nu = Nu; out.T = T; out.n_values = Op.n_values;
  // Φ by columns: the column lists of the norms (ascending in (t, row)) without the state rows of slice 0
  out.phi_seg.assign((size_t)(Nx * T + 1), 0);
  for (int64_t j = 0; j < Nx; ++j)
    for (int32_t e = Op.col_ptr[j]; e < Op.col_ptr[j + 1]; ++e) {
      const int64_t t = Op.col_key[e] / N, r = Op.col_key[e] - t * N;
      if (t == 0 && r < Nx) continue;                          // Sx[0]: Φx[0] := I, its values are never read
      out.phi_seg[(size_t)(j * T + t + 1)]++;
      out.phi_row.push_back((int32_t)r);
      out.phi_perm.push_back(Op.col_perm[e]);
    }
  for (int64_t q = 0; q < Nx * T; ++q) out.phi_seg[(size_t)q + 1] += out.phi_seg[(size_t)q];
  // the defect pattern, column by column and slice by slice: a stamp per row, the rows of a slice sorted
  const sls_csc_f64 *A = P->A, *B2 = P->B2;
  std::vector<int64_t> stamp((size_t)Nx, -1), start((size_t)Nx, -1);
  std::vector<int32_t> rows;
  out.def_ptr.assign((size_t)Nx + 1, 0);
  auto seg = [&](int64_t j, int64_t t) { return std::make_pair(out.phi_seg[(size_t)(j * T + t)], out.phi_seg[(size_t)(j * T + t + 1)]); };
  for (int64_t j = 0; j < Nx; ++j) {
    for (int64_t t = 0; t < T; ++t) {
      const int64_t id = j * T + t;
      rows.clear();
      auto mark = [&](int64_t i) { if (stamp[(size_t)i] != id) { stamp[(size_t)i] = id; start[(size_t)i] = -1; rows.push_back((int32_t)i); } };
      auto a_col = [&](int64_t k) { for (int64_t q = A->colptr[k] - base; q < A->colptr[k + 1] - base; ++q) mark(A->rowval[q] - base); };
      if (t + 1 < T) {
        const auto s1 = seg(j, t + 1);
        for (int32_t e = s1.first; e < s1.second && out.phi_row[(size_t)e] < Nx; ++e) { mark(out.phi_row[(size_t)e]); start[(size_t)out.phi_row[(size_t)e]] = e; }
      }
      if (t == 0) a_col(j);
      const auto s0 = seg(j, t);
      for (int32_t e = s0.first; e < s0.second; ++e) {
        const int64_t r = out.phi_row[(size_t)e];
        if (r < Nx) a_col(r);
        else for (int64_t q = B2->colptr[r - Nx] - base; q < B2->colptr[r - Nx + 1] - base; ++q) mark(B2->rowval[q] - base);
      }
      std::sort(rows.begin(), rows.end());
      if ((int64_t)out.def_key.size() + (int64_t)rows.size() > 0x7ffffff0LL) { msg = "the defect pattern exceeds int32"; return SLS_EUNSUPPORTED; }
      for (int32_t i : rows) {
        out.def_col.push_back((int32_t)j); out.def_key.push_back((int32_t)(t * Nx + i)); out.def_start.push_back((int32_t)start[(size_t)i]);
      }
    }
    out.def_ptr[(size_t)j + 1] = (int32_t)out.def_key.size();
  }
  // by rows: a counting sort of the column order keeps (j, τ) ascending inside a row
  out.row_ptr.assign((size_t)Nx + 1, 0);
  for (int32_t key : out.def_key) out.row_ptr[(size_t)(key % Nx) + 1]++;
  for (int64_t i = 0; i < Nx; ++i) out.row_ptr[(size_t)i + 1] += out.row_ptr[(size_t)i];
  out.row_perm.resize(out.def_key.size());
  std::vector<int32_t> w(out.row_ptr.begin(), out.row_ptr.end() - 1);
  for (size_t d = 0; d < out.def_key.size(); ++d) out.row_perm[(size_t)w[(size_t)(out.def_key[d] % Nx)]++] = (int32_t)d;
  return 0;
}

int margin_host(const MarginTables& Tb, const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval,
                bool per_scenario, double* row_l1, double* col_l1, double* totals, int64_t* row_n, int64_t* col_n, int64_t* tot_n,
                double* row_s, double* col_s, double* tot_s, std::string& msg) {
  if (nscen < 1) { msg = "nscen must be >= 1"; return SLS_EINVAL; }
  const int64_t Nx = Tb.Nx, ns = nscen;
  if ((int64_t)Tb.def_ptr.size() != Nx + 1 || (int64_t)Tb.row_ptr.size() != Nx + 1) { msg = "margin tables missing"; return SLS_EINVAL; }
  if (!values && !Tb.phi_perm.empty()) { msg = "null values"; return SLS_EINVAL; }
  const FirOperator& F = Tb.R.F;
  std::vector<double> phi(Tb.phi_perm.size());
  for (size_t e = 0; e < phi.size(); ++e) phi[e] = values[Tb.phi_perm[e]];
  auto gather = [&](const double* src, const std::vector<int32_t>& from, const std::vector<double>& init, std::vector<double>& dst) {
    dst.resize(from.size() * (size_t)ns);
    for (size_t e = 0; e < from.size(); ++e)
      for (int64_t s = 0; s < ns; ++s)
        dst[e * ns + s] = !src ? init[e] : per_scenario ? src[(size_t)from[e] * ns + s] : src[from[e]];
  };
  std::vector<double> A_val, B2_val;
  gather(A_nzval, Tb.R.A_src, F.A.val, A_val);
  gather(B2_nzval, Tb.R.B2_src, F.B2.val, B2_val);
  const MarginView v{Tb.phi_seg.data(), Tb.phi_row.data(), phi.data(), F.A.ptr.data(), F.A.idx.data(), F.B2.ptr.data(), F.B2.idx.data(),
                     A_val.data(), B2_val.data(), (int32_t)Nx, (int32_t)Tb.Nu, (int32_t)Tb.T, (long long)ns};
  // the terms of an entry: how many, and the sum of their absolute values — margin_entry's walk without the arithmetic
  auto terms = [&](int32_t j, int32_t key, int32_t start, int64_t sc, int64_t& n, long double& s) {
    const int32_t tau = key / (int32_t)Nx, i = key - tau * (int32_t)Nx;
    const int32_t lo = Tb.phi_seg[(size_t)((int64_t)j * Tb.T + tau)], hi = Tb.phi_seg[(size_t)((int64_t)j * Tb.T + tau + 1)];
    n = 0; s = 0.0L;
    if (start >= 0) { ++n; s += std::fabs((long double)phi[(size_t)start]); }
    for (int32_t e = F.A.ptr[i]; e < F.A.ptr[i + 1]; ++e) {
      const int32_t k = F.A.idx[e];
      long double f = 1.0L;
      if (tau == 0) { if (k != j) continue; }
      else { const int32_t p = margin_find(Tb.phi_row.data(), lo, hi, k); if (p < 0) continue; f = phi[(size_t)p]; }
      ++n; s += std::fabs((long double)A_val[(size_t)e * ns + sc] * f);
    }
    for (int32_t e = F.B2.ptr[i]; e < F.B2.ptr[i + 1]; ++e) {
      const int32_t p = margin_find(Tb.phi_row.data(), lo, hi, (int32_t)Nx + F.B2.idx[e]);
      if (p < 0) continue;
      ++n; s += std::fabs((long double)B2_val[(size_t)e * ns + sc] * (long double)phi[(size_t)p]);
    }
  };
  const size_t nd = Tb.def_key.size();
  std::vector<double> absd(nd);
  std::vector<long double> ent_s(nd);
  std::vector<int64_t> ent_n(nd);
  std::vector<long double> rsum((size_t)Nx), csum((size_t)Nx), rs((size_t)Nx), cs((size_t)Nx);
  std::vector<int64_t> rn((size_t)Nx), cn((size_t)Nx);
  for (int64_t sc = 0; sc < ns; ++sc) {
    for (int64_t j = 0; j < Nx; ++j)
      for (int32_t d = Tb.def_ptr[j]; d < Tb.def_ptr[j + 1]; ++d) {
        absd[(size_t)d] = margin_entry(v, (int32_t)j, Tb.def_key[(size_t)d], Tb.def_start[(size_t)d], sc);
        terms((int32_t)j, Tb.def_key[(size_t)d], Tb.def_start[(size_t)d], sc, ent_n[(size_t)d], ent_s[(size_t)d]);
      }
    for (int64_t j = 0; j < Nx; ++j) {
      long double a = 0.0L, s = 0.0L; int64_t n = 0;
      for (int32_t d = Tb.def_ptr[j]; d < Tb.def_ptr[j + 1]; ++d) { a += absd[(size_t)d]; s += ent_s[(size_t)d]; n += ent_n[(size_t)d]; }
      csum[(size_t)j] = a; cs[(size_t)j] = s; cn[(size_t)j] = n;
    }
    for (int64_t i = 0; i < Nx; ++i) {
      long double a = 0.0L, s = 0.0L; int64_t n = 0;
      for (int32_t q = Tb.row_ptr[i]; q < Tb.row_ptr[i + 1]; ++q) {
        const size_t d = (size_t)Tb.row_perm[(size_t)q];
        a += absd[d]; s += ent_s[d]; n += ent_n[d];
      }
      rsum[(size_t)i] = a; rs[(size_t)i] = s; rn[(size_t)i] = n;
    }
    double t0 = 0.0, t1 = 0.0, ts0 = 0.0, ts1 = 0.0;
    int64_t tn0 = 0, tn1 = 0;
    for (int64_t i = 0; i < Nx; ++i) {
      const double r = margin_report((double)rsum[(size_t)i]), c = margin_report((double)csum[(size_t)i]);
      if (row_l1) row_l1[i * ns + sc] = r;
      if (col_l1) col_l1[i * ns + sc] = c;
      if (row_s) row_s[i * ns + sc] = (double)rs[(size_t)i];
      if (col_s) col_s[i * ns + sc] = (double)cs[(size_t)i];
      if (row_n) row_n[i] = rn[(size_t)i];
      if (col_n) col_n[i] = cn[(size_t)i];
      t0 = std::fmax(t0, r); t1 = std::fmax(t1, c);
      ts0 = std::fmax(ts0, (double)rs[(size_t)i]); ts1 = std::fmax(ts1, (double)cs[(size_t)i]);
      tn0 = std::max(tn0, rn[(size_t)i]); tn1 = std::max(tn1, cn[(size_t)i]);
    }
    if (totals) { totals[sc] = t0; totals[ns + sc] = t1; }
    if (tot_s) { tot_s[sc] = ts0; tot_s[ns + sc] = ts1; }
    if (tot_n) { tot_n[0] = tn0; tot_n[1] = tn1; }
  }
  return 0;
}

}  // namespace sls
