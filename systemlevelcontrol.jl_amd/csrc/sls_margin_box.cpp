// sls_margin_box.cpp — host side of the worst-case 𝓛₁ margin over a box of plants (pure C++, no HIP): the active lists that
// sls_margin_set_radius builds, the worst plant of a set of vertices, and the host twin of the device pass — the same tables
// and active lists, d⁰ by margin_entry_signed (sls_margin_box.h), every vertex in long double, plus the term counts and absolute
// sums the tests derive their bounds from.  The GPU tests hold the device to this twin; the non-GPU tests hold the twin to a
// brute force over all vertices with dense long-double matrices that shares no code with it.
#include "sls_margin_box.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace sls {

int build_margin_box_lists(const std::vector<int32_t>& A_ptr, const std::vector<int32_t>& A_src, const std::vector<int32_t>& B2_ptr,
                           const std::vector<int32_t>& B2_src, int64_t nscen, const double* A_rad, const double* B2_rad, bool per_scenario,
                           MarginBoxLists& out, std::string& msg) {
  if (nscen < 1) { msg = "nscen must be >= 1"; return SLS_EINVAL; }
  if (A_ptr.empty() || A_ptr.size() != B2_ptr.size()) { msg = "margin tables missing"; return SLS_EINVAL; }
  const int64_t Nx = (int64_t)A_ptr.size() - 1, ns = nscen;
  const int64_t nA = (int64_t)A_src.size(), nB = (int64_t)B2_src.size();
  const double* src[2] = {A_rad, B2_rad};
  const int64_t nnz[2] = {nA, nB};
  for (int m = 0; m < 2; ++m)
    if (src[m])
      for (int64_t k = 0; k < nnz[m] * (per_scenario ? ns : 1); ++k)
        if (!std::isfinite(src[m][k]) || src[m][k] < 0.0) { msg = "a radius is negative or not finite"; return SLS_EINVAL; }
  MarginBoxLists L;
  L.nscen = ns;
  auto gather = [&](const double* s, const std::vector<int32_t>& from, std::vector<double>& dst) {
    dst.assign(from.size() * (size_t)ns, 0.0);
    if (!s) return;
    for (size_t e = 0; e < from.size(); ++e)
      for (int64_t sc = 0; sc < ns; ++sc) dst[e * (size_t)ns + (size_t)sc] = per_scenario ? s[(size_t)from[e] * (size_t)ns + (size_t)sc] : s[from[e]];
  };
  gather(A_rad, A_src, L.A_rad);
  gather(B2_rad, B2_src, L.B2_rad);
  auto active = [&](const std::vector<double>& rad, int64_t e) {
    for (int64_t sc = 0; sc < ns; ++sc) if (rad[(size_t)(e * ns + sc)] > 0.0) return true;
    return false;
  };
  L.act_ptr.assign((size_t)Nx + 1, 0);
  L.exact.assign((size_t)Nx, 1);
  for (int64_t i = 0; i < Nx; ++i) {
    for (int32_t e = A_ptr[(size_t)i]; e < A_ptr[(size_t)i + 1]; ++e) if (active(L.A_rad, e)) L.act_ent.push_back(e);
    for (int32_t e = B2_ptr[(size_t)i]; e < B2_ptr[(size_t)i + 1]; ++e) if (active(L.B2_rad, e)) L.act_ent.push_back((int32_t)(nA + e));
    L.act_ptr[(size_t)i + 1] = (int32_t)L.act_ent.size();
    const int64_t nb = L.act_ptr[(size_t)i + 1] - L.act_ptr[(size_t)i];
    L.max_bits = std::max(L.max_bits, nb);
    if (nb > kMarginBoxMaxBits) { L.exact[(size_t)i] = 0; ++L.n_inexact_rows; }
    else L.n_vertex_sums += (int64_t)1 << nb;
  }
  out = std::move(L);
  return 0;
}

void margin_box_worst_plant(const std::vector<int32_t>& A_ptr, const std::vector<int32_t>& A_src, const std::vector<int32_t>& B2_ptr,
                            const std::vector<int32_t>& B2_src, const MarginBoxLists& L, const double* A_cen, const double* B2_cen,
                            const int64_t* row_vertex, double* A_out, double* B2_out) {
  const int64_t Nx = (int64_t)A_ptr.size() - 1, ns = L.nscen, nA = (int64_t)A_src.size();
  // every coefficient at its centre first: outside the active lists every radius is 0
  if (A_out) for (size_t e = 0; e < A_src.size(); ++e) for (int64_t sc = 0; sc < ns; ++sc) A_out[(size_t)A_src[e] * (size_t)ns + (size_t)sc] = A_cen[e * (size_t)ns + (size_t)sc];
  if (B2_out) for (size_t e = 0; e < B2_src.size(); ++e) for (int64_t sc = 0; sc < ns; ++sc) B2_out[(size_t)B2_src[e] * (size_t)ns + (size_t)sc] = B2_cen[e * (size_t)ns + (size_t)sc];
  for (int64_t i = 0; i < Nx; ++i)
    for (int32_t a = L.act_ptr[(size_t)i]; a < L.act_ptr[(size_t)i + 1]; ++a) {
      const int b = a - L.act_ptr[(size_t)i];
      const int64_t c = L.act_ent[(size_t)a];
      for (int64_t sc = 0; sc < ns; ++sc) {
        const int64_t code = row_vertex[i * ns + sc];
        const bool up = code < 0 || ((code >> b) & 1);
        if (c < nA) {
          if (A_out) { const double r = L.A_rad[(size_t)(c * ns + sc)]; A_out[(size_t)A_src[(size_t)c] * (size_t)ns + (size_t)sc] = A_cen[c * ns + sc] + (up ? r : -r); }
        } else if (B2_out) {
          const int64_t e = c - nA;
          const double r = L.B2_rad[(size_t)(e * ns + sc)];
          B2_out[(size_t)B2_src[(size_t)e] * (size_t)ns + (size_t)sc] = B2_cen[e * ns + sc] + (up ? r : -r);
        }
      }
    }
}

int margin_box_host(const MarginTables& Tb, const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval,
                    bool per_scenario, const double* A_rad, const double* B2_rad, bool rad_per_scenario, double* row_wc,
                    int64_t* row_vertex, uint8_t* row_exact, double* totals, int64_t* row_n, double* row_s, double* A_worst,
                    double* B2_worst, std::string& msg) {
  if (nscen < 1) { msg = "nscen must be >= 1"; return SLS_EINVAL; }
  const int64_t Nx = Tb.Nx, ns = nscen;
  if ((int64_t)Tb.def_ptr.size() != Nx + 1 || (int64_t)Tb.row_ptr.size() != Nx + 1) { msg = "margin tables missing"; return SLS_EINVAL; }
  if (!values && !Tb.phi_perm.empty()) { msg = "null values"; return SLS_EINVAL; }
  const FirOperator& F = Tb.R.F;
  MarginBoxLists L;
  int rc = build_margin_box_lists(F.A.ptr, Tb.R.A_src, F.B2.ptr, Tb.R.B2_src, ns, A_rad, B2_rad, rad_per_scenario, L, msg);
  if (rc) return rc;
  std::vector<double> phi(Tb.phi_perm.size());
  for (size_t e = 0; e < phi.size(); ++e) phi[e] = values[Tb.phi_perm[e]];
  auto gather = [&](const double* src, const std::vector<int32_t>& from, const std::vector<double>& init, std::vector<double>& dst) {
    dst.resize(from.size() * (size_t)ns);
    for (size_t e = 0; e < from.size(); ++e)
      for (int64_t s = 0; s < ns; ++s)
        dst[e * (size_t)ns + (size_t)s] = !src ? init[e] : per_scenario ? src[(size_t)from[e] * (size_t)ns + (size_t)s] : src[from[e]];
  };
  std::vector<double> A_val, B2_val;
  gather(A_nzval, Tb.R.A_src, F.A.val, A_val);
  gather(B2_nzval, Tb.R.B2_src, F.B2.val, B2_val);
  const int32_t nA = (int32_t)F.A.val.size();
  const MarginView v{Tb.phi_seg.data(), Tb.phi_row.data(), phi.data(), F.A.ptr.data(), F.A.idx.data(), F.B2.ptr.data(), F.B2.idx.data(),
                     A_val.data(), B2_val.data(), (int32_t)Nx, (int32_t)Tb.Nu, (int32_t)Tb.T, (long long)ns};
  const MarginBoxView bv{L.act_ptr.data(), L.act_ent.data(), L.A_rad.data(), L.B2_rad.data(), nA};
  // the centre terms of an entry: how many, and the sum of their absolute values (margin_host's rule)
  auto centre_terms = [&](int32_t j, int32_t key, int32_t start, int64_t sc, int64_t& n, long double& s) {
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
  std::vector<int64_t> vertex((size_t)(Nx * ns), 0);
  if (totals) std::fill(totals, totals + ns, 0.0);
  std::vector<long double> d0, fac, sums;
  std::vector<uint8_t> has;
  for (int64_t i = 0; i < Nx; ++i) {
    const int32_t* ent = L.act_ent.data() + L.act_ptr[(size_t)i];
    const int nb = L.act_ptr[(size_t)i + 1] - L.act_ptr[(size_t)i];
    const int32_t n = Tb.row_ptr[(size_t)i + 1] - Tb.row_ptr[(size_t)i];
    if (row_exact) row_exact[i] = L.exact[(size_t)i];
    for (int64_t sc = 0; sc < ns; ++sc) {
      d0.assign((size_t)n, 0.0L); fac.assign((size_t)n * (size_t)nb, 0.0L); has.assign((size_t)n * (size_t)nb, 0);
      std::vector<long double> rho((size_t)nb);
      for (int b = 0; b < nb; ++b) rho[(size_t)b] = margin_box_radius(bv, ent[b], ns, sc);
      int64_t N = 0; long double S = 0.0L;
      for (int32_t q = 0; q < n; ++q) {
        const size_t d = (size_t)Tb.row_perm[(size_t)(Tb.row_ptr[(size_t)i] + q)];
        d0[(size_t)q] = margin_entry_signed(v, Tb.def_col[d], Tb.def_key[d], Tb.def_start[d], sc);
        int64_t en; long double es;
        centre_terms(Tb.def_col[d], Tb.def_key[d], Tb.def_start[d], sc, en, es);
        N += en; S += es;
        for (int b = 0; b < nb; ++b) {
          double f;
          if (!margin_box_factor(v, nA, ent[b], Tb.def_col[d], Tb.def_key[d], f)) continue;
          has[(size_t)q * nb + b] = 1; fac[(size_t)q * nb + b] = f;
          ++N; S += rho[(size_t)b] * std::fabs((long double)f);
        }
      }
      long double best = -1.0L; int64_t code = 0;
      if (L.exact[(size_t)i]) {
        for (int64_t c = 0; c < ((int64_t)1 << nb); ++c) {
          long double a = 0.0L;
          for (int32_t q = 0; q < n; ++q) {
            long double t = d0[(size_t)q];
            for (int b = 0; b < nb; ++b)
              if (has[(size_t)q * nb + b]) t -= ((c >> b) & 1 ? rho[(size_t)b] : -rho[(size_t)b]) * fac[(size_t)q * nb + b];
            a += std::fabs(t);
          }
          const long double r = a != a ? (long double)INFINITY : a;
          if (r > best) { best = r; code = c; }
        }
      } else {
        long double a = 0.0L;
        for (int32_t q = 0; q < n; ++q) a += std::fabs(d0[(size_t)q]);
        for (int b = 0; b < nb; ++b) {
          long double f = 0.0L;
          for (int32_t q = 0; q < n; ++q) if (has[(size_t)q * nb + b]) f += std::fabs(fac[(size_t)q * nb + b]);
          a += rho[(size_t)b] * f;
        }
        best = a != a ? (long double)INFINITY : a; code = -1;
      }
      vertex[(size_t)(i * ns + sc)] = code;
      if (row_wc) row_wc[i * ns + sc] = (double)best;
      if (row_vertex) row_vertex[i * ns + sc] = code;
      if (row_n) row_n[i] = N;
      if (row_s) row_s[i * ns + sc] = (double)S;
      if (totals) totals[sc] = std::fmax(totals[sc], (double)best);
    }
  }
  if (A_worst || B2_worst)
    margin_box_worst_plant(F.A.ptr, Tb.R.A_src, F.B2.ptr, Tb.R.B2_src, L, A_val.data(), B2_val.data(), vertex.data(), A_worst, B2_worst);
  return 0;
}

int margin_entry_signed_check(const MarginTables& Tb, const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval,
                              bool per_scenario, int64_t* n_entries, int64_t* n_mismatch, int64_t* n_negative, std::string& msg) {
  if (nscen < 1) { msg = "nscen must be >= 1"; return SLS_EINVAL; }
  if (!values && !Tb.phi_perm.empty()) { msg = "null values"; return SLS_EINVAL; }
  const FirOperator& F = Tb.R.F;
  const int64_t ns = nscen;
  std::vector<double> phi(Tb.phi_perm.size());
  for (size_t e = 0; e < phi.size(); ++e) phi[e] = values[Tb.phi_perm[e]];
  auto gather = [&](const double* src, const std::vector<int32_t>& from, const std::vector<double>& init, std::vector<double>& dst) {
    dst.resize(from.size() * (size_t)ns);
    for (size_t e = 0; e < from.size(); ++e)
      for (int64_t s = 0; s < ns; ++s)
        dst[e * (size_t)ns + (size_t)s] = !src ? init[e] : per_scenario ? src[(size_t)from[e] * (size_t)ns + (size_t)s] : src[from[e]];
  };
  std::vector<double> A_val, B2_val;
  gather(A_nzval, Tb.R.A_src, F.A.val, A_val);
  gather(B2_nzval, Tb.R.B2_src, F.B2.val, B2_val);
  const MarginView v{Tb.phi_seg.data(), Tb.phi_row.data(), phi.data(), F.A.ptr.data(), F.A.idx.data(), F.B2.ptr.data(), F.B2.idx.data(),
                     A_val.data(), B2_val.data(), (int32_t)Tb.Nx, (int32_t)Tb.Nu, (int32_t)Tb.T, (long long)ns};
  int64_t n = 0, bad = 0, neg = 0;
  for (size_t d = 0; d < Tb.def_key.size(); ++d)
    for (int64_t sc = 0; sc < ns; ++sc) {
      const double a = margin_entry(v, Tb.def_col[d], Tb.def_key[d], Tb.def_start[d], sc);
      const double s = margin_entry_signed(v, Tb.def_col[d], Tb.def_key[d], Tb.def_start[d], sc);
      const double f = std::fabs(s);
      uint64_t ba, bf;
      static_assert(sizeof(ba) == sizeof(a), "double is 64 bits");
      std::memcpy(&ba, &a, 8); std::memcpy(&bf, &f, 8);
      ++n; bad += ba != bf; neg += s < 0.0;
    }
  if (n_entries) *n_entries = n;
  if (n_mismatch) *n_mismatch = bad;
  if (n_negative) *n_negative = neg;
  return 0;
}

}  // namespace sls
