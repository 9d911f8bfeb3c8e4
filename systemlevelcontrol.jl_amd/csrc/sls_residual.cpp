// sls_residual.cpp — see sls_residual.h.  Pure host code (compiled by hipcc or g++): the serial twin of sls_residual.hip.
#include "sls_residual.h"

#include <algorithm>
#include <cmath>

namespace sls {

int residual_host(const Symbolic& S, const double* values, double* res_inf, double* halo_inf, double* res_l1, double* totals,
                  int64_t* ent_terms, double* ent_abs, int64_t* l1_terms, double* l1_abs, std::vector<int64_t>* halo_ptr,
                  std::vector<int32_t>* halo_rows, std::string& msg) {
  const int64_t ns = (int64_t)S.subs.size(), T = S.T;
  if (S.compact || (S.md_total > 0 && ((int64_t)S.mask_pool.size() != S.md_total || (int64_t)S.dest_pool.size() != S.md_total))) {
    msg = "residual_host needs the explicit mask / destination tables"; return SLS_EINVAL;
  }
  if ((int64_t)S.sub_col.size() != ns || (int64_t)S.A_csr.ptr.size() != S.Nx + 1 || (int64_t)S.B_csr.ptr.size() != S.Nx + 1) {
    msg = "residual_host: the symbolic pass holds no operator or no column list"; return SLS_EINVAL;
  }
  if (!values && S.n_values > 0) { msg = "null value array"; return SLS_EINVAL; }
  std::vector<int64_t> hp;
  std::vector<int32_t> hr;
  build_halo_rows(S.At_csr, S.Bt_csr, S.subs.data(), ns, S.idx_pool.data(), S.sub_col.data(), hp, hr);
  double tot_inf = 0.0, tot_l1 = 0.0;
  for (int64_t q = 0; q < ns; ++q) {
    const SubDesc& sd = S.subs[q];
    const int n = sd.n, nm = sd.n + sd.m;
    const int32_t* sx = S.idx_pool.data() + sd.off_sx;
    const int32_t* su = S.idx_pool.data() + sd.off_su;
    const uint8_t* mk = S.mask_pool.data() + sd.off_mask;
    const int32_t* ds = S.dest_pool.data() + sd.off_dest;
    const int32_t c = S.sub_col[sd.out_index];
    const int32_t* hq = hr.data() + hp[q];
    const int nh = (int)(hp[q + 1] - hp[q]);
    auto zat = [&](int64_t t, int i) -> double {
      const int64_t e = t * nm + i;
      return (mk[e] && ds[e] >= 0) ? values[ds[e]] : 0.0;
    };
    double mx = 0.0, hmx = 0.0, eabs_max = 0.0;
    long double l1 = 0.0L, l1a = 0.0L;
    int64_t eterms_max = 0, l1n = 0;
    for (int64_t t = 0; t <= T; ++t) {
      for (int i = 0; i < n + nh; ++i) {
        const bool local = i < n;
        const int32_t r = local ? sx[i] : hq[i - n];
        long double d = 0.0L, da = 0.0L;
        int64_t nt = 0;
        if (local && t < T) { const double z = zat(t, i); d = z; da = std::fabs(z); ++nt; }
        if (t == 0) {
          if (r == c) { d -= 1.0L; da += 1.0L; ++nt; }
        } else {
          long double acc = 0.0L;
          for (int32_t e = S.A_csr.ptr[(size_t)r]; e < S.A_csr.ptr[(size_t)r + 1]; ++e) {
            const int32_t* f = std::lower_bound(sx, sx + n, S.A_csr.idx[(size_t)e]);
            if (f == sx + n || *f != S.A_csr.idx[(size_t)e]) continue;
            const long double pr = (long double)S.A_csr.val[(size_t)e] * (long double)zat(t - 1, (int)(f - sx));
            acc += pr; da += std::fabs(pr); ++nt;
          }
          for (int32_t e = S.B_csr.ptr[(size_t)r]; e < S.B_csr.ptr[(size_t)r + 1]; ++e) {
            const int32_t* f = std::lower_bound(su, su + sd.m, S.B_csr.idx[(size_t)e]);
            if (f == su + sd.m || *f != S.B_csr.idx[(size_t)e]) continue;
            const long double pr = (long double)S.B_csr.val[(size_t)e] * (long double)zat(t - 1, n + (int)(f - su));
            acc += pr; da += std::fabs(pr); ++nt;
          }
          d -= acc;
        }
        const double dd = (double)d;
        mx = resid_max(mx, dd);
        if (!local) hmx = resid_max(hmx, dd);
        l1 += std::fabs(d); l1a += da; l1n += nt + 1;
        eterms_max = std::max(eterms_max, nt);
        eabs_max = std::max(eabs_max, (double)da);
      }
    }
    const int64_t oi = sd.out_index;
    if (res_inf) res_inf[oi] = mx;
    if (halo_inf) halo_inf[oi] = hmx;
    if (res_l1) res_l1[oi] = (double)l1;
    if (ent_terms) ent_terms[oi] = eterms_max;
    if (ent_abs) ent_abs[oi] = eabs_max;
    if (l1_terms) l1_terms[oi] = l1n;
    if (l1_abs) l1_abs[oi] = (double)l1a;
    tot_inf = resid_max(tot_inf, mx);
    tot_l1 = resid_max(tot_l1, (double)l1);
  }
  if (totals) { totals[0] = tot_inf; totals[1] = tot_l1; }
  if (halo_ptr) halo_ptr->swap(hp);
  if (halo_rows) halo_rows->swap(hr);
  return 0;
}

}  // namespace sls
