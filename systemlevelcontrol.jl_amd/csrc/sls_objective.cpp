// sls_objective.cpp — see sls_objective.h.  Pure host code (compiled by hipcc or g++): the serial twin of sls_objective.hip.
#include "sls_objective.h"

#include <cmath>
#include <vector>

namespace sls {

int objective_host(const Symbolic& S, int objective, const double* values, double* col_objective, double* total,
                   int64_t* col_terms, double* col_abs, std::string& msg) {
  const int64_t ns = (int64_t)S.subs.size(), T = S.T;
  if (S.compact || (S.md_total > 0 && ((int64_t)S.mask_pool.size() != S.md_total || (int64_t)S.dest_pool.size() != S.md_total))) {
    msg = "objective_host needs the explicit mask / destination tables"; return SLS_EINVAL;
  }
  if ((int64_t)S.obj_pool.size() != 2 * ns) { msg = "objective_host: no objective records in this symbolic pass"; return SLS_EINVAL; }
  if (!values && S.n_values > 0) { msg = "null value array"; return SLS_EINVAL; }
  double tot = 0.0;
  std::vector<double> y, ya;
  for (int64_t q = 0; q < ns; ++q) {
    const SubDesc& sd = S.subs[q];
    const int nm = sd.n + sd.m;
    const double scale = S.obj_pool[2 * q], c0 = S.obj_pool[2 * q + 1];
    const uint8_t* mk = S.mask_pool.data() + sd.off_mask;
    const int32_t* ds = S.dest_pool.data() + sd.off_dest;
    auto zat = [&](const uint8_t* mkc, const int32_t* dsc, int64_t t, int i) -> double {
      return mkc[t * nm + i] ? values[dsc[t * nm + i]] : 0.0;
    };
    double val = 0.0, aval = 0.0;
    int64_t nterms = 0;
    if (sd.has_w == 4) {
      val = 0.0;
    } else if (sd.has_w <= 1) {
      const double* hinv = sd.has_w ? S.w_pool.data() + sd.off_w : nullptr;
      const double* g = sd.has_w ? hinv + nm : nullptr;
      double acc = 0.0, aacc = 0.0;
      for (int64_t t = 0; t < T; ++t) {
        double qt = 0.0;
        for (int i = 0; i < nm; ++i) {
          if (!mk[t * nm + i]) continue;
          const double z = values[ds[t * nm + i]];
          const double w = hinv ? 1.0 / hinv[i] : 1.0;
          qt += w * (z * z); ++nterms;
          if (objective == 0) {
            acc += w * (z * z); aacc += w * (z * z);
            if (g) { acc += 2.0 * g[i] * z; aacc += std::fabs(2.0 * g[i] * z); ++nterms; }
          }
        }
        if (objective == 1) { const double nt = std::sqrt(sd.has_w ? qt : scale * qt); acc += nt; aacc += nt; }
      }
      if (objective == 0 && !sd.has_w) { acc *= scale; aacc *= scale; }
      val = acc + c0; aval = aacc + std::fabs(c0);
    } else {
      const GeneralRecord R = parse_general_record(S.w_pool.data() + sd.off_w, nm, sd.has_w == 3);
      const int nc = R.nc;
      y.assign((size_t)nc, 0.0); ya.assign((size_t)nc, 0.0);
      double acc = 0.0, aacc = 0.0;
      for (int64_t t = 0; t < T; ++t) {
        for (int zr = 0; zr < R.nz; ++zr) {
          for (int c = 0; c < nc; ++c) {
            const SubDesc& sc = S.subs[q + c];
            const uint8_t* mkc = S.mask_pool.data() + sc.off_mask;
            const int32_t* dsc = S.dest_pool.data() + sc.off_dest;
            double s = 0.0, sa = 0.0;
            for (int e = (int)R.rp[zr]; e < (int)R.rp[zr + 1]; ++e) {
              const double z = zat(mkc, dsc, t, (int)R.ri[e]);
              s += R.rv[e] * z; sa += std::fabs(R.rv[e] * z); ++nterms;
            }
            y[c] = s; ya[c] = sa;
          }
          for (int c = 0; c < nc; ++c) {
            double r = 0.0, ra = 0.0;
            for (int c2 = 0; c2 < nc; ++c2) {
              const double mcc = R.M ? R.M[(size_t)c * nc + c2] : 1.0;
              r += mcc * y[c2]; ra += std::fabs(mcc) * ya[c2]; ++nterms;
            }
            acc += y[c] * r; aacc += ya[c] * ra; ++nterms;
          }
        }
        for (int c = 0; c < nc; ++c) {
          const SubDesc& sc = S.subs[q + c];
          const uint8_t* mkc = S.mask_pool.data() + sc.off_mask;
          const int32_t* dsc = S.dest_pool.data() + sc.off_dest;
          const double* g = S.w_pool.data() + sc.off_w + nm;
          for (int i = 0; i < nm; ++i) {
            if (!mkc[t * nm + i]) continue;
            const double z = values[dsc[t * nm + i]];
            const double lin = 2.0 * g[i] * z + R.ridge[i] * (z * z);
            acc += lin; aacc += std::fabs(2.0 * g[i] * z) + R.ridge[i] * (z * z); nterms += 2;
          }
        }
      }
      val = acc + c0; aval = aacc + std::fabs(c0);
    }
    if (col_objective) col_objective[q] = val;
    if (col_terms) col_terms[q] = nterms + 1;
    if (col_abs) col_abs[q] = aval;
    tot += val;
  }
  if (total) *total = tot;
  return 0;
}

}  // namespace sls
