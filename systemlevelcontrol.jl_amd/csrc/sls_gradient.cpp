// sls_gradient.cpp — see sls_gradient.h.  Pure host code (compiled by hipcc or g++): the entry tables of the gradient pass and the
// serial twin of sls_gradient.hip.
#include "sls_gradient.h"

#include <algorithm>
#include <cmath>

namespace sls {

void build_gradient_tables(const HostCsr& At, const HostCsr& Bt, const SubDesc* subs, int64_t nsub, const int32_t* idx_pool,
                           GradientTables& G) {
  G = GradientTables{};
  G.nnzA = (int64_t)At.idx.size(); G.nnzB = (int64_t)Bt.idx.size();
  G.Nx = At.nrows; G.Nu = Bt.nrows;
  const int64_t nent = G.nnzA + G.nnzB, nvar = G.Nx + G.Nu;
  G.ent_ptr.assign((size_t)nsub + 1, 0);
  G.w_base.assign((size_t)nsub + 1, 0);
  std::vector<int32_t> loc((size_t)std::max<int64_t>(G.Nx, 1), -1);          // global state → local row of the subproblem at hand
  std::vector<int64_t> cnt((size_t)nent + 1, 0), wcnt((size_t)nvar + 1, 0);
  for (int64_t q = 0; q < nsub; ++q) {
    const SubDesc& sd = subs[q];
    const int32_t* sx = idx_pool + sd.off_sx;
    const int32_t* su = idx_pool + sd.off_su;
    for (int32_t i = 0; i < sd.n; ++i) loc[(size_t)sx[i]] = i;
    for (int half = 0; half < 2; ++half) {
      const HostCsr& M = half ? Bt : At;
      const int32_t* cols = half ? su : sx;
      const int32_t nc = half ? sd.m : sd.n;
      const int64_t first = half ? G.nnzA : 0;
      for (int32_t b = 0; b < nc; ++b) {
        const int32_t gc = cols[b];
        for (int32_t k = M.ptr[(size_t)gc]; k < M.ptr[(size_t)gc + 1]; ++k) {
          const int32_t a = loc[(size_t)M.idx[(size_t)k]];
          if (a < 0) continue;
          G.ent.push_back((int32_t)(first + k)); G.ent.push_back(a); G.ent.push_back(b);
          ++cnt[(size_t)(first + k) + 1];
        }
      }
    }
    for (int32_t i = 0; i < sd.n; ++i) { loc[(size_t)sx[i]] = -1; ++wcnt[(size_t)sx[i] + 1]; }
    for (int32_t i = 0; i < sd.m; ++i) ++wcnt[(size_t)(G.Nx + su[i]) + 1];
    G.ent_ptr[(size_t)q + 1] = (int64_t)G.ent.size() / 3;
    G.w_base[(size_t)q + 1] = G.w_base[(size_t)q] + sd.n + sd.m;
  }
  // inverse maps: a walk over the subproblems in ascending order fills every owner's list in that order
  for (int64_t p = 0; p < nent; ++p) cnt[(size_t)p + 1] += cnt[(size_t)p];
  for (int64_t v = 0; v < nvar; ++v) wcnt[(size_t)v + 1] += wcnt[(size_t)v];
  G.inv_ptr = cnt; G.winv_ptr = wcnt;
  G.inv_slot.assign((size_t)G.ent_ptr[(size_t)nsub], 0); G.inv_sub.assign((size_t)G.ent_ptr[(size_t)nsub], 0);
  G.winv_slot.assign((size_t)G.w_base[(size_t)nsub], 0);
  std::vector<int64_t> at(cnt.begin(), cnt.end() - 1), wat(wcnt.begin(), wcnt.end() - 1);
  for (int64_t q = 0; q < nsub; ++q) {
    const SubDesc& sd = subs[q];
    for (int64_t e = G.ent_ptr[(size_t)q]; e < G.ent_ptr[(size_t)q + 1]; ++e) {
      const int64_t w = at[(size_t)G.ent[(size_t)(3 * e)]]++;
      G.inv_slot[(size_t)w] = e; G.inv_sub[(size_t)w] = (int32_t)q;
    }
    for (int32_t i = 0; i < sd.n + sd.m; ++i) {
      const int64_t v = i < sd.n ? idx_pool[sd.off_sx + i] : G.Nx + idx_pool[sd.off_su + (i - sd.n)];
      G.winv_slot[(size_t)wat[(size_t)v]++] = G.w_base[(size_t)q] + i;
    }
  }
}

int gradient_host(const Symbolic& S, const GradientTables& G, const double* mu, const double* values, const int32_t* status,
                  const double* col_weight, const uint8_t* b_zero, double* gA, double* gB2, double* abs_A, double* abs_B2,
                  int64_t* terms_A, int64_t* terms_B2, std::string& msg) {
  const int64_t ns = (int64_t)S.subs.size(), T = S.T;
  if (S.compact || (S.md_total > 0 && ((int64_t)S.mask_pool.size() != S.md_total || (int64_t)S.dest_pool.size() != S.md_total))) {
    msg = "gradient_host needs the explicit mask / destination tables"; return SLS_EINVAL;
  }
  if ((int64_t)G.ent_ptr.size() != ns + 1) { msg = "gradient_host: the tables belong to another symbolic pass"; return SLS_EINVAL; }
  if ((!mu || !values) && ns > 0) { msg = "null multiplier or value array"; return SLS_EINVAL; }
  const int64_t nent = G.nnzA + G.nnzB;
  std::vector<long double> contrib((size_t)std::max<int64_t>(G.ent_ptr[(size_t)ns], 1), 0.0L), cabs(contrib.size(), 0.0L);
  int64_t mu_off = 0;
  for (int64_t q = 0; q < ns; ++q) {
    const SubDesc& sd = S.subs[q];
    const int n = sd.n, nm = sd.n + sd.m;
    const double* muq = mu + mu_off;
    mu_off += (T + 1) * n;
    const bool live = (!status || status[q] == SLS_COL_OK || status[q] == SLS_COL_TRIVIAL) && !(b_zero && b_zero[q]);
    if (!live) continue;
    const uint8_t* mk = S.mask_pool.data() + sd.off_mask;
    const int32_t* ds = S.dest_pool.data() + sd.off_dest;
    const long double cw = col_weight ? (long double)col_weight[q] : 1.0L;
    for (int64_t e = G.ent_ptr[(size_t)q]; e < G.ent_ptr[(size_t)q + 1]; ++e) {
      const int32_t pos = G.ent[(size_t)(3 * e)], a = G.ent[(size_t)(3 * e + 1)], b = G.ent[(size_t)(3 * e + 2)];
      const int i = pos < G.nnzA ? b : n + b;
      long double acc = 0.0L, aacc = 0.0L;
      for (int64_t k = 1; k <= T; ++k) {
        const int64_t s = (k - 1) * nm + i;
        const double z = (mk[s] && ds[s] >= 0) ? values[ds[s]] : 0.0;
        const long double term = (long double)muq[k * n + a] * (long double)z;
        acc += term; aacc += fabsl(term);
      }
      contrib[(size_t)e] = cw * acc; cabs[(size_t)e] = fabsl(cw) * aacc;
    }
  }
  for (int64_t p = 0; p < nent; ++p) {
    long double g = 0.0L, ga = 0.0L;
    for (int64_t w = G.inv_ptr[(size_t)p]; w < G.inv_ptr[(size_t)p + 1]; ++w) { g += contrib[(size_t)G.inv_slot[(size_t)w]]; ga += cabs[(size_t)G.inv_slot[(size_t)w]]; }
    const int64_t nt = (G.inv_ptr[(size_t)p + 1] - G.inv_ptr[(size_t)p]) * T;
    const bool isA = p < G.nnzA;
    const int64_t k = isA ? p : p - G.nnzA;
    if (double* o = isA ? gA : gB2) o[k] = (double)g;
    if (double* o = isA ? abs_A : abs_B2) o[k] = (double)ga;
    if (int64_t* o = isA ? terms_A : terms_B2) o[k] = nt;
  }
  return 0;
}

}  // namespace sls
