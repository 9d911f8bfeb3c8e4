// Host side of the gradient pass (csrc/sls_gradient.cpp with the symbolic pass of csrc/sls_symbolic.cpp — no HIP in either)
// under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_gradient_host.py::test_host_code_under_sanitizers with g++ -fsanitize=address,undefined.  Drives
// sls::build_gradient_tables and sls::gradient_host over a chain and a grid plant in both index bases, single columns and pair
// groups, a shard of the groups, with random multipliers and values; checks what must hold exactly: every listed entry lies
// inside its subproblem's index sets and names the stored entry it claims, the inverse map is a permutation of the slots in
// ascending subproblem order, a skipped column and a zero column weight contribute 0, Σ|terms| bounds |g|, both index bases
// give the same bits.  Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_gradient.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"

namespace {

struct Csc {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> v;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
  sls_csc_bool boolean() const { return sls_csc_bool{nr, nc, cp.data(), ri.data(), nullptr}; }
};
using Dense = std::vector<std::vector<double>>;
Dense zeros(int64_t r, int64_t c) { return Dense(r, std::vector<double>(c, 0.0)); }
Csc from_dense(const Dense& M, int64_t nr, int64_t nc, int base) {
  Csc m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r)
      if (M[r][c] != 0.0) { m.ri.push_back(r + base); m.v.push_back(M[r][c]); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Out { std::vector<double> gA, gB; int64_t nsub = 0; };

Out run(int64_t Nx, bool grid, bool pairs, int base, int64_t gbeg_frac, int64_t gend_frac) {
  const int64_t T = 5, Nu = (Nx + 1) / 2;
  Dense A = zeros(Nx, Nx), B1 = zeros(Nx, Nx), B2 = zeros(Nx, Nu);
  const int64_t side = grid ? (int64_t)std::llround(std::sqrt((double)Nx)) : 0;
  for (int64_t i = 0; i < Nx; ++i) {
    A[i][i] = 1.0; B1[i][i] = 1.0 + 0.01 * i;
    if (!grid && i + 1 < Nx) { A[i][i + 1] = 0.2; A[i + 1][i] = -0.2; }
    if (grid) {
      if ((i + 1) % side != 0) { A[i][i + 1] = 0.1; A[i + 1][i] = 0.1; }
      if (i + side < Nx) { A[i][i + side] = 0.1; A[i + side][i] = 0.1; }
    }
  }
  B1[3][3] = 0.0;                                                        // a column with a constant cost
  for (int64_t j = 0; j < Nu; ++j) B2[std::min(Nx - 1, 2 * j)][j] = 1.0;
  const Csc cA = from_dense(A, Nx, Nx, base), cB1 = from_dense(B1, Nx, Nx, base), cB2 = from_dense(B2, Nx, Nu, base);
  std::vector<int64_t> gptr, gcols;
  if (pairs) {
    gptr.push_back(0);
    for (int64_t c = 0; c < Nx; c += 2) { gcols.push_back(c + base); if (c + 1 < Nx) gcols.push_back(c + 1 + base); gptr.push_back((int64_t)gcols.size()); }
  }
  sls_dims dims{Nx, Nu, Nx + Nu, Nx, T, base, 0};
  sls_csc_f64 Af = cA.f64(), B1f = cB1.f64(), B2f = cB2.f64();
  std::vector<int64_t> nx(T), nu(T);
  std::string msg;
  EXPECT(sls::localization_masks(&dims, &Af, &B2f, 2, 1.5, nx.data(), nu.data(), nullptr, nullptr, nullptr, nullptr, msg) == 0, "mask recipe (count)");
  std::vector<Csc> mx(T), mu(T);
  std::vector<int64_t*> cpx(T), rvx(T), cpu(T), rvu(T);
  for (int64_t t = 0; t < T; ++t) {
    mx[t].nr = Nx; mx[t].nc = Nx; mx[t].cp.assign(Nx + 1, 0); mx[t].ri.assign(nx[t], 0);
    mu[t].nr = Nu; mu[t].nc = Nx; mu[t].cp.assign(Nx + 1, 0); mu[t].ri.assign(nu[t], 0);
    cpx[t] = mx[t].cp.data(); rvx[t] = mx[t].ri.data(); cpu[t] = mu[t].cp.data(); rvu[t] = mu[t].ri.data();
  }
  EXPECT(sls::localization_masks(&dims, &Af, &B2f, 2, 1.5, nx.data(), nu.data(), cpx.data(), rvx.data(), cpu.data(), rvu.data(), msg) == 0, "mask recipe (fill)");
  std::vector<sls_csc_bool> bx, bu;
  for (int64_t t = 0; t < T; ++t) { bx.push_back(mx[t].boolean()); bu.push_back(mu[t].boolean()); }
  sls_plant plant{&Af, &B1f, &B2f, nullptr, nullptr, nullptr};
  const int64_t ng = gptr.empty() ? 0 : (int64_t)gptr.size() - 1;
  sls::Inputs in{&dims, &plant, bx.data(), bu.data(), ng, ng ? gptr.data() : nullptr, ng ? gcols.data() : nullptr};
  Out R;
  int rc = sls::validate_inputs(in, msg);
  EXPECT(rc == 0, "validate_inputs");
  if (rc) return R;
  const int64_t n_groups = ng ? ng : Nx;
  sls::Symbolic S; S.want_packed = false; S.compact = false;
  rc = sls::build_symbolic(in, n_groups * gbeg_frac / 4, n_groups * gend_frac / 4, S, msg);
  EXPECT(rc == 0, "build_symbolic");
  if (rc) return R;
  const int64_t ns = (int64_t)S.subs.size();
  R.nsub = ns;
  EXPECT((int64_t)S.b_zero.size() == ns, "b_zero per subproblem");
  sls::GradientTables G;
  sls::build_gradient_tables(S.At_csr, S.Bt_csr, S.subs.data(), ns, S.idx_pool.data(), G);
  const int64_t nA = G.nnzA, nB = G.nnzB, nslot = G.ent_ptr[(size_t)ns];
  EXPECT(nA == (int64_t)cA.v.size() && nB == (int64_t)cB2.v.size(), "entry counts");
  EXPECT((int64_t)G.ent.size() == 3 * nslot && (int64_t)G.inv_slot.size() == nslot && G.inv_ptr[(size_t)(nA + nB)] == nslot, "table sizes");
  for (int64_t q = 0; q < ns; ++q) {
    const sls::SubDesc& sd = S.subs[q];
    for (int64_t e = G.ent_ptr[(size_t)q]; e < G.ent_ptr[(size_t)q + 1]; ++e) {
      const int32_t pos = G.ent[3 * e], a = G.ent[3 * e + 1], b = G.ent[3 * e + 2];
      const bool isA = pos < nA;
      EXPECT(a >= 0 && a < sd.n && b >= 0 && b < (isA ? sd.n : sd.m), "local indices inside the index sets");
      const sls::HostCsr& M = isA ? S.At_csr : S.Bt_csr;
      const int64_t k = isA ? pos : pos - nA;
      const int32_t gc = S.idx_pool[(isA ? sd.off_sx : sd.off_su) + b];
      EXPECT(k >= M.ptr[gc] && k < M.ptr[gc + 1] && M.idx[k] == S.idx_pool[sd.off_sx + a], "the slot names its stored entry");
    }
  }
  std::vector<char> seen((size_t)nslot, 0);
  for (int64_t p = 0; p < nA + nB; ++p)
    for (int64_t w = G.inv_ptr[(size_t)p]; w < G.inv_ptr[(size_t)p + 1]; ++w) {
      const int64_t e = G.inv_slot[(size_t)w];
      EXPECT(e >= 0 && e < nslot && !seen[(size_t)e] && G.ent[3 * e] == p, "inverse map");
      if (e >= 0 && e < nslot) seen[(size_t)e] = 1;
      if (w > G.inv_ptr[(size_t)p]) EXPECT(G.inv_sub[(size_t)w] > G.inv_sub[(size_t)w - 1], "ascending subproblems");
    }
  // twin on random multipliers and values
  int64_t nmu = 0;
  for (const sls::SubDesc& sd : S.subs) nmu += (T + 1) * sd.n;
  std::mt19937 g(11);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> muv((size_t)nmu + 1), vals((size_t)S.n_values + 1), cw((size_t)ns, 1.0);
  for (double& v : muv) v = u(g);
  for (double& v : vals) v = u(g);
  std::vector<int32_t> st((size_t)ns, SLS_COL_OK);
  if (ns > 2) { st[1] = SLS_COL_INFEASIBLE; cw[2] = 0.0; }
  R.gA.assign((size_t)nA, -1.0); R.gB.assign((size_t)nB, -1.0);
  std::vector<double> aA((size_t)nA), aB((size_t)nB);
  std::vector<int64_t> tA((size_t)nA), tB((size_t)nB);
  rc = sls::gradient_host(S, G, muv.data(), vals.data(), st.data(), cw.data(), S.b_zero.data(), R.gA.data(), R.gB.data(), aA.data(), aB.data(),
                          tA.data(), tB.data(), msg);
  EXPECT(rc == 0, "gradient_host");
  for (int64_t k = 0; k < nA; ++k) EXPECT(std::isfinite(R.gA[k]) && aA[k] >= std::fabs(R.gA[k]) * (1.0 - 1e-12) && tA[k] >= 0, "value / bound terms (A)");
  for (int64_t k = 0; k < nB; ++k) EXPECT(std::isfinite(R.gB[k]) && aB[k] >= std::fabs(R.gB[k]) * (1.0 - 1e-12) && tB[k] >= 0, "value / bound terms (B2)");
  // with every column skipped the gradient is exactly 0
  std::vector<int32_t> none((size_t)ns, SLS_COL_NOTCONV);
  std::vector<double> zA((size_t)nA, -1.0), zB((size_t)nB, -1.0);
  EXPECT(sls::gradient_host(S, G, muv.data(), vals.data(), none.data(), nullptr, nullptr, zA.data(), zB.data(), nullptr, nullptr, nullptr, nullptr, msg) == 0, "all skipped");
  for (double v : zA) EXPECT(v == 0.0, "skipped columns contribute 0");
  for (double v : zB) EXPECT(v == 0.0, "skipped columns contribute 0");
  EXPECT(sls::gradient_host(S, G, muv.data(), vals.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, msg) == 0, "all outputs null");
  sls::Symbolic Sc; Sc.want_packed = false; Sc.compact = true;
  if (sls::build_symbolic(in, 0, n_groups, Sc, msg) == 0 && Sc.compact && gbeg_frac == 0 && gend_frac == 4)
    EXPECT(sls::gradient_host(Sc, G, muv.data(), vals.data(), nullptr, nullptr, nullptr, zA.data(), zB.data(), nullptr, nullptr, nullptr, nullptr, msg) == SLS_EINVAL, "compact tables accepted");
  return R;
}

}  // namespace

int main() {
  for (int grid = 0; grid < 2; ++grid)
    for (int pairs = 0; pairs < 2; ++pairs) {
      Out r[2];
      for (int base = 0; base < 2; ++base) {
        r[base] = run(grid ? 36 : 30, grid != 0, pairs != 0, base, 0, 4);
        run(grid ? 36 : 30, grid != 0, pairs != 0, base, 1, 3);              // a shard in the middle
      }
      EXPECT(r[0].nsub == r[1].nsub && r[0].gA == r[1].gA && r[0].gB == r[1].gB, "index bases disagree");
      std::printf("%s pairs=%d: %lld subproblems\n", grid ? "grid36" : "chain30", pairs, (long long)r[0].nsub);
    }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_gradient: clean\n");
  return 0;
}
