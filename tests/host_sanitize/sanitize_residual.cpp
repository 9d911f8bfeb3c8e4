// Host residual evaluator (csrc/sls_residual.cpp with the symbolic pass of csrc/sls_symbolic.cpp — no HIP in either) under
// AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_residual_host.py::test_host_twin_under_sanitizers with g++ -fsanitize=address,undefined.  Drives
// sls::residual_host over two cases — a chain whose last mask is narrower than the earlier ones, with an actuator that has a
// second entry five states away (halo rows from A and from B2), and a grid in pair groups (shared index sets) — in both index
// bases, whole and as a shard; checks what must hold exactly (the halo ascends and avoids s_x, halo_inf = 0.0 where it is empty,
// halo_inf ≤ res_inf ≤ res_l1, the totals are the maxima, both index bases give the same bits).  Exit code 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_residual.h"
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

struct Problem {
  int64_t Nx, Nu, T;
  Csc A, B1, B2;
  std::vector<Csc> mx, mu;
  std::vector<sls_csc_bool> bx, bu;
  std::vector<int64_t> gptr, gcols;
};

Problem make(bool grid, int base) {
  Problem p; p.Nx = grid ? 36 : 30; p.T = 5;
  const int64_t Nx = p.Nx, side = 6;
  Dense A = zeros(Nx, Nx), B1 = zeros(Nx, Nx);
  for (int64_t i = 0; i < Nx; ++i) {
    A[i][i] = 1.0; B1[i][i] = 1.0;
    if (!grid && i + 1 < Nx) { A[i][i + 1] = 0.2; A[i + 1][i] = -0.2; }
    if (grid) {
      if ((i + 1) % side != 0) { A[i][i + 1] = 0.1; A[i + 1][i] = 0.1; }
      if (i + side < Nx) { A[i][i + side] = 0.1; A[i + side][i] = 0.1; }
    }
  }
  p.Nu = (Nx + 1) / 2;
  Dense B2 = zeros(Nx, p.Nu);
  for (int64_t j = 0; j < p.Nu; ++j) B2[std::min(Nx - 1, 2 * j)][j] = 1.0;
  p.A = from_dense(A, Nx, Nx, base); p.B1 = from_dense(B1, Nx, Nx, base);
  // masks from the library's own recipe, computed BEFORE the far entry of B2 exists; the chain then gets the previous (wider
  // or equal) step's masks shifted one step later, so that its last mask is the narrowest … and the far entry leaves s_x
  Csc B2m = from_dense(B2, Nx, p.Nu, base);
  if (!grid) B2[15][5] = 0.5;                            // actuator 5 sits on state 10
  p.B2 = from_dense(B2, Nx, p.Nu, base);
  sls_dims dims{Nx, p.Nu, Nx + p.Nu, Nx, p.T, base, 0};
  sls_csc_f64 Af = p.A.f64(), B2f = B2m.f64();
  std::vector<int64_t> nx(p.T), nu(p.T);
  std::string msg;
  EXPECT(sls::localization_masks(&dims, &Af, &B2f, 2, 1.5, nx.data(), nu.data(), nullptr, nullptr, nullptr, nullptr, msg) == 0, "mask recipe (count)");
  p.mx.resize(p.T); p.mu.resize(p.T);
  std::vector<int64_t*> cpx(p.T), rvx(p.T), cpu(p.T), rvu(p.T);
  for (int64_t t = 0; t < p.T; ++t) {
    p.mx[t].nr = Nx; p.mx[t].nc = Nx; p.mx[t].cp.assign(Nx + 1, 0); p.mx[t].ri.assign(nx[t], 0);
    p.mu[t].nr = p.Nu; p.mu[t].nc = Nx; p.mu[t].cp.assign(Nx + 1, 0); p.mu[t].ri.assign(nu[t], 0);
    cpx[t] = p.mx[t].cp.data(); rvx[t] = p.mx[t].ri.data(); cpu[t] = p.mu[t].cp.data(); rvu[t] = p.mu[t].ri.data();
  }
  EXPECT(sls::localization_masks(&dims, &Af, &B2f, 2, 1.5, nx.data(), nu.data(), cpx.data(), rvx.data(), cpu.data(), rvu.data(), msg) == 0, "mask recipe (fill)");
  if (!grid) {                                           // last step: the level-1 masks of step 1 (kx = ku = 1) instead of level 2 / 3
    p.mx[p.T - 1] = p.mx[1]; p.mu[p.T - 1] = p.mu[1];
  } else {                                               // pair groups: columns (c, c + 1) share one index set
    p.gptr.push_back(0);
    for (int64_t c = 0; c < Nx; c += 2) { p.gcols.push_back(c + base); p.gcols.push_back(c + 1 + base); p.gptr.push_back((int64_t)p.gcols.size()); }
  }
  for (int64_t t = 0; t < p.T; ++t) { p.bx.push_back(p.mx[t].boolean()); p.bu.push_back(p.mu[t].boolean()); }
  return p;
}

struct Result { std::vector<double> inf, halo, l1; double totals[2] = {0.0, 0.0}; int64_t nsub = 0, nhalo = 0; };

Result evaluate(const Problem& p, int base, int64_t gbeg_frac, int64_t gend_frac) {
  sls_dims dims{p.Nx, p.Nu, p.Nx + p.Nu, p.Nx, p.T, base, 0};
  sls_csc_f64 A = p.A.f64(), B1 = p.B1.f64(), B2 = p.B2.f64();
  sls_plant plant{&A, &B1, &B2, nullptr, nullptr, nullptr};
  const int64_t ng = p.gptr.empty() ? 0 : (int64_t)p.gptr.size() - 1;
  sls::Inputs in{&dims, &plant, p.bx.data(), p.bu.data(), ng, ng ? p.gptr.data() : nullptr, ng ? p.gcols.data() : nullptr};
  std::string msg;
  Result R;
  int rc = sls::validate_inputs(in, msg);
  EXPECT(rc == 0, "validate_inputs");
  if (rc) return R;
  const int64_t n_groups = ng ? ng : p.Nx;
  sls::Symbolic S; S.want_packed = false; S.compact = false;
  rc = sls::build_symbolic(in, n_groups * gbeg_frac / 4, n_groups * gend_frac / 4, S, msg);
  EXPECT(rc == 0, "build_symbolic");
  if (rc) return R;
  std::vector<double> vals((size_t)S.n_values + 1);
  std::mt19937 g(11);                                  // the same Φ for both index bases
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (double& v : vals) v = u(g);
  R.nsub = (int64_t)S.subs.size();
  R.inf.assign((size_t)R.nsub, -1.0); R.halo.assign((size_t)R.nsub, -1.0); R.l1.assign((size_t)R.nsub, -1.0);
  std::vector<int64_t> et((size_t)R.nsub), lt((size_t)R.nsub), hp;
  std::vector<double> ea((size_t)R.nsub), la((size_t)R.nsub);
  std::vector<int32_t> hr;
  rc = sls::residual_host(S, vals.data(), R.inf.data(), R.halo.data(), R.l1.data(), R.totals, et.data(), ea.data(), lt.data(), la.data(), &hp, &hr, msg);
  EXPECT(rc == 0, "residual_host");
  if (rc) return R;
  EXPECT((int64_t)hp.size() == R.nsub + 1 && hp[0] == 0 && hp[(size_t)R.nsub] == (int64_t)hr.size(), "halo offsets");
  R.nhalo = (int64_t)hr.size();
  double mi = 0.0, ml = 0.0;
  for (int64_t q = 0; q < R.nsub; ++q) {
    const sls::SubDesc& sd = S.subs[q];
    const int64_t oi = sd.out_index;
    const int32_t* sx = S.idx_pool.data() + sd.off_sx;
    for (int64_t k = hp[q]; k < hp[q + 1]; ++k) {
      EXPECT(hr[k] >= 0 && hr[k] < p.Nx && (k == hp[q] || hr[k - 1] < hr[k]), "halo rows ascend inside the plant");
      EXPECT(!std::binary_search(sx, sx + sd.n, hr[k]), "a halo row lies in s_x");
    }
    if (hp[q] == hp[q + 1]) EXPECT(R.halo[oi] == 0.0 && !std::signbit(R.halo[oi]), "empty halo must report 0.0");
    EXPECT(std::isfinite(R.l1[oi]) && R.halo[oi] <= R.inf[oi] && R.inf[oi] <= R.l1[oi], "halo_inf ≤ res_inf ≤ res_l1");
    EXPECT(et[oi] >= 1 && lt[oi] >= et[oi] && ea[oi] >= R.inf[oi] * (1.0 - 1e-12) && la[oi] >= R.l1[oi] * (1.0 - 1e-12), "bound terms");
    mi = std::max(mi, R.inf[oi]); ml = std::max(ml, R.l1[oi]);
  }
  EXPECT(mi == R.totals[0] && ml == R.totals[1], "totals are the maxima");
  // nullable outputs
  EXPECT(sls::residual_host(S, vals.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, msg) == 0, "all outputs null");
  // a compact pass has no explicit tables: refused, not read out of bounds
  sls::Symbolic Sc; Sc.want_packed = false; Sc.compact = true;
  if (sls::build_symbolic(in, 0, n_groups, Sc, msg) == 0 && Sc.compact)
    EXPECT(sls::residual_host(Sc, vals.data(), R.inf.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, msg) == SLS_EINVAL, "compact tables accepted");
  return R;
}

}  // namespace

int main() {
  for (int grid = 0; grid < 2; ++grid) {
    Result r[2];
    for (int base = 0; base < 2; ++base) {
      const Problem p = make(grid != 0, base);
      r[base] = evaluate(p, base, 0, 4);
      evaluate(p, base, 1, 3);                                            // a shard in the middle
    }
    EXPECT(r[0].nsub == r[1].nsub && r[0].inf == r[1].inf && r[0].halo == r[1].halo && r[0].l1 == r[1].l1 &&
           r[0].totals[0] == r[1].totals[0] && r[0].totals[1] == r[1].totals[1], "index bases disagree");
    if (!grid) EXPECT(r[0].nhalo > 0, "the chain case must have halo rows");
    std::printf("%s: %lld subproblems, %lld halo rows, max res_inf %.6g, E1 norm %.6g\n", grid ? "grid36" : "chain30", (long long)r[0].nsub,
                (long long)r[0].nhalo, r[0].totals[0], r[0].totals[1]);
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_residual: clean\n");
  return 0;
}
