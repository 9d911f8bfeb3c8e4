// Host objective evaluator (csrc/sls_objective.cpp with the symbolic pass of csrc/sls_symbolic.cpp — no HIP in either) under
// AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_objective_host.py::test_host_evaluator_under_sanitizers with g++ -fsanitize=address,undefined.  Drives
// sls::objective_host over a chain and a grid plant in both index bases with every kind of objective record: identity cost,
// a b = 0 column, diagonal weights with D11, a dense [C1 D12], coupled groups (non-diagonal B1 block), a ridge term, the
// sum-of-norms objective, a shard of the groups; checks what must hold exactly (members of a coupled group report 0.0, the
// total is the sum, both index bases give the same bits, the identity cost is Σz²).  Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_objective.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"

namespace {

struct Csc {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> v;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
  sls_csc_bool boolean() const { return sls_csc_bool{nr, nc, cp.data(), ri.data(), nullptr}; }
};

Csc from_dense(const std::vector<std::vector<double>>& M, int64_t nr, int64_t nc, int base) {
  Csc m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r)
      if (M[r][c] != 0.0) { m.ri.push_back(r + base); m.v.push_back(M[r][c]); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}
using Dense = std::vector<std::vector<double>>;
Dense zeros(int64_t r, int64_t c) { return Dense(r, std::vector<double>(c, 0.0)); }

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Problem {
  int64_t Nx, Nu, T;
  Csc A, B1, B2, C1, D11, D12;
  bool weights = false;
  std::vector<Csc> mx, mu;
  std::vector<sls_csc_bool> bx, bu;
  std::vector<int64_t> gptr, gcols;
  std::vector<double> rx, ru;
};

// kind: 0 identity cost (one b = 0 column), 1 diagonal weights + D11, 2 banded [C1 D12] + D11, 3 = 2 with B1 coupling the
// columns of pair groups, 4 = identity cost with a ridge term
Problem make(int64_t Nx, bool grid, int kind, int base) {
  Problem p; p.Nx = Nx; p.T = 6;
  Dense A = zeros(Nx, Nx), B1 = zeros(Nx, Nx);
  const int64_t side = grid ? (int64_t)std::llround(std::sqrt((double)Nx)) : 0;
  for (int64_t i = 0; i < Nx; ++i) {
    A[i][i] = 1.0; B1[i][i] = 1.0 + 0.01 * i;
    if (!grid && i + 1 < Nx) { A[i][i + 1] = 0.2; A[i + 1][i] = -0.2; }
    if (grid) {
      if ((i + 1) % side != 0) { A[i][i + 1] = 0.1; A[i + 1][i] = 0.1; }
      if (i + side < Nx) { A[i][i + side] = 0.1; A[i + side][i] = 0.1; }
    }
  }
  if (kind == 0) B1[3][3] = 0.0;
  p.Nu = (Nx + 1) / 2;
  Dense B2 = zeros(Nx, p.Nu);
  for (int64_t j = 0; j < p.Nu; ++j) B2[std::min(Nx - 1, 2 * j)][j] = 1.0;
  const int64_t Nz = Nx + p.Nu;
  if (kind == 3) {
    for (int64_t c = 0; c + 1 < Nx; c += 4) { B1[c][c + 1] = 0.3; B1[c + 1][c] = -0.2; }
    p.gptr.push_back(0);
    for (int64_t c = 0; c < Nx; c += 4) {
      p.gcols.push_back(c + base); if (c + 1 < Nx) p.gcols.push_back(c + 1 + base);
      p.gptr.push_back((int64_t)p.gcols.size());
    }
  }
  p.A = from_dense(A, Nx, Nx, base); p.B1 = from_dense(B1, Nx, Nx, base); p.B2 = from_dense(B2, Nx, p.Nu, base);
  if (kind >= 1 && kind <= 3) {
    p.weights = true;
    Dense W = zeros(Nz, Nz), D11 = zeros(Nz, Nx);
    for (int64_t z = 0; z < Nz; ++z) { W[z][z] = 1.0 + 0.05 * (z % 7); if (kind >= 2 && z + 1 < Nz) W[z][z + 1] = 0.25; }
    for (int64_t c = 0; c < Nx; ++c) { D11[c][c] = 0.1 * (1 + c % 3); D11[(c + 2) % Nz][c] = -0.05; }
    Dense C1 = zeros(Nz, Nx), D12 = zeros(Nz, p.Nu);
    for (int64_t z = 0; z < Nz; ++z) { for (int64_t c = 0; c < Nx; ++c) C1[z][c] = W[z][c]; for (int64_t c = 0; c < p.Nu; ++c) D12[z][c] = W[z][Nx + c]; }
    p.C1 = from_dense(C1, Nz, Nx, base); p.D11 = from_dense(D11, Nz, Nx, base); p.D12 = from_dense(D12, Nz, p.Nu, base);
  }
  if (kind == 4) { p.rx.assign(Nx, 0.0); p.ru.assign(p.Nu, 0.25); for (int64_t i = 0; i < Nx; ++i) p.rx[i] = 0.1 + 0.01 * i; }
  // masks from the library's own recipe
  sls_dims dims{Nx, p.Nu, Nz, Nx, p.T, base, 0};
  sls_csc_f64 Af = p.A.f64(), B2f = p.B2.f64();
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
  for (int64_t t = 0; t < p.T; ++t) { p.bx.push_back(p.mx[t].boolean()); p.bu.push_back(p.mu[t].boolean()); }
  return p;
}

struct Result { std::vector<double> col; double total = 0.0; int64_t nsub = 0; };

Result evaluate(const Problem& p, int base, uint32_t flags, int64_t gbeg_frac, int64_t gend_frac, bool expect_ok = true) {
  sls_dims dims{p.Nx, p.Nu, p.Nx + p.Nu, p.Nx, p.T, base, flags};
  sls_csc_f64 A = p.A.f64(), B1 = p.B1.f64(), B2 = p.B2.f64(), C1 = p.C1.f64(), D11 = p.D11.f64(), D12 = p.D12.f64();
  sls_plant plant{&A, &B1, &B2, p.weights ? &C1 : nullptr, p.weights ? &D11 : nullptr, p.weights ? &D12 : nullptr};
  const int64_t ng = p.gptr.empty() ? 0 : (int64_t)p.gptr.size() - 1;
  sls::Inputs in{&dims, &plant, p.bx.data(), p.bu.data(), ng, ng ? p.gptr.data() : nullptr, ng ? p.gcols.data() : nullptr};
  if (!p.rx.empty()) { in.reg_x = p.rx.data(); in.reg_u = p.ru.data(); }
  std::string msg;
  Result R;
  int rc = sls::validate_inputs(in, msg);
  EXPECT(rc == 0, "validate_inputs");
  if (rc) return R;
  const int64_t n_groups = ng ? ng : p.Nx;
  sls::Symbolic S; S.want_packed = false; S.compact = false;
  rc = sls::build_symbolic(in, n_groups * gbeg_frac / 4, n_groups * gend_frac / 4, S, msg);
  EXPECT((rc == 0) == expect_ok, "build_symbolic");
  if (rc) return R;
  std::vector<double> vals((size_t)S.n_values + 1);
  std::mt19937 g(7);                                   // the same Φ for both index bases
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (double& v : vals) v = u(g);
  R.nsub = (int64_t)S.subs.size();
  R.col.assign((size_t)R.nsub, -1.0);
  std::vector<int64_t> nterms((size_t)R.nsub);
  std::vector<double> cabs((size_t)R.nsub);
  rc = sls::objective_host(S, (flags & SLS_SOLVE_SUM_OF_NORMS) ? 1 : 0, vals.data(), R.col.data(), &R.total, nterms.data(), cabs.data(), msg);
  EXPECT(rc == 0, "objective_host");
  double sum = 0.0;
  for (int64_t q = 0; q < R.nsub; ++q) {
    sum += R.col[q];
    EXPECT(std::isfinite(R.col[q]) && cabs[q] >= std::fabs(R.col[q]) * (1.0 - 1e-12) && nterms[q] >= 1, "value / bound terms");
    if (S.subs[q].has_w == 4) EXPECT(R.col[q] == 0.0, "member of a coupled group must report 0.0");
  }
  EXPECT(sum == R.total, "total is the sum in index order");
  // nullable outputs
  EXPECT(sls::objective_host(S, 0, vals.data(), nullptr, nullptr, nullptr, nullptr, msg) == 0, "all outputs null");
  // a compact pass has no explicit tables: refused, not read out of bounds
  sls::Symbolic Sc; Sc.want_packed = false; Sc.compact = true;
  if (sls::build_symbolic(in, 0, n_groups, Sc, msg) == 0 && Sc.compact)
    EXPECT(sls::objective_host(Sc, 0, vals.data(), R.col.data(), nullptr, nullptr, nullptr, msg) == SLS_EINVAL, "compact tables accepted");
  return R;
}

}  // namespace

int main() {
  for (int grid = 0; grid < 2; ++grid)
    for (int kind = 0; kind < 5; ++kind) {
      Result r[2];
      for (int base = 0; base < 2; ++base) {
        const Problem p = make(grid ? 36 : 30, grid != 0, kind, base);
        r[base] = evaluate(p, base, 0, 0, 4);
        evaluate(p, base, 0, 1, 3);                                         // a shard in the middle
        if (kind == 0 || kind == 1) evaluate(p, base, SLS_SOLVE_SUM_OF_NORMS, 0, 4);
      }
      EXPECT(r[0].nsub == r[1].nsub && r[0].col == r[1].col && r[0].total == r[1].total, "index bases disagree");
      std::printf("%s kind=%d: %lld subproblems, total %.12g\n", grid ? "grid36" : "chain30", kind, (long long)r[0].nsub, r[0].total);
    }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_objective: clean\n");
  return 0;
}
