// Host side of the 𝓗₂ shares and the covariance entries (csrc/sls_norms.cpp with the table builder of csrc/sls_symbolic.cpp — no
// HIP in either) under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_cov_host.py::test_host_code_under_sanitizers with g++ -fsanitize=address,undefined.  Drives sls::norms_h2_host and
// sls::norms_cov_host over two operators — a ladder-like one (Nx 24, Nu 6, T 24: row lengths from 0 to all of the row) and one
// with holes (Nx 9, Nu 3, T 3: an empty state row, an empty input row) — in both index bases, every pair (i, j) of rows in both
// orders, with stored-false mask entries and a value array that is NaN wherever the operator must not read; checks what must
// hold exactly (finite outputs, cov(i,j) = cov(j,i) bit for bit, an empty row gives 0.0, the diagonal is row_h2's sum in the
// same order, both index bases give the same bits, totals) against a dense evaluation, and the refusals of out-of-range pairs.
// Exit code 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_norms.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"

namespace {

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Mask {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<uint8_t> nz;
  sls_csc_bool view() const { return sls_csc_bool{nr, nc, cp.data(), ri.data(), nz.data()}; }
};

// row r of the mask keeps each column with probability dens[r]; entry (fr, fc) is stored false when fr >= 0
Mask make_mask(int64_t nr, int64_t nc, const std::vector<double>& dens, std::mt19937& g, int base, int64_t fr, int64_t fc) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<std::vector<uint8_t>> keep(nr, std::vector<uint8_t>(nc, 0));
  for (int64_t r = 0; r < nr; ++r)
    for (int64_t c = 0; c < nc; ++c) keep[r][c] = u(g) < dens[r] ? 1 : 0;
  Mask m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r) {
      const bool f = r == fr && c == fc;
      if (keep[r][c] || f) { m.ri.push_back(r + base); m.nz.push_back(f ? 0 : 1); }
    }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

struct Run { std::vector<double> row, col, tot, cov; };

Run drive(int64_t Nx, int64_t Nu, int64_t T, int base, bool weighted) {
  std::mt19937 g(23 + (unsigned)T);                      // the same masks and values for both index bases
  const int64_t N = Nx + Nu;
  std::vector<double> dx(Nx), du(Nu);
  for (int64_t i = 0; i < Nx; ++i) dx[i] = i == 0 ? 0.0 : (i == Nx - 1 ? 1.0 : 0.15 + 0.7 * i / Nx);
  for (int64_t j = 0; j < Nu; ++j) du[j] = j == 0 ? 0.0 : (j == Nu - 1 ? 1.0 : 0.5);
  std::vector<Mask> mx, mu;
  for (int64_t t = 0; t < T; ++t) {                      // rows 0 stay empty: the stored-false entries sit there
    mx.push_back(make_mask(Nx, Nx, dx, g, base, t % 2 ? 0 : -1, 2));
    mu.push_back(make_mask(Nu, Nx, du, g, base, t == 0 ? 0 : -1, 1));
  }
  std::vector<sls_csc_bool> bx, bu;
  std::vector<double> vals;
  std::vector<std::vector<double>> G((size_t)N, std::vector<double>((size_t)(T * Nx), 0.0));   // dense rows, column index t·Nx + col
  std::uniform_real_distribution<double> uv(-1.0, 1.0);
  auto fill = [&](std::vector<Mask>& ms, int64_t r0) {
    for (int64_t t = 0; t < T; ++t) {
      const Mask& m = ms[(size_t)t];
      for (int64_t c = 0; c < m.nc; ++c)
        for (int64_t k = m.cp[c] - base; k < m.cp[c + 1] - base; ++k) {
          const double v = m.nz[(size_t)k] ? uv(g) : std::numeric_limits<double>::quiet_NaN();
          vals.push_back(v);
          if (m.nz[(size_t)k]) G[(size_t)(r0 + m.ri[(size_t)k] - base)][(size_t)(t * Nx + c)] = v;
        }
    }
  };
  fill(mx, 0); fill(mu, Nx);
  for (auto& m : mx) bx.push_back(m.view());
  for (auto& m : mu) bu.push_back(m.view());
  std::vector<double> cz((size_t)N), bw((size_t)Nx);
  std::uniform_real_distribution<double> uw(0.25, 4.0);
  for (double& v : cz) v = uw(g);
  for (double& v : bw) v = uw(g);
  if (weighted)
    for (int64_t i = 0; i < N; ++i)
      for (int64_t k = 0; k < T * Nx; ++k) G[(size_t)i][(size_t)k] *= cz[(size_t)i] * bw[(size_t)(k % Nx)];
  sls_dims dims{Nx, Nu, 0, 0, T, base, 0};               // Nz and Nw are not read
  Run R;
  sls::NormsOperator Op;
  std::string msg;
  int rc = sls::build_norms_operator(&dims, bx.data(), bu.data(), Op, msg);
  EXPECT(rc == 0, "build_norms_operator");
  if (rc) return R;
  EXPECT(Op.row_ptr[1] == 0 && Op.row_ptr[Nx + 1] == Op.row_ptr[Nx], "rows 0 must be empty");
  const double* pcz = weighted ? cz.data() : nullptr;
  const double* pb = weighted ? bw.data() : nullptr;
  R.row.assign((size_t)N, -7.0); R.col.assign((size_t)Nx, -7.0); R.tot.assign(2, -7.0);
  rc = sls::norms_h2_host(Op, vals.data(), pcz, pb, R.row.data(), R.col.data(), R.tot.data(), msg);
  EXPECT(rc == 0, "norms_h2_host");
  std::vector<int64_t> pi, pj;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = 0; j < N; ++j) { pi.push_back(i + base); pj.push_back(j + base); }
  R.cov.assign(pi.size(), -7.0);
  rc = sls::norms_cov_host(Op, vals.data(), pcz, pb, base, (int64_t)pi.size(), pi.data(), pj.data(), R.cov.data(), msg);
  EXPECT(rc == 0, "norms_cov_host");
  bool finite = true;
  for (const auto* v : {&R.row, &R.col, &R.tot, &R.cov}) for (double x : *v) finite = finite && std::isfinite(x);
  EXPECT(finite, "outputs must be finite: the NaN poison is never read");
  double sum = 0.0, colsum = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    sum += R.row[(size_t)i];
    EXPECT(R.cov[(size_t)(i * N + i)] == R.row[(size_t)i], "the diagonal entry and row_h2 run the same operations");
    for (int64_t j = 0; j < N; ++j) {
      EXPECT(R.cov[(size_t)(i * N + j)] == R.cov[(size_t)(j * N + i)], "cov(i,j) == cov(j,i)");
      long double d = 0.0L, a = 0.0L;
      for (int64_t k = 0; k < T * Nx; ++k) {
        const long double p = (long double)G[(size_t)i][(size_t)k] * (long double)G[(size_t)j][(size_t)k];
        d += p; a += std::fabs(p);
      }
      EXPECT(std::fabs((long double)R.cov[(size_t)(i * N + j)] - d) <= 1e-12L * a, "cov against the dense evaluation");
      if (a == 0.0L) EXPECT(R.cov[(size_t)(i * N + j)] == 0.0, "no shared key: exactly 0");
    }
  }
  for (double x : R.col) colsum += x;
  EXPECT(R.row[0] == 0.0 && R.row[(size_t)Nx] == 0.0 && R.cov[0] == 0.0, "an empty row reports exactly 0");
  EXPECT(R.tot[0] == sum && R.tot[1] == *std::max_element(R.row.begin(), R.row.end()), "totals");
  EXPECT(std::fabs(sum - colsum) <= 1e-12 * sum, "row shares and column shares add up to the same total");
  // nullable outputs, an empty list, refusals (each names the position and leaves the output untouched)
  EXPECT(sls::norms_h2_host(Op, vals.data(), pcz, pb, nullptr, nullptr, R.tot.data(), msg) == 0 && R.tot[0] == sum, "totals alone");
  EXPECT(sls::norms_h2_host(Op, vals.data(), pcz, pb, nullptr, R.col.data(), nullptr, msg) == 0, "col_h2 alone");
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, 0, nullptr, nullptr, nullptr, msg) == 0, "an empty list");
  double one = -7.0;
  const int64_t lo[1] = {base - 1}, hi[1] = {N + base}, ok[1] = {base};
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, 1, lo, ok, &one, msg) == SLS_EINVAL && msg.find("pair 0 ") == 0, "i below the range accepted");
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, 1, ok, hi, &one, msg) == SLS_EINVAL && msg.find("pair 0 ") == 0, "j above the range accepted");
  const int64_t i3[3] = {base, base + 1, N + base + 5}, j3[3] = {base, base, base};
  double three[3] = {-7.0, -7.0, -7.0};
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, 3, i3, j3, three, msg) == SLS_EINVAL && msg.find("pair 2 ") == 0, "a bad third pair accepted");
  EXPECT(one == -7.0 && three[0] == -7.0, "a refused list must write nothing");
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, -1, ok, ok, &one, msg) == SLS_EINVAL, "npairs < 0 accepted");
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, 1, nullptr, ok, &one, msg) == SLS_EINVAL, "a null list accepted");
  EXPECT(sls::norms_cov_host(Op, vals.data(), pcz, pb, base, 1, ok, ok, nullptr, msg) == SLS_EINVAL, "a null output accepted");
  EXPECT(sls::norms_cov_check(N, base, 1, ok, ok, msg) == 0, "norms_cov_check on a good pair");
  return R;
}

}  // namespace

int main() {
  const int64_t shapes[2][3] = {{24, 6, 24}, {9, 3, 3}};
  for (const auto& sh : shapes)
    for (int weighted = 0; weighted < 2; ++weighted) {
      Run r[2];
      for (int base = 0; base < 2; ++base) r[base] = drive(sh[0], sh[1], sh[2], base, weighted != 0);
      EXPECT(r[0].row == r[1].row && r[0].col == r[1].col && r[0].tot == r[1].tot && r[0].cov == r[1].cov, "index bases disagree");
      std::printf("Nx %lld Nu %lld T %lld weighted %d: %zu pairs\n", (long long)sh[0], (long long)sh[1], (long long)sh[2], weighted,
                  r[0].cov.size());
    }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_cov: clean\n");
  return 0;
}
