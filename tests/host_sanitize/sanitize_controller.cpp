// Host side of the stand-alone controller (csrc/sls_controller.cpp with the table builder of csrc/sls_symbolic.cpp — no HIP in
// either) under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_controller_host.py::test_host_code_under_sanitizers with g++ -fsanitize=address,undefined.  Drives
// sls::build_controller_operator and sls::controller_host over three operators — a ladder-like one (Nx 24, Nu 6, T 24: a ring of
// 32 slots, row lengths from 0 to all of the row), T = 4 (the ring exactly full) and T = 5 (a ring of 8) on Nx 9, Nu 3 — in both
// index bases, each with one stored-false mask entry and a value array that is NaN wherever the operator must not read, for more
// than three turns of the ring; checks what must hold exactly (rows ascend in (τ, c), perm hits no poisoned value, outputs
// finite, an empty row gives 0.0, both index bases give the same bits, ŵ_0 = x_0).  Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_controller.h"
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

struct Run { std::vector<double> u, w; std::vector<int32_t> hoff, perm, bp, up; };

Run drive(int64_t Nx, int64_t Nu, int64_t T, int base, int64_t nscen, int64_t steps) {
  std::mt19937 g(7 + (unsigned)T);                       // the same masks and values for both index bases
  std::vector<double> dx(Nx), du(Nu);
  for (int64_t i = 0; i < Nx; ++i) dx[i] = i == 0 ? 0.0 : (i == Nx - 1 ? 1.0 : 0.15 + 0.7 * i / Nx);
  for (int64_t j = 0; j < Nu; ++j) du[j] = j == 0 ? 0.0 : (j == Nu - 1 ? 1.0 : 0.5);
  std::vector<Mask> mx, mu;
  for (int64_t t = 0; t < T; ++t) {
    mx.push_back(make_mask(Nx, Nx, t == 0 ? std::vector<double>(Nx, 0.3) : dx, g, base, t == T - 1 && T > 1 ? 0 : -1, 2));
    mu.push_back(make_mask(Nu, Nx, du, g, base, t == 0 ? 0 : -1, 1));
  }
  std::vector<sls_csc_bool> bx, bu;
  int64_t nval = 0;
  for (auto& m : mx) { bx.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  for (auto& m : mu) { bu.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  // Φ in mask order: NaN on all of Sx[0] and on stored-false entries
  std::vector<double> vals((size_t)nval);
  std::uniform_real_distribution<double> uv(-1.0, 1.0);
  const double scale = 0.5 / std::sqrt((double)(T * Nx));
  int64_t o = 0;
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mx[t].ri.size(); ++k, ++o) vals[o] = (t == 0 || !mx[t].nz[k]) ? std::numeric_limits<double>::quiet_NaN() : uv(g) * scale;
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mu[t].ri.size(); ++k, ++o) vals[o] = !mu[t].nz[k] ? std::numeric_limits<double>::quiet_NaN() : uv(g) * scale;
  sls_dims dims{Nx, Nu, 0, 0, T, base, 0};               // Nz and Nw are not read
  sls::FirOperator F;
  std::string msg;
  Run R;
  int rc = sls::build_controller_operator(&dims, bx.data(), bu.data(), F, msg);
  EXPECT(rc == 0, "build_controller_operator");
  if (rc) return R;
  EXPECT((int64_t)F.beta_ptr.size() == Nx + 1 && (int64_t)F.u_ptr.size() == Nu + 1 && F.beta_ptr[0] == 0 && F.u_ptr[0] == F.beta_ptr[Nx] &&
         (size_t)F.u_ptr[Nu] == F.hoff.size() && F.hoff.size() == F.perm.size() && F.n_values == nval, "table shapes");
  EXPECT(F.beta_ptr[1] == 0 && F.u_ptr[1] == F.u_ptr[0], "rows 0 must be empty (the stored-false entries sit there)");
  for (int64_t r = 0; r < Nx + Nu; ++r) {
    const int32_t e0 = r < Nx ? F.beta_ptr[r] : F.u_ptr[r - Nx], e1 = r < Nx ? F.beta_ptr[r + 1] : F.u_ptr[r - Nx + 1];
    const int64_t max_lag = r < Nx ? T - 1 : T;
    for (int32_t e = e0; e < e1; ++e) {
      const int64_t lag = sls::controller_lag(F.hoff[e], Nx), col = sls::controller_col(F.hoff[e], Nx);
      EXPECT(lag >= 1 && lag <= max_lag && col >= 0 && col < Nx && lag * Nx - col == F.hoff[e], "lag / column of an entry");
      const int64_t plag = e == e0 ? 0 : sls::controller_lag(F.hoff[e - 1], Nx), pcol = e == e0 ? -1 : sls::controller_col(F.hoff[e - 1], Nx);
      EXPECT(plag < lag || (plag == lag && pcol < col), "a row ascends in (lag, column)");
      EXPECT(F.perm[e] >= 0 && F.perm[e] < nval && std::isfinite(vals[(size_t)F.perm[e]]), "perm points at a poisoned value");
    }
  }
  std::vector<double> x((size_t)(steps * Nx * nscen));
  std::normal_distribution<double> nx(0.0, 1.0);
  for (double& v : x) v = nx(g);
  R.u.assign((size_t)(steps * Nu * nscen), -7.0); R.w.assign((size_t)(steps * Nx * nscen), -7.0);
  rc = sls::controller_host(F, vals.data(), nscen, steps, x.data(), R.u.data(), R.w.data(), msg);
  EXPECT(rc == 0, "controller_host");
  bool finite = true, w0 = true, empty0 = true;
  for (double v : R.u) finite = finite && std::isfinite(v);
  for (double v : R.w) finite = finite && std::isfinite(v);
  for (int64_t i = 0; i < Nx * nscen; ++i) w0 = w0 && R.w[(size_t)i] == x[(size_t)i];
  for (int64_t k = 0; k < steps; ++k)
    for (int64_t s = 0; s < nscen; ++s) empty0 = empty0 && R.u[(size_t)((k * Nu) * nscen + s)] == 0.0;
  EXPECT(finite, "outputs must be finite: the NaN poison is never read");
  EXPECT(w0, "ŵ_0 = x_0");
  EXPECT(empty0, "an empty u row reports exactly 0");
  // nullable outputs, zero steps
  EXPECT(sls::controller_host(F, vals.data(), nscen, steps, x.data(), nullptr, nullptr, msg) == 0, "null outputs");
  EXPECT(sls::controller_host(F, vals.data(), nscen, 0, nullptr, nullptr, nullptr, msg) == 0, "zero steps");
  EXPECT(sls::controller_host(F, vals.data(), 0, steps, x.data(), nullptr, nullptr, msg) == SLS_EINVAL, "nscen = 0 accepted");
  R.hoff = F.hoff; R.perm = F.perm; R.bp = F.beta_ptr; R.up = F.u_ptr;
  return R;
}

}  // namespace

int main() {
  const int64_t shapes[3][3] = {{24, 6, 24}, {9, 3, 4}, {9, 3, 5}};
  for (const auto& sh : shapes) {
    const int64_t R = sls::controller_ring_slots(sh[2]);
    EXPECT(R >= sh[2] && R < 2 * sh[2] && (R & (R - 1)) == 0, "ring slots");
    const int64_t steps = 3 * R + 5;
    Run r[2];
    for (int base = 0; base < 2; ++base) r[base] = drive(sh[0], sh[1], sh[2], base, 3, steps);
    EXPECT(r[0].u == r[1].u && r[0].w == r[1].w && r[0].hoff == r[1].hoff && r[0].perm == r[1].perm && r[0].bp == r[1].bp && r[0].up == r[1].up,
           "index bases disagree");
    std::printf("Nx %lld Nu %lld T %lld: ring %lld, %zu entries, %lld steps\n", (long long)sh[0], (long long)sh[1], (long long)sh[2], (long long)R,
                r[0].hoff.size(), (long long)steps);
  }
  // refusals of the table builder
  {
    sls::FirOperator F; std::string msg;
    sls_dims bad{9, 3, 0, 0, 0, 0, 0};
    EXPECT(sls::build_controller_operator(&bad, nullptr, nullptr, F, msg) == SLS_EINVAL, "null masks accepted");
    sls_csc_bool none{};
    EXPECT(sls::build_controller_operator(&bad, &none, &none, F, msg) == SLS_EINVAL, "T = 0 accepted");
    sls_dims big{int64_t(1) << 30, 1, 0, 0, 3, 0, 0};
    EXPECT(sls::build_controller_operator(&big, &none, &none, F, msg) == SLS_EUNSUPPORTED, "(T+1)·Nx beyond int32 accepted");
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_controller: clean\n");
  return 0;
}
