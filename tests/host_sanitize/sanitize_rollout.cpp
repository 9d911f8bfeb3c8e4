// Host side of the ensemble rollout (csrc/sls_rollout.cpp with the table builders of csrc/sls_symbolic.cpp — no HIP in either)
// under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_rollout_host.py::test_host_code_under_sanitizers with g++ -fsanitize=address,undefined.  Drives
// sls::build_rollout_tables and sls::RolloutHost over four shapes — a ladder-like one (Nx 24, Nu 6, T 24: a ring of 32 slots), T = 4
// (the ring exactly full), T = 5 (a ring of 8) on Nx 9, Nu 3, and Nu = 0 — in both index bases, with a banded A, a B₂ that has a
// shared actuator and an orphan, per-scenario plant values, a non-zero x_0, a Φ that is NaN wherever the operator must not read, for
// more than three turns of the ring; checks what must hold exactly (sources are a permutation that reproduces the CSR values,
// every actuator has one owner, outputs finite, chunked = single, both index bases give the same bits, a reset repeats the run).
// Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_rollout.h"
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

Mask make_mask(int64_t nr, int64_t nc, double dens, std::mt19937& g, int base, int64_t fr, int64_t fc) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  Mask m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r) {
      const bool f = r == fr && c == fc, keep = u(g) < dens;
      if (keep || f) { m.ri.push_back(r + base); m.nz.push_back(f ? 0 : 1); }
    }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

struct Mat {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> nz;
  sls_csc_f64 view() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), nz.data()}; }
};

template <class F>
Mat make_mat(int64_t nr, int64_t nc, int base, F&& value) {          // value(r, c): 0.0 = not stored
  Mat m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r) {
      const double v = value(r, c);
      if (v != 0.0) { m.ri.push_back(r + base); m.nz.push_back(v); }
    }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

struct Out { std::vector<double> x, u, xe, cost, px, pu; };

Out drive(int64_t Nx, int64_t Nu, int64_t T, int base, int64_t nscen, int64_t steps) {
  std::mt19937 g(11 + (unsigned)T);                        // the same problem for both index bases
  Out R;
  std::vector<Mask> mx, mu;
  for (int64_t t = 0; t < T; ++t) {
    mx.push_back(make_mask(Nx, Nx, t == 0 ? 0.3 : 0.45, g, base, t == T - 1 && T > 1 ? 0 : -1, 2));
    mu.push_back(make_mask(Nu, Nx, 0.5, g, base, t == 0 && Nu > 0 ? 0 : -1, 1));
  }
  std::vector<sls_csc_bool> bx, bu;
  int64_t nval = 0;
  for (auto& m : mx) { bx.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  for (auto& m : mu) { bu.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  std::vector<double> vals((size_t)nval);
  std::uniform_real_distribution<double> uv(-1.0, 1.0);
  const double scale = 0.5 / std::sqrt((double)(T * Nx));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int64_t o = 0;
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mx[t].ri.size(); ++k, ++o) vals[o] = (t == 0 || !mx[t].nz[k]) ? nan : uv(g) * scale;
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mu[t].ri.size(); ++k, ++o) vals[o] = !mu[t].nz[k] ? nan : uv(g) * scale;
  // A: a band of half-width 2 with one empty row; B₂: actuator j drives state 3j+1, actuator 1 also state 0 (shared), the last
  // actuator drives nothing (orphan); B₁ = I
  Mat A = make_mat(Nx, Nx, base, [&](int64_t r, int64_t c) { return (r != 5 && std::llabs(r - c) <= 2) ? 0.1 + 0.01 * (double)(r + 2 * c) : 0.0; });
  Mat B1 = make_mat(Nx, Nx, base, [&](int64_t r, int64_t c) { return r == c ? 1.0 : 0.0; });
  Mat B2 = make_mat(Nx, Nu, base, [&](int64_t r, int64_t c) {
    if (c == Nu - 1 && Nu > 1) return 0.0;
    if (r == 3 * c + 1) return 1.0 - 0.1 * (double)c;
    return (c == 1 && r == 0) ? -0.5 : 0.0;
  });
  sls_csc_f64 a = A.view(), b1 = B1.view(), b2 = B2.view();
  sls_plant P{&a, &b1, &b2, nullptr, nullptr, nullptr};
  sls_dims dims{Nx, Nu, Nx + Nu, Nx, T, base, 0};
  sls::RolloutTables Tb;
  std::string msg;
  int rc = sls::build_rollout_tables(&dims, &P, bx.data(), bu.data(), Tb, msg);
  EXPECT(rc == 0, "build_rollout_tables");
  if (rc) return R;
  const sls::FirOperator& F = Tb.F;
  EXPECT(Tb.A_src.size() == A.nz.size() && Tb.B2_src.size() == B2.nz.size() && Tb.b2_owner.size() == B2.nz.size(), "table sizes");
  std::vector<int> hit(A.nz.size(), 0);
  for (size_t e = 0; e < Tb.A_src.size(); ++e) {
    EXPECT(Tb.A_src[e] >= 0 && (size_t)Tb.A_src[e] < A.nz.size() && A.nz[(size_t)Tb.A_src[e]] == F.A.val[e], "A_src reproduces the CSR values");
    if (Tb.A_src[e] >= 0 && (size_t)Tb.A_src[e] < hit.size()) hit[(size_t)Tb.A_src[e]]++;
  }
  for (int h : hit) EXPECT(h == 1, "A_src is a permutation");
  std::vector<int> owners((size_t)Nu, 0);
  for (size_t e = 0; e < Tb.B2_src.size(); ++e) {
    EXPECT(B2.nz[(size_t)Tb.B2_src[e]] == F.B2.val[e], "B2_src reproduces the CSR values");
    if (Tb.b2_owner[e]) owners[(size_t)F.B2.idx[e]]++;
  }
  for (int32_t j : F.orphan) owners[(size_t)j]++;
  for (int64_t j = 0; j < Nu; ++j) EXPECT(owners[(size_t)j] == 1, "one owner per actuator");
  EXPECT(Nu < 2 || F.orphan.size() == 1, "the orphan");

  // per-scenario values in CSC order, x_0, w, weights
  std::uniform_real_distribution<double> uf(0.8, 1.2);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::vector<double> Av(A.nz.size() * (size_t)nscen), Bv(B2.nz.size() * (size_t)nscen), x0((size_t)(Nx * nscen)), w((size_t)(steps * Nx * nscen));
  for (size_t k = 0; k < A.nz.size(); ++k) for (int64_t s = 0; s < nscen; ++s) Av[k * nscen + s] = A.nz[k] * uf(g);
  for (size_t k = 0; k < B2.nz.size(); ++k) for (int64_t s = 0; s < nscen; ++s) Bv[k * nscen + s] = B2.nz[k] * uf(g);
  for (double& v : x0) v = nd(g);
  for (double& v : w) v = 0.5 * nd(g);
  std::vector<double> q((size_t)Nx), r((size_t)Nu);
  for (double& v : q) v = 0.5 + 1.5 * std::fabs(uv(g));
  for (double& v : r) v = 0.5 + 1.5 * std::fabs(uv(g));

  sls::RolloutHost H;
  EXPECT(H.init(Tb, 0, msg) == SLS_EINVAL, "nscen = 0 accepted");
  EXPECT(H.init(Tb, nscen, msg) == 0, "init");
  EXPECT(H.run(nullptr, 1, nullptr, nullptr, msg) == SLS_EINVAL, "run before load accepted");
  EXPECT(H.run(nullptr, 0, nullptr, nullptr, msg) == 0, "zero steps before load");
  H.load(vals.data());
  H.set_plant(Av.data(), nullptr, true);
  H.set_plant(nullptr, Bv.data(), true);
  H.set_weights(q.data(), Nu ? r.data() : nullptr);
  H.reset(x0.data());
  R.x.assign((size_t)(steps * Nx * nscen), -7.0); R.u.assign((size_t)(steps * Nu * nscen), -7.0);
  EXPECT(H.run(w.data(), steps, R.x.data(), R.u.data(), msg) == 0, "run");
  EXPECT(H.steps_done() == steps, "step count");
  R.xe.assign(H.state(), H.state() + Nx * nscen);
  R.cost.resize((size_t)nscen); R.px = R.cost; R.pu = R.cost;
  H.stats(R.cost.data(), R.px.data(), R.pu.data());
  bool finite = true, first = true;
  for (double v : R.x) finite = finite && std::isfinite(v);
  for (double v : R.u) finite = finite && std::isfinite(v);
  for (double v : R.cost) finite = finite && std::isfinite(v) && v > 0.0;
  for (int64_t i = 0; i < Nx * nscen; ++i) first = first && R.x[(size_t)i] == x0[(size_t)i];
  EXPECT(finite, "outputs must be finite: the NaN poison is never read");
  EXPECT(first, "row 0 of x is x_0");
  // reset and the same run in chunks, without recording: the same state and stats
  H.reset(x0.data());
  const int64_t Rs = sls::controller_ring_slots(T);
  const int64_t chunk[6] = {1, 2, Rs - 1, Rs, Rs + 1, steps - (3 * Rs + 3)};
  int64_t done = 0;
  for (int64_t c : chunk) { EXPECT(c >= 0 && H.run(w.data() + done * Nx * nscen, c, nullptr, nullptr, msg) == 0, "chunk"); done += c; }
  EXPECT(done == steps && H.steps_done() == steps, "chunks add up");
  std::vector<double> c2((size_t)nscen), px2((size_t)nscen), pu2((size_t)nscen);
  H.stats(c2.data(), px2.data(), pu2.data());
  EXPECT(c2 == R.cost && px2 == R.px && pu2 == R.pu && std::vector<double>(H.state(), H.state() + Nx * nscen) == R.xe, "chunked run differs");
  H.stats(nullptr, nullptr, nullptr);
  // shared values: one array for all scenarios, null w
  H.set_plant(A.nz.data(), B2.nz.empty() ? nullptr : B2.nz.data(), false);
  H.reset(nullptr);
  EXPECT(H.run(nullptr, 3, nullptr, nullptr, msg) == 0, "null w");
  for (int64_t i = 0; i < Nx * nscen; ++i) EXPECT(H.state()[i] == 0.0, "x_0 = 0 and w = 0 stay at 0");
  return R;
}

}  // namespace

int main() {
  const int64_t shapes[4][3] = {{24, 6, 24}, {9, 3, 4}, {9, 3, 5}, {9, 0, 3}};
  for (const auto& sh : shapes) {
    const int64_t R = sls::controller_ring_slots(sh[2]);
    const int64_t steps = 3 * R + 5;
    Out r[2];
    for (int base = 0; base < 2; ++base) r[base] = drive(sh[0], sh[1], sh[2], base, 3, steps);
    EXPECT(r[0].x == r[1].x && r[0].u == r[1].u && r[0].xe == r[1].xe && r[0].cost == r[1].cost && r[0].px == r[1].px && r[0].pu == r[1].pu,
           "index bases disagree");
    std::printf("Nx %lld Nu %lld T %lld: ring %lld, %lld steps, cost[0] %.6g\n", (long long)sh[0], (long long)sh[1], (long long)sh[2],
                (long long)R, (long long)steps, r[0].cost.empty() ? 0.0 : r[0].cost[0]);
  }
  {
    sls::RolloutTables Tb; std::string msg;
    EXPECT(sls::build_rollout_tables(nullptr, nullptr, nullptr, nullptr, Tb, msg) == SLS_EINVAL, "null arguments accepted");
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_rollout: clean\n");
  return 0;
}
