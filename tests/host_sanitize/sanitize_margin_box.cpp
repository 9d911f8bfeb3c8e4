// Host side of the worst-case margin over a box of plants (csrc/sls_margin_box.cpp with csrc/sls_margin.cpp, csrc/sls_rollout.cpp
// and the table builders of csrc/sls_symbolic.cpp — no HIP in any of them) under AddressSanitizer + UndefinedBehaviorSanitizer: test
// infrastructure, built and run by tests/test_margin_box_host.py::test_host_code_under_sanitizers with g++
// -fsanitize=address,undefined.  Drives sls::build_margin_box_lists, sls::margin_box_host, sls::margin_box_worst_plant and
// sls::margin_entry_signed_check over three shapes — Nx 14, Nu 4, T 4 with a dense row of 10 and one of 11 active coefficients;
// T = 1; and Nu = 0 — in both index bases, with per-scenario centres and radii (some zero, some active in one scenario only) and a
// Φ that is NaN wherever it must not be read; checks what must hold exactly (the lists are consistent, the signed entry equals
// the unsigned one bit for bit, all radii zero gives margin_host's rows, a scenario does not depend on nscen, the worst plant sits
// on the box's vertices and margin_host on it never exceeds the triangle bound, bad radii are refused).  Exit code 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_margin_box.h"
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

struct Out { std::vector<double> wc, tot, rs, Aw, Bw; std::vector<int64_t> ver, rn; std::vector<uint8_t> ex; };

Out drive(int64_t Nx, int64_t Nu, int64_t T, int base, int64_t nscen) {
  std::mt19937 g(41 + (unsigned)T);                        // the same problem for both index bases
  Out R;
  std::vector<Mask> mx, mu;
  for (int64_t t = 0; t < T; ++t) {
    mx.push_back(make_mask(Nx, Nx, t == 0 ? 0.3 : 0.4, g, base, t == T - 1 && T > 1 ? 0 : -1, 2));
    mu.push_back(make_mask(Nu, Nx, 0.5, g, base, t == 0 && Nu > 0 ? 0 : -1, 1));
  }
  std::vector<sls_csc_bool> bx, bu;
  int64_t nval = 0;
  for (auto& m : mx) { bx.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  for (auto& m : mu) { bu.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  std::vector<double> vals((size_t)nval);
  std::uniform_real_distribution<double> uv(-1.0, 1.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int64_t o = 0;
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mx[t].ri.size(); ++k, ++o) vals[o] = (t == 0 || !mx[t].nz[k]) ? nan : uv(g);
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mu[t].ri.size(); ++k, ++o) vals[o] = !mu[t].nz[k] ? nan : uv(g);
  // row 0: 10 coefficients when Nu ≥ 2 (8 of A, 2 of B₂), row 1: 11 (9 + 2), row 5 empty, the others banded
  Mat A = make_mat(Nx, Nx, base, [&](int64_t r, int64_t c) {
    if (r == 0) return c < 8 ? 0.1 + 0.01 * (double)c : 0.0;
    if (r == 1) return c < 9 ? -0.1 - 0.01 * (double)c : 0.0;
    return (r != 5 && std::llabs(r - c) <= 1) ? 0.1 + 0.01 * (double)(r + 2 * c) : 0.0;
  });
  Mat B1 = make_mat(Nx, Nx, base, [&](int64_t r, int64_t c) { return r == c ? 1.0 : 0.0; });
  Mat B2 = make_mat(Nx, Nu, base, [&](int64_t r, int64_t c) {
    if (r <= 1) return c < 2 ? 0.7 + 0.1 * (double)c : 0.0;
    return r == 2 * c + 2 ? 1.0 - 0.1 * (double)c : 0.0;
  });
  sls_csc_f64 a = A.view(), b1 = B1.view(), b2 = B2.view();
  sls_plant P{&a, &b1, &b2, nullptr, nullptr, nullptr};
  sls_dims dims{Nx, Nu, Nx + Nu, Nx, T, base, 0};
  sls::MarginTables Tb;
  std::string msg;
  int rc = sls::build_margin_tables(&dims, &P, bx.data(), bu.data(), Tb, msg);
  EXPECT(rc == 0, "build_margin_tables");
  if (rc) return R;
  const sls::FirOperator& F = Tb.R.F;
  const size_t nA = A.nz.size(), nB = B2.nz.size();
  std::uniform_real_distribution<double> uf(0.8, 1.2);
  std::vector<double> Av(nA * (size_t)nscen), Bv(nB * (size_t)nscen), Ar(Av.size()), Br(Bv.size());
  for (size_t k = 0; k < nA; ++k)
    for (int64_t s = 0; s < nscen; ++s) {
      Av[k * nscen + s] = A.nz[k] * uf(g);
      // row 3 of A: radius 0 everywhere; row 4: active in scenario 1 only
      const int64_t r = A.ri[k] - base;
      Ar[k * nscen + s] = r == 3 ? 0.0 : (r == 4 && s != 1) ? 0.0 : 0.05 * (double)(1 + s % 3) * std::fabs(A.nz[k]);
    }
  for (size_t k = 0; k < nB; ++k)
    for (int64_t s = 0; s < nscen; ++s) { Bv[k * nscen + s] = B2.nz[k] * uf(g); Br[k * nscen + s] = 0.05 * (double)(1 + s % 3) * std::fabs(B2.nz[k]); }
  auto ptr = [](std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };

  // the lists
  sls::MarginBoxLists L;
  EXPECT(sls::build_margin_box_lists(F.A.ptr, Tb.R.A_src, F.B2.ptr, Tb.R.B2_src, nscen, ptr(Ar), ptr(Br), true, L, msg) == 0, "build_margin_box_lists");
  EXPECT((int64_t)L.act_ptr.size() == Nx + 1 && L.act_ptr.front() == 0 && L.act_ptr.back() == (int32_t)L.act_ent.size(), "list sizes");
  int64_t sums = 0, inexact = 0, maxb = 0;
  for (int64_t i = 0; i < Nx; ++i) {
    const int64_t nb = L.act_ptr[(size_t)i + 1] - L.act_ptr[(size_t)i];
    maxb = std::max(maxb, nb);
    if (nb > sls::kMarginBoxMaxBits) ++inexact; else sums += (int64_t)1 << nb;
    EXPECT(L.exact[(size_t)i] == (nb <= sls::kMarginBoxMaxBits), "exact flag");
    for (int32_t q = L.act_ptr[(size_t)i]; q < L.act_ptr[(size_t)i + 1]; ++q) {
      const int32_t c = L.act_ent[(size_t)q];
      EXPECT(q == L.act_ptr[(size_t)i] || L.act_ent[(size_t)q - 1] < c, "codes ascend: A before B2, each in CSR order");
      const bool isA = c < (int32_t)nA;
      const int32_t e = isA ? c : c - (int32_t)nA;
      const auto& pp = isA ? F.A.ptr : F.B2.ptr;
      EXPECT(e >= pp[(size_t)i] && e < pp[(size_t)i + 1], "a coefficient of its own row");
      bool pos = false;
      for (int64_t s = 0; s < nscen; ++s) pos = pos || (isA ? L.A_rad : L.B2_rad)[(size_t)(e * nscen + s)] > 0.0;
      EXPECT(pos, "active means a positive radius somewhere");
    }
  }
  EXPECT(L.max_bits == maxb && L.n_inexact_rows == inexact && L.n_vertex_sums == sums, "the counts of the lists");
  if (Nu >= 2 && Nx >= 9) EXPECT(L.act_ptr[1] == 10 && L.act_ptr[2] - L.act_ptr[1] == 11 && inexact == 1, "rows of 10 and 11 coefficients");
  EXPECT(L.act_ptr[4] == L.act_ptr[3], "a row whose radii are all 0 has an empty list");
  // refusals leave `out` alone
  {
    sls::MarginBoxLists K = L;
    std::vector<double> bad = Ar;
    const double poison[4] = {-1e-300, std::numeric_limits<double>::infinity(), nan, -1.0};
    for (double p : poison) {
      bad[bad.size() / 2] = p;
      EXPECT(sls::build_margin_box_lists(F.A.ptr, Tb.R.A_src, F.B2.ptr, Tb.R.B2_src, nscen, bad.data(), ptr(Br), true, K, msg) == SLS_EINVAL, "a bad radius accepted");
      EXPECT(K.act_ent == L.act_ent && K.A_rad == L.A_rad, "a refusal changed the lists");
    }
    EXPECT(sls::build_margin_box_lists(F.A.ptr, Tb.R.A_src, F.B2.ptr, Tb.R.B2_src, 0, nullptr, nullptr, false, K, msg) == SLS_EINVAL, "nscen = 0 accepted");
  }
  // the signed entry
  {
    int64_t n = 0, bad = -1, neg = 0;
    EXPECT(sls::margin_entry_signed_check(Tb, vals.data(), nscen, Av.data(), ptr(Bv), true, &n, &bad, &neg, msg) == 0, "margin_entry_signed_check");
    EXPECT(n == (int64_t)Tb.def_key.size() * nscen && bad == 0 && neg > 0 && neg < n, "fabs(margin_entry_signed) == margin_entry bit for bit");
  }
  auto run = [&](int64_t ns, const double* Ap, const double* Bp, const double* Arp, const double* Brp, bool per, Out& o2) {
    o2.wc.assign((size_t)(Nx * ns), -7.0); o2.rs = o2.wc; o2.tot.assign((size_t)ns, -7.0);
    o2.ver.assign((size_t)(Nx * ns), -7); o2.rn.assign((size_t)Nx, -1); o2.ex.assign((size_t)Nx, 7);
    o2.Aw.assign(nA * (size_t)ns, nan); o2.Bw.assign(nB * (size_t)ns, nan);
    return sls::margin_box_host(Tb, vals.data(), ns, Ap, Bp, per, Arp, Brp, per, o2.wc.data(), o2.ver.data(), o2.ex.data(), o2.tot.data(),
                                o2.rn.data(), o2.rs.data(), ptr(o2.Aw), ptr(o2.Bw), msg);
  };
  EXPECT(run(nscen, Av.data(), ptr(Bv), ptr(Ar), ptr(Br), true, R) == 0, "margin_box_host");
  // margin_host at the centre and on the worst plant
  std::vector<double> row0((size_t)(Nx * nscen)), roww(row0.size());
  EXPECT(sls::margin_host(Tb, vals.data(), nscen, Av.data(), ptr(Bv), true, row0.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, msg) == 0, "margin_host (centre)");
  EXPECT(sls::margin_host(Tb, vals.data(), nscen, R.Aw.data(), ptr(R.Bw), true, roww.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, msg) == 0, "margin_host (worst plant)");
  bool ok = true, onbox = true;
  for (int64_t i = 0; i < Nx; ++i)
    for (int64_t s = 0; s < nscen; ++s) {
      const double wc = R.wc[(size_t)(i * nscen + s)], slack = 1e-12 * (1.0 + wc);
      ok = ok && std::isfinite(wc) && wc >= row0[(size_t)(i * nscen + s)] - slack;
      if (R.ex[(size_t)i]) ok = ok && std::fabs(roww[(size_t)(i * nscen + s)] - wc) <= slack && R.ver[(size_t)(i * nscen + s)] >= 0;
      else ok = ok && roww[(size_t)(i * nscen + s)] <= wc + slack && R.ver[(size_t)(i * nscen + s)] == -1;
    }
  EXPECT(ok, "centre <= worst case; the worst plant attains it on exact rows and stays below the bound elsewhere");
  for (size_t k = 0; k < nA; ++k)
    for (int64_t s = 0; s < nscen; ++s) {
      const double d = std::fabs(R.Aw[k * nscen + s] - Av[k * nscen + s]), r = Ar[k * nscen + s];
      onbox = onbox && std::fabs(d - r) <= 1e-15 * (std::fabs(Av[k * nscen + s]) + r);
    }
  EXPECT(onbox, "every coefficient of the worst plant sits at centre ± radius");
  for (int64_t s = 0; s < nscen; ++s) {
    double m0 = 0.0;
    for (int64_t i = 0; i < Nx; ++i) m0 = std::max(m0, R.wc[(size_t)(i * nscen + s)]);
    EXPECT(R.tot[(size_t)s] == m0, "totals are the maxima");
  }
  // all radii zero: margin_host's rows, bit for bit
  Out zero;
  EXPECT(run(nscen, Av.data(), ptr(Bv), nullptr, nullptr, true, zero) == 0, "zero radii");
  EXPECT(zero.wc == row0, "all radii zero gives margin_host's row_l1");
  EXPECT(zero.Aw == Av && zero.Bw == Bv, "the worst plant of a point is the point");
  // scenario 1 alone: the same values
  std::vector<double> A1(nA), B1v(nB), Ar1(nA), Br1(nB);
  for (size_t k = 0; k < nA; ++k) { A1[k] = Av[k * nscen + 1]; Ar1[k] = Ar[k * nscen + 1]; }
  for (size_t k = 0; k < nB; ++k) { B1v[k] = Bv[k * nscen + 1]; Br1[k] = Br[k * nscen + 1]; }
  Out one;
  EXPECT(run(1, A1.data(), ptr(B1v), ptr(Ar1), ptr(Br1), false, one) == 0, "nscen = 1");
  bool same = one.tot[0] == R.tot[1];
  for (int64_t i = 0; i < Nx; ++i) same = same && one.wc[(size_t)i] == R.wc[(size_t)(i * nscen + 1)];
  EXPECT(same, "a scenario does not depend on nscen or on how its values arrive");
  return R;
}

}  // namespace

int main() {
  const int64_t shapes[3][3] = {{14, 4, 4}, {12, 3, 1}, {12, 0, 3}};
  for (const auto& sh : shapes) {
    Out r[2];
    for (int base = 0; base < 2; ++base) r[base] = drive(sh[0], sh[1], sh[2], base, 3);
    EXPECT(r[0].wc == r[1].wc && r[0].ver == r[1].ver && r[0].tot == r[1].tot && r[0].rn == r[1].rn && r[0].rs == r[1].rs && r[0].Aw == r[1].Aw,
           "index bases disagree");
    std::printf("Nx %lld Nu %lld T %lld: l1_wc[0] %.6g\n", (long long)sh[0], (long long)sh[1], (long long)sh[2], r[0].tot.empty() ? 0.0 : r[0].tot[0]);
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_margin_box: clean\n");
  return 0;
}
