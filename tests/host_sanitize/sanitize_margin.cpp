// Host side of the robust-stability margins (csrc/sls_margin.cpp with csrc/sls_rollout.cpp and the table builders of
// csrc/sls_symbolic.cpp — no HIP in any of them) under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built
// and run by tests/test_margin_host.py::test_host_code_under_sanitizers with g++ -fsanitize=address,undefined.  Drives
// sls::build_margin_tables and sls::margin_host over four shapes — Nx 24, Nu 6, T 24; T = 1 (one slice: D[0] = −A − B₂·Φu[0]);
// T = 5 on Nx 9, Nu 3; and Nu = 0 — in both index bases, with a banded A that has an empty row, a B₂ with a shared actuator and an
// orphan, per-scenario plant values and a Φ that is NaN wherever it must not be read; checks what must hold exactly (the tables
// are consistent, outputs finite, both index bases and shared / replicated values give the same bits, a scenario does not depend on
// nscen, the totals are the maxima, the term counts of rows and columns add up to the same number).  Exit code 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_margin.h"
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

struct Out { std::vector<double> row, col, tot, rs, cs, ts; std::vector<int64_t> rn, cn, tn; };

Out drive(int64_t Nx, int64_t Nu, int64_t T, int base, int64_t nscen) {
  std::mt19937 g(23 + (unsigned)T);                        // the same problem for both index bases
  Out R;
  std::vector<Mask> mx, mu;
  for (int64_t t = 0; t < T; ++t) {
    mx.push_back(make_mask(Nx, Nx, t == 0 ? 0.3 : 0.35, g, base, t == T - 1 && T > 1 ? 0 : -1, 2));
    mu.push_back(make_mask(Nu, Nx, 0.5, g, base, t == 0 && Nu > 0 ? 0 : -1, 1));
  }
  std::vector<sls_csc_bool> bx, bu;
  int64_t nval = 0;
  for (auto& m : mx) { bx.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  for (auto& m : mu) { bu.push_back(m.view()); nval += (int64_t)m.ri.size(); }
  std::vector<double> vals((size_t)nval);
  std::uniform_real_distribution<double> uv(-1.0, 1.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int64_t o = 0, n_read = 0;
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mx[t].ri.size(); ++k, ++o) { vals[o] = (t == 0 || !mx[t].nz[k]) ? nan : uv(g); n_read += !std::isnan(vals[o]); }
  for (int64_t t = 0; t < T; ++t)
    for (size_t k = 0; k < mu[t].ri.size(); ++k, ++o) { vals[o] = !mu[t].nz[k] ? nan : uv(g); n_read += !std::isnan(vals[o]); }
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
  sls::MarginTables Tb;
  std::string msg;
  int rc = sls::build_margin_tables(&dims, &P, bx.data(), bu.data(), Tb, msg);
  EXPECT(rc == 0, "build_margin_tables");
  if (rc) return R;
  // the tables: sizes, ascending segments, keys ascending inside a column, start positions, the by-row grouping a permutation
  const int64_t ne = (int64_t)Tb.phi_perm.size(), nd = (int64_t)Tb.def_key.size();
  EXPECT(ne == n_read, "every read value once");
  EXPECT((int64_t)Tb.phi_seg.size() == Nx * T + 1 && Tb.phi_seg.front() == 0 && Tb.phi_seg.back() == ne && (int64_t)Tb.phi_row.size() == ne, "Φ list sizes");
  for (int64_t q = 0; q < Nx * T; ++q) {
    EXPECT(Tb.phi_seg[(size_t)q] <= Tb.phi_seg[(size_t)q + 1], "segments ascend");
    for (int32_t e = Tb.phi_seg[(size_t)q]; e < Tb.phi_seg[(size_t)q + 1]; ++e) {
      EXPECT(Tb.phi_row[(size_t)e] >= (q % T == 0 ? Nx : 0) && Tb.phi_row[(size_t)e] < Nx + Nu, "row range (no state row in slice 0)");
      EXPECT(e == Tb.phi_seg[(size_t)q] || Tb.phi_row[(size_t)e - 1] < Tb.phi_row[(size_t)e], "rows ascend inside a segment");
      EXPECT(Tb.phi_perm[(size_t)e] >= 0 && Tb.phi_perm[(size_t)e] < nval && !std::isnan(vals[(size_t)Tb.phi_perm[(size_t)e]]), "perm points at a read value");
      EXPECT(sls::margin_find(Tb.phi_row.data(), Tb.phi_seg[(size_t)q], Tb.phi_seg[(size_t)q + 1], Tb.phi_row[(size_t)e]) == e, "margin_find finds every entry");
    }
    EXPECT(sls::margin_find(Tb.phi_row.data(), Tb.phi_seg[(size_t)q], Tb.phi_seg[(size_t)q + 1], (int32_t)(Nx + Nu)) == -1, "margin_find misses above");
    EXPECT(sls::margin_find(Tb.phi_row.data(), Tb.phi_seg[(size_t)q], Tb.phi_seg[(size_t)q + 1], -1) == -1, "margin_find misses below");
  }
  EXPECT((int64_t)Tb.def_ptr.size() == Nx + 1 && Tb.def_ptr.back() == nd && (int64_t)Tb.def_start.size() == nd, "defect list sizes");
  for (int64_t j = 0; j < Nx; ++j)
    for (int32_t d = Tb.def_ptr[(size_t)j]; d < Tb.def_ptr[(size_t)j + 1]; ++d) {
      EXPECT(Tb.def_key[(size_t)d] >= 0 && Tb.def_key[(size_t)d] < T * Nx, "key range");
      EXPECT(d == Tb.def_ptr[(size_t)j] || Tb.def_key[(size_t)d - 1] < Tb.def_key[(size_t)d], "keys ascend inside a column");
      const int64_t tau = Tb.def_key[(size_t)d] / Nx, i = Tb.def_key[(size_t)d] % Nx;
      const int32_t st = Tb.def_start[(size_t)d];
      if (tau + 1 < T) EXPECT(st == sls::margin_find(Tb.phi_row.data(), Tb.phi_seg[(size_t)(j * T + tau + 1)], Tb.phi_seg[(size_t)(j * T + tau + 2)], (int32_t)i), "start position");
      else EXPECT(st == -1, "no start value in the last slice");
    }
  std::vector<int> hit((size_t)nd, 0);
  EXPECT((int64_t)Tb.row_ptr.size() == Nx + 1 && Tb.row_ptr.back() == nd && (int64_t)Tb.row_perm.size() == nd, "row list sizes");
  for (int64_t i = 0; i < Nx; ++i)
    for (int32_t q = Tb.row_ptr[(size_t)i]; q < Tb.row_ptr[(size_t)i + 1]; ++q) {
      const int32_t d = Tb.row_perm[(size_t)q];
      EXPECT(d >= 0 && d < nd && Tb.def_key[(size_t)d] % Nx == i, "row_perm groups by row");
      EXPECT(q == Tb.row_ptr[(size_t)i] || Tb.row_perm[(size_t)q - 1] < d, "row lists ascend");
      if (d >= 0 && d < nd) hit[(size_t)d]++;
    }
  for (int h : hit) EXPECT(h == 1, "row_perm is a permutation");

  std::uniform_real_distribution<double> uf(0.8, 1.2);
  std::vector<double> Av(A.nz.size() * (size_t)nscen), Bv(B2.nz.size() * (size_t)nscen);
  for (size_t k = 0; k < A.nz.size(); ++k) for (int64_t s = 0; s < nscen; ++s) Av[k * nscen + s] = A.nz[k] * uf(g);
  for (size_t k = 0; k < B2.nz.size(); ++k) for (int64_t s = 0; s < nscen; ++s) Bv[k * nscen + s] = B2.nz[k] * uf(g);
  auto run = [&](int64_t ns, const double* Ap, const double* Bp, bool per, Out& o2) {
    o2.row.assign((size_t)(Nx * ns), -7.0); o2.col = o2.row; o2.rs = o2.row; o2.cs = o2.row;
    o2.tot.assign((size_t)(2 * ns), -7.0); o2.ts = o2.tot;
    o2.rn.assign((size_t)Nx, -1); o2.cn = o2.rn; o2.tn.assign(2, -1);
    return sls::margin_host(Tb, vals.data(), ns, Ap, Bp, per, o2.row.data(), o2.col.data(), o2.tot.data(), o2.rn.data(), o2.cn.data(),
                            o2.tn.data(), o2.rs.data(), o2.cs.data(), o2.ts.data(), msg);
  };
  EXPECT(run(0, nullptr, nullptr, false, R) == SLS_EINVAL, "nscen = 0 accepted");
  EXPECT(run(nscen, Av.data(), Bv.empty() ? nullptr : Bv.data(), true, R) == 0, "margin_host");
  bool finite = true;
  for (double v : R.row) finite = finite && std::isfinite(v) && v >= 0.0;
  for (double v : R.col) finite = finite && std::isfinite(v) && v >= 0.0;
  EXPECT(finite, "outputs must be finite: the NaN poison is never read");
  int64_t sr = 0, sc = 0;
  for (int64_t i = 0; i < Nx; ++i) { sr += R.rn[(size_t)i]; sc += R.cn[(size_t)i]; }
  EXPECT(sr == sc && sr >= nd, "rows and columns count the same terms");
  for (int64_t s = 0; s < nscen; ++s) {
    double m0 = 0.0, m1 = 0.0;
    for (int64_t i = 0; i < Nx; ++i) { m0 = std::max(m0, R.row[(size_t)(i * nscen + s)]); m1 = std::max(m1, R.col[(size_t)(i * nscen + s)]); }
    EXPECT(R.tot[(size_t)s] == m0 && R.tot[(size_t)(nscen + s)] == m1, "totals are the maxima");
  }
  // scenario 1 alone, as shared values: the same bits
  std::vector<double> A1(A.nz.size()), B1v(B2.nz.size());
  for (size_t k = 0; k < A1.size(); ++k) A1[k] = Av[k * nscen + 1];
  for (size_t k = 0; k < B1v.size(); ++k) B1v[k] = Bv[k * nscen + 1];
  Out one;
  EXPECT(run(1, A1.data(), B1v.empty() ? nullptr : B1v.data(), false, one) == 0, "nscen = 1");
  bool same = one.tot[0] == R.tot[1] && one.tot[1] == R.tot[(size_t)nscen + 1];
  for (int64_t i = 0; i < Nx; ++i) same = same && one.row[(size_t)i] == R.row[(size_t)(i * nscen + 1)] && one.col[(size_t)i] == R.col[(size_t)(i * nscen + 1)];
  EXPECT(same, "a scenario does not depend on nscen or on how its values arrive");
  // NULL keeps the tables' values = the CSC arrays given as shared values
  Out keep, given;
  EXPECT(run(2, nullptr, nullptr, false, keep) == 0 && run(2, A.nz.data(), B2.nz.empty() ? nullptr : B2.nz.data(), false, given) == 0, "design values");
  EXPECT(keep.row == given.row && keep.col == given.col && keep.tot == given.tot, "NULL keeps the plan's values");
  return R;
}

}  // namespace

int main() {
  const int64_t shapes[4][3] = {{24, 6, 24}, {9, 3, 1}, {9, 3, 5}, {9, 0, 3}};
  for (const auto& sh : shapes) {
    Out r[2];
    for (int base = 0; base < 2; ++base) r[base] = drive(sh[0], sh[1], sh[2], base, 3);
    EXPECT(r[0].row == r[1].row && r[0].col == r[1].col && r[0].tot == r[1].tot && r[0].rn == r[1].rn && r[0].rs == r[1].rs, "index bases disagree");
    std::printf("Nx %lld Nu %lld T %lld: l1[0] %.6g e1[0] %.6g\n", (long long)sh[0], (long long)sh[1], (long long)sh[2],
                r[0].tot.empty() ? 0.0 : r[0].tot[0], r[0].tot.size() < 4 ? 0.0 : r[0].tot[3]);
  }
  {
    sls::MarginTables Tb; std::string msg;
    EXPECT(sls::build_margin_tables(nullptr, nullptr, nullptr, nullptr, Tb, msg) == SLS_EINVAL, "null arguments accepted");
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_margin: clean\n");
  return 0;
}
