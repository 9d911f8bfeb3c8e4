// Affected-column marks on the host (csrc/sls_symbolic.cpp — no HIP) under AddressSanitizer + UndefinedBehaviorSanitizer: test
// infrastructure, built and run by tests/test_partial_host.py::test_affected_under_sanitizers with
// g++ -fsanitize=address,undefined.  Drives operator_csr_checked, build_operator_value_map and mark_affected_host over a banded
// and a random plant in both index bases, with hand-made subproblem tables (windows of states and actuators: ñx = 1, ñu = 0, the
// whole plant, and windows in between) against a brute-force statement of the rule; marks accumulate, untouched bytes stay, and
// a map of the wrong plant is refused.  Exit code 0 = clean.
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"

namespace {

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Csc {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> v;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
};

// pattern(r, c) decides what is stored
template <class F>
Csc make(int64_t nr, int64_t nc, int base, F pattern) {
  Csc m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r)
      if (pattern(r, c)) { m.ri.push_back(r + base); m.v.push_back(1.0 + 0.01 * (double)(r + c)); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

void run(int kind, int base) {
  const int64_t Nx = kind == 0 ? 40 : 33, Nu = kind == 0 ? 70 : 7;
  std::mt19937 g(3 + kind);
  std::vector<char> rA((size_t)(Nx * Nx), 0), rB((size_t)(Nx * Nu), 0);
  for (auto& c : rA) c = (g() % 6) == 0;
  for (auto& c : rB) c = (g() % 4) == 0;
  // kind 0: banded A, B2 with one dense row of 70 entries (row 20) on top of a diagonal; kind 1: random
  const Csc A = kind == 0 ? make(Nx, Nx, base, [](int64_t r, int64_t c) { return r - c <= 2 && c - r <= 2; })
                          : make(Nx, Nx, base, [&](int64_t r, int64_t c) { return r == c || rA[(size_t)(r * Nx + c)]; });
  const Csc B = kind == 0 ? make(Nx, Nu, base, [](int64_t r, int64_t c) { return r == 20 || r == c; })
                          : make(Nx, Nu, base, [&](int64_t r, int64_t c) { return rB[(size_t)(r * Nu + c)] != 0; });
  sls_dims dims{Nx, Nu, Nx + Nu, Nx, 4, base, 0};
  sls_csc_f64 a = A.f64(), b = B.f64();
  std::string msg;
  sls::Symbolic S;
  EXPECT(sls::operator_csr_checked(&dims, &a, &b, S, msg) == 0, "operator_csr_checked");
  sls::OperatorValueMap M;
  sls::build_operator_value_map(S, M);
  const int64_t nA = (int64_t)A.v.size(), nB = (int64_t)B.v.size();

  // subproblem tables: (first state, states, first actuator, actuators), ascending global indices in idx_pool
  struct Win { int64_t x0, n, u0, m; };
  std::vector<Win> wins = {{0, 1, 0, 0}, {Nx - 1, 1, Nu - 1, 1}, {0, Nx, 0, Nu}, {5, 9, 0, 3}, {18, 5, 10 % Nu, Nu - 10 % Nu}, {19, 3, 0, 0}, {0, 21, 2, 4}};
  for (int64_t c = 0; c < Nx; c += 3) wins.push_back({c, std::min<int64_t>(6, Nx - c), c % Nu, std::min<int64_t>(2, Nu - c % Nu)});
  S.subs.resize(wins.size());
  for (size_t q = 0; q < wins.size(); ++q) {
    sls::SubDesc sd{};
    sd.n = (int32_t)wins[q].n; sd.m = (int32_t)wins[q].m;
    sd.off_sx = (int64_t)S.idx_pool.size();
    for (int64_t i = 0; i < wins[q].n; ++i) S.idx_pool.push_back((int32_t)(wins[q].x0 + i));
    sd.off_su = (int64_t)S.idx_pool.size();
    for (int64_t i = 0; i < wins[q].m; ++i) S.idx_pool.push_back((int32_t)(wins[q].u0 + i));
    sd.out_index = (int64_t)(wins.size() - 1 - q);      // col_status order need not be table order
    S.subs[q] = sd;
  }

  auto brute = [&](const std::vector<uint8_t>& cA, const std::vector<uint8_t>& cB, std::vector<uint8_t>& out) {
    for (size_t q = 0; q < wins.size(); ++q) {
      const Win& w = wins[q];
      bool hit = false;
      for (int64_t c = 0; c < Nx && !hit; ++c)
        for (int64_t k = A.cp[c] - base; k < A.cp[c + 1] - base && !hit; ++k) {
          const int64_t r = A.ri[k] - base;
          hit = cA[(size_t)k] && r >= w.x0 && r < w.x0 + w.n && c >= w.x0 && c < w.x0 + w.n;
        }
      for (int64_t c = 0; c < Nu && !hit; ++c)
        for (int64_t k = B.cp[c] - base; k < B.cp[c + 1] - base && !hit; ++k) {
          const int64_t r = B.ri[k] - base;
          hit = cB[(size_t)k] && r >= w.x0 && r < w.x0 + w.n && c >= w.u0 && c < w.u0 + w.m;
        }
      if (hit) out[wins.size() - 1 - q] = 1;
    }
  };

  int64_t some = 0;
  for (int trial = 0; trial < 40; ++trial) {
    std::vector<uint8_t> cA((size_t)nA, 0), cB((size_t)nB, 0);
    if (trial == 0) { /* nothing changed */ }
    else if (trial == 1) std::fill(cA.begin(), cA.end(), (uint8_t)1);
    else if (trial == 2) std::fill(cB.begin(), cB.end(), (uint8_t)1);
    else if (trial == 3 && kind == 0) {                 // the dense row of B2 alone
      for (int64_t c = 0; c < Nu; ++c)
        for (int64_t k = B.cp[c] - base; k < B.cp[c + 1] - base; ++k) if (B.ri[k] - base == 20) cB[(size_t)k] = 1;
    } else {
      const int na = (int)(g() % 3), nb = (int)(g() % 3);
      for (int i = 0; i < na; ++i) cA[(size_t)(g() % (uint64_t)nA)] = 1;
      for (int i = 0; i < nb; ++i) cB[(size_t)(g() % (uint64_t)nB)] = 1;
    }
    std::vector<uint8_t> got(wins.size() + 1, 0), want(wins.size() + 1, 0);
    got[wins.size()] = want[wins.size()] = 9;            // a guard byte behind the marks
    EXPECT(sls::mark_affected_host(S, M, cA.data(), cB.data(), got.data(), msg) == 0, "mark_affected_host");
    brute(cA, cB, want);
    EXPECT(got == want, "marks == brute force");
    for (uint8_t v : want) some += v == 1;
    if (trial == 0) for (size_t q = 0; q < wins.size(); ++q) EXPECT(got[q] == 0, "no change, no mark");
    // one matrix at a time accumulates to the same marks; a NULL array means none of its entries changed
    std::vector<uint8_t> acc(wins.size() + 1, 0);
    acc[wins.size()] = 9;
    EXPECT(sls::mark_affected_host(S, M, cA.data(), nullptr, acc.data(), msg) == 0, "A alone");
    EXPECT(sls::mark_affected_host(S, M, nullptr, cB.data(), acc.data(), msg) == 0, "B2 alone");
    EXPECT(acc == want, "marks accumulate");
  }
  EXPECT(some > 0, "some trial marked something");

  // a map that does not belong to this pass is refused before anything is read
  {
    std::vector<uint8_t> cA((size_t)nA, 1), cB((size_t)nB, 1), out(wins.size(), 0);
    sls::OperatorValueMap Mn = M;
    Mn.nnzA += 1;
    EXPECT(sls::mark_affected_host(S, Mn, cA.data(), cB.data(), out.data(), msg) == SLS_EINVAL, "map of another plant");
    sls::OperatorValueMap Ms = M;
    Ms.row_pos.pop_back();
    EXPECT(sls::mark_affected_host(S, Ms, cA.data(), cB.data(), out.data(), msg) == SLS_EINVAL, "truncated map");
    sls::Symbolic Sempty;
    EXPECT(sls::mark_affected_host(Sempty, M, cA.data(), cB.data(), out.data(), msg) == SLS_EINVAL, "empty symbolic pass");
    for (uint8_t v : out) EXPECT(v == 0, "a refused call marks nothing");
  }
  std::printf("kind=%d base=%d: nnz(A)=%lld nnz(B2)=%lld subproblems=%zu marks=%lld\n", kind, base, (long long)nA, (long long)nB, wins.size(), (long long)some);
}

}  // namespace

int main() {
  for (int kind = 0; kind < 2; ++kind)
    for (int base = 0; base < 2; ++base) run(kind, base);
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_affected: clean\n");
  return 0;
}
