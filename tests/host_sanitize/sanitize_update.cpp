// Operator update on the host (csrc/sls_symbolic.cpp — no HIP) under AddressSanitizer + UndefinedBehaviorSanitizer: test
// infrastructure, built and run by tests/test_plant_update_host.py::test_update_under_sanitizers with
// g++ -fsanitize=address,undefined.  Drives operator_csr_checked, build_operator_value_map, check_operator_update and
// apply_operator_update over a chain, a banded plant with stored zeros and a random plant in both index bases: an update must
// leave exactly the arrays a fresh conversion of the new matrices gives; a refused update (zero rule, NaN, inf) and an update
// through a map or arrays of the wrong length must leave them untouched.  Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"

namespace {

struct Csc {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> v;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
};

// stored[r][c] != 0 keeps the entry; its value is val[r][c] (which may be 0.0: a stored zero)
Csc from_dense(const std::vector<std::vector<double>>& val, const std::vector<std::vector<char>>& stored, int64_t nr, int64_t nc, int base) {
  Csc m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r)
      if (stored[r][c]) { m.ri.push_back(r + base); m.v.push_back(val[r][c]); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Plant { int64_t Nx = 0, Nu = 0; Csc A, B2; };

// kind 0: chain, 1: banded with stored zeros on the ±3 diagonals of A and the −3 diagonal of B2, 2: random with stored zeros
Plant make(int kind, int base) {
  Plant p;
  p.Nx = kind == 2 ? 41 : 48; p.Nu = kind == 0 ? (p.Nx + 1) / 2 : (kind == 1 ? p.Nx : 9);
  std::vector<std::vector<double>> A(p.Nx, std::vector<double>(p.Nx, 0.0)), B(p.Nx, std::vector<double>(p.Nu, 0.0));
  std::vector<std::vector<char>> sA(p.Nx, std::vector<char>(p.Nx, 0)), sB(p.Nx, std::vector<char>(p.Nu, 0));
  auto setA = [&](int64_t r, int64_t c, double v) { if (r >= 0 && r < p.Nx && c >= 0 && c < p.Nx) { A[r][c] = v; sA[r][c] = 1; } };
  auto setB = [&](int64_t r, int64_t c, double v) { if (r >= 0 && r < p.Nx && c >= 0 && c < p.Nu) { B[r][c] = v; sB[r][c] = 1; } };
  std::mt19937 g(11 + kind);
  std::uniform_real_distribution<double> u(0.1, 1.0);
  for (int64_t i = 0; i < p.Nx; ++i) {
    setA(i, i, 1.0);
    if (kind == 0) { setA(i, i + 1, 0.2); setA(i + 1, i, -0.2); }
    if (kind == 1) { setA(i, i + 1, 0.2); setA(i + 1, i, -0.2); setA(i, i + 2, 0.1); setA(i + 2, i, -0.1); setA(i, i + 3, 0.0); setA(i + 3, i, 0.0); }
    if (kind == 2) for (int q = 0; q < 4; ++q) setA((int64_t)(g() % p.Nx), i, (q == 3) ? 0.0 : u(g));
  }
  for (int64_t j = 0; j < p.Nu; ++j) {
    if (kind == 0) setB(2 * j < p.Nx ? 2 * j : p.Nx - 1, j, 1.0);
    if (kind == 1) { setB(j, j, 1.0); setB(j + 1, j, 0.5); setB(j + 2, j, -0.25); setB(j + 3, j, 0.0); }
    if (kind == 2) for (int q = 0; q < 5; ++q) setB((int64_t)(g() % p.Nx), j, (q == 0) ? 0.0 : u(g));
  }
  p.A = from_dense(A, sA, p.Nx, p.Nx, base); p.B2 = from_dense(B, sB, p.Nx, p.Nu, base);
  return p;
}

bool same(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}
bool same_operator(const sls::Symbolic& X, const sls::Symbolic& Y) {
  return same(X.A_csr.val, Y.A_csr.val) && same(X.At_csr.val, Y.At_csr.val) && same(X.B_csr.val, Y.B_csr.val) && same(X.Bt_csr.val, Y.Bt_csr.val) &&
         X.A_csr.idx == Y.A_csr.idx && X.A_csr.ptr == Y.A_csr.ptr && X.B_csr.idx == Y.B_csr.idx && X.B_csr.ptr == Y.B_csr.ptr;
}

void run(int kind, int base) {
  const Plant p = make(kind, base);
  sls_dims dims{p.Nx, p.Nu, p.Nx + p.Nu, p.Nx, 4, base, 0};
  sls_csc_f64 A = p.A.f64(), B2 = p.B2.f64();
  std::string msg;
  sls::Symbolic S0;
  EXPECT(sls::operator_csr_checked(&dims, &A, &B2, S0, msg) == 0, "operator_csr_checked");
  sls::OperatorValueMap M;
  sls::build_operator_value_map(S0, M);
  const int64_t nA = (int64_t)p.A.v.size(), nB = (int64_t)p.B2.v.size();
  EXPECT(M.nnzA == nA && M.nnzB == nB && (int64_t)M.row_pos.size() == nA + nB && M.zero.size() == M.row_pos.size(), "map sizes");
  int64_t nzero = 0;
  for (int64_t k = 0; k < nA + nB; ++k) {
    const double v = k < nA ? p.A.v[k] : p.B2.v[k - nA];
    EXPECT((M.zero[k] != 0) == (v == 0.0), "zero mark");
    EXPECT(M.row_pos[k] >= 0 && M.row_pos[k] < (k < nA ? nA : nB), "map range");
    nzero += M.zero[k];
  }
  if (kind != 0) EXPECT(nzero > 0, "the plant has stored zeros");

  // new values: every stored value scaled, stored zeros stay zero; one non-zero goes to 0.0
  std::mt19937 g(5);
  std::uniform_real_distribution<double> u(0.8, 1.2);
  Plant q = p;
  for (double& v : q.A.v) v *= u(g);
  for (double& v : q.B2.v) v *= u(g);
  for (int64_t k = 0; k < nA; ++k) if (q.A.v[k] != 0.0 && k % 13 == 5) { q.A.v[k] = 0.0; break; }
  sls_csc_f64 Aq = q.A.f64(), Bq = q.B2.f64();
  sls::Symbolic Sq, Sa, Sb;
  EXPECT(sls::operator_csr_checked(&dims, &Aq, &Bq, Sq, msg) == 0, "operator_csr_checked (new plant)");
  sls::Symbolic S = S0;
  EXPECT(sls::apply_operator_update(S, M, q.A.v.data(), q.B2.v.data(), msg) == 0, "apply both");
  EXPECT(same_operator(S, Sq), "update == fresh conversion");
  // one matrix at a time, then nothing
  EXPECT(sls::operator_csr_checked(&dims, &Aq, &B2, Sa, msg) == 0 && sls::operator_csr_checked(&dims, &A, &Bq, Sb, msg) == 0, "mixed plants");
  S = S0; EXPECT(sls::apply_operator_update(S, M, q.A.v.data(), nullptr, msg) == 0 && same_operator(S, Sa), "A alone");
  S = S0; EXPECT(sls::apply_operator_update(S, M, nullptr, q.B2.v.data(), msg) == 0 && same_operator(S, Sb), "B2 alone");
  S = S0; EXPECT(sls::apply_operator_update(S, M, nullptr, nullptr, msg) == 0 && same_operator(S, S0), "nothing given");
  // and back: the round trip restores the plan-time arrays
  S = Sq; EXPECT(sls::apply_operator_update(S, M, p.A.v.data(), p.B2.v.data(), msg) == 0 && same_operator(S, S0), "round trip");

  // refusals: the arrays stay as they were, the message names the matrix and the position
  const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
  for (int b = 0; b < 3; ++b)
    for (int which = 0; which < 2; ++which) {
      Plant r = q;
      const int64_t k = (which ? nB : nA) - 1;
      (which ? r.B2.v : r.A.v)[k] = bad[b];
      S = S0;
      EXPECT(sls::apply_operator_update(S, M, r.A.v.data(), r.B2.v.data(), msg) == SLS_EINVAL && same_operator(S, S0), "non-finite refused, untouched");
      EXPECT(msg.find(std::string(which ? "B2" : "A") + " nzval position " + std::to_string(k) + " ") != std::string::npos, "message names the entry");
      EXPECT(sls::check_operator_update(M, which ? nullptr : r.A.v.data(), which ? r.B2.v.data() : nullptr, msg) == SLS_EINVAL, "check alone");
    }
  for (int64_t k = 0; k < nA + nB; ++k) {
    if (!M.zero[k]) continue;
    Plant r = q;
    (k < nA ? r.A.v[k] : r.B2.v[k - nA]) = 1e-300;
    S = S0;
    EXPECT(sls::apply_operator_update(S, M, r.A.v.data(), r.B2.v.data(), msg) == SLS_EINVAL && same_operator(S, S0), "zero rule refused, untouched");
    (k < nA ? r.A.v[k] : r.B2.v[k - nA]) = -0.0;
    S = S0;
    EXPECT(sls::apply_operator_update(S, M, r.A.v.data(), r.B2.v.data(), msg) == 0, "−0.0 on a plan-time zero is a zero");
  }

  // malformed: a map of another plant, a truncated map, arrays that lost an entry — refused before anything is read or written
  {
    sls::OperatorValueMap Mshort = M;
    Mshort.row_pos.pop_back();
    S = S0; EXPECT(sls::apply_operator_update(S, Mshort, q.A.v.data(), q.B2.v.data(), msg) == SLS_EINVAL && same_operator(S, S0), "truncated map");
    sls::OperatorValueMap Mz = M;
    Mz.zero.pop_back();
    S = S0; EXPECT(sls::apply_operator_update(S, Mz, q.A.v.data(), q.B2.v.data(), msg) == SLS_EINVAL && same_operator(S, S0), "truncated marks");
    sls::OperatorValueMap Mn = M;
    Mn.nnzA += 1;
    S = S0; EXPECT(sls::apply_operator_update(S, Mn, q.A.v.data(), q.B2.v.data(), msg) == SLS_EINVAL && same_operator(S, S0), "map of another plant");
    sls::Symbolic Scut = S0;
    Scut.A_csr.val.pop_back();
    EXPECT(sls::apply_operator_update(Scut, M, q.A.v.data(), q.B2.v.data(), msg) == SLS_EINVAL, "operator array of the wrong length");
    sls::Symbolic Sempty;
    EXPECT(sls::apply_operator_update(Sempty, M, q.A.v.data(), q.B2.v.data(), msg) == SLS_EINVAL, "empty symbolic pass");
    // malformed matrices never reach the map
    Csc broken = p.A; broken.cp[1] = broken.cp[2] + 1;
    sls_csc_f64 Ab = broken.f64();
    sls::Symbolic Sx;
    EXPECT(sls::operator_csr_checked(&dims, &Ab, &B2, Sx, msg) != 0, "a colptr that is not monotone is refused");
    sls_dims wrong = dims; wrong.Nu += 1;
    EXPECT(sls::operator_csr_checked(&wrong, &A, &B2, Sx, msg) != 0, "wrong dimensions are refused");
    EXPECT(sls::operator_csr_checked(&dims, nullptr, &B2, Sx, msg) != 0, "null matrix is refused");
  }
  std::printf("kind=%d base=%d: nnz(A)=%lld nnz(B2)=%lld stored zeros=%lld\n", kind, base, (long long)nA, (long long)nB, (long long)nzero);
}

}  // namespace

int main() {
  for (int kind = 0; kind < 3; ++kind)
    for (int base = 0; base < 2; ++base) run(kind, base);
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_update: clean\n");
  return 0;
}
