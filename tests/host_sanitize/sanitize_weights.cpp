// Weights update on the host (csrc/sls_weights.cpp with the symbolic pass of csrc/sls_symbolic.cpp — no HIP in either) under
// AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_weights_host.py::test_weights_under_sanitizers with g++ -fsanitize=address,undefined.  Drives the updatable
// symbolic pass (SLS_PLAN_WEIGHTS_UPDATABLE), weights_shape_check, check_weights_update and weight_records_host over a chain plant
// with band masks in both index bases, with and without a ridge term: an update must leave exactly the weight pool a fresh pass on
// the re-weighted plant gives; refused values (NaN, inf, a zero weight without a ridge) keep their old records and are counted;
// shapes that are not updatable, an unflagged pass and passes of another size are refused; the records of the device-resident
// symbolic route (localized_weight_records) equal the flagged pass's.  Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_weights.h"

namespace {

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Csc {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> v;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
  sls_csc_bool mask() const { return sls_csc_bool{nr, nc, cp.data(), ri.data(), nullptr}; }
  void add_col(const std::vector<std::pair<int64_t, double>>& ents, int base) {
    if (cp.empty()) cp.push_back(base);
    for (auto& e : ents) { ri.push_back(e.first + base); v.push_back(e.second); }
    cp.push_back((int64_t)ri.size() + base); ++nc;
  }
};

struct Problem {
  int64_t Nx = 24, Nu = 12, T = 3;
  int base = 0;
  Csc A, B1, B2, C1, D12, D11;
  std::vector<Csc> Sx, Su;
  std::vector<sls_csc_bool> sx, su;
  std::vector<double> c, d;
};

// chain plant, B1 = diag (one zero entry: a b = 0 column), B2 column j drives state 2j, band masks of half-width 2
void make(Problem& p, int base, const std::vector<double>& c, const std::vector<double>& d) {
  p = Problem(); p.base = base; p.c = c; p.d = d;
  const int64_t Nx = p.Nx, Nu = p.Nu;
  p.A.nr = p.B1.nr = p.B2.nr = Nx; p.C1.nr = p.D12.nr = p.D11.nr = Nx + Nu;
  for (int64_t j = 0; j < Nx; ++j) {
    std::vector<std::pair<int64_t, double>> col;
    if (j > 0) col.push_back({j - 1, 0.2});
    col.push_back({j, 1.0});
    if (j + 1 < Nx) col.push_back({j + 1, -0.2});
    p.A.add_col(col, base);
    p.B1.add_col({{j, j == 5 ? 0.0 : 1.0 + 0.05 * (double)j}}, base);
    p.C1.add_col({{j, c[(size_t)j]}}, base);
    p.D11.add_col({}, base);
  }
  for (int64_t j = 0; j < Nu; ++j) { p.B2.add_col({{2 * j, 1.0}}, base); p.D12.add_col({{Nx + j, d[(size_t)j]}}, base); }
  p.Sx.resize((size_t)p.T); p.Su.resize((size_t)p.T);
  for (int64_t t = 0; t < p.T; ++t) {
    p.Sx[(size_t)t].nr = Nx; p.Su[(size_t)t].nr = Nu;
    for (int64_t col = 0; col < Nx; ++col) {
      std::vector<std::pair<int64_t, double>> ex, eu;
      for (int64_t r = 0; r < Nx; ++r) if (std::llabs(r - col) <= 2) ex.push_back({r, 1.0});
      for (int64_t j = 0; j < Nu; ++j) if (std::llabs(2 * j - col) <= 2) eu.push_back({j, 1.0});
      p.Sx[(size_t)t].add_col(ex, base); p.Su[(size_t)t].add_col(eu, base);
    }
  }
  for (int64_t t = 0; t < p.T; ++t) { p.sx.push_back(p.Sx[(size_t)t].mask()); p.su.push_back(p.Su[(size_t)t].mask()); }
}

int pass(const Problem& p, uint32_t flags, const double* rx, const double* ru, sls::Symbolic& S, std::string& msg, const Csc* C1 = nullptr,
         const Csc* D11 = nullptr, const Csc* B1 = nullptr, int64_t ngroups = 0, const int64_t* gptr = nullptr, const int64_t* gcols = nullptr) {
  sls_dims dims{p.Nx, p.Nu, p.Nx + p.Nu, p.Nx, p.T, p.base, flags};
  sls_csc_f64 A = p.A.f64(), b1 = (B1 ? *B1 : p.B1).f64(), B2 = p.B2.f64(), c1 = (C1 ? *C1 : p.C1).f64(), d12 = p.D12.f64(), d11 = (D11 ? *D11 : p.D11).f64();
  sls_plant P{&A, &b1, &B2, &c1, &d11, &d12};
  sls::Inputs in{&dims, &P, p.sx.data(), p.su.data(), ngroups, gptr, gcols};
  int rc = sls::validate_inputs(in, msg);
  if (rc) return rc;
  in.reg_x = rx; in.reg_u = ru;
  std::vector<int64_t> gp, gc;
  sls::normalise_groups(in, gp, gc);
  S = sls::Symbolic();
  S.want_packed = false; S.compact = false;
  return sls::build_symbolic(in, 0, (int64_t)gp.size() - 1, S, msg);
}

bool same(const sls::pool_vec<double>& a, const sls::pool_vec<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

std::vector<double> draw(std::mt19937& g, int64_t n) {
  std::uniform_real_distribution<double> u(0.5, 2.0);
  std::vector<double> v((size_t)n);
  for (double& x : v) x = u(g);
  return v;
}

void run(int base, bool ridge) {
  std::mt19937 g(11);
  Problem p, q;
  make(p, base, draw(g, 24), draw(g, 12));
  make(q, base, draw(g, 24), draw(g, 12));
  std::vector<double> rx, ru;
  if (ridge) { std::uniform_real_distribution<double> u(0.01, 0.3); rx.resize(24); ru.resize(12); for (double& x : rx) x = u(g); for (double& x : ru) x = u(g); }
  const double* prx = ridge ? rx.data() : nullptr; const double* pru = ridge ? ru.data() : nullptr;
  std::string msg;
  sls::Symbolic Sp, Sq, Su0;
  EXPECT(pass(p, SLS_PLAN_WEIGHTS_UPDATABLE, prx, pru, Sp, msg) == 0, "flagged pass");
  EXPECT(pass(q, SLS_PLAN_WEIGHTS_UPDATABLE, prx, pru, Sq, msg) == 0, "flagged pass on the re-weighted plant");
  EXPECT(pass(p, 0, prx, pru, Su0, msg) == 0 && !Su0.wu.updatable && Su0.wu.b2.empty(), "unflagged pass keeps nothing");
  EXPECT(same(Su0.w_pool, Sp.w_pool), "non-uniform weights: the flag changes no record");
  EXPECT(Sp.wu.updatable && Sp.wu.b2.size() == Sp.subs.size() && (int64_t)Sp.wu.owner.size() == p.Nx + p.Nu, "kept tables");
  for (const sls::SubDesc& sd : Sp.subs) EXPECT(sd.has_w == ((ridge || sd.out_index != 5) ? 1 : 0), "a record for every b != 0 column");

  // the update gives the fresh pass's pool, bit for bit; dirty where a record changed; the diagonals follow
  sls::pool_vec<double> w = Sp.w_pool;
  std::vector<double> diag = Sp.wu.diag;
  std::vector<uint8_t> dirty(Sp.subs.size(), 0);
  int64_t rej = -1;
  EXPECT(sls::weight_records_host(Sp, q.c.data(), q.d.data(), w.data(), diag.data(), dirty.data(), &rej, msg) == 0 && rej == 0, "update");
  EXPECT(same(w, Sq.w_pool) && diag == Sq.wu.diag, "update == fresh pass");
  for (const sls::SubDesc& sd : Sp.subs) EXPECT(dirty[(size_t)sd.out_index] == (sd.has_w && Sp.wu.b2[(size_t)sd.out_index] != 0.0 ? 1 : 0), "dirty marks");
  // one half at a time, then back
  sls::pool_vec<double> w2 = Sp.w_pool;
  EXPECT(sls::weight_records_host(Sp, q.c.data(), nullptr, w2.data(), nullptr, nullptr, nullptr, msg) == 0, "C1 alone");
  EXPECT(sls::weight_records_host(Sp, nullptr, q.d.data(), w2.data(), nullptr, nullptr, nullptr, msg) == 0 && same(w2, Sq.w_pool), "then D12");
  EXPECT(sls::weight_records_host(Sp, p.c.data(), p.d.data(), w2.data(), nullptr, nullptr, nullptr, msg) == 0 && same(w2, Sp.w_pool), "round trip");
  std::fill(dirty.begin(), dirty.end(), (uint8_t)0);
  EXPECT(sls::weight_records_host(Sp, p.c.data(), p.d.data(), w2.data(), nullptr, dirty.data(), nullptr, msg) == 0, "same values again");
  for (uint8_t b : dirty) EXPECT(b == 0, "nothing changed, nothing marked");

  // refused values: the host path's check names them; the twin skips them, keeps their records and counts them
  const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), 0.0};
  for (int b = 0; b < 3; ++b)
    for (int which = 0; which < 2; ++which) {
      std::vector<double> c = q.c, d = q.d;
      const int64_t k = which ? 7 : 13;
      (which ? d : c)[(size_t)k] = bad[b];
      const bool refused = b < 2 || !ridge;                     // 0.0 passes with a positive ridge
      const int rc = sls::check_weights_update(Sp.wu, p.Nx, p.Nu, c.data(), d.data(), msg);
      EXPECT(rc == (refused ? SLS_EINVAL : 0), "value rule");
      if (refused) EXPECT(msg.find(std::string(which ? "D12" : "C1") + " diagonal position " + std::to_string(k) + " ") != std::string::npos, "message names the value");
      sls::pool_vec<double> w3 = Sp.w_pool;
      std::vector<double> dg = Sp.wu.diag;
      EXPECT(sls::weight_records_host(Sp, c.data(), d.data(), w3.data(), dg.data(), nullptr, &rej, msg) == 0 && rej == (refused ? 1 : 0), "count");
      if (refused) {
        Problem r; std::vector<double> ck = c, dk = d;
        (which ? dk : ck)[(size_t)k] = (which ? p.d : p.c)[(size_t)k];
        make(r, base, ck, dk);
        sls::Symbolic Sr;
        EXPECT(pass(r, SLS_PLAN_WEIGHTS_UPDATABLE, prx, pru, Sr, msg) == 0 && same(w3, Sr.w_pool) && dg == Sr.wu.diag, "offender kept, the rest updated");
      }
    }

  // not updatable: an unflagged pass, tables of another size, shapes outside the rule
  EXPECT(sls::weight_records_host(Su0, q.c.data(), q.d.data(), w.data(), nullptr, nullptr, nullptr, msg) == SLS_EINVAL, "unflagged pass refused");
  { sls::Symbolic Sc = Sp; Sc.wu.owner.pop_back();
    EXPECT(sls::weight_records_host(Sc, q.c.data(), q.d.data(), w.data(), nullptr, nullptr, nullptr, msg) == SLS_EINVAL, "truncated tables refused");
    EXPECT(sls::check_weights_update(Sc.wu, p.Nx, p.Nu, q.c.data(), nullptr, msg) == SLS_EINVAL, "truncated tables refused by the check"); }
  sls::Symbolic Sx;
  { Csc C = p.C1; C.ri[3] += 1;                                                  // an entry off its own row
    EXPECT(pass(p, SLS_PLAN_WEIGHTS_UPDATABLE, prx, pru, Sx, msg, &C) == SLS_EUNSUPPORTED && msg.find("own z-row") != std::string::npos, "off-row entry"); }
  { Csc C; C.nr = p.Nx + p.Nu;                                                   // two entries in column 2
    for (int64_t j = 0; j < p.Nx; ++j) { if (j == 2) C.add_col({{2, 1.0}, {3, 0.5}}, base); else C.add_col({{j, 1.0}}, base); }
    EXPECT(pass(p, SLS_PLAN_WEIGHTS_UPDATABLE, prx, pru, Sx, msg, &C) == SLS_EUNSUPPORTED && msg.find("exactly one entry per column") != std::string::npos, "two entries"); }
  { Csc D; D.nr = p.Nx + p.Nu;                                                   // D11 on a selected row of column 4
    for (int64_t j = 0; j < p.Nx; ++j) { if (j == 4) D.add_col({{4, 0.3}}, base); else D.add_col({}, base); }
    EXPECT(pass(p, SLS_PLAN_WEIGHTS_UPDATABLE, prx, pru, Sx, msg, nullptr, &D) == SLS_EUNSUPPORTED && msg.find("D11") != std::string::npos, "D11 on a selected row"); }
  { Csc B; B.nr = p.Nx;                                                          // B1[8, 9] couples the group {8, 9}
    for (int64_t j = 0; j < p.Nx; ++j) { if (j == 9) B.add_col({{8, 0.5}, {9, 1.0}}, base); else B.add_col({{j, 1.0}}, base); }
    const int64_t gptr[2] = {0, 2}, gcols[2] = {8 + base, 9 + base};
    EXPECT(pass(p, SLS_PLAN_WEIGHTS_UPDATABLE, nullptr, nullptr, Sx, msg, nullptr, nullptr, &B, 1, gptr, gcols) == SLS_EUNSUPPORTED &&
           msg.find("coupled") != std::string::npos, "coupled group"); }
  if (!ridge) {
    // The records of the device-resident symbolic route (localized_weight_records) from what that route holds behind its fill
    // pass — descriptors without records, the index sets, the plan-time diagonals — against the flagged host pass: b², the value
    // rule's scale, which columns have a record, every record's content and the objective scales.  off_w legitimately differs:
    // the host pass packs the records back to back (none for the b = 0 column 5), the device route puts column c's at 2·idx_off[c].
    sls_dims dims{p.Nx, p.Nu, p.Nx + p.Nu, p.Nx, p.T, p.base, SLS_PLAN_WEIGHTS_UPDATABLE};
    sls_csc_f64 b1 = p.B1.f64();
    sls::Symbolic D;
    D.Nx = p.Nx; D.Nu = p.Nu; D.T = p.T; D.subs = Sp.subs; D.idx_pool = Sp.idx_pool;
    D.wu.updatable = true; D.wu.diag = Sp.wu.diag;
    D.obj_pool.assign(2 * Sp.subs.size(), 0.0);
    sls::LocalizedLayout lay;
    for (size_t c = 0; c < D.subs.size(); ++c) {
      D.subs[c].has_w = 0; D.subs[c].off_w = 0; D.obj_pool[2 * c] = c == 5 ? 1.0 : Sp.wu.b2[c];     // as localized_layout leaves them
      lay.idx_off.push_back(D.subs[c].off_sx);
    }
    lay.idx_total = (int64_t)D.idx_pool.size();
    EXPECT(sls::localized_weight_records(&dims, &b1, lay, D, msg) == 0, "localized_weight_records");
    EXPECT(D.wu.b2 == Sp.wu.b2 && D.wu.owner == Sp.wu.owner, "device route: b2 and the value rule's scale");
    EXPECT((int64_t)D.w_pool.size() == 2 * lay.idx_total && D.obj_pool.size() == Sp.obj_pool.size(), "device route: pool sizes");
    for (size_t c = 0; c < D.subs.size(); ++c) {
      const sls::SubDesc &a = D.subs[c], &b = Sp.subs[c];
      EXPECT(a.has_w == b.has_w && (a.has_w == 0 || a.off_w == 2 * lay.idx_off[c]), "device route: which columns have a record, and where");
      EXPECT(D.obj_pool[2 * c] == Sp.obj_pool[2 * c] && D.obj_pool[2 * c + 1] == Sp.obj_pool[2 * c + 1], "device route: objective record");
      if (a.has_w == 1 && b.has_w == 1)
        EXPECT(std::memcmp(D.w_pool.data() + a.off_w, Sp.w_pool.data() + b.off_w, 2 * (size_t)(a.n + a.m) * sizeof(double)) == 0, "device route: record content");
    }
    // a plan-time weight that breaks the value rule is refused with the route's suffix
    D.wu.diag[0] = 0.0;
    EXPECT(sls::localized_weight_records(&dims, &b1, lay, D, msg) == SLS_EUNSUPPORTED && msg.find("(plan-time weights)") != std::string::npos, "zero plan-time weight accepted");
  }
  std::printf("base=%d ridge=%d: %zu subproblems, %zu pool doubles\n", base, (int)ridge, Sp.subs.size(), Sp.w_pool.size());
}

}  // namespace

int main() {
  for (int base = 0; base < 2; ++base)
    for (int ridge = 0; ridge < 2; ++ridge) run(base, ridge != 0);
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_weights: clean\n");
  return 0;
}
