// Host symbolic pass (csrc/sls_symbolic.cpp — no HIP in it) under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure,
// built and run by tests/test_host.py::test_symbolic_pass_under_sanitizers with g++ -fsanitize=address,undefined.  Drives every
// host-only entry the C ABI forwards to — mask recipe, validation, index sets, the full symbolic pass in its four table layouts
// (explicit / compact × packed / mask order), shard ranges, caller groups (decoupled and coupled), cost model, the inputs of
// the two device passes (also on the hub, long-range, dense and stored-zero plants of tests/symbolic_cases.py), their LDS list plans
// (csrc/sls_symbolic_device.h) and the host arithmetic of the device-resident route (localized_layout, against the host pass), the closed-loop FIR operator (restated exactly from the masks: check_fir), kernel selection (csrc/sls_routing.cpp: the launch list of every shard for
// 1, 8 and 256 CUs, both objectives, with and without force_tile) — on a chain, a 2-D grid and a random plant, in both index bases, plus
// malformed inputs that must be refused without touching memory out of bounds; and the host arithmetic of plan construction: the arena's
// layout (csrc/sls_arena.h) against offsets worked out by hand, the scratch workspace against its formula written out, the solver
// knobs (every parse and clamp in lab mode; "defaults" as the first argument: the defaults, with lab mode off and every knob set),
// the sum-of-norms weights check.  Exit code 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_arena.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_routing.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic.h"
#include "../../systemlevelcontrol.jl_amd/csrc/sls_symbolic_device.h"

namespace {

struct Csc {
  int64_t nr = 0, nc = 0;
  std::vector<int64_t> cp, ri;
  std::vector<double> v;
  std::vector<uint8_t> b;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
  sls_csc_bool boolean() const { return sls_csc_bool{nr, nc, cp.data(), ri.data(), b.empty() ? nullptr : b.data()}; }
};

// dense pattern → CSC in the given index base
Csc from_dense(const std::vector<std::vector<double>>& M, int64_t nr, int64_t nc, int base) {
  Csc m; m.nr = nr; m.nc = nc; m.cp.assign(nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r)
      if (M[r][c] != 0.0) { m.ri.push_back(r + base); m.v.push_back(M[r][c]); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}

struct Plant { int64_t Nx, Nu; Csc A, B1, B2; };

Plant chain(int64_t Nx, int base, bool coupled_b1) {
  std::vector<std::vector<double>> A(Nx, std::vector<double>(Nx, 0.0)), B1(Nx, std::vector<double>(Nx, 0.0));
  for (int64_t i = 0; i < Nx; ++i) {
    A[i][i] = 1.0; B1[i][i] = 1.0 + 0.01 * i;
    if (i + 1 < Nx) { A[i][i + 1] = 0.2; A[i + 1][i] = -0.2; if (coupled_b1 && i % 4 == 0) B1[i][i + 1] = 0.3; }
  }
  const int64_t Nu = (Nx + 2) / 3;
  std::vector<std::vector<double>> B2(Nx, std::vector<double>(Nu, 0.0));
  for (int64_t j = 0; j < Nu; ++j) B2[std::min(Nx - 1, 3 * j)][j] = 1.0;
  return Plant{Nx, Nu, from_dense(A, Nx, Nx, base), from_dense(B1, Nx, Nx, base), from_dense(B2, Nx, Nu, base)};
}

Plant grid(int64_t n, int base) {
  const int64_t Nx = n * n;
  std::vector<std::vector<double>> A(Nx, std::vector<double>(Nx, 0.0)), B1(Nx, std::vector<double>(Nx, 0.0));
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) {
      const int64_t k = i * n + j;
      A[k][k] = 0.9; B1[k][k] = 1.0;
      if (i + 1 < n) { A[k][k + n] = 0.1; A[k + n][k] = 0.1; }
      if (j + 1 < n) { A[k][k + 1] = 0.1; A[k + 1][k] = 0.1; }
    }
  const int64_t Nu = (Nx + 1) / 2;
  std::vector<std::vector<double>> B2(Nx, std::vector<double>(Nu, 0.0));
  for (int64_t j = 0; j < Nu; ++j) B2[std::min(Nx - 1, 2 * j)][j] = 1.0;
  return Plant{Nx, Nu, from_dense(A, Nx, Nx, base), from_dense(B1, Nx, Nx, base), from_dense(B2, Nx, Nu, base)};
}

Plant random_plant(int64_t Nx, int base, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<std::vector<double>> A(Nx, std::vector<double>(Nx, 0.0)), B1(Nx, std::vector<double>(Nx, 0.0));
  for (int64_t i = 0; i < Nx; ++i) {
    A[i][i] = 1.0; B1[i][i] = 0.5 + u(g);
    for (int64_t j = 0; j < Nx; ++j) if (i != j && u(g) < 0.05) A[i][j] = u(g) - 0.5;
  }
  Plant P{Nx, 0, from_dense(A, Nx, Nx, base), from_dense(B1, Nx, Nx, base), {}};
  // stored zeros in A: (A .≠ 0) is by value
  for (size_t k = 0; k < P.A.v.size(); k += 7) if (P.A.ri[k] - base != (int64_t)0) P.A.v[k] = (k % 14 == 0) ? 0.0 : P.A.v[k];
  const int64_t Nu = Nx / 2;
  std::vector<std::vector<double>> B2(Nx, std::vector<double>(Nu, 0.0));
  for (int64_t j = 0; j < Nu; ++j) { B2[2 * j][j] = 1.0; if (u(g) < 0.3) B2[(2 * j + 5) % Nx][j] = 0.5; }
  P.Nu = Nu; P.B2 = from_dense(B2, Nx, Nu, base);
  return P;
}

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

struct Masks { std::vector<Csc> x, u; std::vector<sls_csc_bool> bx, bu; };

Masks make_masks(const Plant& P, int64_t d, int64_t T, double alpha, int base) {
  sls_dims dims{P.Nx, P.Nu, P.Nx + P.Nu, P.Nx, T, base, 0};
  sls_csc_f64 A = P.A.f64(), B2 = P.B2.f64();
  std::vector<int64_t> nx(T), nu(T);
  std::string msg;
  int rc = sls::localization_masks(&dims, &A, &B2, d, alpha, nx.data(), nu.data(), nullptr, nullptr, nullptr, nullptr, msg);
  EXPECT(rc == 0, "mask recipe (count)");
  Masks M; M.x.resize(T); M.u.resize(T);
  std::vector<int64_t*> cpx(T), rvx(T), cpu(T), rvu(T);
  for (int64_t t = 0; t < T; ++t) {
    M.x[t].nr = P.Nx; M.x[t].nc = P.Nx; M.x[t].cp.assign(P.Nx + 1, 0); M.x[t].ri.assign(nx[t], 0);
    M.u[t].nr = P.Nu; M.u[t].nc = P.Nx; M.u[t].cp.assign(P.Nx + 1, 0); M.u[t].ri.assign(nu[t], 0);
    cpx[t] = M.x[t].cp.data(); rvx[t] = M.x[t].ri.data(); cpu[t] = M.u[t].cp.data(); rvu[t] = M.u[t].ri.data();
  }
  rc = sls::localization_masks(&dims, &A, &B2, d, alpha, nx.data(), nu.data(), cpx.data(), rvx.data(), cpu.data(), rvu.data(), msg);
  EXPECT(rc == 0, "mask recipe (fill)");
  for (int64_t t = 0; t < T; ++t) { M.bx.push_back(M.x[t].boolean()); M.bu.push_back(M.u[t].boolean()); }
  return M;
}

// Kernel selection on a finished symbolic pass.  Invariants only (the launch lists themselves: tests/golden/launch_lists.json):
// every column that is neither too large nor a member of a coupled group sits in exactly one launch's slice of S.order,
// grid ≥ 1, LDS within 160 KiB, the launches' workspace regions disjoint and inside the reported totals.
void check_routing(const sls::Symbolic& S0) {
  for (int ncu : {1, 8, 256})
    for (int objective = 0; objective < 2; ++objective)
      for (int force_tile = 0; force_tile < 2; ++force_tile) {
        sls::Symbolic S = S0;
        sls::RoutingResult R;
        std::string msg;
        const int rc = sls::build_launch_list(S, (int)S.T, objective, ncu, force_tile != 0, sls::RoutingKnobs{}, R, msg);
        if (rc == SLS_EUNSUPPORTED) continue;
        EXPECT(rc == 0, "build_launch_list");
        std::vector<int> seen(S.subs.size(), 0);
        for (int32_t q : R.too_large) seen[(size_t)q] -= 1 << 20;
        int64_t fac_end = 0, vec_end = 0, big_end = 0;       // offsets ascend in submission order: disjoint iff each starts at the last end
        for (const sls::LaunchSpec& L : R.launches) {
          EXPECT(L.grid >= 1 && L.nsub >= 1 && L.lds <= (size_t)sls::kMaxLds, "launch grid / LDS");
          EXPECT(L.order_off >= 0 && (size_t)L.order_off + (size_t)L.nsub <= S.order.size(), "launch slice of S.order");
          for (int i = 0; i < L.nsub; ++i) seen[(size_t)S.order[(size_t)L.order_off + i]] += 1;
          EXPECT(L.fac_off >= fac_end, "factor workspace regions overlap"); fac_end = L.fac_off + L.fac_stride * L.grid;
          if (!L.vec_in_lds) { EXPECT(L.vec_off >= vec_end, "vector workspace regions overlap"); vec_end = L.vec_off + L.vec_stride * L.grid; }
          if (L.big) { EXPECT(L.big_off >= big_end, "carve workspace regions overlap"); big_end = L.big_off + L.big_stride * L.grid; }
        }
        EXPECT((size_t)fac_end <= R.fac_doubles && (size_t)vec_end <= R.vec_doubles && (size_t)big_end <= R.big_bytes, "workspace totals");
        for (size_t q = 0; q < S.subs.size(); ++q) {
          const bool member = S0.subs[q].has_w == 4;
          EXPECT(seen[q] == (member ? 0 : 1) || (seen[q] == -(1 << 20) && !member), "column not in exactly one launch");
        }
      }
}

// build_fir_operator against an exact restatement from the CSC masks.  The value array is the slices' stored entries back to
// back, Sx[0..T−1] then Su[0..T−1]; the operator holds the stored-true entries of Sx[1..T−1] (lag τ = t) and Su[0..T−1] (lag
// τ = t + 1), β rows first, inside a row ascending in (τ, c), each as hoff = τ·Nx − c and perm = its index in the value array.
void csr_equals_csc(const sls::HostCsr& R, const Csc& m, int base) {
  EXPECT(R.nrows == m.nr && R.ncols == m.nc && (int64_t)R.ptr.size() == m.nr + 1, "CSR copy: shape");
  EXPECT(R.idx.size() == m.ri.size() && R.val.size() == m.ri.size(), "CSR copy: number of entries");
  if ((int64_t)R.ptr.size() != m.nr + 1 || R.idx.size() != m.ri.size() || R.val.size() != m.ri.size()) return;
  EXPECT(R.ptr[0] == 0 && R.ptr[m.nr] == (int32_t)m.ri.size(), "CSR copy: row pointer ends");
  std::vector<std::vector<std::pair<int32_t, double>>> rows((size_t)m.nr);       // columns ascend: entries arrive in (r, c) order
  for (int64_t c = 0; c < m.nc; ++c)
    for (int64_t k = m.cp[c] - base; k < m.cp[c + 1] - base; ++k) rows[(size_t)(m.ri[k] - base)].push_back({(int32_t)c, m.v[k]});
  for (int64_t r = 0; r < m.nr; ++r) {
    const bool len_ok = R.ptr[r] >= 0 && R.ptr[r + 1] - R.ptr[r] == (int32_t)rows[r].size() && R.ptr[r + 1] <= (int32_t)R.idx.size();
    EXPECT(len_ok, "CSR copy: row length");
    if (!len_ok) return;
    for (size_t q = 0; q < rows[r].size(); ++q)
      EXPECT(R.idx[R.ptr[r] + q] == rows[r][q].first && R.val[R.ptr[r] + q] == rows[r][q].second, "CSR copy: entry");
  }
}

void check_fir(const Plant& P, const Masks& M, int64_t T, int base) {
  sls_dims dims{P.Nx, P.Nu, P.Nx + P.Nu, P.Nx, T, base, 0};
  sls_csc_f64 A = P.A.f64(), B1 = P.B1.f64(), B2 = P.B2.f64();
  std::string msg;
  sls::FirOperator F;
  const int rc = sls::build_fir_operator(&dims, &A, &B1, &B2, M.bx.data(), M.bu.data(), F, msg);
  EXPECT(rc == 0, "build_fir_operator");
  if (rc) { std::fprintf(stderr, "  %s\n", msg.c_str()); return; }
  struct Entry { int64_t row, lag, col, perm; };
  std::vector<Entry> eb, eu;                           // expected β and u entries
  std::vector<int64_t> forbidden;                      // value-array indices the operator must not read: Sx[0], stored false
  int64_t off = 0, n_true = 0;
  for (int part = 0; part < 2; ++part)
    for (int64_t t = 0; t < T; ++t) {
      const Csc& m = part ? M.u[t] : M.x[t];
      for (int64_t c = 0; c < P.Nx; ++c)
        for (int64_t k = m.cp[c] - base; k < m.cp[c + 1] - base; ++k) {
          const bool stored_true = m.b.empty() || m.b[k];
          if ((part == 0 && t == 0) || !stored_true) { forbidden.push_back(off + k); continue; }
          (part ? eu : eb).push_back(Entry{m.ri[k] - base, part ? t + 1 : t, c, off + k});
          ++n_true;
        }
      off += (int64_t)m.ri.size();
    }
  auto by_row = [](const Entry& a, const Entry& b) { return a.row != b.row ? a.row < b.row : a.lag != b.lag ? a.lag < b.lag : a.col < b.col; };
  std::sort(eb.begin(), eb.end(), by_row); std::sort(eu.begin(), eu.end(), by_row);
  EXPECT(F.Nx == P.Nx && F.Nu == P.Nu && F.Nw == P.Nx && F.T == T && F.n_values == off, "FIR dimensions");
  // pointer arrays
  EXPECT((int64_t)F.beta_ptr.size() == P.Nx + 1 && (int64_t)F.u_ptr.size() == P.Nu + 1, "FIR pointer array lengths");
  if ((int64_t)F.beta_ptr.size() != P.Nx + 1 || (int64_t)F.u_ptr.size() != P.Nu + 1) return;
  EXPECT(F.beta_ptr[0] == 0, "beta_ptr[0]");
  for (int64_t r = 0; r < P.Nx; ++r) EXPECT(F.beta_ptr[r] <= F.beta_ptr[r + 1], "beta_ptr monotone");
  for (int64_t r = 0; r < P.Nu; ++r) EXPECT(F.u_ptr[r] <= F.u_ptr[r + 1], "u_ptr monotone");
  EXPECT(F.u_ptr[0] == F.beta_ptr[P.Nx] && F.u_ptr[0] == (int64_t)eb.size(), "u_ptr[0] == beta_ptr[Nx]");
  EXPECT(F.u_ptr[P.Nu] == n_true, "u_ptr[Nu] == stored-true entries of Sx[1..T-1] and Su");
  EXPECT((int64_t)F.hoff.size() == n_true && (int64_t)F.perm.size() == n_true, "FIR entry count");
  if ((int64_t)F.hoff.size() != n_true || (int64_t)F.perm.size() != n_true || F.u_ptr[P.Nu] != n_true) return;
  // entries, row by row
  for (int part = 0; part < 2; ++part) {
    const std::vector<Entry>& ex = part ? eu : eb;
    const std::vector<int32_t>& ptr = part ? F.u_ptr : F.beta_ptr;
    const int64_t first = part ? (int64_t)eb.size() : 0;
    for (size_t q = 0; q < ex.size(); ++q) {
      const int64_t e = first + (int64_t)q;
      EXPECT(ptr[ex[q].row] <= e && e < ptr[ex[q].row + 1], "FIR entry in its row");
      EXPECT(F.hoff[e] == ex[q].lag * P.Nx - ex[q].col, "FIR hoff == lag*Nx - col");
      EXPECT(F.perm[e] == ex[q].perm, "FIR perm == slice offset + position in the slice");
    }
  }
  // perm as a whole: injective, never into Sx[0], never at a stored-false entry
  std::vector<int32_t> sorted(F.perm);
  std::sort(sorted.begin(), sorted.end());
  EXPECT(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "FIR perm injective");
  EXPECT(sorted.empty() || (sorted.front() >= (int64_t)M.x[0].ri.size() && sorted.back() < off), "FIR perm outside Sx[0], inside the array");
  for (int64_t f : forbidden) EXPECT(!std::binary_search(sorted.begin(), sorted.end(), (int32_t)f), "FIR perm points at Sx[0] or a stored-false entry");
  // history addresses: 1 ≤ hoff ≤ T·Nx, so that (k+T)·Nx − hoff stays inside the T zero slots in front at k = 1
  for (int32_t h : F.hoff) EXPECT(h >= 1 && h <= T * P.Nx, "FIR hoff range");
  // orphans and the row-oriented plant
  std::vector<int32_t> orphans;
  for (int64_t j = 0; j < P.Nu; ++j) if (P.B2.cp[j + 1] == P.B2.cp[j]) orphans.push_back((int32_t)j);
  EXPECT(F.orphan == orphans, "orphan list == empty B2 columns");
  csr_equals_csc(F.A, P.A, base); csr_equals_csc(F.B1, P.B1, base); csr_equals_csc(F.B2, P.B2, base);
}

// random masks that no recipe produced: slice `empty_x` of Sx and `empty_u` of Su hold nothing, one entry of Sx[1] (when there
// is one) and one of Su[0] are stored false
Masks random_masks(int64_t Nx, int64_t Nu, int64_t T, int base, unsigned seed, int64_t empty_x, int64_t empty_u) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  Masks M; M.x.resize(T); M.u.resize(T);
  auto fill = [&](Csc& m, int64_t nr, double density) {
    m.nr = nr; m.nc = Nx; m.cp.assign(Nx + 1, base);
    for (int64_t c = 0; c < Nx; ++c) {
      for (int64_t r = 0; r < nr; ++r) if (u(g) < density) m.ri.push_back(r + base);
      m.cp[c + 1] = (int64_t)m.ri.size() + base;
    }
  };
  for (int64_t t = 0; t < T; ++t) {
    fill(M.x[t], Nx, t == empty_x ? 0.0 : t == 0 ? 0.1 : 0.35);
    fill(M.u[t], Nu, t == empty_u ? 0.0 : 0.4);
  }
  if (T > 1 && M.x[1].ri.size() > 2) { M.x[1].b.assign(M.x[1].ri.size(), 1); M.x[1].b[2] = 0; }
  if (M.u[0].ri.size() > 1) { M.u[0].b.assign(M.u[0].ri.size(), 1); M.u[0].b.back() = 0; }
  for (int64_t t = 0; t < T; ++t) { M.bx.push_back(M.x[t].boolean()); M.bu.push_back(M.u[t].boolean()); }
  return M;
}

// the closed-loop operator at its small edges: T = 1 (no β entries), Nu = 0, an empty slice next to stored-false entries,
// an actuator without a state
void exercise_fir_edges(int base) {
  Plant P = random_plant(11, base, 5u);                                  // Nu = 5
  check_fir(P, random_masks(P.Nx, P.Nu, 1, base, 21u, -1, -1), 1, base);
  check_fir(P, random_masks(P.Nx, P.Nu, 5, base, 22u, 2, 3), 5, base);
  {                                                                      // actuator 1 drives nothing: an empty B2 column
    std::vector<std::vector<double>> B2(P.Nx, std::vector<double>(P.Nu, 0.0));
    for (int64_t j = 0; j < P.Nu; ++j) if (j != 1) { B2[2 * j][j] = 1.0; if (j == 3) B2[9][j] = -0.5; }
    Plant Q = P; Q.B2 = from_dense(B2, P.Nx, P.Nu, base);
    check_fir(Q, random_masks(Q.Nx, Q.Nu, 4, base, 23u, -1, 0), 4, base);
  }
  Plant Z = P; Z.Nu = 0; Z.B2 = from_dense(std::vector<std::vector<double>>(P.Nx), P.Nx, 0, base);
  check_fir(Z, random_masks(Z.Nx, 0, 3, base, 24u, -1, -1), 3, base);
  std::printf("fir_edges base=%d: done\n", base);
}

void exercise(const Plant& P, int64_t d, int64_t T, int base, bool irregular, const char* name) {
  Masks M = make_masks(P, d, T, 1.5, base);
  if (irregular) {                                    // a stored-false entry: forces the explicit tables (no compact layout)
    Csc& m = M.x[T - 1];
    m.b.assign(m.ri.size(), 1);
    if (m.b.size() > 3) m.b[3] = 0;
    M.bx[T - 1] = m.boolean();
  }
  sls_dims dims{P.Nx, P.Nu, P.Nx + P.Nu, P.Nx, T, base, 0};
  sls_csc_f64 A = P.A.f64(), B1 = P.B1.f64(), B2 = P.B2.f64();
  sls_plant plant{&A, &B1, &B2, nullptr, nullptr, nullptr};
  std::string msg;
  // caller groups: pairs of neighbours, a singleton, a triple
  std::vector<int64_t> gptr{0}, gcols;
  for (int64_t c = 0; c + 1 < P.Nx; c += 5) {
    gcols.push_back(c + base); if (c % 10 == 0) gcols.push_back(c + 1 + base);
    if (c % 15 == 0 && c + 2 < P.Nx) gcols.push_back(c + 2 + base);
    gptr.push_back((int64_t)gcols.size());
  }
  const int64_t ng = (int64_t)gptr.size() - 1;
  for (int variant = 0; variant < 2; ++variant) {
    sls::Inputs in{&dims, &plant, M.bx.data(), M.bu.data(), variant ? ng : 0, variant ? gptr.data() : nullptr, variant ? gcols.data() : nullptr};
    int rc = sls::validate_inputs(in, msg);
    EXPECT(rc == 0, "validate_inputs");
    if (rc) { std::fprintf(stderr, "  %s: %s\n", name, msg.c_str()); return; }
    const int64_t n_groups = variant ? ng : P.Nx;
    std::vector<double> cost;
    EXPECT(sls::group_costs(in, cost, msg) == 0 && (int64_t)cost.size() == n_groups, "group_costs");
    for (int packed = 0; packed < 2; ++packed)
      for (int compact = 0; compact < 2; ++compact) {
        const int64_t cuts[4] = {0, n_groups / 3, n_groups / 3, n_groups};      // an empty shard in the middle
        int64_t total_packed = 0, nvals = -1;
        for (int s = 0; s < 3; ++s) {
          sls::Symbolic S; S.want_packed = packed; S.compact = compact && !packed;
          rc = sls::build_symbolic(in, cuts[s], cuts[s + 1], S, msg);
          if (rc == SLS_EUNSUPPORTED) continue;                                  // e.g. a coupled group beyond the kernels' limits
          EXPECT(rc == 0, "build_symbolic");
          if (rc) { std::fprintf(stderr, "  %s: %s\n", name, msg.c_str()); continue; }
          total_packed += S.n_packed;
          check_routing(S);
          EXPECT(nvals < 0 || nvals == S.n_values, "n_values differs between shards");
          nvals = S.n_values;
          if (packed) {
            EXPECT((int64_t)S.packed_to_final.size() == S.n_packed, "packed_to_final length");
            for (int64_t k = 0; k < S.n_packed; ++k) EXPECT(S.packed_to_final[k] >= 0 && S.packed_to_final[k] < S.n_values, "packed_to_final range");
          }
          if (!S.compact)
            for (size_t k = 0; k < S.dest_pool.size(); ++k) EXPECT(S.dest_pool[k] >= -1 && S.dest_pool[k] < S.n_values, "dest range");
        }
        (void)total_packed;
      }
  }
  // inputs of the device passes
  std::vector<int32_t> kx, ku, a_cp, a_ri, b_rp, b_ci, sx_cp, sx_ri, su_cp, su_ri;
  int kmax = 0;
  EXPECT(sls::mask_recipe_inputs(&dims, &A, &B2, d, 1.5, kx, ku, kmax, a_cp, a_ri, b_rp, b_ci, msg) == 0, "mask_recipe_inputs");
  EXPECT(sls::index_set_inputs(&dims, &A, &M.bx[T - 1], &M.bu[T - 1], a_cp, a_ri, sx_cp, sx_ri, su_cp, su_ri, msg) == 0, "index_set_inputs");
  // closed-loop operator
  check_fir(P, M, T, base);
  // malformed inputs must be refused, not read out of bounds
  {
    Csc bad = P.A; if (!bad.ri.empty()) bad.ri[0] = P.Nx + 5 + base;             // row out of range
    sls_csc_f64 Ab = bad.f64(); sls_plant pb{&Ab, &B1, &B2, nullptr, nullptr, nullptr};
    sls::Inputs in{&dims, &pb, M.bx.data(), M.bu.data(), 0, nullptr, nullptr};
    EXPECT(sls::validate_inputs(in, msg) != 0, "row index out of range accepted");
    Csc bad2 = P.A; bad2.cp[P.Nx] = (int64_t)bad2.ri.size() + base + 3;           // colptr past the arrays: caught by monotone/nnz checks?
    bad2.cp[P.Nx] = bad2.cp[P.Nx - 1] - 1;                                        // non-monotone
    sls_csc_f64 Ab2 = bad2.f64(); sls_plant pb2{&Ab2, &B1, &B2, nullptr, nullptr, nullptr};
    sls::Inputs in2{&dims, &pb2, M.bx.data(), M.bu.data(), 0, nullptr, nullptr};
    EXPECT(sls::validate_inputs(in2, msg) != 0, "non-monotone colptr accepted");
    std::vector<int64_t> gp{0, 2}, gc{(int64_t)base, (int64_t)base};             // a column twice in a group
    sls::Inputs in3{&dims, &plant, M.bx.data(), M.bu.data(), 1, gp.data(), gc.data()};
    EXPECT(sls::validate_inputs(in3, msg) != 0, "duplicate column accepted");
    std::vector<int64_t> gc2{(int64_t)(P.Nx + base), (int64_t)(P.Nx + 1 + base)};   // columns out of range
    sls::Inputs in4{&dims, &plant, M.bx.data(), M.bu.data(), 1, gp.data(), gc2.data()};
    EXPECT(sls::validate_inputs(in4, msg) != 0, "column out of range accepted");
  }
  std::printf("%s base=%d irregular=%d: done\n", name, base, (int)irregular);
}


// ---- the plants of the device-pass edge cases (tests/symbolic_cases.py), restated: hub, long-range chain, dense, holes ----
// built by column (no dense image: the long-range chain has 4200 states); stored zeros are kept as stored entries
Csc from_columns(const std::vector<std::vector<std::pair<int64_t, double>>>& cols, int64_t nr, int base) {
  Csc m; m.nr = nr; m.nc = (int64_t)cols.size(); m.cp.assign(cols.size() + 1, base);
  for (size_t c = 0; c < cols.size(); ++c) {
    std::vector<std::pair<int64_t, double>> col = cols[c];
    std::sort(col.begin(), col.end());
    for (auto& e : col) { m.ri.push_back(e.first + base); m.v.push_back(e.second); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}
Csc identity(int64_t n, int base) {
  std::vector<std::vector<std::pair<int64_t, double>>> cols((size_t)n);
  for (int64_t i = 0; i < n; ++i) cols[(size_t)i].push_back({i, 1.0});
  return from_columns(cols, n, base);
}
std::vector<std::vector<std::pair<int64_t, double>>> chain_columns(int64_t Nx) {
  std::vector<std::vector<std::pair<int64_t, double>>> cols((size_t)Nx);
  for (int64_t i = 0; i < Nx; ++i) {
    cols[(size_t)i].push_back({i, 1.0});
    if (i + 1 < Nx) { cols[(size_t)i].push_back({i + 1, -0.2}); cols[(size_t)i + 1].push_back({i, 0.2}); }
  }
  return cols;
}
// unit diagonal, state 0 feeds states 1…m: a level of m + 1 states
Plant hub_plant(int64_t Nx, int64_t m, int base) {
  std::vector<std::vector<std::pair<int64_t, double>>> cols((size_t)Nx);
  for (int64_t i = 0; i < Nx; ++i) cols[(size_t)i].push_back({i, 1.0});
  for (int64_t j = 1; j <= m; ++j) cols[0].push_back({j, 0.3});
  return Plant{Nx, Nx, from_columns(cols, Nx, base), identity(Nx, base), identity(Nx, base)};
}
// chain with edges 5→2100, 5→4190, 2060→3, 4199→0; an actuator on every third state
Plant far_plant(int base) {
  const int64_t Nx = 4200, Nu = Nx / 3;
  auto cols = chain_columns(Nx);
  cols[5].push_back({2100, 0.15}); cols[5].push_back({4190, 0.15}); cols[2060].push_back({3, 0.15}); cols[4199].push_back({0, 0.15});
  std::vector<std::vector<std::pair<int64_t, double>>> b((size_t)Nu);
  for (int64_t j = 0; j < Nu; ++j) b[(size_t)j].push_back({3 * j, 1.0});
  return Plant{Nx, Nu, from_columns(cols, Nx, base), identity(Nx, base), from_columns(b, Nx, base)};
}
Plant dense_plant(int64_t Nx, int base) {
  std::vector<std::vector<std::pair<int64_t, double>>> cols((size_t)Nx), b;
  for (int64_t c = 0; c < Nx; ++c) for (int64_t r = 0; r < Nx; ++r) cols[(size_t)c].push_back({r, 1.0});
  for (int64_t j = 0; j < Nx; j += 2) b.push_back({{j, 1.0}});
  return Plant{Nx, (int64_t)b.size(), from_columns(cols, Nx, base), identity(Nx, base), from_columns(b, Nx, base)};
}
// stored zeros in A and B2; column 7 of A holds stored zeros only (empty level 1); states 3, 4, 10 drive no actuator; Nu = 0 variant
Plant holes_plant(int base, bool no_inputs) {
  const int64_t Nx = 14;
  auto cols = chain_columns(Nx);
  cols[2].push_back({0, 0.5}); cols[12].push_back({9, 0.5});
  for (auto& e : cols[7]) e.second = 0.0;
  for (auto& e : cols[2]) if (e.first == 1) e.second = 0.0;
  for (auto& e : cols[11]) if (e.first == 12) e.second = 0.0;
  std::vector<std::vector<std::pair<int64_t, double>>> b = {{{0, 1.0}, {1, 1.0}}, {{2, 1.0}, {4, 0.0}}, {{5, 1.0}, {6, 1.0}, {7, 1.0}}, {{8, 1.0}, {9, 1.0}}, {{11, 1.0}, {12, 1.0}, {13, 1.0}}};
  if (no_inputs) b.clear();
  return Plant{Nx, (int64_t)b.size(), from_columns(cols, Nx, base), identity(Nx, base), from_columns(b, Nx, base)};
}

// mask recipe and the inputs of the two device passes on such a plant: every mask a valid CSC pattern (pointers monotone,
// rows ascending and in range), 𝓢x[0] = I, the patterns handed to the device by value (A) and structurally (masks)
void exercise_device_inputs(const Plant& P, int64_t d, int64_t T, double alpha, int base, int64_t want_level, const char* name) {
  Masks M = make_masks(P, d, T, alpha, base);
  int64_t biggest = 0;
  for (int part = 0; part < 2; ++part)
    for (int64_t t = 0; t < T; ++t) {
      const Csc& m = part ? M.u[t] : M.x[t];
      const int64_t nr = part ? P.Nu : P.Nx;
      EXPECT(m.cp[0] == base && m.cp[P.Nx] == (int64_t)m.ri.size() + base, "mask pointer ends");
      for (int64_t c = 0; c < P.Nx; ++c) {
        EXPECT(m.cp[c] <= m.cp[c + 1], "mask pointers monotone");
        biggest = std::max(biggest, m.cp[c + 1] - m.cp[c]);
        for (int64_t k = m.cp[c] - base; k < m.cp[c + 1] - base; ++k) {
          EXPECT(m.ri[k] - base >= 0 && m.ri[k] - base < nr, "mask row in range");
          EXPECT(k == m.cp[c] - base || m.ri[k - 1] < m.ri[k], "mask rows ascending");
        }
      }
    }
  EXPECT((int64_t)M.x[0].ri.size() == P.Nx, "Sx[0] is the identity");
  EXPECT(want_level < 0 || biggest == want_level, "largest mask column");
  sls_dims dims{P.Nx, P.Nu, P.Nx + P.Nu, P.Nx, T, base, 0};
  sls_csc_f64 A = P.A.f64(), B2 = P.B2.f64();
  std::string msg;
  std::vector<int32_t> kx, ku, a_cp, a_ri, b_rp, b_ci, sx_cp, sx_ri, su_cp, su_ri;
  int kmax = 0;
  EXPECT(sls::mask_recipe_inputs(&dims, &A, &B2, d, alpha, kx, ku, kmax, a_cp, a_ri, b_rp, b_ci, msg) == 0, "mask_recipe_inputs");
  int64_t nzA = 0, nzB = 0;
  for (double v : P.A.v) nzA += v != 0.0;
  for (double v : P.B2.v) nzB += v != 0.0;
  EXPECT((int64_t)a_cp.size() == P.Nx + 1 && a_cp.back() == nzA && (int64_t)a_ri.size() == nzA, "A pattern by value");
  EXPECT((int64_t)b_rp.size() == P.Nx + 1 && b_rp.back() == nzB && (int64_t)b_ci.size() == nzB, "B2 row pattern by value");
  for (int32_t r : a_ri) EXPECT(r >= 0 && r < P.Nx, "A row in range");
  for (int32_t j : b_ci) EXPECT(j >= 0 && j < P.Nu, "B2 column in range");
  EXPECT((int64_t)kx.size() == T && (int64_t)ku.size() == T && kmax <= d + 1, "level schedule");
  // last masks with stored-false entries: they still count
  Csc& lx = M.x[T - 1]; Csc& lu = M.u[T - 1];
  lx.b.assign(lx.ri.size(), 1); lu.b.assign(lu.ri.size(), 1);
  for (size_t k = 0; k < lx.b.size(); k += 3) lx.b[k] = 0;
  for (size_t k = 0; k < lu.b.size(); k += 4) lu.b[k] = 0;
  sls_csc_bool bx = lx.boolean(), bu = lu.boolean();
  EXPECT(sls::index_set_inputs(&dims, &A, &bx, &bu, a_cp, a_ri, sx_cp, sx_ri, su_cp, su_ri, msg) == 0, "index_set_inputs");
  EXPECT(sx_ri.size() == lx.ri.size() && su_ri.size() == lu.ri.size() && (int64_t)a_ri.size() == nzA, "index-set inputs: masks structural, A by value");
  EXPECT((int64_t)sx_cp.size() == P.Nx + 1 && (int64_t)su_cp.size() == P.Nx + 1, "index-set input pointers");
  std::printf("%s base=%d: largest mask column %lld: done\n", name, base, (long long)biggest);
}

// ---- LDS list plans of the device passes (csrc/sls_symbolic_device.h) ----
// cap_limit against the numbers tests/test_symbolic_cases_host.py derives from the reference; the launch of a capacity at 1, 8 and
// 256 CUs; the bitmap refusal on both sides of 96 KiB.
void check_list_plans() {
  using namespace sls;
  EXPECT(kMaxLds == 160 * 1024 && kBitmapLimit == 96 * 1024, "LDS limits");
  EXPECT(mask_list_plan(1100, 1100).cap_limit == 1100 && mask_list_plan(1100, 1100).cap0 == kMaskCap0, "hub1024: mask lists");
  EXPECT(mask_list_plan(40, 1300).cap_limit == 1300 && index_list_plan(40, 1300).cap_limit == 1300, "hub_wideB: the actuator list sets cap_limit");
  EXPECT(mask_list_plan(40, 20).cap_limit == 40 && index_list_plan(40, 20).cap_limit == 40, "dense40: cap_limit = Nx");
  EXPECT(mask_list_plan(40, 20).cap0 == 40 && index_list_plan(40, 20).cap0 == 40, "dense40: first capacity = cap_limit");
  EXPECT(mask_list_plan(14000, 14000).cap_limit == (kMaxLds - 2 * 438 * 4) / 12, "too_big_mask: what LDS holds");
  // cap_limit_tables of tests/symbolic_cases.py restated with literals: an independent twin of the header's arithmetic (the Python
  // value itself is held against the reference by tests/test_symbolic_cases_host.py)
  auto tables_limit = [](int64_t Nx, int64_t Nu, int64_t T) {
    const int64_t bitmap = ((Nx + 31) / 32 + (std::max<int64_t>(Nu, 1) + 31) / 32) * 4;
    return (int)((160 * 1024 - (bitmap + 2 * 68 * 4 + 4 * T * 4)) / 8);
  };
  EXPECT(tables_list_plan(4200, 1400, 4).cap_limit == tables_limit(4200, 1400, 4), "far4200: tables pools");
  EXPECT(tables_list_plan(23, 9, 130).cap_limit == tables_limit(23, 9, 130), "T = 130: tables pools");
  EXPECT(tables_list_plan(335, 335, 3).cap_limit == 20395, "fits_pool: 20395 entries are what 160 KiB hold");
  EXPECT(tables_list_plan(4200, 1400, 4).cap0 == kTablesCap0 && tables_list_plan(4200, 1400, 4).entry_bytes == 8, "tables: first capacity");
  const ListPlan plans[3] = {mask_list_plan(4200, 1400), index_list_plan(4200, 1400), tables_list_plan(4200, 1400, 4)};
  for (const ListPlan& p : plans)
    for (int ncu : {1, 8, 256})
      for (int64_t Nx : {(int64_t)1, (int64_t)7, (int64_t)4200})
        for (int cap = p.cap0; cap <= p.cap_limit; cap = cap < p.cap_limit ? std::min(p.cap_limit, 2 * cap) : cap + 1) {
          const ListLaunch l = list_launch(p, cap, ncu, Nx);
          EXPECT(l.cap == cap && l.lds == (size_t)(p.fixed_bytes + (int64_t)p.entry_bytes * cap) && l.lds <= (size_t)kMaxLds, "list launch: LDS");
          EXPECT(l.per_cu >= 1 && l.per_cu <= 8 && (l.per_cu == 8 || (size_t)(l.per_cu + 1) * l.lds > (size_t)kMaxLds), "list launch: waves per CU");
          EXPECT(l.per_cu == 1 || (size_t)l.per_cu * l.lds <= (size_t)kMaxLds, "list launch: the waves of a CU fit its LDS");
          EXPECT(l.grid == (int)std::min<int64_t>(Nx, (int64_t)ncu * l.per_cu), "list launch: grid = min(Nx, ncu * per_cu)");
        }
  // bitmap of 96 KiB exactly: 24576 words, e.g. 24575 state words + 1 input word
  const int64_t Nx_fit = 24575 * 32, Nx_over = Nx_fit + 1;
  EXPECT(mask_list_plan(Nx_fit, 1).fixed_bytes == 96 * 1024 && mask_list_plan(Nx_fit, 1).fits() && index_list_plan(Nx_fit, 0).fits(), "bitmap of 96 KiB accepted");
  EXPECT(!mask_list_plan(Nx_over, 1).fits() && !index_list_plan(Nx_over, 1).fits(), "bitmap over 96 KiB refused");
  EXPECT(tables_list_plan(Nx_fit, 1, 1).fixed_bytes == 96 * 1024 + 2 * 68 * 4 + 16 && !tables_list_plan(Nx_fit, 1, 1).fits(), "tables: the fixed words count");
  EXPECT(tables_list_plan(Nx_fit - 32 * 140, 1, 1).fits() && !tables_list_plan(Nx_fit - 32 * 139, 1, 1).fits(), "tables: both sides of 96 KiB");
  std::printf("list plans: done\n");
}

// ---- host arithmetic of the device-resident symbolic route (localized_layout) against the host pass ----
// build_symbolic in the compact, mask-order layout on the recipe's own masks gives what column_tables_kernel's count pass
// reports (col_info from its SubDescs, level totals from the masks' sizes); localized_layout must then place everything where
// build_symbolic did.
int levels_beyond_kmax = 0, levels_within_kmax = 0;      // cases with kx[T−1] + 1 > kmax (the index sets need a level no mask uses) / ≤ kmax

void check_localized_layout(const Plant& P, int64_t d, int64_t T, double alpha, int base, const char* name) {
  Masks M = make_masks(P, d, T, alpha, base);
  sls_dims dims{P.Nx, P.Nu, P.Nx + P.Nu, P.Nx, T, base, 0};
  sls_csc_f64 A = P.A.f64(), B1 = P.B1.f64(), B2 = P.B2.f64();
  sls_plant plant{&A, &B1, &B2, nullptr, nullptr, nullptr};
  std::string msg;
  sls::Inputs in{&dims, &plant, M.bx.data(), M.bu.data(), 0, nullptr, nullptr};
  sls::Symbolic H; H.want_packed = false; H.compact = true;
  int rc = sls::build_symbolic(in, 0, P.Nx, H, msg);
  EXPECT(rc == 0 && H.compact, "host pass, compact mask-order layout");
  if (rc || !H.compact) { std::fprintf(stderr, "  %s: %s\n", name, msg.c_str()); return; }
  sls::Symbolic Hp; Hp.want_packed = true;                      // the packed pass of the same inputs: n_packed, pk_base
  EXPECT(sls::build_symbolic(in, 0, P.Nx, Hp, msg) == 0, "host pass, packed layout");
  sls::Symbolic S;
  sls::LocalizedHost L;
  rc = sls::localized_prepare(&dims, &plant, d, alpha, S, L, msg);
  EXPECT(rc == 0, "localized_prepare");
  if (rc) return;
  ++(L.kx[T - 1] + 1 > L.kmax ? levels_beyond_kmax : levels_within_kmax);
  // the count pass's outputs
  const int K1 = L.kmax + 1;
  std::vector<int64_t> totx((size_t)K1, -1), totu((size_t)K1, -1);
  for (int64_t t = 0; t < T; ++t) { totx[(size_t)L.kx[t]] = (int64_t)M.x[t].ri.size(); totu[(size_t)L.ku[t]] = (int64_t)M.u[t].ri.size(); }
  std::vector<int32_t> info((size_t)P.Nx * 6);
  for (int64_t c = 0; c < P.Nx; ++c) {
    const sls::SubDesc& sd = H.subs[(size_t)c];
    const int32_t ci[6] = {sd.n, sd.m, sd.pos, sd.nnzA, sd.nnzB, (int32_t)(Hp.pk_base[(size_t)c + 1] - Hp.pk_base[(size_t)c])};
    std::copy(ci, ci + 6, info.begin() + 6 * c);
  }
  sls::LocalizedLayout lay;
  rc = sls::localized_layout(&dims, &B1, L, totx.data(), totu.data(), info.data(), S, lay, msg);
  EXPECT(rc == 0, "localized_layout");
  if (rc) return;
  EXPECT(S.off_x == H.off_x && S.off_u == H.off_u && S.n_values == H.n_values, "value-array offsets");
  EXPECT(S.n_total_subproblems == H.n_total_subproblems && S.first_sub_index == H.first_sub_index, "subproblem numbering");
  EXPECT(S.subs.size() == H.subs.size() && S.sub_col.size() == H.sub_col.size(), "one subproblem per column");
  if (S.subs.size() != H.subs.size()) return;
  for (size_t c = 0; c < H.subs.size(); ++c) {
    const sls::SubDesc &a = S.subs[c], &b = H.subs[c];
    EXPECT(a.n == b.n && a.m == b.m && a.pos == b.pos && a.nnzA == b.nnzA && a.nnzB == b.nnzB && a.cls == b.cls, "SubDesc sizes, position, class");
    EXPECT(a.off_sx == b.off_sx && a.off_su == b.off_su && a.off_mask == b.off_mask && a.off_dest == b.off_dest, "SubDesc offsets");
    EXPECT(a.out_index == b.out_index && a.has_w == b.has_w && a.off_w == b.off_w && S.sub_col[c] == H.sub_col[c], "SubDesc output index, weights, column");
    EXPECT(lay.cw_off[c] == H.coff[c] && lay.idx_off[c] == b.off_sx, "first mask word / first index of the column");
  }
  EXPECT(lay.idx_total == (int64_t)H.idx_pool.size() && lay.cw_total == (int64_t)H.cmask.size(), "pool totals");
  EXPECT(S.md_total == H.md_total && S.max_n == H.max_n && S.max_m == H.max_m && S.max_nm == H.max_nm, "md_total, max sizes");
  EXPECT(S.max_nnzA == H.max_nnzA && S.max_nnzB == H.max_nnzB, "max nnz");
  EXPECT(S.n_packed == Hp.n_packed && S.n_packed == H.n_packed && S.pk_base == Hp.pk_base, "packed bases");
  EXPECT(S.obj_pool.size() == H.obj_pool.size() && std::equal(S.obj_pool.begin(), S.obj_pool.end(), H.obj_pool.begin()), "objective records");
  // sums of positive terms taken in another order (the host pass sums per thread range): Nx roundings at most
  const double tol = (double)P.Nx * 0x1p-52;
  EXPECT(std::abs(S.flops_alg - H.flops_alg) <= tol * H.flops_alg && std::abs(S.bytes_alg - H.bytes_alg) <= tol * H.bytes_alg, "cost model");
  // the order is the plan's launch order: a permutation, ñx non-increasing, stable among equal ñx — and then the host pass's
  std::vector<int32_t> seen(S.order);
  std::sort(seen.begin(), seen.end());
  bool perm = (int64_t)seen.size() == P.Nx;
  for (size_t q = 0; perm && q < seen.size(); ++q) perm = seen[q] == (int32_t)q;
  EXPECT(perm, "order is a permutation of the columns");
  for (size_t q = 0; perm && q + 1 < S.order.size(); ++q) {
    const int32_t a = S.order[q], b = S.order[q + 1];
    EXPECT(S.subs[(size_t)a].n > S.subs[(size_t)b].n || (S.subs[(size_t)a].n == S.subs[(size_t)b].n && a < b), "order: descending n, stable");
  }
  EXPECT(S.order == H.order, "order equals the host pass's");
  // fabricated totals past 2^31 values: refused, nothing else asked of S
  std::vector<int64_t> big((size_t)K1, (int64_t)1 << 31);
  sls::Symbolic S2; sls::LocalizedHost L2; sls::LocalizedLayout lay2;
  EXPECT(sls::localized_prepare(&dims, &plant, d, alpha, S2, L2, msg) == 0, "localized_prepare");
  EXPECT(sls::localized_layout(&dims, &B1, L2, big.data(), totu.data(), info.data(), S2, lay2, msg) == SLS_EUNSUPPORTED && msg.find("2^31") != std::string::npos,
         "more than 2^31 values accepted");
  std::printf("localized layout %s base=%d T=%lld d=%lld alpha=%g (kx[T-1]+1 %s kmax): done\n", name, base, (long long)T, (long long)d, alpha,
              L.kx[T - 1] + 1 > L.kmax ? ">" : "<=");
}

// ---- host arithmetic of plan construction (csrc/sls_arena.h, csrc/sls_routing.h) ----
// The arena's ranked layout, against offsets worked out by hand from the rule: tables of at most 256 KiB first (staged), larger
// tables next, then empty tables and buffers, declaration order within each; every block takes max(bytes, 16) rounded up to 256.
void check_arena_layout() {
  using sls::Arena;
  const std::vector<char> t100(100), t300k(300 << 10), tempty, t4k(4 << 10);
  const char *p100, *p300k, *pempty, *p4k;
  char *b64, *b2m, *b8;
  auto same = [](const std::vector<size_t>& got, std::initializer_list<size_t> want) { return got == std::vector<size_t>(want); };
  {
    Arena a;
    a.table(t100, &p100); a.table(t300k, &p300k); a.table(tempty, &pempty);
    a.buffer(64, &b64); a.buffer((size_t)2 << 20, &b2m); a.buffer(8, &b8);
    a.table(t4k, &p4k);
    const Arena::Layout L = a.lay_out((size_t)256 << 10);
    // 100 B at 0, 4 KiB at 256 → staged prefix 4352; 300 KiB (1200 · 256) at 4352 → 311552; the empty table's 256 B there; 64 B at
    // 311808; 2 MiB at 312064 → 2409216; 8 B there; 2409472 in all
    EXPECT(same(L.off, {0, 4352, 311552, 311808, 312064, 2409216, 256}), "arena: offsets of the mixed list");
    EXPECT(L.total == 2409472 && a.bytes() == 2409472 && L.staged_end == 4352, "arena: total and staged prefix");
    EXPECT(L.clear_begin == 311808 && L.clear_end == 2409224 && !L.clear_hull, "arena: the 2 MiB buffer splits the clear in two");
    // every table staged (the localized route): 300 KiB joins the prefix, in declaration order
    const Arena::Layout A = a.lay_out();
    EXPECT(same(A.off, {0, 256, 311552, 311808, 312064, 2409216, 307456}) && A.staged_end == 311552 && A.total == 2409472, "arena: everything staged");
  }
  {
    Arena a;
    a.table(t100, &p100); a.table(t300k, &p300k); a.table(tempty, &pempty);
    a.buffer(64, &b64); a.buffer(8, &b8);
    a.table(t4k, &p4k);
    const Arena::Layout L = a.lay_out((size_t)256 << 10);
    EXPECT(same(L.off, {0, 4352, 311552, 311808, 312064, 256}) && L.total == 312320 && L.staged_end == 4352, "arena: offsets without the large buffer");
    EXPECT(L.clear_begin == 311808 && L.clear_end == 312072 && L.clear_hull, "arena: one clear over the hull");
  }
  {
    Arena a;                                      // tables only: nothing to clear
    a.table(t100, &p100);
    const Arena::Layout L = a.lay_out();
    EXPECT(L.clear_begin == L.clear_end && L.clear_hull && L.total == 256 && L.staged_end == 256, "arena: no buffer, no clear");
    EXPECT(Arena().lay_out().total == 0 && Arena().lay_out().staged_end == 0, "arena: empty");
  }
  std::printf("arena layout: done\n");
}

// the scratch workspace against the formula plan construction used before it was a function, written out
void check_scratch_layout() {
  const size_t cases[4][3] = {{0, 0, 0}, {33, 0, 0}, {1000, 77, 0}, {1000, 77, 4096}};
  for (const auto& c : cases) {
    const size_t fac = c[0], vec = c[1], big = c[2];
    const sls::ScratchLayout L = sls::scratch_layout(fac, vec, big);
    EXPECT(L.bytes == (std::max<size_t>(fac, 1) + vec + 32) * sizeof(double) + 512 + big + 256, "scratch: bytes");
    EXPECT(L.vec_off == ((fac + 31) / 32) * 32, "scratch: vector workspace behind the factor doubles rounded to 32");
    EXPECT(L.big_off == ((((fac + 31) / 32) * 32 + vec + 32) * sizeof(double) + 255) / 256 * 256, "scratch: carve buffers");
    EXPECT((L.vec_off + vec) * sizeof(double) <= L.bytes && L.big_off + big <= L.bytes && (vec == 0 || L.vec_off >= fac), "scratch: regions inside");
  }
  const sls::ScratchLayout L = sls::scratch_layout(1000, 77, 4096);
  EXPECT(L.bytes == 13736 && L.vec_off == 1024 && L.big_off == 9216, "scratch: (1000, 77, 4096) by hand");
  std::printf("scratch layout: done\n");
}

const char* const kSolverKnobs[] = {"SLS_SON_MAXIT", "SLS_SON_TOL", "SLS_SON_ANDERSON", "SLS_SON_AA_START", "SLS_DELTA_FIRST", "SLS_STAG", "SLS_MAX_ITERS",
                                    "SLS_MAX_ITERS_SLOW", "SLS_TOL", "SLS_DELTA_REL", "SLS_PHASE_TIMERS", "SLS_KNOCK_OUT", "SLS_T4_PRESTATIC"};

bool solver_defaults(const sls::SolverKnobs& k) {
  return k.delta_rel == 1e-12 && k.tol == 1e-12 && k.tol_ok == 1e-9 && k.max_iters == 8 && k.stag == 0.5 && k.son_maxit == 4000 && k.son_tol == 1e-9 &&
         k.son_anderson == 1 && k.son_aa_start == 20 && k.delta_first == 1e-15 && k.max_iters_slow == 48 && k.dbg_level == 0 && k.knock_out == 0 &&
         k.t4_prestatic;
}

// what the knobs write into the kernel parameters, and nothing else of them
void check_apply(const sls::SolverKnobs& k) {
  sls::KernelParams kp;
  std::memset(&kp, 0x5a, sizeof kp);
  sls::KernelParams before = kp;
  k.apply(kp);
  EXPECT(kp.delta_rel == k.delta_rel && kp.tol == k.tol && kp.tol_ok == k.tol_ok && kp.max_iters == k.max_iters && kp.stag == k.stag, "apply: 𝓗₂ parameters");
  EXPECT(kp.son_maxit == k.son_maxit && kp.son_tol == k.son_tol && kp.son_anderson == k.son_anderson && kp.son_aa_start == k.son_aa_start, "apply: sum-of-norms parameters");
  EXPECT(kp.delta_first == k.delta_first && kp.max_iters_slow == k.max_iters_slow && kp.dbg_level == k.dbg_level && kp.knock_out == k.knock_out, "apply: the rest");
  EXPECT(kp.T == before.T && kp.nsub == before.nsub && kp.objective == before.objective && kp.dbg == before.dbg && kp.out == before.out, "apply: touches nothing else");
}

// lab mode off (SLS_LAB is latched on first use, so this is a process of its own): every knob is set and none is read
int check_solver_defaults() {
  unsetenv("SLS_LAB");
  for (const char* name : kSolverKnobs) setenv(name, "7", 1);
  const sls::SolverKnobs k = sls::SolverKnobs::from_env();
  EXPECT(solver_defaults(k), "solver knobs: defaults outside lab mode");
  check_apply(k);
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_symbolic: defaults clean\n");
  return 0;
}

// lab mode on: nothing set gives the defaults; every knob's parse and clamp
void check_solver_knobs() {
  for (const char* name : kSolverKnobs) unsetenv(name);
  EXPECT(solver_defaults(sls::SolverKnobs::from_env()), "solver knobs: defaults in lab mode");
  auto with = [](std::initializer_list<std::pair<const char*, const char*>> env) {
    for (const char* name : kSolverKnobs) unsetenv(name);
    for (const auto& e : env) setenv(e.first, e.second, 1);
    const sls::SolverKnobs k = sls::SolverKnobs::from_env();
    for (const char* name : kSolverKnobs) unsetenv(name);
    return k;
  };
  sls::SolverKnobs k = with({{"SLS_SON_MAXIT", "123"}, {"SLS_SON_TOL", "1e-6"}, {"SLS_SON_ANDERSON", "0"}, {"SLS_SON_AA_START", "5"}, {"SLS_DELTA_FIRST", "1e-13"},
                            {"SLS_STAG", "0.25"}, {"SLS_MAX_ITERS", "12"}, {"SLS_MAX_ITERS_SLOW", "7"}, {"SLS_TOL", "1e-10"}, {"SLS_DELTA_REL", "1e-11"},
                            {"SLS_PHASE_TIMERS", "2"}, {"SLS_KNOCK_OUT", "3"}, {"SLS_T4_PRESTATIC", "0"}});
  EXPECT(k.son_maxit == 123 && k.son_tol == 1e-6 && k.son_anderson == 0 && k.son_aa_start == 5 && k.delta_first == 1e-13, "solver knobs: parse (1)");
  EXPECT(k.stag == 0.25 && k.max_iters == 12 && k.max_iters_slow == 7 && k.tol == 1e-10 && k.delta_rel == 1e-11 && k.tol_ok == 1e-9, "solver knobs: parse (2)");
  EXPECT(k.dbg_level == 2 && k.knock_out == 3 && !k.t4_prestatic, "solver knobs: parse (3)");
  check_apply(k);
  k = with({{"SLS_MAX_ITERS", "0"}, {"SLS_SON_MAXIT", "-4"}, {"SLS_SON_AA_START", "-3"}, {"SLS_MAX_ITERS_SLOW", "-1"}, {"SLS_DELTA_FIRST", "0"},
            {"SLS_PHASE_TIMERS", "0"}, {"SLS_SON_ANDERSON", "1"}, {"SLS_T4_PRESTATIC", "1"}});
  EXPECT(k.max_iters == 1 && k.son_maxit == 1 && k.son_aa_start == 0 && k.max_iters_slow == 0, "solver knobs: clamps");
  EXPECT(k.delta_first == 0.0 && k.dbg_level == 1 && k.son_anderson == 1 && k.t4_prestatic, "solver knobs: DELTA_FIRST=0, PHASE_TIMERS=0 → level 1");
  k = with({{"SLS_MAX_ITERS_SLOW", "0"}, {"SLS_SON_ANDERSON", "yes"}, {"SLS_PHASE_TIMERS", "x"}});
  EXPECT(k.max_iters_slow == 0 && k.son_anderson == 1 && k.dbg_level == 1 && k.max_iters == 8, "solver knobs: 0 stays 0, anything but '0' is on");
  std::printf("solver knobs: done\n");
}

// the sum-of-norms weights check: diagonal weights (has_w 0 / 1 with D11 = 0) pass; a dense Hessian and a D11 entry are refused
void check_son_weights() {
  const std::string text = "SLS_SOLVE_SUM_OF_NORMS needs a diagonal [C1 D12]'[C1 D12] and D11 = 0";
  auto sub = [](int n, int m, int has_w, int64_t off_w) { sls::SubDesc sd{}; sd.n = n; sd.m = m; sd.has_w = has_w; sd.off_w = off_w; return sd; };
  sls::Symbolic S;
  S.subs.push_back(sub(2, 1, 0, 0));
  S.subs.push_back(sub(2, 1, 1, 0));
  S.w_pool.assign(6, 0.0); S.w_pool[0] = 2.0; S.w_pool[1] = 3.0; S.w_pool[2] = 0.5;     // diagonal, then a zero D11 part
  std::string msg = "untouched";
  EXPECT(sls::check_sum_of_norms_weights(S, msg) == 0 && msg == "untouched", "sum-of-norms weights: diagonal accepted");
  sls::Symbolic D = S;
  D.subs[0].has_w = 2;
  EXPECT(sls::check_sum_of_norms_weights(D, msg) == SLS_EUNSUPPORTED && msg == text, "sum-of-norms weights: dense Hessian refused");
  sls::Symbolic F = S;
  F.w_pool[5] = 1e-300;                                                                 // the last D11 entry of the second column
  msg.clear();
  EXPECT(sls::check_sum_of_norms_weights(F, msg) == SLS_EUNSUPPORTED && msg == text, "sum-of-norms weights: D11 entry refused");
  EXPECT(sls::check_sum_of_norms_weights(sls::Symbolic{}, msg) == 0, "sum-of-norms weights: no subproblem");
  std::printf("sum-of-norms weights: done\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "defaults") == 0) return check_solver_defaults();
  setenv("SLS_LAB", "1", 1);                             // latched by the first knob read: before everything else
  check_solver_knobs();
  check_arena_layout();
  check_scratch_layout();
  check_son_weights();
  check_list_plans();
  for (int base = 0; base < 2; ++base)
    for (int64_t T : {(int64_t)1, (int64_t)4})
      for (int pair = 0; pair < 2; ++pair) {
        // (d, α) = (1, 1.5): at T = 4 ku reaches d + 1 = kmax, kx[T−1] + 1 = kmax;  (3, 0.5): kx[T−1] = ku[T−1] = kmax, so the
        // index sets need level kx[T−1] + 1 > kmax
        const int64_t d = pair ? 3 : 1;
        const double alpha = pair ? 0.5 : 1.5;
        check_localized_layout(chain(5, base, false), d, T, alpha, base, "chain5");
        check_localized_layout(grid(3, base), d, T, alpha, base, "grid3");
        // the route needs a full diagonal of A (else a mask row lies outside its column's index set): random_plant's stored
        // zeros stay off the diagonal here
        Plant R = random_plant(12, base, 3u);
        for (int64_t c = 0; c < R.Nx; ++c)
          for (int64_t k = R.A.cp[c] - base; k < R.A.cp[c + 1] - base; ++k) if (R.A.ri[k] - base == c) R.A.v[k] = 1.0;
        check_localized_layout(R, d, T, alpha, base, "random12");
      }
  EXPECT(levels_beyond_kmax > 0 && levels_within_kmax > 0, "localized layout: both kx[T-1] + 1 > kmax and <= kmax must be covered");
  for (int base = 0; base < 2; ++base) {
    exercise(chain(59, base, false), 9, 29, base, false, "chain59");
    exercise(chain(40, base, true), 4, 10, base, false, "chain40_coupled_B1");
    exercise(chain(30, base, false), 3, 8, base, true, "chain30_irregular");
    exercise(grid(9, base), 2, 6, base, false, "grid9");
    exercise(random_plant(70, base, 11u + base), 2, 7, base, false, "random70");
    exercise_fir_edges(base);
    // the device passes' edge plants (tests/symbolic_cases.py): a level of 1025 states, states 4000 apart in one level, every
    // level full, stored zeros with an empty level, no inputs at all, 62 levels
    exercise_device_inputs(hub_plant(1100, 1024, base), 1, 3, 1.5, base, 1025, "hub1025");
    exercise_device_inputs(far_plant(base), 2, 4, 1.5, base, -1, "far4200");
    exercise_device_inputs(dense_plant(40, base), 2, 3, 1.5, base, 40, "dense40");
    exercise_device_inputs(holes_plant(base, false), 2, 4, 1.5, base, -1, "holes");
    exercise_device_inputs(holes_plant(base, true), 2, 4, 0.5, base, -1, "holes_no_inputs");
    exercise_device_inputs(hub_plant(70, 20, base), 60, 24, 3.0, base, 21, "hub_deep60");
  }
  // worker pool: a pass large enough for several threads (Nx/256 ≥ 2)
  exercise(chain(600, 0, false), 6, 12, 0, false, "chain600");
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_symbolic: clean\n");
  return 0;
}
