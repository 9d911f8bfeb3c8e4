// Host arithmetic of the one-shot calls (csrc/sls_dropin_host.cpp with the input checks of csrc/sls_symbolic.cpp — no HIP in
// either) under AddressSanitizer + UndefinedBehaviorSanitizer: test infrastructure, built and run by
// tests/test_dropin_host.py::test_dropin_host_under_sanitizers with g++ -fsanitize=address,undefined.  Known answers, each worked
// out by hand in the comment beside it, for the layering of overlapping groups, the shard cuts, the refinement selection at its
// thresholds, the block-diagonal composite of a batch and its split back, the unpack of packed shards and the status fold —
// in both index bases wherever a base enters.  Every array has its exact size, so a write past an output is an ASan report.
// Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../systemlevelcontrol.jl_amd/csrc/sls_dropin_host.h"

namespace {

int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++fails; } } while (0)

using I64 = std::vector<int64_t>;
using I32 = std::vector<int32_t>;

// ---------------------------------------------------------------- layers
struct Groups { I64 ptr{0}, cols; void add(int64_t lo, int64_t hi, int base) { for (int64_t c = lo; c <= hi; ++c) cols.push_back(c + base); ptr.push_back((int64_t)cols.size()); } };

void test_layers(int base) {
  const int64_t Nx = 59;
  // the groups of test_overlapping_groups_are_summed_like_the_reference: columns 10..19 twice, 25 three times, 44 twice
  Groups G;
  G.add(0, 19, base); G.add(10, 29, base); G.add(25, 25, base); G.add(25, 25, base); G.add(40, 44, base); G.add(44, 44, base);
  I32 layer_of; int nlayers = 0;
  EXPECT(sls::assign_group_layers(Nx, base, 6, G.ptr.data(), G.cols.data(), layer_of, nlayers) == sls::GroupLayering::Layered, "overlapping list");
  EXPECT((layer_of == I32{0, 1, 2, 3, 0, 1}) && nlayers == 4, "layer_of = [0,1,2,3,0,1], four layers");
  I64 lptr, lcols, lpos;
  sls::layer_group_list(0, layer_of, G.ptr.data(), G.cols.data(), lptr, lcols, lpos);
  I64 want_cols, want_pos;                               // groups 0 and 4: flat positions 0..19 and 20 + 20 + 1 + 1 = 42 .. 46
  for (int64_t c = 0; c < 20; ++c) { want_cols.push_back(c + base); want_pos.push_back(c); }
  for (int64_t c = 40; c < 45; ++c) { want_cols.push_back(c + base); want_pos.push_back(42 + (c - 40)); }
  EXPECT((lptr == I64{0, 20, 25}) && lcols == want_cols && lpos == want_pos, "layer 0 = groups 0 and 4");
  sls::layer_group_list(3, layer_of, G.ptr.data(), G.cols.data(), lptr, lcols, lpos);
  EXPECT((lptr == I64{0, 1}) && (lcols == I64{25 + base}) && (lpos == I64{41}), "layer 3 = the third listing of column 25");

  Groups D;                                              // disjoint, not ascending between groups, first and last column used
  D.add(30, 58, base); D.add(0, 9, base); D.add(10, 10, base);
  EXPECT(sls::assign_group_layers(Nx, base, 3, D.ptr.data(), D.cols.data(), layer_of, nlayers) == sls::GroupLayering::None, "disjoint list");
  EXPECT((layer_of == I32{0, 0, 0}) && nlayers == 1, "disjoint list: one layer");

  // An empty group is a valid group (validate_inputs accepts it) and names no column: it lands in layer 0 and changes nothing
  Groups E;
  E.add(0, 4, base); E.ptr.push_back(E.ptr.back()); E.add(5, 9, base);
  EXPECT(sls::assign_group_layers(Nx, base, 3, E.ptr.data(), E.cols.data(), layer_of, nlayers) == sls::GroupLayering::None, "empty group, disjoint");
  E.add(9, 9, base);
  EXPECT(sls::assign_group_layers(Nx, base, 4, E.ptr.data(), E.cols.data(), layer_of, nlayers) == sls::GroupLayering::Layered, "empty group, overlapping");
  EXPECT((layer_of == I32{0, 0, 0, 1}) && nlayers == 2, "empty group sits in layer 0");
  sls::layer_group_list(0, layer_of, E.ptr.data(), E.cols.data(), lptr, lcols, lpos);
  EXPECT((lptr == I64{0, 5, 5, 10}) && lcols.size() == 10 && lpos.size() == 10, "layer 0 keeps the empty group");

  Groups M;                                              // malformed lists: reported, nothing read or written out of bounds
  M.add(0, 4, base); M.add(3, 6, base);
  M.ptr[2] = 2;                                          // descending group_ptr: [0, 5, 2]
  EXPECT(sls::assign_group_layers(Nx, base, 2, M.ptr.data(), M.cols.data(), layer_of, nlayers) == sls::GroupLayering::Malformed, "descending group_ptr");
  EXPECT(layer_of.size() == 2, "layer_of has one entry per group");
  Groups O1; O1.add(0, 4, base); O1.add(59, 59, base);   // one past the last column
  EXPECT(sls::assign_group_layers(Nx, base, 2, O1.ptr.data(), O1.cols.data(), layer_of, nlayers) == sls::GroupLayering::Malformed, "column Nx");
  Groups O2; O2.add(0, 4, base); O2.add(-1, -1, base);   // one before the first
  EXPECT(sls::assign_group_layers(Nx, base, 2, O2.ptr.data(), O2.cols.data(), layer_of, nlayers) == sls::GroupLayering::Malformed, "column -1");

  sls_stats tot{}, a{}, b{};
  a.n_subproblems = 25; a.n_not_ok = 1; a.n_free = 100; a.n_refined = 2; a.n_values_x = 7; a.n_values_u = 5; a.n_devices = 1; a.max_nx = 9; a.max_nu = 4;
  a.max_iters = 3; a.max_residual = 1e-12; a.flops_alg = 1.5; a.bytes_alg = 2.5; a.t_symbolic_s = 0.25; a.t_upload_s = 0.5; a.t_solve_s = 1.0; a.t_download_s = 2.0;
  b = a; b.n_subproblems = 20; b.n_not_ok = 0; b.max_nx = 7; b.max_nu = 6; b.max_iters = 8; b.max_residual = 1e-10; b.n_refined = 0;
  sls::accumulate_layer_stats(tot, a); sls::accumulate_layer_stats(tot, b);
  EXPECT(tot.n_subproblems == 45 && tot.n_not_ok == 1 && tot.n_free == 200 && tot.n_refined == 2, "layer stats: sums");
  EXPECT(tot.n_values_x == 7 && tot.n_values_u == 5 && tot.n_devices == 1, "layer stats: sizes are those of one layer, not sums");
  EXPECT(tot.max_nx == 9 && tot.max_nu == 6 && tot.max_iters == 8 && tot.max_residual == 1e-10, "layer stats: maxima");
  EXPECT(tot.flops_alg == 3.0 && tot.bytes_alg == 5.0 && tot.t_symbolic_s == 0.5 && tot.t_upload_s == 1.0 && tot.t_solve_s == 2.0 && tot.t_download_s == 4.0,
         "layer stats: work and times add up");
}

// ---------------------------------------------------------------- cuts
I64 cuts_of(const std::vector<double>& cost, int nshards) {
  I64 cuts((size_t)nshards + 1, -7);
  sls::balanced_cuts(cost, nshards, cuts.data());
  return cuts;
}

void test_cuts() {
  EXPECT((cuts_of(std::vector<double>(8, 1.0), 4) == I64{0, 2, 4, 6, 8}), "equal costs divide evenly");
  // [1,1,1,100] in 3: target 34.3 is passed only inside the last group, so the cursor stops at 3 and is pulled back to 2 (two
  // shards still to come); target 68.7 again lands in the last group, pulled back to 3
  EXPECT((cuts_of({1, 1, 1, 100}, 3) == I64{0, 2, 3, 4}), "a dominant last group leaves the later shards one group each");
  // [100,1,1,1] in 3: half of the first group (50) already exceeds target 34.3 — nothing before the first cut; target 68.7 takes it
  EXPECT((cuts_of({100, 1, 1, 1}, 3) == I64{0, 0, 1, 4}), "a dominant first group");
  // two groups, four shards: max_g = 2 − (4 − s) holds the cursor at 0, 0, 1
  EXPECT((cuts_of({1, 1}, 4) == I64{0, 0, 0, 1, 2}), "fewer groups than shards: non-decreasing, ends at ng");
  EXPECT((cuts_of({3, 1, 2}, 1) == I64{0, 3}), "one shard");
  EXPECT((cuts_of({}, 2) == I64{0, 0, 0}), "no groups");
}

// ---------------------------------------------------------------- refinement selection
void test_refinement(int base) {
  const double above_1e11 = std::nextafter(1e-11, 1.0), below_1e6 = std::nextafter(1e-6, 0.0);
  struct Sub { int32_t cls; char tw; int32_t stt, its; double res; };
  const std::vector<Sub> subs = {
      {0, 0, SLS_COL_OK, 3, 1e-9},                 //  0  three passes: no
      {0, 0, SLS_COL_OK, 4, 1e-9},                 //  1  four: yes
      {0, 0, SLS_COL_OK, 4, 1e-11},                //  2  at the residual threshold: no
      {0, 0, SLS_COL_OK, 4, above_1e11},           //  3  just above: yes
      {0, 0, SLS_COL_INFEASIBLE, 3, 1e-6},         //  4  at 1e-6, not on a twisted launch: no
      {0, 0, SLS_COL_INFEASIBLE, 3, below_1e6},    //  5  just below: yes
      {0, 1, SLS_COL_INFEASIBLE, 3, 1e-6},         //  6  at 1e-6 on a twisted launch: yes
      {0, 1, SLS_COL_INFEASIBLE, 2, 1e-7},         //  7  flagged at the second pass: no, whatever else holds
      {0, 0, SLS_COL_INFEASIBLE, 3, 1e-7},         //  8  the same at the third: yes
      {0, 0, SLS_COL_NOTCONV, 1, 1.0},             //  9  yes
      {-1, 1, SLS_COL_NOTCONV, 9, 1e-9},           // 10  solved by the tile kernel already: no
      {0, 0, SLS_COL_OK, 1, 1e-14},                // 11  | a group of two, taken whole
      {0, 0, SLS_COL_NOTCONV, 5, 1e-3},            // 12  | for this member
      {-1, 0, SLS_COL_NOTCONV, 5, 1e-3},           // 13  | a group of two whose only candidate is a tile column:
      {0, 0, SLS_COL_OK, 1, 1e-14},                // 14  | not taken
  };
  I64 gptr, gcols;                                                      // normalised list: 0-based columns 2q + 1
  for (int64_t g = 0; g <= 11; ++g) gptr.push_back(g);
  gptr.push_back(13); gptr.push_back(15);
  I32 cls, stt, its; std::vector<char> tw; std::vector<double> res;
  for (size_t q = 0; q < subs.size(); ++q) {
    gcols.push_back(2 * (int64_t)q + 1);
    cls.push_back(subs[q].cls); tw.push_back(subs[q].tw); stt.push_back(subs[q].stt); its.push_back(subs[q].its); res.push_back(subs[q].res);
  }
  I64 rp, rc, rd;
  sls::select_refinement_groups(0, 13, gptr, gcols, base, cls.data(), tw.data(), stt.data(), its.data(), res.data(), rp, rc, rd);
  const I64 want_q = {1, 3, 5, 6, 8, 9, 11, 12};
  I64 want_cols; for (int64_t q : want_q) want_cols.push_back(2 * q + 1 + base);
  EXPECT((rp == I64{0, 1, 2, 3, 4, 5, 6, 8}) && rc == want_cols && rd == want_q, "selection over the whole list");
  // the shard of groups [5, 13): its arrays start at subproblem 5, and so does rg_dst
  sls::select_refinement_groups(5, 13, gptr, gcols, base, cls.data() + 5, tw.data() + 5, stt.data() + 5, its.data() + 5, res.data() + 5, rp, rc, rd);
  want_cols.erase(want_cols.begin(), want_cols.begin() + 2);
  EXPECT((rp == I64{0, 1, 2, 3, 4, 6}) && rc == want_cols && (rd == I64{0, 1, 3, 4, 6, 7}), "selection on a shard is relative to the shard");
  // exact-size copies of the shard [11, 13) = subproblems 11 .. 14: nothing before or behind them is read
  const I32 c2(cls.begin() + 11, cls.end()), s2(stt.begin() + 11, stt.end()), i2(its.begin() + 11, its.end());
  const std::vector<char> t2(tw.begin() + 11, tw.end()); const std::vector<double> r2(res.begin() + 11, res.end());
  sls::select_refinement_groups(11, 13, gptr, gcols, base, c2.data(), t2.data(), s2.data(), i2.data(), r2.data(), rp, rc, rd);
  EXPECT((rp == I64{0, 2}) && (rc == I64{23 + base, 25 + base}) && (rd == I64{0, 1}), "last shard");
  const I32 ok(15, SLS_COL_OK), one(15, 1); const std::vector<double> small(15, 1e-14);
  sls::select_refinement_groups(0, 13, gptr, gcols, base, cls.data(), tw.data(), ok.data(), one.data(), small.data(), rp, rc, rd);
  EXPECT((rp == I64{0}) && rc.empty() && rd.empty(), "nothing qualifies");
}

// ---------------------------------------------------------------- batch composite
using Dense = std::vector<std::vector<double>>;
Dense zeros(int64_t r, int64_t c) { return Dense((size_t)r, std::vector<double>((size_t)c, 0.0)); }
struct Csc {
  int64_t nr = 0, nc = 0;
  I64 cp, ri;
  std::vector<double> v;
  sls_csc_f64 f64() const { return sls_csc_f64{nr, nc, cp.data(), ri.data(), v.data()}; }
  sls_csc_bool boolean() const { return sls_csc_bool{nr, nc, cp.data(), ri.data(), nullptr}; }
};
Csc from_dense(const Dense& M, int64_t nr, int64_t nc, int base) {
  Csc m; m.nr = nr; m.nc = nc; m.cp.assign((size_t)nc + 1, base);
  for (int64_t c = 0; c < nc; ++c) {
    for (int64_t r = 0; r < nr; ++r)
      if (M[r][c] != 0.0) { m.ri.push_back(r + base); m.v.push_back(M[r][c]); }
    m.cp[c + 1] = (int64_t)m.ri.size() + base;
  }
  return m;
}
template <class V>
Dense to_dense(const V& m, int base) {                    // sls_csc_f64 / sls_csc_bool view → dense (bool entries as 1.0)
  Dense D = zeros(m.nrows, m.ncols);
  for (int64_t c = 0; c < m.ncols; ++c)
    for (int64_t e = m.colptr[c] - base; e < m.colptr[c + 1] - base; ++e) D[(size_t)(m.rowval[e] - base)][(size_t)c] = m.nzval ? (double)m.nzval[e] : 1.0;
  return D;
}
// every entry a value of its own: 1000·tag + 10·row + col + 1
Dense tagged(int64_t nr, int64_t nc, int tag, bool full) {
  Dense D = zeros(nr, nc);
  for (int64_t r = 0; r < nr; ++r)
    for (int64_t c = 0; c < nc; ++c)
      if (full || r == c || r == c + 1) D[r][c] = 1000.0 * tag + 10.0 * r + c + 1;
  return D;
}

struct Plant {
  sls_dims dims;
  Dense dA, dB1, dB2, dC1, dD11, dD12;
  std::vector<Dense> dSx, dSu;
  Csc A, B1, B2, C1, D11, D12;
  std::vector<Csc> mx, mu;
  sls_csc_f64 fA, fB1, fB2, fC1, fD11, fD12;
  std::vector<sls_csc_bool> bx, bu;
  sls_plant view(bool c1, bool d12, bool d11) const { return sls_plant{&fA, &fB1, &fB2, c1 ? &fC1 : nullptr, d11 ? &fD11 : nullptr, d12 ? &fD12 : nullptr}; }
};
void make_plant(Plant& p, int which, int64_t Nx, int64_t Nu, int64_t Nw, int64_t T, int base) {
  p.dims = sls_dims{Nx, Nu, Nx + Nu, Nw, T, base, 0};
  const int tag = 10 * (which + 1);
  p.dA = tagged(Nx, Nx, tag + 1, false); p.dB1 = tagged(Nx, Nw, tag + 2, true); p.dB2 = tagged(Nx, Nu, tag + 3, true);
  p.dC1 = tagged(Nx + Nu, Nx, tag + 4, true); p.dD11 = tagged(Nx + Nu, Nw, tag + 5, true); p.dD12 = tagged(Nx + Nu, Nu, tag + 6, true);
  p.A = from_dense(p.dA, Nx, Nx, base); p.B1 = from_dense(p.dB1, Nx, Nw, base); p.B2 = from_dense(p.dB2, Nx, Nu, base);
  p.C1 = from_dense(p.dC1, Nx + Nu, Nx, base); p.D11 = from_dense(p.dD11, Nx + Nu, Nw, base); p.D12 = from_dense(p.dD12, Nx + Nu, Nu, base);
  p.fA = p.A.f64(); p.fB1 = p.B1.f64(); p.fB2 = p.B2.f64(); p.fC1 = p.C1.f64(); p.fD11 = p.D11.f64(); p.fD12 = p.D12.f64();
  for (int64_t t = 0; t < T; ++t) {                     // t even: band masks, t odd: full ones — the counts per plant and step differ
    p.dSx.push_back(tagged(Nx, Nx, 0, t % 2 == 1)); p.dSu.push_back(tagged(Nu, Nx, 0, t % 2 == 0));
    p.mx.push_back(from_dense(p.dSx.back(), Nx, Nx, base)); p.mu.push_back(from_dense(p.dSu.back(), Nu, Nx, base));
  }
  for (int64_t t = 0; t < T; ++t) { p.bx.push_back(p.mx[t].boolean()); p.bu.push_back(p.mu[t].boolean()); }
}
int64_t nnz_of(const Dense& D) { int64_t n = 0; for (const auto& r : D) for (double v : r) n += v != 0.0; return n; }

void test_batch(int base) {
  const int64_t T = 2;
  Plant p[2];
  make_plant(p[0], 0, 3, 2, 4, T, base);                  // Nw = 4 > Nx = 3: one surplus disturbance channel
  make_plant(p[1], 1, 2, 1, 2, T, base);
  const int64_t NX = 5, NU = 3, xo[3] = {0, 3, 5}, uo[3] = {0, 2, 3};
  sls_dims dims[2] = {p[0].dims, p[1].dims};
  sls_plant P[2] = {p[0].view(true, true, true), p[1].view(true, true, false)};      // D11 on plant 0 only
  const sls_csc_bool* Sx[2] = {p[0].bx.data(), p[1].bx.data()};
  const sls_csc_bool* Su[2] = {p[0].bu.data(), p[1].bu.data()};
  std::vector<std::vector<double>> ox[2], ou[2];
  std::vector<double*> px[2], pu[2];
  for (int i = 0; i < 2; ++i)
    for (int64_t t = 0; t < T; ++t) { ox[i].emplace_back((size_t)nnz_of(p[i].dSx[t]), -1.0); ou[i].emplace_back((size_t)nnz_of(p[i].dSu[t]), -1.0); }
  for (int i = 0; i < 2; ++i)
    for (int64_t t = 0; t < T; ++t) { px[i].push_back(ox[i][t].data()); pu[i].push_back(ou[i][t].data()); }
  double* const* phix[2] = {px[0].data(), px[1].data()};
  double* const* phiu[2] = {pu[0].data(), pu[1].data()};
  std::string msg;
  {
    sls::BatchComposite C;
    EXPECT(C.build(2, dims, P, Sx, Su, phix, phiu, msg) == 0, "composite of two plants");
    EXPECT(C.dims.Nx == NX && C.dims.Nu == NU && C.dims.Nw == NX && C.dims.Nz == NX + NU && C.dims.T == T && C.dims.index_base == base, "composite dims, Nw = NX");
    EXPECT((C.xo == I64{0, 3, 5}) && (C.uo == I64{0, 2, 3}), "plant offsets");
    // the expected composite, placed entry by entry from the dense plants
    Dense eA = zeros(NX, NX), eB1 = zeros(NX, NX), eB2 = zeros(NX, NU), eC1 = zeros(NX + NU, NX), eD11 = zeros(NX + NU, NX), eD12 = zeros(NX + NU, NU);
    std::vector<Dense> eSx(T, zeros(NX, NX)), eSu(T, zeros(NU, NX));
    for (int i = 0; i < 2; ++i) {
      const int64_t nx = dims[i].Nx, nu = dims[i].Nu;
      auto zrow = [&](int64_t r) { return r < nx ? xo[i] + r : NX + uo[i] + (r - nx); };     // z = [x of all plants; u of all plants]
      for (int64_t r = 0; r < nx; ++r) {
        for (int64_t c = 0; c < nx; ++c) { eA[xo[i] + r][xo[i] + c] = p[i].dA[r][c]; eB1[xo[i] + r][xo[i] + c] = p[i].dB1[r][c]; }   // first Nx_i columns of B1 only
        for (int64_t c = 0; c < nu; ++c) eB2[xo[i] + r][uo[i] + c] = p[i].dB2[r][c];
      }
      for (int64_t r = 0; r < nx + nu; ++r) {
        for (int64_t c = 0; c < nx; ++c) { eC1[zrow(r)][xo[i] + c] = p[i].dC1[r][c]; if (i == 0) eD11[zrow(r)][xo[i] + c] = p[i].dD11[r][c]; }
        for (int64_t c = 0; c < nu; ++c) eD12[zrow(r)][uo[i] + c] = p[i].dD12[r][c];
      }
      for (int64_t t = 0; t < T; ++t)
        for (int64_t c = 0; c < nx; ++c) {
          for (int64_t r = 0; r < nx; ++r) eSx[t][xo[i] + r][xo[i] + c] = p[i].dSx[t][r][c] != 0.0;
          for (int64_t r = 0; r < nu; ++r) eSu[t][uo[i] + r][xo[i] + c] = p[i].dSu[t][r][c] != 0.0;
        }
    }
    EXPECT(to_dense(*C.plant.A, base) == eA, "A is block-diagonal");
    EXPECT(to_dense(*C.plant.B1, base) == eB1, "B1: the first Nx_i columns of each plant at xo[i]");
    EXPECT(C.plant.B1->ncols == NX && C.plant.B1->colptr[NX] - base == 3 * 3 + 2 * 2, "B1: the surplus column of plant 0 is absent");
    EXPECT(to_dense(*C.plant.B2, base) == eB2, "B2");
    EXPECT(C.plant.C1 && C.plant.D12 && to_dense(*C.plant.C1, base) == eC1 && to_dense(*C.plant.D12, base) == eD12, "C1 / D12 with the z-row shift");
    EXPECT(to_dense(*C.plant.D11, base) == eD11, "D11: plant 0's first Nx columns, none of plant 1");
    for (int64_t t = 0; t < T; ++t) {
      EXPECT(to_dense(C.Sx[t], base) == eSx[t] && to_dense(C.Su[t], base) == eSu[t], "masks are block-diagonal");
      // mask columns of plant i sit at xo[i]: the column pointers there bracket exactly its entries
      EXPECT(C.Sx[t].colptr[xo[1]] - base == nnz_of(p[0].dSx[t]) && C.Sx[t].colptr[NX] - base == nnz_of(p[0].dSx[t]) + nnz_of(p[1].dSx[t]), "Sx columns");
      EXPECT(C.Su[t].colptr[xo[1]] - base == nnz_of(p[0].dSu[t]) && C.Su[t].colptr[NX] - base == nnz_of(p[0].dSu[t]) + nnz_of(p[1].dSu[t]), "Su columns");
    }
    // split: composite values 0, 1, 2, … come back as each plant's own contiguous run, statuses cut at xo
    for (int64_t t = 0; t < T; ++t) {
      for (int64_t k = 0; k < C.Sx[t].colptr[NX] - base; ++k) C.px[t][k] = (double)k;
      for (int64_t k = 0; k < C.Su[t].colptr[NX] - base; ++k) C.pu[t][k] = 1000.0 + (double)k;
    }
    for (int64_t k = 0; k < NX; ++k) C.status[(size_t)k] = 10 + (int32_t)k;
    I32 s0(3, -1), s1(2, -1);
    int32_t* cs[2] = {s0.data(), s1.data()};
    EXPECT(C.split(phix, phiu, cs, msg) == 0, "split");
    for (int64_t t = 0; t < T; ++t)
      for (int i = 0; i < 2; ++i) {
        const double x0 = i ? (double)nnz_of(p[0].dSx[t]) : 0.0, u0 = 1000.0 + (i ? (double)nnz_of(p[0].dSu[t]) : 0.0);
        bool ok = true;
        for (size_t k = 0; k < ox[i][t].size(); ++k) ok = ok && ox[i][t][k] == x0 + (double)k;
        for (size_t k = 0; k < ou[i][t].size(); ++k) ok = ok && ou[i][t][k] == u0 + (double)k;
        EXPECT(ok, "each plant gets its own contiguous runs");
      }
    EXPECT((s0 == I32{10, 11, 12}) && (s1 == I32{13, 14}), "status split at xo");
    int32_t* cs_half[2] = {nullptr, s1.data()};
    EXPECT(C.split(phix, phiu, cs_half, msg) == 0 && C.split(phix, phiu, nullptr, msg) == 0, "nullable status arrays");
    std::vector<double*> hole = px[1]; hole[1] = nullptr;
    double* const* phix_hole[2] = {px[0].data(), hole.data()};
    EXPECT(C.split(phix_hole, phiu, cs, msg) == SLS_EINVAL && msg == "null phix_vals[i][t]", "split: null value array");
    std::vector<double> cx, cu;
    C.tile_ridge({0.5, 0.25}, {2.0}, cx, cu);
    EXPECT((cx == std::vector<double>{0.5, 0.25, 0.5, 0.25}) && (cu == std::vector<double>{2.0, 2.0}), "ridge tiled per plant");
  }
  {                                                       // default weights on every plant: the composite leaves them NULL too
    sls_plant Pd[2] = {p[0].view(false, false, true), p[1].view(false, false, false)};
    sls::BatchComposite C;
    EXPECT(C.build(2, dims, Pd, Sx, Su, phix, phiu, msg) == 0 && !C.plant.C1 && !C.plant.D12 && C.plant.D11, "default weights stay default");
  }
  auto refused = [&](const sls_dims* d, const sls_plant* Pl, double* const* const* hx, int code, const char* text, const char* what) {
    sls::BatchComposite C;
    std::string m;
    const int rc = C.build(2, d, Pl, Sx, Su, hx, phiu, m);
    EXPECT(rc == code && m == text, what);
  };
  sls_plant Pmix[2] = {p[0].view(true, true, true), p[1].view(false, false, false)};
  refused(dims, Pmix, phix, SLS_EINVAL, "plants of one batch must all give C1, D12 or all leave them NULL", "mixed NULL and non-NULL C1");
  sls_plant Phalf[2] = {p[0].view(true, true, true), p[1].view(true, false, false)};
  refused(dims, Phalf, phix, SLS_EINVAL, "plant 1: C1 and D12 must be given together", "C1 without D12");
  sls_dims dT[2] = {dims[0], dims[1]}; dT[1].T = 3;
  refused(dT, P, phix, SLS_EINVAL, "plants of one batch must share T, index_base and flags", "differing T");
  sls_dims dZ[2] = {dims[0], dims[1]}; dZ[1].Nz = 4;
  refused(dZ, P, phix, SLS_ENOTSF, "Nz must equal Nx + Nu (state feedback with z = [x; u] rows)", "Nz != Nx + Nu");
  double* const* phix_null[2] = {px[0].data(), nullptr};
  refused(dims, P, phix_null, SLS_EINVAL, "null per-plant argument", "null per-plant output array");
}

// ---------------------------------------------------------------- unpack
void test_unpack() {
  // T = 3; Φx[1] and Φu[2] hold no values.  Value indices: Φx[0] 0..2, Φx[2] 3..4, Φu[0] 5..6, Φu[1] 7..8
  const int64_t T = 3;
  const I64 off_x = {0, 3, 3, 5}, off_u = {5, 7, 9, 9};
  const I64 shard[2] = {{0, 5, 2, 8, 4}, {1, 6, 3, 7}};    // together a permutation of 0..8, each crossing slice boundaries
  std::vector<std::vector<double>> vx = {std::vector<double>(3, -1.0), {}, std::vector<double>(2, -1.0)};
  std::vector<std::vector<double>> vu = {std::vector<double>(2, -1.0), std::vector<double>(2, -1.0), {}};
  std::vector<double*> px, pu;
  for (int64_t t = 0; t < T; ++t) { px.push_back(vx[t].data()); pu.push_back(vu[t].data()); }
  I32 slice_of;
  for (int s = 0; s < 2; ++s) {
    std::vector<double> stage;
    for (int64_t f : shard[s]) stage.push_back(100.0 + (double)f);
    sls::unpack_packed_shard(T, off_x.data(), off_u.data(), 9, shard[s].data(), (int64_t)shard[s].size(), stage.data(), slice_of, px.data(), pu.data());
    EXPECT((slice_of == I32{0, 0, 0, 2, 2, 3, 3, 4, 4}), "slice table: built by the first shard, kept by the second");
    if (s == 0) EXPECT(vx[0][1] == -1.0 && vx[2][0] == -1.0 && vu[0][1] == -1.0 && vu[1][0] == -1.0, "the first shard leaves the second's values alone");
  }
  EXPECT((vx[0] == std::vector<double>{100, 101, 102}) && (vx[2] == std::vector<double>{103, 104}), "Φx values at their places");
  EXPECT((vu[0] == std::vector<double>{105, 106}) && (vu[1] == std::vector<double>{107, 108}), "Φu values at their places");
  sls::unpack_packed_shard(T, off_x.data(), off_u.data(), 9, nullptr, 0, nullptr, slice_of, px.data(), pu.data());   // a shard without free variables
}

// ---------------------------------------------------------------- status fold
void test_fold() {
  const I32 stt = {SLS_COL_OK, SLS_COL_TRIVIAL, SLS_COL_INFEASIBLE, SLS_COL_NOTCONV, SLS_COL_UNSUPPORTED}, its = {2, 0, 9, 48, 1};
  const std::vector<double> res = {1e-12, 3e-10, 0.5, 0.25, 7.0};
  I32 cs(7, -1);
  sls_stats st{};
  sls::fold_column_status(stt.data(), res.data(), its.data(), 5, cs.data() + 1, st);
  EXPECT((cs == I32{-1, SLS_COL_OK, SLS_COL_TRIVIAL, SLS_COL_INFEASIBLE, SLS_COL_NOTCONV, SLS_COL_UNSUPPORTED, -1}), "statuses copied at the offset, nothing beside them");
  EXPECT(st.n_not_ok == 3 && st.max_residual == 3e-10 && st.max_iters == 48, "residual of OK / TRIVIAL columns only, iterations of all");
  const I32 stt2 = {SLS_COL_OK}, its2 = {3}; const std::vector<double> res2 = {1e-9};
  sls::fold_column_status(stt2.data(), res2.data(), its2.data(), 1, nullptr, st);                 // a second shard, no status array
  EXPECT(st.n_not_ok == 3 && st.max_residual == 1e-9 && st.max_iters == 48, "a second shard folds into the same stats");
  sls::fold_column_status(nullptr, nullptr, nullptr, 0, nullptr, st);
}

}  // namespace

int main() {
  for (int base = 0; base < 2; ++base) { test_layers(base); test_refinement(base); test_batch(base); }
  test_cuts();
  test_unpack();
  test_fold();
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("sanitize_dropin: clean\n");
  return 0;
}
