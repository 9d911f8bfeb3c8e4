// sls_routing.cpp — kernel selection of a plan (see sls_routing.h).  No HIP: builds with the host compiler alone.
#include "sls_routing.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace sls {

namespace {
bool knob_is(const char* name, char c) { const char* e = sls_knob(name); return e && e[0] == c; }
char knob_char(const char* name) { const char* e = sls_knob(name); return e ? e[0] : 0; }
int knob_int(const char* name, int dflt) { const char* e = sls_knob(name); return e ? std::atoi(e) : dflt; }
double knob_double(const char* name, double dflt) { const char* e = sls_knob(name); return e ? std::atof(e) : dflt; }
size_t round_up(size_t b, size_t to) { return (b + to - 1) / to * to; }

enum class Bin { Wave, General, Wide, TileLds, TileGlb, TileBig };   // what a bin's columns run on (TileLds / TileGlb: where the block lives)
enum TileBin { kLdsSmall, kLds, kGlbSmall, kGlb, kBig, kNumTileBins };   // small: two workgroups per CU (LDS: ≤ 6 tile rows; workspace: two panels fit twice)
}  // namespace

RoutingKnobs RoutingKnobs::from_env() {
  RoutingKnobs k;
  k.force_general = knob_is("SLS_FORCE_GENERAL", '1');
  k.wave64 = knob_is("SLS_WAVE64", '1');
  k.tile = knob_char("SLS_TILE");
  k.tile_big = knob_char("SLS_TILE_BIG");
  k.tile_global = knob_is("SLS_TILE_GLOBAL", '1');
  k.tile_lds_maxnt = knob_int("SLS_TILE_LDS_MAXNT", 6);
  k.son_tile = knob_is("SLS_SON_TILE", '1');
  k.absorb = !knob_is("SLS_ABSORB", '0');
  k.tile_one_per_cu = knob_is("SLS_TILE_ONE_PER_CU", '1');
  if (sls_knob("SLS_GW_TWO")) k.gw_two = knob_is("SLS_GW_TWO", '1');
  k.vec_global = knob_is("SLS_VEC_GLOBAL", '1');
  k.vec_lds = knob_is("SLS_VEC_LDS", '1');
  k.no_twisted = knob_is("SLS_NO_TWISTED", '1');
  k.p_lds = knob_is("SLS_P_LDS", '1');
  k.twisted4 = !knob_is("SLS_TWISTED4", '0');
  k.t4_nmin = knob_int("SLS_T4_NMIN", 13);
  k.t4_tmin = knob_int("SLS_T4_TMIN", 7);
  k.per_cu_any = sls_knob("SLS_PER_CU_ANY") != nullptr;
  k.max_per_cu = knob_int("SLS_MAX_PER_CU", INT_MAX);
  k.full_grid = sls_knob("SLS_FULL_GRID") != nullptr;
  k.no_tiny_first = sls_knob("SLS_NO_TINY_FIRST") != nullptr;
  k.tiny_first = sls_knob("SLS_TINY_FIRST") != nullptr;
  if (sls_knob("SLS_TILE_WPE")) k.tile_wpe = knob_is("SLS_TILE_WPE", '4');
  return k;
}

SolverKnobs SolverKnobs::from_env() {
  SolverKnobs k;
  k.delta_rel = knob_double("SLS_DELTA_REL", k.delta_rel);
  k.tol = knob_double("SLS_TOL", k.tol);
  k.max_iters = std::max(1, knob_int("SLS_MAX_ITERS", k.max_iters));
  k.stag = knob_double("SLS_STAG", k.stag);
  k.son_maxit = std::max(1, knob_int("SLS_SON_MAXIT", k.son_maxit));
  k.son_tol = knob_double("SLS_SON_TOL", k.son_tol);
  k.son_anderson = !knob_is("SLS_SON_ANDERSON", '0');
  k.son_aa_start = std::max(0, knob_int("SLS_SON_AA_START", k.son_aa_start));
  k.delta_first = knob_double("SLS_DELTA_FIRST", k.delta_first);
  k.max_iters_slow = std::max(0, knob_int("SLS_MAX_ITERS_SLOW", k.max_iters_slow));
  if (sls_knob("SLS_PHASE_TIMERS")) k.dbg_level = std::max(1, knob_int("SLS_PHASE_TIMERS", 1));
  k.knock_out = knob_int("SLS_KNOCK_OUT", 0);
  k.t4_prestatic = !knob_is("SLS_T4_PRESTATIC", '0');
  return k;
}

void SolverKnobs::apply(KernelParams& kp) const {
  kp.delta_rel = delta_rel; kp.tol = tol; kp.tol_ok = tol_ok; kp.max_iters = max_iters; kp.stag = stag;
  kp.son_maxit = son_maxit; kp.son_tol = son_tol; kp.son_anderson = son_anderson; kp.son_aa_start = son_aa_start;
  kp.delta_first = delta_first; kp.max_iters_slow = max_iters_slow; kp.dbg_level = dbg_level; kp.knock_out = knock_out;
}

int check_sum_of_norms_weights(const Symbolic& S, std::string& err) {
  for (const SubDesc& sd : S.subs) {
    bool bad = sd.has_w >= 2;
    if (sd.has_w == 1) for (int32_t i = 0; i < sd.n + sd.m && !bad; ++i) bad = S.w_pool[(size_t)sd.off_w + sd.n + sd.m + i] != 0.0;
    if (bad) { err = "SLS_SOLVE_SUM_OF_NORMS needs a diagonal [C1 D12]'[C1 D12] and D11 = 0"; return SLS_EUNSUPPORTED; }
  }
  return 0;
}

ScratchLayout scratch_layout(size_t fac_doubles, size_t vec_doubles, size_t big_bytes) {
  ScratchLayout L;
  // the slack (32 doubles, 512 + 256 bytes) covers the two roundings below whatever the sizes
  L.bytes = (std::max<size_t>(fac_doubles, 1) + vec_doubles + 32) * sizeof(double) + 512 + big_bytes + 256;
  L.vec_off = round_up(fac_doubles, 32);
  L.big_off = round_up((L.vec_off + vec_doubles + 32) * sizeof(double), 256);
  return L;
}

T4Pools t4_pool_layout(const std::vector<LaunchSpec>& launches, int T, bool prestatic) {
  T4Pools P;
  P.slots.resize(launches.size());
  for (size_t li = 0; li < launches.size(); ++li) {
    const LaunchSpec& L = launches[li];
    if (!(L.kind == LaunchKind::Twisted && L.four)) continue;
    T4Slot& s = P.slots[li];
    s.t4_off = P.records; P.records += L.nsub;
    s.t4s_stride = twisted4_static_doubles(L.cls, T);
    s.t4s_off = P.static_doubles; P.static_doubles += s.t4s_stride * L.nsub;
    s.t4i_stride = twisted4_image_doubles(L.cls, T);
    s.t4i_off = P.image_doubles; P.image_doubles += s.t4i_stride * L.nsub;
  }
  P.keep_static = P.records > 0 && prestatic && (P.static_doubles + P.image_doubles) * (int64_t)sizeof(double) <= kT4StaticBudget;
  return P;
}

// small wave classes (0..5) → ONE multi-class launch; mid classes (6..8) → one launch each;
// everything else (ñx > 64, ñu > 64, or LDS over budget) → the tile kernel (or the round-1 workgroup kernel, SLS_TILE).
int build_launch_list(Symbolic& S, int T, int objective, int ncu, bool force_tile, const RoutingKnobs& K, RoutingResult& out,
                      std::string& err, bool one_wave_only) {
  const bool force_general = force_tile || K.force_general;
  if (one_wave_only) {
    // SLS_PLAN_MULTIPLIERS: only the one-wave kernel of the 16- and 32-lane classes exports its multipliers
    if (objective == 1) { err = "SLS_PLAN_MULTIPLIERS: the sum-of-norms objective keeps no multiplier of the 𝓗₂ cost"; return SLS_EUNSUPPORTED; }
    if (force_tile) { err = "SLS_PLAN_MULTIPLIERS: the tile kernel holds no accumulated multiplier"; return SLS_EUNSUPPORTED; }
    for (const SubDesc& sd : S.subs) {
      if (sd.has_w == 3 || sd.has_w == 4) { err = "SLS_PLAN_MULTIPLIERS: coupled column groups (non-diagonal B1[c_j,c_j]) are not supported"; return SLS_EUNSUPPORTED; }
      if (sd.has_w == 2) { err = "SLS_PLAN_MULTIPLIERS: a dense cost Hessian is not supported (diagonal weights only)"; return SLS_EUNSUPPORTED; }
      if (sd.cls < 0 || sd.cls >= kNumSmallWaveClasses) {
        err = "SLS_PLAN_MULTIPLIERS: a column with ñx = " + std::to_string(sd.n) + " (ñu = " + std::to_string(sd.m) +
              ") runs on the tile kernel, which holds no accumulated multiplier (one-wave classes only: ñx ≤ 32, ñu ≤ 64)";
        return SLS_EUNSUPPORTED;
      }
    }
  }
  const int capA = S.max_row_A, capAc = S.max_row_At, capB = S.max_row_B, capBc = S.max_row_Bt;
  std::vector<int32_t> bins[kNumWaveClasses + 1];   // [c] wave class c, [kNumWaveClasses] general
  std::vector<int32_t>& too_large = out.too_large;  // beyond the LDS budget of every kernel of this build
  std::vector<int32_t> wide_bin;                    // general kernel, wide variant
  // Latency regime (the whole batch fits in one wave of workgroups, e.g. the README chain's 59 columns): the
  // launch lasts as long as its slowest column whatever class the small ones run in, so use ONE class — the
  // largest needed — and skip the multi-stream fork/join (≈0.1 ms per step measured with four classes).
  int merge_cls = -1;
  if (!force_general && (int64_t)S.subs.size() <= 4LL * ncu) {
    for (const SubDesc& sd : S.subs)
      if (K.wave64 || sd.cls < kNumSmallWaveClasses) merge_cls = std::max(merge_cls, sd.cls);   // (64-lane columns go to the tile kernel)
  }
  // Every subproblem outside the wave classes (ñx > 64 or ñu > 64) runs on the MFMA tile kernel.  SLS_TILE (experiments and
  // the tests of the round-1 kernels): "0" = never (round-1 launch list: workgroup kernel up to ñx = 144, beyond that
  // SLS_COL_UNSUPPORTED), "large" = only what the workgroup kernel cannot hold.
  const bool tile_off = K.tile == '0' && !force_tile;
  const bool tile_all = !tile_off && K.tile != 'l';
  std::vector<int32_t> tile_bins[2][kNumTileBins];                      // [1]: dense cost Hessian, the build with the CG loop (no small bins)
  const bool big_off = K.tile_big == '0';                               // experiments: restore SLS_COL_UNSUPPORTED beyond LDS
  const bool big_all = K.tile_big == 'a';                               // tests: every tile column through the big variant
  auto tile_need = [&](const SubDesc& sd, bool mlds) {
    return tile_kernel_lds_bytes(sd.n, std::max(sd.m, 1), std::max(sd.nnzA, 1), std::max(sd.nnzB, 1), mlds);
  };
  // carve beyond LDS (panels / lists, ñx ≳ 250): the big variant moves it to a global buffer
  auto beyond_lds = [&](int cg, int32_t q) { (big_off ? too_large : tile_bins[cg][kBig]).push_back(q); };
  auto to_tile = [&](int32_t q) {
    const SubDesc& sd = S.subs[q];
    if (tile_off) { too_large.push_back(q); return; }
    const int cg = (sd.has_w >= 2 || objective == 1) ? 1 : 0;
    // beyond 6 tile rows (SLS_TILE_LDS_MAXNT) the LDS-resident block leaves room for one workgroup per CU only; in the
    // workspace two share the CU (random10000_d2: 69 → 65 ms)
    const bool mlds_ok = !K.tile_global;
    std::vector<int32_t>* b = tile_bins[cg];
    if (big_all) b[kBig].push_back(q);
    else if (!cg && mlds_ok && tile_nt(sd.n) <= 6 && tile_need(sd, true) <= kMaxLds / 2) b[kLdsSmall].push_back(q);
    else if (mlds_ok && tile_nt(sd.n) <= K.tile_lds_maxnt && tile_need(sd, true) <= kMaxLds) b[kLds].push_back(q);
    else if (!cg && tile_need(sd, false) <= kMaxLds / 2) b[kGlbSmall].push_back(q);
    else if (tile_need(sd, false) <= kMaxLds) b[kGlb].push_back(q);
    else beyond_lds(cg, q);
  };
  // sum-of-norms objective: columns of the light wave classes (ñx ≤ 32) run the ADMM loop inside the one-wave kernel (its own
  // solve as the projection, 8× the tile kernel's rate on chain-4096); everything else on the tile kernel's CG / ADMM build
  if (objective == 1) merge_cls = -1;
  std::vector<int32_t> mid_cols;                           // ñx 33…64: tile kernel or 64-lane one-wave class, see below
  for (int32_t q : S.order) {
    SubDesc& sd = S.subs[q];
    if (sd.has_w == 4) { sd.cls = -1; continue; }                   // member of a coupled group: solved by the group's first column
    const bool son_wave = objective == 1 && !K.son_tile && !force_general && sd.has_w < 2 && sd.cls >= 0 && sd.cls < kNumSmallWaveClasses;
    const bool cg_build = sd.has_w >= 2 || (objective == 1 && !son_wave);      // dense cost Hessian / coupled group / sum-of-norms: tile kernel, CG build
    int cls = (force_general || cg_build) ? -1 : sd.cls;
    // ñx 33…64: the 64-lane one-wave classes hold a whole SIMD's registers and 57–117 KiB of LDS per column for ONE wave; the
    // tile kernel (512 threads, MFMA tiles) is faster on every workload measured — chain ñx = 43: 2.96 → 2.16 ms, ñx = 59:
    // 7.09 → 3.70 ms, grid-32 (its 252 boundary columns next to the tile launch): 5.45 → 4.19 ms — and converges to smaller
    // residuals.  SLS_WAVE64=1 restores the round-1 routing (tests of those classes, experiments).
    if (cls >= kNumSmallWaveClasses && tile_all && !K.wave64) { mid_cols.push_back(q); continue; }      // decided after the loop
    if (cls >= 0 && merge_cls >= 0 && cls <= merge_cls) cls = merge_cls;      // (never down: merge_cls leaves the 64-lane classes out)
    if (cls >= 0) {
      const int64_t need = wave_kernel_lds_bytes(cls, T, std::max(sd.m, 1), capA, capAc, capB, capBc, sd.n + sd.m);
      if (need > kMaxLds) cls = -1;
    }
    sd.cls = cls;
    if (cls < 0) {
      if (tile_all || cg_build) { to_tile(q); continue; }
      const int64_t need = general_kernel_lds_bytes(sd.n, std::max(sd.m, 1), std::max(sd.nnzA, 1), std::max(sd.nnzB, 1), T, false);
      if (need > kMaxLds || sd.n > 96) {
        const int64_t needw = general_kernel_lds_bytes(sd.n, std::max(sd.m, 1), std::max(sd.nnzA, 1), std::max(sd.nnzB, 1), T, false, true);
        if (needw <= kMaxLds && sd.n <= 144) wide_bin.push_back(q);
        else to_tile(q);
        continue;
      }
    }
    bins[cls < 0 ? kNumWaveClasses : cls].push_back(q);
  }
  if (!mid_cols.empty()) {
    // The tile kernel wins on these columns (see above) — unless putting them into the launch of the LDS-resident blocks
    // costs every column of that launch LDS: a launch is sized by the maxima over its bin, and a wide ñu or long sparse
    // rows among the ñx ≤ 64 columns shrink the Ã·Q strip (or the workgroups per CU) of all of them (random10000_d2:
    // 145 such columns next to 5013: 64 → 70 ms).  Then they keep their one-wave classes.
    const std::vector<int32_t>& lds_small = tile_bins[0][kLdsSmall];
    auto plan_of = [&](const std::vector<int32_t>& a, const std::vector<int32_t>* b2) {
      int nmax = 1, mmax = 1, na = 1, nb = 1;
      auto acc = [&](const std::vector<int32_t>& v) {
        for (int32_t q : v) { const SubDesc& sd = S.subs[q]; nmax = std::max(nmax, sd.n); mmax = std::max(mmax, sd.m); na = std::max(na, sd.nnzA); nb = std::max(nb, sd.nnzB); }
      };
      acc(a); if (b2) acc(*b2);
      int per_cu = 1;
      if (tile_kernel_lds_bytes(nmax, mmax, na, nb, true, 16) <= kMaxLds / 2) per_cu = 2;
      int rows = 16;
      const int npadL = 16 * tile_nt(nmax);
      while (rows < npadL && tile_kernel_lds_bytes(nmax, mmax, na, nb, true, rows + 16) <= kMaxLds / per_cu) rows += 16;
      return std::make_pair(per_cu, rows);
    };
    bool to_tile_ok = true;
    if (!lds_small.empty()) to_tile_ok = plan_of(lds_small, &mid_cols) == plan_of(lds_small, nullptr);
    // … and unless they are a sliver of that launch anyway: a few per cent of extra columns at the END of its queue (it is
    // ordered by descending ñx) only lengthen its tail, while their own one-wave launches run beside it from t = 0
    // (random10000_d2: 145 next to 5013 — 64.0 ms in their one-wave classes, 69.2 ms on the tile queue; grid-32: 252 next
    // to 772 — 5.45 ms against 4.19 ms)
    if (to_tile_ok && mid_cols.size() * 10 < lds_small.size()) to_tile_ok = false;
    for (int32_t q : mid_cols) {
      SubDesc& sd = S.subs[q];
      if (to_tile_ok) { sd.cls = -1; to_tile(q); }
      else {
        const int64_t need = wave_kernel_lds_bytes(sd.cls, T, std::max(sd.m, 1), capA, capAc, capB, capBc, sd.n + sd.m);
        if (need > kMaxLds) { sd.cls = -1; to_tile(q); } else bins[sd.cls].push_back(q);
      }
    }
  }
  // A sliver of a small one-wave class — under 2 % of the columns of the most populated larger class (chain-4096: 22 edge columns
  // in three classes next to 4074 interior ones) — runs in that class's launch: a launch of its own saves those few columns
  // some registers and costs every step a stream fork and join (rocprof: kernel 1.55 ms, step 1.67 ms with four launches).
  // Larger classes hold every smaller column (the latency regime above merges the same way).  SLS_ABSORB=0: off.
  if (objective == 0 && K.absorb) {
    for (int c = 0; c < kNumSmallWaveClasses; ++c) {
      if (bins[c].empty()) continue;
      int big = -1;
      for (int c2 = c + 1; c2 < kNumSmallWaveClasses; ++c2)
        if (!bins[c2].empty() && (big < 0 || bins[c2].size() > bins[big].size())) big = c2;
      if (big < 0 || bins[c].size() * 50 > bins[big].size()) continue;
      // … as long as it does not raise that launch's LDS plan (a launch is sized by the maxima over its bin)
      auto need_in_big = [&](const SubDesc& sd) { return wave_kernel_lds_bytes(big, T, std::max(sd.m, 1), capA, capAc, capB, capBc, sd.n + sd.m); };
      int64_t big_need = 0;
      for (int32_t q : bins[big]) big_need = std::max(big_need, need_in_big(S.subs[q]));
      std::vector<int32_t> stay;
      for (int32_t q : bins[c]) {
        SubDesc& sd = S.subs[q];
        if (need_in_big(sd) <= big_need) { sd.cls = big; bins[big].push_back(q); }
        else stay.push_back(q);
      }
      bins[c].swap(stay);
      std::stable_sort(bins[big].begin(), bins[big].end(), [&](int32_t a, int32_t b) { return S.subs[a].n > S.subs[b].n; });
    }
  }
  // a workgroup launch is sized by the maxima over its bin (ñx, ñu, nnz separately): move the widest on until the combination fits
  auto need_bin = [&](Bin kind, int n, int m, int a, int b) -> int64_t {
    if (kind == Bin::TileLds || kind == Bin::TileGlb) return tile_kernel_lds_bytes(n, m, a, b, kind == Bin::TileLds);
    return general_kernel_lds_bytes(n, m, a, b, T, false, kind == Bin::Wide);
  };
  auto shrink = [&](std::vector<int32_t>& gb, Bin kind, std::vector<int32_t>& overflow, int64_t limit = kMaxLds) {
    auto need_of = [&](const SubDesc& sd) { return need_bin(kind, sd.n, std::max(sd.m, 1), std::max(sd.nnzA, 1), std::max(sd.nnzB, 1)); };
    auto combined = [&]() {
      int nmax = 1, mmax = 1, a = 1, b = 1;
      for (int32_t q : gb) { const SubDesc& sd = S.subs[q]; nmax = std::max(nmax, sd.n); mmax = std::max(mmax, sd.m); a = std::max(a, sd.nnzA); b = std::max(b, sd.nnzB); }
      return need_bin(kind, nmax, mmax, a, b);
    };
    while (!gb.empty() && combined() > limit) {
      size_t worst = 0; int64_t wneed = -1;
      for (size_t i = 0; i < gb.size(); ++i) { const int64_t nd = need_of(S.subs[gb[i]]); if (nd > wneed) { wneed = nd; worst = i; } }
      overflow.push_back(gb[worst]);
      gb.erase(gb.begin() + worst);
    }
  };
  {
    std::vector<int32_t> spill, spill2;
    shrink(bins[kNumWaveClasses], Bin::General, spill);
    for (int32_t q : spill) {             // did not fit next to the others: try the wide variant
      const SubDesc& sd = S.subs[q];
      if (general_kernel_lds_bytes(sd.n, std::max(sd.m, 1), std::max(sd.nnzA, 1), std::max(sd.nnzB, 1), T, false, true) <= kMaxLds && sd.n <= 144) wide_bin.push_back(q);
      else to_tile(q);
    }
    shrink(wide_bin, Bin::Wide, spill2);
    for (int32_t q : spill2) to_tile(q);
    // tile bins, in this order (it decides which columns end up where): what does not fit next to the others moves from a small
    // bin to the full one, from the LDS-resident block to the workspace if its own carve fits there, else beyond LDS
    for (int cg = 0; cg < 2; ++cg)
      for (int b = kLdsSmall; b <= kGlb; ++b) {
        const bool lds = b == kLdsSmall || b == kLds, small = b == kLdsSmall || b == kGlbSmall;
        std::vector<int32_t> over;
        shrink(tile_bins[cg][b], lds ? Bin::TileLds : Bin::TileGlb, over, small ? kMaxLds / 2 : kMaxLds);
        for (int32_t q : over) {
          if (small) tile_bins[cg][b + 1].push_back(q);
          else if (lds && tile_need(S.subs[q], false) <= kMaxLds) tile_bins[cg][kGlb].push_back(q);
          else beyond_lds(cg, q);
        }
      }
    // launches walk their bin in descending ñx (S.order is sorted that way; spilled entries were appended out of order)
    auto by_n = [&](int32_t a, int32_t b) { return S.subs[a].n > S.subs[b].n; };
    std::stable_sort(wide_bin.begin(), wide_bin.end(), by_n);
    for (auto& build : tile_bins)
      for (auto& v : build) std::stable_sort(v.begin(), v.end(), by_n);
  }
  std::vector<int32_t> order2;
  std::vector<LaunchSpec>& launches = out.launches;
  auto add_launch = [&](Bin kind, int cls, const std::vector<int32_t>& v) {
    if (v.empty()) return;
    LaunchSpec L{};
    L.cls = cls; L.order_off = (int)order2.size(); L.nsub = (int)v.size();
    int mcap = 1, nm_max = 1, nmax = 1, mmax = 1, nnzA = 1, nnzB = 1; int64_t lds = 0;
    for (int32_t q : v) {
      const SubDesc& sd = S.subs[q];
      L.work += (double)sd.n * sd.n * sd.n; L.n_longest = std::max(L.n_longest, sd.n);
      mcap = std::max(mcap, sd.m); nm_max = std::max(nm_max, sd.n + sd.m);
      nmax = std::max(nmax, sd.n); mmax = std::max(mmax, sd.m);
      nnzA = std::max(nnzA, sd.nnzA); nnzB = std::max(nnzB, sd.nnzB);
    }
    if (kind == Bin::TileLds || kind == Bin::TileGlb || kind == Bin::TileBig) {
      out.has_tile = true;
      L.kind = LaunchKind::Tile; L.mlds = kind == Bin::TileLds; L.big = kind == Bin::TileBig;
      L.nmax = nmax; L.mmax = mmax; L.nnzA_cap = nnzA; L.nnzB_cap = nnzB;
      // LDS plan: two workgroups per CU (80 KiB each) when the block, the lists and a 16-row strip of the Ã·Q image fit —
      // the serial pivot-tile factorisation of one column then overlaps the other column's work; else one per CU.  The
      // Ã·Q image gets as many rows (multiples of 16) as the chosen budget leaves.
      const int npadL = 16 * tile_nt(nmax);
      bool any_general = false;
      int ncol_max = 1;                                   // columns of the largest coupled group of the launch
      for (int32_t q : v) {
        any_general = any_general || S.subs[q].has_w >= 2 || objective == 1;
        if (S.subs[q].has_w == 3) ncol_max = std::max(ncol_max, S.subs[q].pad_);
      }
      L.gw = any_general;
      // the CG / ADMM build needs 256 VGPRs (one 512-thread workgroup per CU); the sum-of-norms loop is thousands of
      // latency-bound steps per column, where two workgroups of the 128-VGPR build per CU win (chain-4096: 25.7 → 19.6 s)
      const bool gw2 = any_general && L.mlds && (K.gw_two >= 0 ? K.gw_two == 1 : objective == 1);
      const int max_wg = (L.big || K.tile_one_per_cu || (any_general && !gw2)) ? 1 : (kTileThreads == 256 ? 4 : 2);
      L.per_cu = 1;
      for (int wg = max_wg; wg > 1; wg /= 2)
        if (tile_kernel_lds_bytes(nmax, mmax, nnzA, nnzB, L.mlds, 16) <= kMaxLds / wg) { L.per_cu = wg; break; }
      // more than two waves per SIMD: the 128-VGPR build (SLS_TILE_WPE, experiments: the compile variant independent of the grid)
      L.two_per_cu = K.tile_wpe >= 0 ? K.tile_wpe == 1 : L.per_cu * kTileWaves > 8;
      const int64_t budget = kMaxLds / L.per_cu;
      L.oth_rows = 16;
      while (!L.big && L.oth_rows < npadL && tile_kernel_lds_bytes(nmax, mmax, nnzA, nnzB, L.mlds, L.oth_rows + 16) <= budget) L.oth_rows += 16;
      lds = tile_kernel_lds_bytes(nmax, mmax, nnzA, nnzB, L.mlds, L.oth_rows);
      if (L.big) {                                       // the carve goes to global memory; LDS only holds the block-reduction words
        L.big_stride = (int64_t)round_up(lds, 256);
        lds = 256;
      }
      L.vec_in_lds = 0;
      L.fac_stride = tile_kernel_fac_doubles(nmax, T);
      L.vec_stride = 3LL * (T + 1) * nmax + 2LL * T * (nmax + mmax);   // Δλ, r, r′; the primal iterate and its trial point
      if (any_general) L.vec_stride += 5LL * T * (nmax + mmax);            // CG on a dense Hessian: iterate, gradient, direction, G·direction (+ one temporary for coupled groups)
      L.fac_stride *= ncol_max; L.vec_stride *= ncol_max;                     // a coupled group keeps every column's factor and vectors
      if (objective == 1) L.vec_stride += 26LL * T * (nmax + mmax);      // sum-of-norms: warm-start vector + Anderson history (see the kernel)
    } else if (kind == Bin::General || kind == Bin::Wide) {
      const bool wide = kind == Bin::Wide;
      L.kind = LaunchKind::Workgroup; L.wide = wide;
      L.nmax = nmax; L.mmax = mmax; L.nnzA_cap = nnzA; L.nnzB_cap = nnzB;
      lds = general_kernel_lds_bytes(nmax, mmax, nnzA, nnzB, T, true, wide);
      L.vec_in_lds = 1;
      if (lds > kMaxLds) { lds = general_kernel_lds_bytes(nmax, mmax, nnzA, nnzB, T, false, wide); L.vec_in_lds = 0; }
      L.fac_stride = (int64_t)(T + 1 + (wide ? 1 : 0)) * nmax * nmax + (wide ? (int64_t)nmax * mmax : 0);   // wide: + Ã·Q image + dense B̃
      L.vec_stride = 3LL * (T + 1) * nmax;
      L.per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(8, kMaxLds / std::max<int64_t>(lds, 1)));
    } else {
      L.kind = LaunchKind::OneWave;
      int rpl_max = 0;
      // throughput regime (more columns than fit at once): the two T-sized vectors go to a global workspace so that
      // twice as many waves are resident; the latency regime keeps them in LDS (SLS_VEC_GLOBAL / SLS_VEC_LDS: tests / experiments)
      const bool vg = cls < kNumSmallWaveClasses && (K.vec_global || objective == 1 || (merge_cls < 0 && !K.vec_lds));
      L.vec_in_lds = vg ? 0 : 1;
      L.vec_stride = vg ? 2LL * (T + 1) * wave_class(cls).npl : 0;
      if (objective == 1) L.vec_stride += 30LL * T * nm_max;            // sum-of-norms: linear term, y, u, v per (t, variable) + Anderson history (g, F, g of the last step, 2·5 differences; each 2 vectors)
      for (int32_t q : v) {
        const int c = S.subs[q].cls;
        lds = std::max(lds, wave_kernel_lds_bytes(c, T, mcap, capA, capAc, capB, capBc, nm_max, vg));
        rpl_max = std::max(rpl_max, wave_class(c).rpl);
      }
      L.mcap = mcap; L.nm_max = nm_max;
      L.fac_stride = (int64_t)(T + 1) * rpl_max * 64;
      // latency regime: two waves per column (twisted factorisation) when there are far fewer columns than SIMDs
      if (!K.no_twisted && !one_wave_only && !vg && merge_cls >= 0 && cls == merge_cls && cls < kNumSmallWaveClasses && T >= 3 &&
          (int64_t)v.size() <= 2LL * ncu) {
        const int64_t tl = twisted_kernel_lds_bytes(cls, T, mcap, capA, capAc, capB, capBc, nm_max);
        if (tl <= kMaxLds) {
          L.kind = LaunchKind::Twisted; lds = tl;
          // Opt-in (SLS_P_LDS=1): keep the pivot blocks in LDS when the whole column fits in the CU.  It removes the P_k
          // workspace traffic (README: 23.8 MB → ≈0.7 MB per launch) but measured 6 % SLOWER (0.171 vs 0.161 ms): the
          // P_k reads then queue on the same LDS pipe / lgkmcnt as the gathers of the step instead of overlapping on
          // the VMEM path, and 150 GB/s of workspace traffic is far from any HBM limit.  Default = the faster one.
          const int64_t pl_bytes = (int64_t)(T + 1) * nmax * nmax * 8;
          if (K.p_lds && tl + pl_bytes <= kMaxLds) { L.pl_off = (int)tl; lds = tl + pl_bytes; }
          // Round 3: at most one column per CU → FOUR waves per column (sls_twisted4_kernel.hip): each direction's chain wave
          // keeps only Gauss–Jordan + store + sweep, a helper wave on another SIMD builds the next block behind its pivots.
          // NPL = 32 classes (the 8×8 lane grid); SLS_TWISTED4=0 restores the two-wave kernel.
          // OPEN DEFECT of the four-wave kernel, fenced off here (found by the end-of-round fuzz, tools/t4_vs_t2_scan.py,
          // tools/t4_small_T.py): on short horizons (T ≤ 6) columns with small index sets (ñx ≤ 12: members of the 16-lane classes
          // that a one-launch latency plan merges into its 32-lane class) come out with residuals of 1e-8…1e-6 that do not
          // contract, where the two-wave kernel reaches 1e-16 on the same launch (fuzz seeds 11, 65, 290, 297; the same
          // plant and columns are clean from T = 7 on, and the README chain's edge columns — ñx = 11 at T = 29 — always were).
          // Traced (tools/t4_dump_P.py): one diagonal entry of block c+1 whose Schur complement cancels to zero — the
          // elimination form resolves it to δ exactly where the explicit products land on ±1e-6, and the 1/δ entry amplifies the
          // residual's rounding noise into a floor of 1e-7.  Until such a direction is damped, a launch that combines a horizon
          // below 7 (SLS_T4_TMIN) with an index set below 13 (SLS_T4_NMIN) takes the two-wave kernel.  470 fuzz seeds: no status or
          // value difference between the two kernels with the fence.
          int n_least = 1 << 30;
          for (int32_t q : v) n_least = std::min(n_least, S.subs[q].n);
          if (!L.pl_off && wave_class(cls).npl == 32 && (int64_t)v.size() <= (int64_t)ncu && K.twisted4 && (n_least >= K.t4_nmin || T >= K.t4_tmin)) {
            const int64_t t4l = twisted4_kernel_lds_bytes(cls, T, mcap, capA, capAc, capB, capBc, nm_max);
            if (t4l <= kMaxLds) { L.four = true; L.lds_two = (size_t)lds; lds = t4l; }
          }
        }
      }
      L.per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(cls < kNumSmallWaveClasses ? 16 : 8, kMaxLds / std::max<int64_t>(lds, 1)));
      if (L.four) L.per_cu = 1;
      // whole waves per SIMD: a ninth wave on a CU puts three on one SIMD, and a round lasts as long as its slowest wave
      // (chain Nx = 65 536: 29 rounds of 2260 waves 34.2 ms, 32 rounds of 2048 waves → see DESIGN §6)
      if (L.per_cu > 8 && !K.per_cu_any) L.per_cu -= L.per_cu % 4;      // (below two per SIMD every wave counts)
    }
    L.lds = (size_t)lds;
    L.per_cu = std::max(1, std::min(L.per_cu, K.max_per_cu));   // SLS_MAX_PER_CU: experiments
    L.grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)L.nsub, (int64_t)ncu * L.per_cu));
    // Static round-robin kernels (one wave per column): every wave of a full grid does ⌈nsub/grid⌉ columns whether or not
    // the last round is full, so the launch lasts that many rounds anyway — give each wave exactly that many and keep the
    // fewest waves resident (chain-4096: 4074 columns on 2304 slots = 2 rounds; 2037 waves, 8 per CU instead of 9, each
    // SIMD holds 2 waves instead of up to 3).  The tile kernel takes work from a queue and keeps its full grid.
    if (L.big) {
      // a big column's factor slots are tens of MB (ñx = 1024, T = 25: 119 MB): the resident workgroups are capped by memory, the
      // work queue feeds them the rest
      const double per_wg = 8.0 * ((double)L.fac_stride + (double)L.vec_stride) + (double)L.big_stride;
      const int64_t cap = (int64_t)std::max(1.0, (48.0 * 1024 * 1024 * 1024) / per_wg);
      L.grid = (int)std::max<int64_t>(1, std::min<int64_t>(L.grid, cap));
    }
    if (kind == Bin::Wave && objective == 1) out.has_tile = true;          // sum-of-norms: the one-wave kernel draws columns from a queue too
    if (kind == Bin::Wave && objective != 1 && !K.full_grid) {
      const int64_t rounds = ((int64_t)L.nsub + L.grid - 1) / L.grid;
      L.grid = (int)(((int64_t)L.nsub + rounds - 1) / rounds);
    }
    order2.insert(order2.end(), v.begin(), v.end());
    launches.push_back(L);
  };
  for (int c = kNumWaveClasses - 1; c >= 0; --c) add_launch(Bin::Wave, c, bins[c]);     // largest (longest) class first
  add_launch(Bin::General, -1, bins[kNumWaveClasses]);
  add_launch(Bin::Wide, -1, wide_bin);
  for (auto& build : tile_bins) {
    add_launch(Bin::TileGlb, -1, build[kGlb]);
    add_launch(Bin::TileGlb, -1, build[kGlbSmall]);
    add_launch(Bin::TileLds, -1, build[kLds]);
    add_launch(Bin::TileLds, -1, build[kLdsSmall]);
  }
  for (auto& build : tile_bins) add_launch(Bin::TileBig, -1, build[kBig]);
  S.order.swap(order2);
  // A CU-saturating persistent launch leaves no LDS for the workgroups of the other size classes, which could then only
  // start in its tail.  Keep that many workgroup slots free: the small launches run beside it whenever they are dispatched.
  // Submission order: launches of a handful of workgroups (edge classes of a chain: 6–8 columns) go first.  Behind a launch
  // that fills every LDS slot they would wait for its first round to drain and then run alone as the tail of the pass
  // (chain-4096: the three edge classes ended 0.35 ms after the 4074-column launch); submitted first they start at t = 0
  // and the big launch fills in around them.
  // Submission order = critical path first: the launch that outlasts the others takes its slots first and the shorter ones run
  // in the slots its last round leaves idle.  grid-32: the tile kernel (772 columns on 512 slots: its second round uses half of them)
  // alone 4.05 ms, the 252 one-wave columns alone 1.60 ms; submitted wave-first the wave workgroups' 84 KiB of LDS kept
  // every CU at ONE tile workgroup for those 1.6 ms and the pass took the sum, 5.47 ms.
  if (launches.size() > 1 && !K.no_tiny_first) {
    std::stable_sort(launches.begin(), launches.end(), [&](const LaunchSpec& a, const LaunchSpec& b) {
      // the launch holding the longest columns first (random10000_d2: 119 columns of ñx up to 322 take ≈25 ms each — started
      // third they were the tail of the pass: 78 ms against 62), then by total work
      if (a.n_longest != b.n_longest) return a.n_longest > b.n_longest;
      return a.work > b.work;
    });
    if (K.tiny_first)
      std::stable_partition(launches.begin(), launches.end(), [&](const LaunchSpec& L) { return (int64_t)L.grid * 16 <= ncu; });
  }
  if (launches.size() > 1) {
    auto& L0 = launches[0];
    int64_t others = 0; bool fit = true;
    for (size_t li = 1; li < launches.size(); ++li) { others += launches[li].grid; fit = fit && launches[li].lds <= L0.lds; }
    if (fit && L0.kind == LaunchKind::OneWave && (int64_t)L0.grid == (int64_t)ncu * L0.per_cu && others < L0.grid / 4) L0.grid -= (int)others;
  }
  // The four-wave twisted kernel owns a whole CU (256 threads at up to 512 registers): beside another launch — grid-32's four
  // corner columns next to the tile kernel's persistent workgroups — it can only start once a CU has drained completely
  // (rocprof: dispatched at t = 0, finished with the pass).  It is the pure latency regime's kernel: plans with one launch.
  if (launches.size() > 1)
    for (auto& L : launches)
      if (L.four) {
        L.four = false; L.lds = L.lds_two;
        L.per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(16, kMaxLds / std::max<int64_t>((int64_t)L.lds, 1)));
        L.grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)L.nsub, (int64_t)ncu * L.per_cu));
      }
  for (const auto& L : launches)
    if (L.lds > (size_t)kMaxLds) {
      err = "internal: a launch needs " + std::to_string(L.lds) + " B of LDS (160 KiB available)";
      return SLS_EUNSUPPORTED;
    }
  if (one_wave_only)
    for (const auto& L : launches)
      if (L.kind != LaunchKind::OneWave || L.cls >= kNumSmallWaveClasses) {
        err = "SLS_PLAN_MULTIPLIERS: a column's working set is beyond the one-wave kernel's LDS (it would run on another kernel)";
        return SLS_EUNSUPPORTED;
      }
  if (one_wave_only && !out.too_large.empty()) { err = "SLS_PLAN_MULTIPLIERS: a column is beyond every kernel's LDS budget"; return SLS_EUNSUPPORTED; }
  // launches of one execute run CONCURRENTLY: disjoint workspace regions
  for (auto& L : launches) {
    L.fac_stride = (L.fac_stride + 31) / 32 * 32;        // every workgroup's region starts on a 256-B boundary
    L.vec_stride = (L.vec_stride + 31) / 32 * 32;
    L.fac_off = (int64_t)out.fac_doubles; out.fac_doubles += (size_t)L.fac_stride * L.grid;
    if (!L.vec_in_lds) { L.vec_off = (int64_t)out.vec_doubles; out.vec_doubles += (size_t)L.vec_stride * L.grid; }
    if (L.big) { L.big_off = (int64_t)out.big_bytes; out.big_bytes += (size_t)L.big_stride * L.grid; }
  }
  return 0;
}

std::string describe_launch(const LaunchSpec& L) {
  char line[256];
  const WaveClass w = L.cls >= 0 ? wave_class(L.cls) : WaveClass{0, 0};
  if (L.kind == LaunchKind::Tile)
    std::snprintf(line, sizeof line, "h2_column_tile_kernel<%s%s%s> nsub=%d grid=%d block=512 lds=%zu nmax=%d per_cu=%d;", L.mlds ? "block_in_LDS" : "block_in_workspace", L.big ? ",carve_in_workspace" : "", L.gw ? ",dense_hessian_cg" : "", L.nsub, L.grid, L.lds, L.nmax, L.per_cu);
  else if (L.kind == LaunchKind::Workgroup)
    std::snprintf(line, sizeof line, "h2_column_general_kernel%s nsub=%d grid=%d block=256 lds=%zu;", L.wide ? "<wide>" : "", L.nsub, L.grid, L.lds);
  else if (L.kind == LaunchKind::Twisted && L.four)
    std::snprintf(line, sizeof line, "h2_column_twisted4_kernel<%d,%d> nsub=%d grid=%d block=256 lds=%zu;", w.npl, w.rpl, L.nsub, L.grid, L.lds);
  else if (L.kind == LaunchKind::Twisted)
    std::snprintf(line, sizeof line, "h2_column_twisted_kernel<%d,%d,%s> nsub=%d grid=%d block=128 lds=%zu;", w.npl, w.rpl,
                  L.pl_off ? "P_in_LDS" : "P_in_workspace", L.nsub, L.grid, L.lds);
  else
    std::snprintf(line, sizeof line, "h2_column_wave_kernel<%d,%d> nsub=%d grid=%d block=64 lds=%zu;", w.npl, w.rpl, L.nsub, L.grid, L.lds);
  return line;
}

}  // namespace sls
