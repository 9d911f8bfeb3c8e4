// sls_routing.h — kernel selection of a plan (pure C++, no HIP): which kernel every column runs on, the launch list with its
// LDS plans, grids and submission order, and the layout of the launches' workspaces; with it the rest of plan construction's
// host arithmetic (sls_plan_build.cpp): the solver parameters, the sum-of-norms weights check, the scratch workspace and the
// four-wave pools.  Host arithmetic over the symbolic pass's result, so it is tested without a device (tests/test_host.py:
// golden launch lists, sanitizer build).
#pragma once
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "sls_symbolic.h"

namespace sls {

constexpr int kMaxLds = 160 * 1024;

enum class LaunchKind { OneWave, Workgroup, Twisted, Tile };   // the kernel family a launch executes

// Everything kernel selection decides about one launch (sls_plan adds the stream and event it runs on).
struct LaunchSpec {
  LaunchKind kind = LaunchKind::OneWave;
  int cls = -1, order_off = 0, nsub = 0, grid = 1, per_cu = 1;
  size_t lds = 0;
  int64_t fac_stride = 0, vec_stride = 0, fac_off = 0, vec_off = 0;
  int mcap = 0, nm_max = 0, pl_off = 0;                       // wave kernels
  int nmax = 0, mmax = 0, nnzA_cap = 0, nnzB_cap = 0, vec_in_lds = 0;   // general kernel
  bool wide = false;                                // general kernel, ñx 97..144: Ã·Q image in the global workspace
  bool mlds = false;                                // tile kernel: block being inverted lives in LDS
  int oth_rows = 16;                                // tile kernel: rows of the Ã·Q image of the block build held in LDS
  bool two_per_cu = false;                          // tile kernel: 4-waves-per-SIMD build, two workgroups per CU (SLS_TILE_WPE overrides)
  bool gw = false;                                  // tile kernel: the build with the projected-CG loop (dense cost Hessians)
  bool four = false;                                // twisted kernel: four waves per column (chain + helper wave per direction)
  size_t lds_two = 0;                               // … LDS of the two-wave kernel for the same launch (used when the plan has other launches)
  bool big = false;                                 // tile kernel: the carve (panels, lists, staging) in a global per-workgroup buffer, not LDS
  int64_t big_stride = 0, big_off = 0;              // … bytes per workgroup / offset of the launch's region
  double work = 0.0;                                // Σ ñx³ over the launch's columns (submission order)
  int n_longest = 0;                                // largest ñx of the launch: its longest column
};

// The diagnostic knobs that steer kernel selection (dead unless SLS_LAB=1), read once per plan.
struct RoutingKnobs {
  bool force_general = false;      // SLS_FORCE_GENERAL=1
  bool wave64 = false;             // SLS_WAVE64=1: the round-1 routing of ñx 33…64
  char tile = 0;                   // SLS_TILE: '0' never, 'l' (large) only what the workgroup kernel cannot hold
  char tile_big = 0;               // SLS_TILE_BIG: '0' SLS_COL_UNSUPPORTED beyond LDS, 'a' (all) every tile column through the big variant
  bool tile_global = false;        // SLS_TILE_GLOBAL=1: no LDS-resident block
  int tile_lds_maxnt = 6;          // SLS_TILE_LDS_MAXNT
  bool son_tile = false;           // SLS_SON_TILE=1
  bool absorb = true;              // SLS_ABSORB=0 turns it off
  bool tile_one_per_cu = false;    // SLS_TILE_ONE_PER_CU=1
  int gw_two = -1;                 // SLS_GW_TWO: -1 unset (the objective decides), else 0 / 1
  bool vec_global = false;         // SLS_VEC_GLOBAL=1
  bool vec_lds = false;            // SLS_VEC_LDS=1
  bool no_twisted = false;         // SLS_NO_TWISTED=1
  bool p_lds = false;              // SLS_P_LDS=1
  bool twisted4 = true;            // SLS_TWISTED4=0 turns it off
  int t4_nmin = 13, t4_tmin = 7;   // SLS_T4_NMIN, SLS_T4_TMIN: the four-wave fence
  bool per_cu_any = false;         // SLS_PER_CU_ANY (set to anything)
  int max_per_cu = INT_MAX;        // SLS_MAX_PER_CU
  bool full_grid = false;          // SLS_FULL_GRID (set to anything)
  bool no_tiny_first = false;      // SLS_NO_TINY_FIRST (set to anything)
  bool tiny_first = false;         // SLS_TINY_FIRST (set to anything)
  int tile_wpe = -1;               // SLS_TILE_WPE: -1 unset, else 1 for "4" (the 4-waves-per-SIMD build whatever the grid) / 0
  static RoutingKnobs from_env();
};

struct RoutingResult {
  std::vector<LaunchSpec> launches;          // submission order; strides rounded, workspace offsets assigned
  std::vector<int32_t> too_large;            // subproblems beyond every kernel's LDS budget: never launched
  bool has_tile = false;                     // some launch draws its columns from a work queue
  size_t fac_doubles = 0, vec_doubles = 0, big_bytes = 0;   // totals of the launches' disjoint workspace regions
};

// Bins the subproblems by size class and builds the launch list.  Rewrites S.order (launch by launch) and S.subs[].cls (the
// class a column runs in, -1 outside the one-wave classes).  0, or SLS_EUNSUPPORTED with `err` filled.
// one_wave_only (plans built with SLS_PLAN_MULTIPLIERS): every column on the one-wave kernel of the 16- and 32-lane classes — no
// two-wave and no four-wave launch; SLS_EUNSUPPORTED, naming the reason, when some column cannot run there.
int build_launch_list(Symbolic& S, int T, int objective, int ncu, bool force_tile, const RoutingKnobs& knobs, RoutingResult& out,
                      std::string& err, bool one_wave_only = false);

// one launch as sls_plan_describe prints it
std::string describe_launch(const LaunchSpec& L);

// The solver's parameters and their diagnostic knobs (dead unless SLS_LAB=1), read once per plan.
struct SolverKnobs {
  double delta_rel = 1e-12, tol = 1e-12, tol_ok = 1e-9;   // SLS_DELTA_REL, SLS_TOL; δ scan: tools/iters_hist.py, DESIGN.md §3
  int max_iters = 8;               // SLS_MAX_ITERS (≥ 1), experiments only
  double stag = 0.5;               // SLS_STAG, experiments only
  int son_maxit = 4000;            // SLS_SON_MAXIT (≥ 1)
  double son_tol = 1e-9;           // SLS_SON_TOL
  int son_anderson = 1;            // SLS_SON_ANDERSON=0 turns it off
  int son_aa_start = 20;           // SLS_SON_AA_START (≥ 0)
  double delta_first = 1e-15;      // SLS_DELTA_FIRST: one-wave (throughput) kernel only; 0 = single attempt with delta_rel
  int max_iters_slow = 48;         // SLS_MAX_ITERS_SLOW (≥ 0); 0: rounds 1–2 rule
  int dbg_level = 0;               // SLS_PHASE_TIMERS (≥ 1 when set): the plan then holds the phase counters
  int knock_out = 0;               // SLS_KNOCK_OUT
  bool t4_prestatic = true;        // SLS_T4_PRESTATIC=0: no plan-time static blocks
  static SolverKnobs from_env();
  void apply(KernelParams& kp) const;
};

// SLS_SOLVE_SUM_OF_NORMS takes diagonal weights without feed-through only (a dense Hessian or a D11 column would change the
// cone structure): 0, or SLS_EUNSUPPORTED with `err` filled.
int check_sum_of_norms_weights(const Symbolic& S, std::string& err);

// The scratch workspace of a plan, from the totals of kernel selection: the factor workspace at its start, the vector workspace
// vec_off doubles in (behind the factor doubles rounded up to 32), the big launches' carve buffers big_off bytes in.
struct ScratchLayout { size_t bytes = 0, vec_off = 0, big_off = 0; };
ScratchLayout scratch_layout(size_t fac_doubles, size_t vec_doubles, size_t big_bytes);

// The pools of the four-wave launches (layouts: sls_device.h).  A launch has at most one column per compute unit, a column
// (T + 1) slots of 3 or 5 KiB: the README chain takes 5.3 MiB, 256 columns at T = 29 take 23 MiB.  Beyond the budget (256
// columns: horizons past 84 in the three-tile classes, past 50 in the four-tile ones) the plan keeps no pool of static blocks
// and its launches use the rebuild instantiation.  The setup images (15 KiB a column on the README chain: 0.9 MiB) belong to
// the same decision and the same budget.
constexpr int64_t kT4StaticBudget = 64ll << 20;   // bytes of plan-time static blocks a plan may hold
struct T4Slot {                          // where a four-wave launch's columns sit in the pools
  int64_t t4_off = 0;                    // its first record
  int64_t t4s_off = 0, t4s_stride = 0;   // its first double among the static blocks, doubles per column
  int64_t t4i_off = 0, t4i_stride = 0;   // … and among the setup images
};
struct T4Pools {
  std::vector<T4Slot> slots;             // one per launch (zeros for the others)
  int64_t records = 0, static_doubles = 0, image_doubles = 0;
  bool keep_static = false;              // static blocks and images are kept: within the budget and not SLS_T4_PRESTATIC=0
};
T4Pools t4_pool_layout(const std::vector<LaunchSpec>& launches, int T, bool prestatic);

}  // namespace sls
