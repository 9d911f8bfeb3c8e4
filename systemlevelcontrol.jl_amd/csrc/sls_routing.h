// sls_routing.h — kernel selection of a plan (pure C++, no HIP): which kernel every column runs on, the launch list with its
// LDS plans, grids and submission order, and the layout of the launches' workspaces.  Host arithmetic over the symbolic
// pass's result, so it is tested without a device (tests/test_host.py: golden launch lists, sanitizer build).
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
int build_launch_list(Symbolic& S, int T, int objective, int ncu, bool force_tile, const RoutingKnobs& knobs, RoutingResult& out,
                      std::string& err);

// one launch as sls_plan_describe prints it
std::string describe_launch(const LaunchSpec& L);

}  // namespace sls
