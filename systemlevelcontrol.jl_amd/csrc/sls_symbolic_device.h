// sls_symbolic_device.h — the LDS list plan of one wave of the three device symbolic passes (sls_masks.hip), shared by their host
// drivers (sls_symbolic_device.cpp) and the kernels.  Pure C++, no HIP (tests/host_sanitize/sanitize_symbolic.cpp).  A wave keeps a
// fixed part — two bitmaps (states, inputs), for the tables kernel also level starts, regularity counters and the staged schedule —
// and lists of `cap` entries: the count pass starts at a first capacity and doubles it while a list overflows, up to what LDS holds.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>

#include "sls_routing.h"

namespace sls {

constexpr int kMaskCap0 = 1024;          // first capacities of the lists
constexpr int kIndexCap0 = 1024;
constexpr int kTablesCap0 = 2048;
constexpr int kMaskEntryBytes = 12;      // bytes per unit of capacity: three level lists (current, next, actuators)
constexpr int kIndexEntryBytes = 4;      // one list
constexpr int kTablesEntryBytes = 8;     // two level pools
constexpr int kLevelStarts = 68;         // tables kernel: level starts per pool (KL + 2 ≤ 64 in use)
constexpr int kBitmapLimit = 96 * 1024;  // fixed part beyond which the passes refuse (Nx ≈ 7e5)

struct ListPlan {                        // cap0 = min(first capacity, cap_limit)
  int64_t fixed_bytes; int entry_bytes, cap0, cap_limit;
  bool fits() const { return fixed_bytes <= kBitmapLimit; }
};
// fixed part = the two bitmaps + `extra` bytes; no list is longer than `longest`
inline ListPlan make_list_plan(int64_t Nx, int64_t Nu, int64_t extra, int entry_bytes, int first_cap, int64_t longest) {
  const int64_t fixed_bytes = ((Nx + 31) / 32 + (std::max<int64_t>(Nu, 1) + 31) / 32) * 4 + extra;
  const int cap_limit = (int)std::min<int64_t>(longest, (kMaxLds - fixed_bytes) / entry_bytes);
  return ListPlan{fixed_bytes, entry_bytes, std::min(cap_limit, first_cap), cap_limit};
}
// a level or an index set holds at most max(Nx, Nu) entries; a pool of the tables kernel holds the levels of one column back to back
inline ListPlan mask_list_plan(int64_t Nx, int64_t Nu) { return make_list_plan(Nx, Nu, 0, kMaskEntryBytes, kMaskCap0, std::max(Nx, Nu)); }
inline ListPlan index_list_plan(int64_t Nx, int64_t Nu) { return make_list_plan(Nx, Nu, 0, kIndexEntryBytes, kIndexCap0, std::max(Nx, Nu)); }
inline ListPlan tables_list_plan(int64_t Nx, int64_t Nu, int64_t T) {
  return make_list_plan(Nx, Nu, 2 * kLevelStarts * 4 + 4 * T * 4, kTablesEntryBytes, kTablesCap0, INT_MAX);
}

// the launch of a pass at capacity `cap`: LDS bytes of a wave, waves per CU (1…8, by LDS), grid = min(Nx, CUs · per_cu)
struct ListLaunch { int cap; size_t lds; int per_cu, grid; };
inline ListLaunch list_launch(const ListPlan& p, int cap, int ncu, int64_t Nx) {
  const size_t lds = (size_t)p.fixed_bytes + (size_t)p.entry_bytes * (size_t)cap;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)kMaxLds / std::max<size_t>(lds, 1)));
  return ListLaunch{cap, lds, per_cu, (int)std::min<int64_t>(Nx, (int64_t)ncu * per_cu)};
}

}  // namespace sls
