// sls_partial.hip — which columns a plant update touched, and the launch lists of a run over a subset of the columns
// (sls_plan_track_changes, sls_plan_execute_columns, sls_plan_execute_dirty).
//
// Subproblem q reads the plant only through Ã = A[s_x(q), s_x(q)] and B̃2 = B2[s_x(q), s_u(q)] (SubDesc, sls_device.h).  So a
// change of A[i,j] can move column q only if i, j ∈ s_x(q), and a change of B2[i,k] only if i ∈ s_x(q) and k ∈ s_u(q).
//   changed_entries_kernel   before operator_update_kernel overwrites the old values: a flag per entry whose accepted new value
//                            differs in its bits from the plan's, at the entry's row-order position, and a byte per plant row
//   mark_affected_kernel     one wavefront per subproblem over the flagged rows of s_x(q): dirty[out_index] = 1 on any hit
//   compact_order_kernel     one wavefront per launch: the marked work items of the launch's slice of `order`, order kept
// None of them is on the path of a full execute.  Not measured on their own: a few thousand entries and subproblems each,
// launch-bound at every shape the project benchmarks.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sls_device.h"

namespace sls {

namespace {

constexpr int kChgBlock = 256;

__global__ __launch_bounds__(kChgBlock) void changed_entries_kernel(const ChangedEntriesParams p) {
  const OperatorUpdateParams& u = p.up;
  const int64_t n = u.nnzA + u.nnzB;
  const int64_t stride = (int64_t)gridDim.x * kChgBlock;
  for (int64_t k = (int64_t)blockIdx.x * kChgBlock + threadIdx.x; k < n; k += stride) {
    const bool isA = k < u.nnzA;
    const double* src = isA ? u.newA : u.newB;
    const int64_t j = isA ? k : k - u.nnzA;
    const int64_t at = (isA ? 0 : u.nnzA) + u.row_pos[k];
    bool changed = false;
    if (src) {
      const double v = src[j];
      // the accept rule of operator_update_kernel: finite, and a plan-time zero stays zero
      const bool finite = (v < 0.0 ? -v : v) <= 1.7976931348623157e308;
      const bool accepted = finite && !(u.zero[k] && v != 0.0);
      const double old = (isA ? u.At_val : u.Bt_val)[j];
      changed = accepted && __double_as_longlong(v) != __double_as_longlong(old);   // bits: 0.0 → −0.0 is a change
    }
    p.chg[at] = changed ? 1 : 0;
    if (changed) p.row_chg[(isA ? p.rowA : p.rowB)[j]] = 1;      // same value from every writer
  }
}

// is v in the ascending list a[0 .. n)?
__device__ inline bool in_sorted(const int32_t* __restrict__ a, int n, int32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < n && a[lo] == v;
}

__global__ __launch_bounds__(64) void mark_affected_kernel(const MarkAffectedParams p) {
  const int q = blockIdx.x;
  if (q >= p.nsub) return;                       // uniform over the wavefront; the kernel has no barrier
  const SubDesc sd = p.subs[q];
  const int32_t* sx = p.idx_pool + sd.off_sx;
  const int32_t* su = p.idx_pool + sd.off_su;
  bool hit = false;
  for (int ii = threadIdx.x; ii < sd.n && !hit; ii += 64) {
    const int32_t r = sx[ii];
    if (!p.row_chg[r]) continue;
    for (int32_t e = p.A_rowptr[r]; e < p.A_rowptr[r + 1] && !hit; ++e)
      if (p.chg[e] && in_sorted(sx, sd.n, p.A_colidx[e])) hit = true;
    for (int32_t e = p.B_rowptr[r]; e < p.B_rowptr[r + 1] && !hit; ++e)
      if (p.chg[p.nnzA + e] && in_sorted(su, sd.m, p.B_colidx[e])) hit = true;
  }
  if (hit) p.dirty[sd.out_index] = 1;            // several lanes may store the same byte
}

__global__ __launch_bounds__(64) void compact_order_kernel(const CompactOrderParams p) {
  const int l = blockIdx.x;
  if (l >= p.nlaunch) return;
  const int lane = threadIdx.x;
  const int off = p.launch_tab[3 * l], nsub = p.launch_tab[3 * l + 1];
  const bool groups = p.launch_tab[3 * l + 2] != 0;
  int kept = 0, cols = 0;                        // the same in every lane
  for (int base = 0; base < nsub; base += 64) {
    const int s = base + lane;
    bool keep = false;
    int ncol = 0, q = 0;
    if (s < nsub) {
      q = p.order[off + s];
      const SubDesc sd = p.subs[q];
      ncol = (groups && sd.has_w == 3) ? sd.pad_ : 1;          // a coupled group is one work item: consecutive subproblems
      keep = p.marks[sd.out_index] != 0;
      for (int c = 1; c < ncol && !keep; ++c) keep = p.marks[p.subs[q + c].out_index] != 0;
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int at = off + kept + __popcll(m & ((1ull << lane) - 1ull));
      p.sel_order[at] = q;
      p.sel_pos[at] = s;
    }
    kept += __popcll(m);
    int c = keep ? ncol : 0;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    cols += c;
  }
  if (lane == 0) { p.count[l] = kept; p.count[p.nlaunch + l] = cols; }
}

}  // namespace

hipError_t launch_changed_entries(const ChangedEntriesParams& p, hipStream_t st) {
  const int64_t n = p.up.nnzA + p.up.nnzB;
  if (n <= 0) return hipSuccess;
  const int grid = (int)std::min<int64_t>((n + kChgBlock - 1) / kChgBlock, 1024);
  hipLaunchKernelGGL(changed_entries_kernel, dim3(grid), dim3(kChgBlock), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_mark_affected(const MarkAffectedParams& p, hipStream_t st) {
  if (p.nsub <= 0) return hipSuccess;
  hipLaunchKernelGGL(mark_affected_kernel, dim3(p.nsub), dim3(64), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_compact_order(const CompactOrderParams& p, hipStream_t st) {
  if (p.nlaunch <= 0) return hipSuccess;
  hipLaunchKernelGGL(compact_order_kernel, dim3(p.nlaunch), dim3(64), 0, st, p);
  return hipGetLastError();
}

}  // namespace sls
