// sls_internal.h — what the translation units behind include/sls_mi355x.h share: the context object, error plumbing, the slot's
// pinned staging paths (host → device, device → host, the download ring) and the launchers of the .hip units.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_device.h"
#include "sls_launch.h"
#include "sls_objective.h"
#include "sls_gradient.h"
#include "sls_residual.h"

struct sls_ctx {
  std::vector<int> devs;
  std::vector<int> ncu;
  std::string err;
  uint32_t flags = 0;
  std::vector<double> ridge_x, ridge_u;   // sls_set_ridge (empty = none)
  // sls_ctx_want_objective: the one-shot calls evaluate every column's objective before their download and leave it here
  bool want_objective = false;
  int obj_state = 0;                      // 0: nothing to report, 1: last_objective / last_total valid, 2: the last call summed layers
  std::vector<double> last_objective;     // col_status order
  double last_total = 0.0;
  // Per device slot: streams and the big scratch workspace are created once and lent to plans (hipStreamCreate costs
  // ≈4 ms and a GB-sized hipMalloc ≈10 ms on this stack — more than a whole README solve).  One context is used by one
  // thread at a time (header), so a simple "in use" flag is enough; a second concurrent plan gets its own.
  struct Slot {
    std::vector<hipStream_t> streams;   // [0] main, [1..] aux
    hipStream_t refine_stream = nullptr; // main stream of the refinement plan of sls_h2_sf_solve (it lives beside the main plan)
    std::vector<hipStream_t> streams_lo; // aux streams of the lowest priority (launches of a handful of workgroups)
    int streams_in_use = 0;
    void* scratch = nullptr; size_t scratch_bytes = 0; bool scratch_in_use = false;
    void* arena = nullptr; size_t arena_bytes = 0; bool arena_in_use = false;      // plan tables (one-shot calls: same size every time)
    void* ltab = nullptr; size_t ltab_bytes = 0; bool ltab_in_use = false;         // device-built tables of the localized route (same idea)
    // pinned staging ring of the download (sls_plan_download): kDlLanes lanes, each its own stream and pinned chunk
    void* pinned = nullptr; size_t pinned_bytes = 0;
    // An update leaves an asynchronous H2D copy reading the pinned buffer (pinned_read_until): the next user waits for this event first.
    // Plain state like the "in use" flags above: it relies on the same rule, one thread at a time per context.
    hipEvent_t pinned_busy = nullptr; bool pinned_pending = false;
    std::vector<hipStream_t> dl_streams;
  };
  std::vector<Slot> slots;
};

namespace sls {
// record the message on the context (and globally, for sls_last_error(NULL)) and hand back `code`
int fail(sls_ctx* ctx, int code, const std::string& msg);
int hipfail(sls_ctx* ctx, hipError_t e, const char* what);
// a plan / loop object may outlive its context (host-language GC order): checked before touching it
bool ctx_is_live(const sls_ctx* ctx);
// The context slot's pinned staging memory (created on first use, 8 MiB): nullptr when unavailable or too small.  Waits first
// for an asynchronous H2D copy that still reads it (Slot::pinned_pending); whoever has enqueued such a copy on `st` says "the
// buffer is read until here" with pinned_read_until: nothing else sets Slot::pinned_busy and Slot::pinned_pending.
unsigned char* slot_pinned(sls_ctx* ctx, int slot, size_t bytes);
int pinned_read_until(sls_ctx* ctx, int slot, hipStream_t st);
// Host values to a device staging array on `st`: a → d_stage[0, na), b → d_stage[na, na + nb); a NULL array, or one of length 0,
// enqueues nothing.  Through the pinned buffer when it takes na + nb doubles; else from the caller's arrays, and `st` is waited for.
int stage_to_device(sls_ctx* ctx, int slot, hipStream_t st, double* d_stage, const double* a, size_t na, const double* b, size_t nb);
// Device bytes to the host on `st`, which is waited for: through the pinned buffer when it fits, else straight into `dst`.
int fetch_to_host(sls_ctx* ctx, int slot, hipStream_t st, void* dst, const void* d_src, size_t bytes);
// Device → host copy of a flat array of 8-byte elements into the caller's pageable slices (slice i = elements [beg[i], beg[i+1]) →
// ptrs[i]) through the slot's pinned ring.  0, a negative error, or 1 when the ring is not available (the caller falls back).
int pinned_download(sls_ctx* ctx, int slot, int dev, const void* d_src, const std::vector<int64_t>& beg, const std::vector<void*>& ptrs);
// the launchers of the .hip units
hipError_t launch_general(const KernelParams& p, int grid, size_t lds_bytes, hipStream_t stream, bool wide, const LaunchEvents* ev = nullptr);
hipError_t launch_scatter(const double* src, const int64_t* idx, int64_t n, double* dst, hipStream_t stream);
hipError_t launch_wave(int cls, const KernelParams& p, int grid, size_t lds_bytes, hipStream_t stream, const LaunchEvents* ev = nullptr);
hipError_t launch_twisted(int cls, const KernelParams& p, int grid, size_t lds_bytes, hipStream_t stream, const LaunchEvents* ev = nullptr);
hipError_t launch_twisted4(int cls, const KernelParams& p, int grid, size_t lds_bytes, hipStream_t stream, const LaunchEvents* ev = nullptr);
hipError_t launch_twisted4_prepare(int cls, const KernelParams& p, unsigned char* pool, hipStream_t stream);
hipError_t launch_tile(const KernelParams& p, int grid, size_t lds_bytes, hipStream_t stream, bool mlds, bool two_per_cu,
                       bool general_weights, bool big, const LaunchEvents* ev = nullptr);
hipError_t launch_expand_tables(const SubDesc* subs, int nsub, int T, const uint64_t* cmask, const int32_t* cbase, const int64_t* coff,
                                uint8_t* mask_pool, int32_t* dest_pool, hipStream_t stream);
hipError_t launch_mask_levels(const MaskParams& p, bool fill, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t launch_index_sets(const IndexSetParams& p, bool fill, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t launch_column_tables(const ColumnTableParams& p, bool fill, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t launch_level_prefix(const int32_t* cntx, const int32_t* cntu, int Nx, int K1, int64_t* prex, int64_t* preu, int64_t* totx,
                               int64_t* totu, hipStream_t stream);
hipError_t launch_objective(const ObjectiveParams& p, int lds_doubles, double* d_total, hipStream_t stream);
hipError_t launch_residual(const ResidualParams& p, double* d_totals, hipStream_t stream);
hipError_t launch_gradient(const GradientParams& p, int lds_doubles, hipStream_t stream);
hipError_t launch_tile_invert(const double* d_A, int n, double* d_ws, double* d_out, bool mlds, hipStream_t stream);
hipError_t launch_operator_update(const OperatorUpdateParams& p, hipStream_t stream);
hipError_t launch_weights_update(const WeightsUpdateParams& p, hipStream_t stream);
// sls_partial.hip: the entries an update changes, the subproblems they touch, the compacted launch lists of a selected run
hipError_t launch_changed_entries(const ChangedEntriesParams& p, hipStream_t stream);
hipError_t launch_mark_affected(const MarkAffectedParams& p, hipStream_t stream);
hipError_t launch_compact_order(const CompactOrderParams& p, hipStream_t stream);
}  // namespace sls

#define HIPCHK(ctx, call)                                        \
  do {                                                           \
    hipError_t e__ = (call);                                     \
    if (e__ != hipSuccess) return sls::hipfail(ctx, e__, #call); \
  } while (0)
