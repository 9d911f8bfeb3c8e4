// sls_plan.h — the resident plan as the units behind the C ABI see it: sls_plan_build.cpp builds and destroys it, sls_api.cpp runs
// and reads it, sls_plan_update.cpp (updates and partial re-solves), sls_dropin.cpp (the one-shot calls), sls_symbolic_device.cpp
// (the device-resident symbolic route, which ends in plan_finish) and sls_debug.cpp (include/sls_mi355x_debug.h) are its clients.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "sls_internal.h"
#include "sls_routing.h"
#include "sls_symbolic.h"

namespace sls {
constexpr int kEventPool = 64;
}  // namespace sls

struct sls_plan {
  sls_ctx* ctx = nullptr;
  int dev = 0;
  int slot = 0;
  bool streams_borrowed = false, scratch_borrowed = false, arena_borrowed = false, stream_external = false, ltab_borrowed = false;
  hipEvent_t ev_batch = nullptr, ev_batch_done = nullptr;     // sls_plan_execute_batch fork / join edges
  void* own_scratch = nullptr;
  sls::Symbolic sym;       // host copy (pools are cleared after upload except what download needs; its operator values are the plan-time ones)
  sls_plan_info info{};
  hipStream_t stream = nullptr;
  // device buffers
  std::vector<void*> dev_allocs;
  sls::KernelParams kp{};  // dest_pool / out are patched per execute
  const int32_t* d_dest = nullptr;
  const int32_t* d_pdest = nullptr;
  int32_t* d_counters = nullptr;      // one work-queue counter per launch (tile kernel)
  unsigned char* d_big = nullptr;     // big tile launches: their carve buffers (inside the scratch workspace)
  bool has_tile = false;
  // Prepared records of the four-wave columns (twisted4_prepare_kernel, layout: sls_device.h), written in plan_finish.
  // They hold index lists AND the gathered values of A / B2, taken from the plan's own copy of the operator:
  // sls_plan_update_plant reruns the kernel behind every change of that copy.
  unsigned char* d_t4 = nullptr;
  int64_t t4_stride = 0, t4_records = 0;
  // The static blocks S_k of the same columns (layout: sls_device.h, twisted4_static_doubles), written by the same kernel from
  // the same copy.  NULL — the launches rebuild the blocks themselves — when the pool would exceed kT4StaticBudget or with
  // SLS_T4_PRESTATIC=0 (lab mode).
  double* d_t4s = nullptr;
  int64_t t4s_doubles = 0;
  // The setup images (Ã's dense image and the weight table Wx, sls_device.h: twisted4_image_doubles) of the same columns, from
  // the same kernel; kept exactly when d_t4s is, and counted in the same budget.
  double* d_t4i = nullptr;
  int64_t t4i_doubles = 0;
  // what kernel selection decided + where a four-wave launch's columns sit in d_t4, d_t4s, d_t4i + what the launch runs on
  struct Launch : sls::LaunchSpec, sls::T4Slot {
    explicit Launch(const sls::LaunchSpec& spec) : sls::LaunchSpec(spec) {}
    hipStream_t stream = nullptr;      // aux stream (launch 0 runs on the caller's stream)
    hipEvent_t done = nullptr;
  };
  std::vector<Launch> launches;
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_done = nullptr;         // recorded on the caller's stream at the end of an execute that the event pool could not time
  hipEvent_t last_done = nullptr;       // the end of the last execute: its ev_stop (timed) or ev_done (untimed); what status reads and downloads wait for
  // An execute that enqueues one solve kernel and nothing else, behind an execute still in flight (one_kernel_run), binds those
  // events to the kernel's own dispatch (LaunchEvents, sls_launch.h) instead of recording them around it; SLS_EXEC_MARKERS=1
  // (lab mode, read when the plan is built) keeps the records everywhere.
  bool exec_markers = false;
  // event timing
  hipEvent_t ev_start[sls::kEventPool], ev_stop[sls::kEventPool];
  int ev_used = 0;
  double ev_acc_ms = 0.0;
  int64_t ev_acc_n = 0;
  bool events_ok = false;
  sls::pool_vec<double> host_stage; // D2H staging (small Φ only)
  std::vector<int32_t> too_large_subs;  // subproblems beyond every kernel's LDS budget: never launched, status SLS_COL_UNSUPPORTED
  std::vector<int32_t> status_init;     // initial content of the device status words
  int64_t gbeg = 0, gend = 0, ngroups_in = 0;   // the shard of the caller's group list this plan covers
  sls_plan* refine = nullptr;           // sls_plan_refine: the near-singular groups once more on the tile kernel, run after every execute
  std::vector<int64_t> refine_dst;      // subproblem of this plan each subproblem of `refine` replaces
  int64_t info_unsupported = 0;
  // objective evaluation (sls_plan_objective): the records of Symbolic::obj_pool, the work list of the general build and the
  // plan-owned result buffer of sls_plan_fetch_objective (n_subproblems values, then the total)
  const double* d_obj = nullptr;
  const int32_t* d_gen = nullptr;
  double* d_colobj = nullptr;
  std::vector<int32_t> obj_gen;
  int obj_lds_doubles = 0;
  // operator update (sls_plan_update_plant): the value map and plan-time-zero marks (host copy: the host path's check), their
  // device copies, a staging array for host values (nnzA + nnzB doubles), the refusal counter of the device path and the end
  // of the last update on the stream it was enqueued on
  sls::OperatorValueMap opmap;
  const int32_t* d_upd_pos = nullptr;
  const uint8_t* d_upd_zero = nullptr;
  double* d_upd_stage = nullptr;
  unsigned long long* d_upd_rejected = nullptr;
  hipEvent_t ev_upd = nullptr;
  bool upd_recorded = false;
  // weights update (sls_plan_update_weights), only in a plan built with SLS_PLAN_WEIGHTS_UPDATABLE (sym.wu holds
  // the host copies the host path checks against): b² per subproblem, the value rule's scale and the ridge per variable (NULL:
  // none), the diagonals the plan holds now, a staging array for host values (Nx + Nu doubles each) and the refusal counter.
  // An update records ev_upd like the operator update: both are "the plan's last update" to everything that waits for one.
  const double* d_w_b2 = nullptr;
  const double* d_w_owner = nullptr;
  const double* d_w_ridge = nullptr;
  double* d_w_diag = nullptr;
  double* d_w_stage = nullptr;
  unsigned long long* d_w_rejected = nullptr;
  bool w_upd_recorded = false;
  // partial re-solve (sls_plan_execute_columns / _dirty, sls_plan_track_changes): one device allocation made by
  // the first of those calls (partial_ensure) — a plan that never uses them holds none of it and reports the same
  // workspace_bytes.  Layouts: sls_device.h (ChangedEntriesParams, MarkAffectedParams, CompactOrderParams).
  struct Partial {
    bool ready = false, track = false;
    uint8_t* dirty = nullptr;         // [nsub] marks of the tracked updates
    uint8_t* marks = nullptr;         // [nsub] the list of an sls_plan_execute_columns call
    uint8_t* chg = nullptr;           // [nnzA + nnzB]
    uint8_t* row_chg = nullptr;       // [Nx]
    int32_t* sel_order = nullptr;     // [order entries]
    int32_t* sel_pos = nullptr;
    int32_t* count = nullptr;         // [2 · launches]
    const int32_t* launch_tab = nullptr;   // [launches][3]
    std::vector<int32_t> h_count;
    std::vector<uint8_t> h_marks;
  } part;
  // achievability residual (sls_plan_residual): the halo lists, the subproblems' global columns and the plan-owned
  // result buffer of sls_plan_fetch_residual (three arrays of n_subproblems values, then the two totals) — one device allocation
  // made by the first call (residual_ensure), not counted in workspace_bytes
  struct Residual {
    bool ready = false;
    const int32_t* sub_col = nullptr;
    const int64_t* halo_ptr = nullptr;
    const int32_t* halo_rows = nullptr;
    double* out = nullptr;            // [3 · nsub + 2]
  } resid;
  // multipliers and gradient (SLS_PLAN_MULTIPLIERS; sls_plan_gradient).  d_mu — an allocation of its own, made
  // with the plan, n_subproblems slots of mu_slot_doubles(T) — is kp.mu of every execute; the rest is one device allocation
  // made by the first gradient call (gradient_ensure).  Neither is counted in workspace_bytes.  Layouts: sls_gradient.h.
  struct Gradient {
    double* d_mu = nullptr;
    bool executed = false;            // some execute has written multipliers
    bool ready = false;
    int lds_doubles = 0;
    int64_t nnzA = 0, nnzB = 0;
    const uint8_t* b_zero = nullptr;
    const int64_t* ent_ptr = nullptr;  const int32_t* ent = nullptr;
    const int64_t* inv_ptr = nullptr;  const int64_t* inv_slot = nullptr;
    const int64_t* w_base = nullptr;   const int64_t* winv_ptr = nullptr;  const int64_t* winv_slot = nullptr;
    double* contrib = nullptr;        // one per listed entry
    double* wcontrib = nullptr;       // Σ(ñx+ñu), plans with updatable weights only
    double* col_weight = nullptr;     // [nsub] staging of sls_plan_fetch_gradient's host weights
    double* out = nullptr;            // [nnzA + nnzB + Nx + Nu] results of sls_plan_fetch_gradient
  } grad;
};

namespace sls {

// want_packed = false (the one-device drop-in call, which only ever runs packed = 0) skips the packed numbering on the host
// and its 4 B/variable table on the device.  Everything that steers a plan's construction is an explicit argument (no
// mutable context state, no environment writes): a flag left on by an early return would silently re-route later plans.
struct PlanOpts {
  bool force_tile = false;                          // every column on the tile kernel (the refinement pass)
  const std::vector<int64_t>* pk_override = nullptr; // with force_tile: packed bases of the subproblems inside the refined plan's packed array
  int host_tables = -1;                             // mask / destination tables: 1 built on the host, 0 expanded on the device, -1 = SLS_HOST_TABLES decides
  bool multipliers = false;                         // SLS_PLAN_MULTIPLIERS: every column on the one-wave kernel, which exports λ
};

// sls_api.cpp
double now_s();
// SLS_DEBUG_TIMING: the time since the last call (or since construction) to stderr, as "[prefix] what          1.234 ms"
struct DebugTicker {
  const char* prefix; int width; bool on; double last;
  DebugTicker(const char* prefix_, int width_) : prefix(prefix_), width(width_), on(sls_knob("SLS_DEBUG_TIMING") != nullptr), last(now_s()) {}
  void operator()(const char* what) {
    if (!on) return;
    const double n = now_s();
    std::fprintf(stderr, "[%s] %-*s %8.3f ms\n", prefix, width, what, 1e3 * (n - last));
    last = n;
  }
};
// sls_plan_build.cpp
int plan_create(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t group_begin, int64_t group_end,
                bool want_packed, const PlanOpts& opt, sls_plan** plan_out);
struct DeviceTables {            // sls_h2_sf_plan_localized (sls_symbolic_device.cpp): tables built on the device, owned by the plan
  const int32_t* d_idx = nullptr; const uint64_t* d_cmask = nullptr;
  const int32_t* d_cbase = nullptr; const int64_t* d_coff = nullptr;
};
// Second half of plan creation, shared by plan_create (host symbolic pass) and sls_h2_sf_plan_localized: kernel selection, launch list,
// uploads, workspaces.  `dt` != NULL: index sets and compact tables are used where they sit on the device.  Owns `pl`: a failure destroys it.
int plan_finish(sls_ctx* ctx, int dev_slot, const sls_dims* dims, sls_plan* pl, double t0, bool want_packed, const PlanOpts& opt,
                const DeviceTables* dt, sls_plan** plan_out);
// sls_api.cpp (what sls_plan_update.cpp needs of it: wait_plan_done, enqueue_launches)
// Host waits for the plan's last execute (and for nothing else on the device: a status read or a download must not stall on
// a collective or on another plan running on some other stream).
int wait_plan_done(sls_plan* pl);
// A run over a subset of the columns (sls_plan_execute_columns): the compacted order of compact_order_kernel, laid out like the
// plan's own order, with the host's copy of the per-launch counts.
struct SelectedRun {
  const int32_t* order;     // device
  const int32_t* pos;       // device: position of each kept item in its launch (the four-wave records are indexed by it)
  const int32_t* count;     // host: work items kept per launch
};
// The launches of one execute on the caller's stream `st`: launch 0 there, the others on plan-owned streams that fork from /
// join back into it (event edges only; nothing blocks the host).  sel = NULL: every launch in full.  Otherwise the same kernels,
// LDS plans, workspaces and launch parameters over the kept items of each launch; a launch that keeps none is skipped.
// `ev` != NULL: the events go to the kernel's dispatch; only for a run of one kernel (one_kernel_run).
int enqueue_launches(sls_plan* plan, const KernelParams& kp, hipStream_t st, const SelectedRun* sel, const LaunchEvents* ev = nullptr);
// Whether a run (sel = NULL: a full execute) may bind its events to the dispatch: it enqueues exactly one kernel, the plan does
// not ask for markers (exec_markers), `st` is not being captured into a graph, and — a full execute — the plan's last execute is
// still in flight (a caller that waits for every execute keeps the markers: DESIGN §6, "One launch, no markers").
bool one_kernel_run(const sls_plan* plan, hipStream_t st, const SelectedRun* sel);
// sls_plan_build.cpp: the prepared records of every four-wave launch of the plan, from the operator values the plan holds now
hipError_t launch_twisted4_prepares(sls_plan* pl, hipStream_t stream);
// sls_api.cpp: the plan's own status words, without those of an attached refinement (sls_plan_fetch_status merges the two)
int fetch_status_raw(sls_plan* plan, int32_t* col_status, double* residual, int32_t* iters);
// sls_plan_build.cpp: the groups select_refinement_groups (sls_dropin_host.h) names get a second plan on the tile kernel (PlanOpts::force_tile), run
// into the same device array after the first and attached to `pl`, so that later executes and status reads include it; stt /
// res / its come back merged.  Waits for `stream`; costs one status read when nothing qualifies.
int attach_refinement(sls_plan* pl, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                      int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, hipStream_t stream, double* d_values,
                      int64_t* n_refined, std::vector<int32_t>& stt, std::vector<double>& res, std::vector<int32_t>& its, int packed);

}  // namespace sls
