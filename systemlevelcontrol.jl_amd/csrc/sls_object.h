// sls_object.h — what the objects that evaluate a resident Φ share (closed loop, controller, rollout, margin and its box, norms and
// its covariance): the arena every one of them keeps its tables and buffers in (sls_arena.h), the gather that brings Φ from mask order into
// the object's own order, the scenario slots of a wave, and the per-scenario plant values of rollout and margin.  DESIGN §3.17.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sls_arena.h"
#include "sls_internal.h"

namespace sls {

// vals[k] = values[perm[k]], k < n: Φ from the solve's mask order into the order of an object's table; nothing for n = 0.
// A launch error is recorded on `ctx`.
int launch_gather_phi(sls_ctx* ctx, const double* d_values, const int32_t* d_perm, int64_t n, double* d_vals, hipStream_t stream);

// scenario slots of a wave: the smallest power of two ≥ nscen, at most 64
inline int scenario_slots(int64_t nscen) {
  int scn = 1;
  while (scn < 64 && scn < nscen) scn <<= 1;
  return scn;
}

// the argument checks a plan call with scenarios begins with; `who` is its name, `rest` whether its other pointers are there
template <class Obj>
int check_plan_args(sls_ctx* ctx, const std::string& who, Obj** out, bool rest, int dev_slot, int64_t nscen) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, who + ": null context");
  if (!out || !rest) return fail(ctx, SLS_EINVAL, who + ": null argument");
  *out = nullptr;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, who + ": dev_slot out of range");
  if (nscen < 1) return fail(ctx, SLS_EINVAL, who + ": nscen must be >= 1");
  if (nscen > 65535LL * 64) return fail(ctx, SLS_EUNSUPPORTED, who + ": nscen exceeds 65535 chunks of 64 scenarios");
  return 0;
}

// The values of A and B₂ of every scenario, by rows with the scenario innermost — val[e][s], contiguous along the scenario
// lanes of the kernels that read them.  The caller's arrays are in the CSC nzval order of the plan's patterns; src[e] is the
// CSC position of CSR entry e.
struct PlantEnsemble {
  const int32_t *d_A_src = nullptr, *d_B2_src = nullptr;
  double *d_A_val = nullptr, *d_B2_val = nullptr;
  double* d_stage = nullptr;           // max(nnz(A), nnz(B₂))·nscen doubles: where the host path of set lands
  int64_t nnzA = 0, nnzB = 0, nscen = 0;

  // the refusal of an ensemble whose gather would not fit a grid; `who` is the plan call's name
  static int check_size(sls_ctx* ctx, const std::string& who, size_t nnzA, size_t nnzB, int64_t nscen);
  // the two declarations in an object's arena: the src tables among its tables, then the two value arrays and the staging
  // buffer among its buffers.  lay_out_values returns the bytes of the two value arrays.
  void lay_out_tables(Arena& a, const std::vector<int32_t>& A_src, const std::vector<int32_t>& B2_src);
  size_t lay_out_values(Arena& a, int64_t nscen);
  // every scenario starts from P's values (ones where nzval is NULL): staged like a host-path set, and waited for.  A HIP error
  // is reported with `what`.
  int init_from(sls_ctx* ctx, const sls_plant* P, const char* what);
  // New values for all scenarios (nnz each) or per scenario ([nnz][nscen]); NULL keeps an array.  Device arrays: one gather
  // launch each on `st`, nothing waits.  A host array is copied to the staging buffer on `st` and the call waits for `st`, so
  // that the caller's array is free on return; the gather that empties the buffer is ordered before the next copy by `st`.
  int set(sls_ctx* ctx, hipStream_t st, const double* A_nzval, const double* B2_nzval, int on_device, int per_scenario);
};

}  // namespace sls
