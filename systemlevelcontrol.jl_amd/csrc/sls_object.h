// sls_object.h — what the objects that evaluate a resident Φ share (closed loop, controller, rollout, margin and its box, norms and
// its covariance): the arena every one of them keeps its tables and buffers in, the gather that brings Φ from mask order into
// the object's own order, the scenario slots of a wave, and the per-scenario plant values of rollout and margin.  DESIGN §3.17.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sls_internal.h"

namespace sls {

// One device allocation per object, laid out in the order of the declarations: tables to upload and buffers the object owns.
// Nothing touches the device before commit; the object that receives the arena owns it and frees it with hipFree.
class Arena {
 public:
  // the room a block of b bytes takes: at least 16 bytes, rounded up to 256
  static size_t al(size_t b) { return (std::max<size_t>(b, 16) + 255) / 256 * 256; }
  // a table to upload; *out is its device copy after commit
  template <class T>
  void table(const std::vector<T>& v, const T** out) { add(v.data(), v.size() * sizeof(T), reinterpret_cast<const void**>(out)); }
  // n elements the object owns, uninitialised; *out after commit
  template <class T>
  void buffer(size_t n, T** out) { add(nullptr, n * sizeof(T), reinterpret_cast<const void**>(const_cast<const T**>(out))); }
  // bytes laid out so far: the offset of the next declaration, and after the last one the size of the arena
  size_t bytes() const { return total_; }
  // hipMalloc on the current device, the uploads (synchronous), the pointers.  On a failure nothing stays allocated, *arena is
  // NULL and the result is hipfail's, with `what_malloc` or `what_upload`.
  int commit(sls_ctx* ctx, void** arena, const char* what_malloc, const char* what_upload);
  // The same layout inside bytes() of device memory the caller owns: the tables, declared first, are staged on the host and go
  // up in ONE synchronous copy.  A failure is hipfail's with `what_upload`.
  int commit_in(sls_ctx* ctx, void* base, const char* what_upload);

 private:
  struct Req { const void* src; size_t bytes; const void** out; };
  void add(const void* src, size_t bytes, const void** out) { reqs_.push_back({src, bytes, out}); total_ += al(bytes); }
  std::vector<Req> reqs_;
  size_t total_ = 0;
};

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
