// sls_rollout.h — streaming closed-loop rollout of a resident Φ against an ensemble of plants (pure C++, no HIP).
//
// Steps are numbered k = 0, 1, … since the last reset, as in sls_controller.h.  Scenario s has its own VALUES of A and B₂ on the
// shared non-zero patterns; B₁ and Φ are shared by all scenarios.  Step k:
//     ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
//     u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
//     β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}
//     x_{k+1} = A⁽ˢ⁾·x_k + B₁·w_k + B₂⁽ˢ⁾·u_k
//     J⁽ˢ⁾   += Σ_i (q_i·x_k[i])² + Σ_j (r_j·u_k[j])²         peak_x⁽ˢ⁾ = max(peak_x⁽ˢ⁾, max_i |x_k[i]|), peak_u likewise
// x_0 comes from the reset (default 0; a non-zero x_0 acts as a disturbance at time 0: ŵ_0 = x_0).  After K steps J and the peaks
// cover k = 0 … K−1; the current state x_K is not counted yet.  With the design plant, x_0 = 0 and one run these are the rows of
// sls_closed_loop_run: row k of the simulator's x, u is step k here.
//
// The step is closed_loop_step_kernel (sls_closed_loop.hip) restated on the controller's ring: the wave of state row i evaluates
// β_{k+1}[i], every u_k[j] its B₂ row references, the plant row A⁽ˢ⁾[i,:]·x_k + B₁[i,:]·w_k and the fma chain over B₂⁽ˢ⁾[i,j]·u_k[j];
// one more wave per orphan actuator (an empty B₂ column) evaluates that u_k[j] alone.  Same expression, same lanes, same order;
// the two differences are that plant values are read at [e][scen] and that ŵ comes from the mirrored ring.
//
// Memory of one object (all of it allocated at plan time, none of it grows with the number of steps):
//     hist  [2·R][Nx][nscen]   the mirrored ring of sls_controller.h, R = 2^⌈log₂T⌉: ŵ_k at slot s = k mod R and at s + R
//     beta  [2][Nx][nscen]     β_k in copy k & 1
//     x     [2][Nx][nscen]     x_k in copy k & 1
//     acc_cost, acc_peak [Nx + Nu][nscen]   per-row accumulators (below)
//     A_val [nnz(A)][nscen], B2_val [nnz(B₂)][nscen]   plant values in CSR order, scenario innermost
//
// THE RING CHECK for this step's read and write set.  Let s = k mod R and p = s + R.  Inside the launch of step k
//     reads:   hist positions p+1−T … p−1 (the entries of lag 2 … T; lag 1 is x_k − β_k, not in the ring yet),
//              x copy k & 1 (the A row, the lag-1 entries, the accumulators' x_k[i]),  β copy k & 1 (the lag-1 entries, ŵ_k[i]),
//              the plant values, Φ, q, r, w_k;
//     writes:  hist positions s and p (ŵ_k[i], by the wave of row i),  x copy (k+1) & 1,  β copy (k+1) & 1 (each [i] by row i),
//              acc_cost / acc_peak row i and the u rows this wave owns, the caller's x_k / u_k record rows.
// s < p + 1 − T because T ≤ R, and p is above every position read, so no wave reads a ring position another wave writes (with
// T = R the slot written is the one just below the oldest read).  x and β are double-buffered by the parity of k, so x_{k+1} and
// β_{k+1} never overwrite what another wave of the same launch still reads.  An accumulator element has exactly one owner (next
// paragraph).  A u_k[j] that several waves evaluate is stored by each of them with the same bits.  Hence no grid-wide dependency
// inside a step, and consecutive steps are ordered by the stream.
//
// OWNERS.  The accumulators are [Nx + Nu][nscen]: row i < Nx belongs to the wave of state row i; row Nx + j belongs to the FIRST
// state row (ascending i) whose B₂ row stores column j — flagged per CSR entry of B₂ at plan time (b2_owner) — or, for an orphan
// actuator, to its orphan wave.  The other evaluations of u_k[j] are bit-identical duplicates and are not counted.  Per element,
//     t = q·v (rounded);   acc_cost = fma(t, t, acc_cost);   acc_peak = fmax(acc_peak, |v|)
// with v = x_k[i] or u_k[j]: one owner, a fixed order in k, no floating-point atomics — bit-identical from run to run and
// independent of how the steps are split into calls.
//
// STATS reduce over the rows in ascending order, serially, one scenario per thread:
//     cost[s] = (((0 + acc_cost[0][s]) + acc_cost[1][s]) + … + acc_cost[Nx+Nu−1][s]),
//     peak_x[s] = max_{i<Nx} acc_peak[i][s],   peak_u[s] = max_{j<Nu} acc_peak[Nx+j][s]   (0 when Nu = 0).
// fmax drops a NaN, so a NaN in x or u shows in the cost and not in the peaks.
//
// TRAFFIC per step from HBM: 12 B per stored Φ entry (value + hoff) plus 8·(nnz(A) + nnz(B₂))·nscen B of plant values, contiguous
// along the scenario lanes; the ring, x, β and the accumulators (8·(2·Nx + 2·(Nx+Nu))·nscen B touched per step) stay in L2.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sls_controller.h"
#include "sls_symbolic.h"

namespace sls {

// What sls_rollout_plan builds on the host: the simulator's operator (FirOperator with the plant by rows and the orphan list),
// where the gather of sls_rollout_set_plant finds each CSR entry in the caller's CSC nzval array, and the owner flags.
struct RolloutTables {
  FirOperator F;
  std::vector<int32_t> A_src, B2_src;   // CSR position e of A / B₂ → CSC position (the walk of csc_to_csr)
  std::vector<uint8_t> b2_owner;        // per CSR entry of B₂: 1 where this state row is the first that stores the entry's column
};
// dims, P->A, P->B1, P->B2 and the masks are read (C1, D11, D12 are not).  Errors and limits: build_fir_operator's.
int build_rollout_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, RolloutTables& out,
                         std::string& msg);

// doubles of the buffers a reset clears: ring, β (two copies), x (two copies), the two accumulators
static inline int64_t rollout_state_doubles(int64_t Nx, int64_t Nu, int64_t T, int64_t nscen) {
  return controller_hist_doubles(Nx, T, nscen) + controller_beta_doubles(Nx, nscen) + 2 * Nx * nscen + 2 * (Nx + Nu) * nscen;
}

// What the device step (sls_rollout.hip) reads and writes; every pointer is a device pointer.
struct RolloutParams {
  const int32_t *beta_ptr, *u_ptr, *hoff;
  const double* vals;                         // Φ entries in row order (sls_rollout_load)
  const int32_t *A_ptr, *A_idx, *B1_ptr, *B1_idx, *B2_ptr, *B2_idx, *orphan;
  const uint8_t* B2_own;                      // owner flag per CSR entry of B₂
  const double *A_val, *B2_val;               // [nnz][nscen]
  const double* B1_val;                       // [nnz(B₁)], shared
  const double *q, *r;                        // Nx, Nu
  int32_t Nx, Nu, Nw, T, R, n_orphan;
  long long nscen;
  double *hist, *beta, *x;                    // [2·R][Nx][nscen], [2][Nx][nscen], [2][Nx][nscen]
  double *acc_cost, *acc_peak;                // [Nx + Nu][nscen]
};

// Host twin of the object behind sls_rollout_*: the same tables, ring, double buffers, owner flags and stats reduction in serial
// loops, rows accumulated in long double and rounded to double where the device stores a double (β, u, x, ŵ, t, the accumulators).
class RolloutHost {
 public:
  // every scenario starts from the values of `tables` (the plant given at plan time); q = r = 1; the reset state
  int init(const RolloutTables& tables, int64_t nscen, std::string& msg);
  void load(const double* values);                                             // Φ in mask order
  // caller's CSC nzval order; NULL keeps what is there; per_scenario: [nnz][nscen] instead of [nnz]
  void set_plant(const double* A_nzval, const double* B2_nzval, bool per_scenario);
  void set_weights(const double* q, const double* r);                          // Nx / Nu doubles, NULL keeps
  void reset(const double* x0);                                                // [Nx][nscen] or NULL
  // w [steps][Nw][nscen] or NULL; x_rec / u_rec [steps][Nx|Nu][nscen] or NULL
  int run(const double* w, int64_t steps, double* x_rec, double* u_rec, std::string& msg);
  void stats(double* cost, double* peak_x, double* peak_u) const;              // [nscen] each, nullable
  const double* state() const { return x_.data() + (k_ & 1) * T_.F.Nx * ns_; } // x_K, [Nx][nscen]
  int64_t steps_done() const { return k_; }

 private:
  RolloutTables T_;
  int64_t ns_ = 0, k_ = 0, R_ = 1;
  bool loaded_ = false;
  std::vector<double> vals_, A_val_, B2_val_, q_, r_, hist_, beta_, x_, acc_cost_, acc_peak_;
};

}  // namespace sls
