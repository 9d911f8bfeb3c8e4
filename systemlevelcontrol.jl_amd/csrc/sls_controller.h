// sls_controller.h — the stand-alone SLS controller: one step from a measured state to u (pure C++, no HIP).
//
// Steps are numbered k = 0, 1, … since the last reset.  Step k takes the measured state x_k of `nscen` scenarios and gives
//     ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
//     u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
//     β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}
// (τ and the Φ indices 1-based as in reference README.md:62-72; row k of the simulator's x, u arrays is step k here).  No plant
// appears: the state comes from outside, so the plant may differ from the design model, be non-linear, or be measured.
// The operator is the simulator's (FirOperator, sls_symbolic.h: β rows then u rows, entries ascending in (τ, c),
// hoff = τ·Nx − c), built from the masks alone by build_controller_operator (sls_symbolic.h).
//
// History.  ŵ lives in a MIRRORED RING of R = 2^⌈log₂T⌉ slots of [Nx][nscen] doubles, 2·R slots in memory: step k writes ŵ_k
// at slot s = k mod R and again at s + R.  With p = s + R the position of ŵ_k, the T positions p+1−T … p hold ŵ_{k+1−T} … ŵ_k
// contiguously whatever s is (p − j ≥ R holds the upper copy of step k − j when j ≤ s, and p − j < R its lower copy when
// j > s), so an entry reads the history at (p + 1)·Nx − hoff — the simulator's addressing with (p + 1) in the place of
// (k + T), no lag test and no wrap.  Inside one launch the positions read are p+1−T … p−1 and the positions written are s and
// p; s < p + 1 − T because T ≤ R, so no wave reads what another writes (with T = R the slot written is the one just below the
// oldest read).  ŵ_k itself, lag τ = 1 (hoff ≤ Nx), is not in the ring yet: such an entry reads x_k[c] − β_k[c], the same
// single subtraction the owner of row c stores, hence the same double.  β is double-buffered by the parity of k so that
// β_{k+1} never overwrites a β_k another wave still reads.
//
// The device step is csrc/sls_controller.hip; this header holds what the kernel and the host twin (csrc/sls_controller.cpp)
// share: the slot arithmetic and the parameter block.
#pragma once
#include <cstdint>
#include <string>

#include "sls_symbolic.h"

#if defined(__HIPCC__)
#define SLS_CTL_HD __host__ __device__
#else
#define SLS_CTL_HD
#endif

namespace sls {

// R: the smallest power of two ≥ T
SLS_CTL_HD static inline int64_t controller_ring_slots(int64_t T) {
  int64_t R = 1;
  while (R < T) R <<= 1;
  return R;
}
// slot s of step k (the second copy goes to s + R)
SLS_CTL_HD static inline int64_t controller_slot(int64_t k, int64_t R) { return k & (R - 1); }
// element offset (in units of nscen doubles) the entries' hoff is subtracted from at a step whose slot is s: (s + R + 1)·Nx
SLS_CTL_HD static inline int64_t controller_window_end(int64_t s, int64_t R, int64_t Nx) { return (s + R + 1) * Nx; }
// lag τ (1-based) and column c (0-based) of an entry: hoff = τ·Nx − c with 0 ≤ c < Nx
SLS_CTL_HD static inline int64_t controller_lag(int64_t hoff, int64_t Nx) { return (hoff + Nx - 1) / Nx; }
SLS_CTL_HD static inline int64_t controller_col(int64_t hoff, int64_t Nx) { return controller_lag(hoff, Nx) * Nx - hoff; }
// doubles of the three state buffers of a controller: history, β (two copies)
SLS_CTL_HD static inline int64_t controller_hist_doubles(int64_t Nx, int64_t T, int64_t nscen) {
  return 2 * controller_ring_slots(T) * Nx * nscen;
}
SLS_CTL_HD static inline int64_t controller_beta_doubles(int64_t Nx, int64_t nscen) { return 2 * Nx * nscen; }

// What the device step (sls_controller.hip: launch_controller_step) reads and writes; every pointer is a device pointer.
struct ControllerParams {
  const int32_t* row_ptr;     // Nx + Nu + 1: β rows, then u rows
  const int32_t* hoff;        // n_entries
  const double* vals;         // Φ entries in row order (sls_controller_load)
  int32_t Nx, Nu, T, R;
  long long nscen;
  double* hist;               // [2·R][Nx][nscen]
  double* beta;               // [2][Nx][nscen]: β_k in copy k & 1
};

// Host twin of the device step: `steps` steps from a reset state through F's tables and the ring above, one serial loop per
// row in ascending entry order, accumulated in long double and rounded to double where the device stores a double (β, ŵ, u).
// values: Φ in mask order (F.n_values doubles; only perm[] positions are read).  x [steps][Nx][nscen]; outputs, each nullable:
// u [steps][Nu][nscen], what [steps][Nx][nscen].
int controller_host(const FirOperator& F, const double* values, int64_t nscen, int64_t steps, const double* x, double* u,
                    double* what, std::string& msg);

}  // namespace sls
