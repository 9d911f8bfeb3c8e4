/* sls_mi355x.h — C ABI of the MI355X-native column-separable H2 SLS engine.
 *
 * Drop-in boundary for ONE path of aaltoKEPO/SystemLevelControl.jl:
 *     Φx,Φu = SLS_𝓗₂(P, [𝓢x,𝓢u]; 𝓘)            (reference src/synthesis.jl:11-32)
 * i.e. the @distributed per-column loop _SLS_𝓗₂ (src/synthesis.jl:34-72) with
 * sparsity_dim_reduction (src/reduction.jl:11-27) and the JuMP/Ipopt solve
 * (src/synthesis.jl:46-62) replaced by batched HIP kernels for gfx950.
 *
 * Conventions
 *  - plain C, plain pointers and sizes; no C++/torch types cross this boundary.
 *  - every matrix is handed over exactly as Julia stores a SparseMatrixCSC{Tv,Int}
 *    (reference src/types/GeneralizedPlant.jl:47-55): colptr[ncols+1], rowval[nnz]
 *    (sorted within a column), nzval[nnz]; indices are int64 and may be 1-based
 *    (Julia) or 0-based (C/Python) — sls_dims.index_base says which.
 *  - the caller owns every buffer; the library keeps no host pointer after a
 *    call returns.  Calls block.  No callbacks, no signal handlers, no abort():
 *    every failure is a negative return code plus sls_last_error().
 *  - return codes: 0 = ok; <0 = SLS_E*; >0 (solve calls only) = number of
 *    subproblems whose status is not SLS_COL_OK (their values are still written;
 *    see col_status).  The reference itself never checks the solver status
 *    (src/synthesis.jl:62-65 goes straight from optimize! to value.).
 */
#ifndef SLS_MI355X_H
#define SLS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLS_ABI_VERSION 2   /* 2: sls_stats.n_refined appended (round 2) */

/* ---- error codes (negative returns) ---- */
#define SLS_EINVAL      (-1)  /* bad argument / inconsistent dimensions           */
#define SLS_ENOTSF      (-2)  /* weights not LQR-shaped: Nz != Nx+Nu (the reference's
                                 view() hard-codes z-rows [s_x; Nx+s_u],
                                 src/reduction.jl:15)                              */
#define SLS_EUNSUPPORTED (-3) /* valid input this build cannot solve (a cost
                                 that leaves a free variable without weight; a
                                 coupled group with a column outside its s_x)      */
#define SLS_EHIP        (-4)  /* HIP runtime error (message in sls_last_error)     */
#define SLS_ENOMEM      (-5)
#define SLS_ENODEVICE   (-6)  /* no gfx950 device / kernels not loadable          */

/* ---- per-subproblem status words (col_status[], one per column of every group) ---- */
#define SLS_COL_OK          0
#define SLS_COL_INFEASIBLE  1 /* E z = f has no solution: the residual stops contracting above the acceptance level (a pass
                                 that leaves more than half of it AND no longer removes 10 % per pass / 19 % over two: a slowly
                                 but steadily contracting column — nearly dependent constraints — is carried on, up to 48
                                 passes); values are the minimum-norm least-squares point — except when the factorisation itself
                                 broke down on an inconsistent, nearly rank-deficient column (reported residual = inf): the column
                                 is flagged all the same, its values are then unspecified.  The reference hands every column to
                                 Ipopt and never reads its status (src/synthesis.jl:62-65).                          */
#define SLS_COL_NOTCONV     2 /* refinement hit the iteration cap above tolerance   */
#define SLS_COL_TRIVIAL     3 /* column not in its own s_x (Ĩ column is zero): Φ = 0 */
#define SLS_COL_SKIPPED     4 /* not owned by this plan's shard                     */
#define SLS_COL_UNSUPPORTED 5 /* not solved, values stay 0.0 (the other columns of the call are solved as usual).  Since round 3
                                 the default build never reports it: an index set whose working set exceeds LDS runs the tile
                                 kernel with that working set in a global buffer (no size limit but device memory).  Only the
                                 experiment switches SLS_TILE=0 / SLS_TILE_BIG=0 (round-1 / round-2 launch lists) bring it back. */

/* ---- sls_create flags ---- */
#define SLS_CREATE_DEFAULT  0u

/* ---- sls_dims.flags ---- */
#define SLS_SOLVE_DEFAULT   0u
#define SLS_SOLVE_SUM_OF_NORMS 1u /* per column: minimise Σ_t ‖[C̃1 D̃12]Φ̃[t]B̃1‖₂ (sum of the per-time-step norms) instead of the 𝓗₂
                                    sum of squares, over the same index sets, masks and achievability constraints — the
                                    column-separable bound of the 𝓗∞ norm, a second-order cone program per column.  NOT in the
                                    reference (it has no 𝓗∞ synthesis; BASELINE configs[3] names one).  Needs a diagonal
                                    [C1 D12]ᵀ[C1 D12] and D11 = 0, else SLS_EUNSUPPORTED.  ADMM whose projection step is the 𝓗₂ machinery (one-wave
                                    kernel for ñx ≤ 32, tile kernel beyond); status SLS_COL_NOTCONV when the step cap is hit. */
#define SLS_PLAN_WEIGHTS_UPDATABLE 2u /* sls_h2_sf_plan / sls_h2_sf_plan_localized: the plan can take new LQR weights later
                                    (sls_plan_update_weights below, which states the shape the plant must have; SLS_EUNSUPPORTED
                                    otherwise).  Every column with B1[c,c] ≠ 0 then gets a weight record, uniform weights
                                    included; without the flag a plan is built exactly as before.  The one-shot and batch calls
                                    (sls_h2_sf_solve, _solve_batch, _solve_localized) ACCEPT the flag and apply the same shape
                                    rule and the same records — they keep no plan, so there is nothing to update afterwards. */
#define SLS_PLAN_MULTIPLIERS 4u /* sls_h2_sf_plan / sls_h2_sf_plan_localized: every execute also keeps the multiplier of the
                                    achievability constraints of every column, which sls_plan_gradient (below) turns into the
                                    derivative of the 𝓗₂ cost in the stored entries of A and B2.  Every column then runs on the
                                    one-wave kernel (no two-wave, no four-wave launch).  SLS_EUNSUPPORTED, with the reason, for a plan
                                    with a column beyond the 32-lane one-wave classes (ñx > 32), a dense cost Hessian, a coupled
                                    group or SLS_SOLVE_SUM_OF_NORMS, and from the one-shot calls (they keep no plan).  Without the
                                    flag a plan is built, routed and sized exactly as before. */

/* Julia SparseMatrixCSC{Float64,Int}  (reference src/types/GeneralizedPlant.jl:47-52) */
typedef struct sls_csc_f64 {
  int64_t nrows, ncols;
  const int64_t* colptr;   /* ncols+1 */
  const int64_t* rowval;   /* nnz     */
  const double*  nzval;    /* nnz     */
} sls_csc_f64;

/* Julia SparseMatrixCSC{Bool,Int}: one byte per stored entry.  nzval == NULL means
 * "every stored entry is true".  A stored `false` is NOT in the mask (the reference
 * tests `.≠ 1`, src/synthesis.jl:58-59) but IS part of the structural pattern that
 * sparsity_dim_reduction sees through findnz (src/reduction.jl:14).                */
typedef struct sls_csc_bool {
  int64_t nrows, ncols;
  const int64_t* colptr;
  const int64_t* rowval;
  const uint8_t* nzval;
} sls_csc_bool;

/* P.Nx, P.Nu, P.Nz, P.Nw (reference src/types/GeneralizedPlant.jl:56) and
 * T = length(𝓢x) (src/synthesis.jl:20). */
typedef struct sls_dims {
  int64_t Nx, Nu, Nz, Nw, T;
  int32_t index_base;      /* 1 = Julia, 0 = C   (applies to every colptr/rowval/group_cols) */
  uint32_t flags;          /* SLS_SOLVE_*        */
} sls_dims;

/* The nine-block plant as SLS_𝓗₂ reads it (state feedback: C2 = I, D21/D22 empty are
 * implied and not passed — reference src/types/GeneralizedPlant.jl:91-95).
 * C1, D11, D12 may each be NULL: then the 3-argument Plant(A,B1,B2) defaults apply
 * ([C1 D12] = I, D11 = 0 — src/types/GeneralizedPlant.jl:105-110).                  */
typedef struct sls_plant {
  const sls_csc_f64 *A, *B1, *B2, *C1, *D11, *D12;
} sls_plant;

typedef struct sls_stats {
  int64_t n_subproblems;       /* Σ_groups |c_j|                                   */
  int64_t n_not_ok;
  int64_t n_values_x, n_values_u;   /* Σ_t nnz(𝓢x[t]), Σ_t nnz(𝓢u[t])                */
  int64_t n_free;              /* Σ free variables actually solved for              */
  int32_t max_nx, max_nu;      /* max |s_x|, |s_u| over subproblems                 */
  int32_t max_iters;           /* max refinement passes used by any subproblem      */
  int32_t n_devices;
  double  max_residual;        /* max over OK subproblems of ‖E z − f‖∞             */
  double  flops_alg;           /* Σ F_alg, algorithmic FP64 flops      */
  double  bytes_alg;           /* Σ B_alg, algorithmic HBM bytes       */
  double  t_symbolic_s;        /* host symbolic pass (replaces src/reduction.jl)    */
  double  t_upload_s;          /* H2D of the shared operator + per-column tables    */
  double  t_solve_s;           /* device solve, wall clock around the launches      */
  double  t_download_s;        /* D2H of Φ values                                    */
  int64_t n_refined;           /* columns solved a second time on the tile kernel (slow convergence: near-singular) */
} sls_stats;

typedef struct sls_ctx  sls_ctx;
typedef struct sls_plan sls_plan;

/* ---- context ------------------------------------------------------------------
 * One context owns `ndev` HIP devices (device ordinals in devs[]); the reference
 * analogue is the worker pool of `julia -p N` (src/synthesis.jl:16 nworkers()).
 * devs == NULL selects devices 0..ndev-1.  Returns NULL on failure
 * (sls_last_error(NULL) then describes it).                                       */
sls_ctx* sls_create(const int* devs, int ndev, uint32_t flags);
void     sls_destroy(sls_ctx* ctx);
const char* sls_last_error(const sls_ctx* ctx);   /* ctx may be NULL                 */
int      sls_abi_version(void);
int      sls_device_count(void);                  /* gfx950 devices visible, <0 on error */

/* ---- the drop-in call  (replaces reference src/synthesis.jl:11-32 + :34-72) -----
 *  P        : plant blocks (see sls_plant)
 *  Sx, Su   : arrays of T masks (Nx×Nx and Nu×Nx)               — 𝓢 = [𝓢x, 𝓢u]
 *  groups   : 𝓘 as CSR-like lists: group g holds columns
 *             group_cols[group_ptr[g] .. group_ptr[g+1]) (index_base applies to
 *             group_cols, group_ptr is always 0-based offsets).  ngroups = 0 and
 *             NULL pointers select the default [[i] for i in 1:Nx]
 *             (src/synthesis.jl:15).  Columns ascend strictly inside a group.  A column
 *             listed in several groups is solved once per group, with that group's index
 *             sets, and the contributions are ADDED — what the reference's Φ̃ += … and
 *             (+) fold do (src/synthesis.jl:24,67).  (Only this call: a plan gives every
 *             subproblem its own destinations, so sls_h2_sf_plan / sls_shard_groups /
 *             sls_h2_sf_packed_layout answer such a list with SLS_EINVAL.)
 *  phix_vals[t] / phiu_vals[t] : caller-allocated arrays of nnz(𝓢x[t]) / nnz(𝓢u[t])
 *             doubles, filled IN THE MASK'S CSC nzval ORDER, so that
 *             SparseMatrixCSC(Nx,Nx,𝓢x[t].colptr,𝓢x[t].rowval,phix_vals[t]) is Φx[t]
 *             with a pattern that is the mask's bit for bit (entries the reference
 *             would drop as numerical zeros are stored 0.0; src/synthesis.jl:65-67).
 *             Columns that belong to no group keep 0.0.
 *  col_status : NULL or int32[Σ|c_j|], in group order (SLS_COL_*)
 *  stats      : NULL or filled on return
 * A column's subproblem is solved with its group's index sets s_x, s_u
 * (src/reduction.jl:14).  Cost weights: any [C1 D12] with Nz = Nx+Nu rows
 * (src/synthesis.jl:50,76-83); when [C1 D12]ᵀ[C1 D12] is diagonal on (s_x,s_u) (every
 * Plant(A,B1,B2), every diagonally weighted LQR) the column runs on the kernel of its
 * size class, otherwise on the tile kernel with projected conjugate gradients over the
 * diagonal-weight solve.  The cost couples the columns of a multi-column group only
 * through the block B1[c_j,c_j] (src/synthesis.jl:42): diagonal block ⇒ the group's QP
 * separates by column; otherwise the group is solved jointly (one work item of the tile
 * kernel: conjugate gradients over all its columns, Hessian (B̃1B̃1ᵀ)⊗[C̃1 D̃12]ᵀ[C̃1 D̃12]);
 * a group containing an infeasible column is then flagged as a whole.
 * Columns of the small size classes that converged slowly (four or more passes and a residual above 1e-11, or
 * SLS_COL_NOTCONV: a near-singular constraint matrix) are solved once more on the tile kernel's minimal-residual iteration
 * before the download; stats->n_refined counts them.                                     */
int sls_h2_sf_solve(sls_ctx* ctx, const sls_dims* dims, const sls_plant* P,
                    const sls_csc_bool* Sx, const sls_csc_bool* Su,
                    int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                    double* const* phix_vals, double* const* phiu_vals,
                    int32_t* col_status, sls_stats* stats);

/* The reference's objective is norm(H, 𝓗₂) + L⁺([Φ̃x,Φ̃u], c_j) with the hook L⁺ hard-wired to 0 (src/synthesis.jl:21,52).
 * Its diagonal quadratic instance — the ridge term  Σ_t Σ_i rx[i]·Φx[t][i,c]² + Σ_j ru[j]·Φu[t][j,c]²  added to every column's
 * cost — is available on the context: the weights (≥ 0, lengths Nx and Nu of the plants solved afterwards; 0 = none for that
 * part) apply to every later sls_h2_sf_solve / sls_h2_sf_plan / batch call on `ctx` until replaced; (0, NULL, 0, NULL) clears.
 * With default weights and B1 = I this equals solving with [C1 D12] = diag(√(1 + r)).  Not built for the sum-of-norms mode. */
int sls_set_ridge(sls_ctx* ctx, int64_t nx, const double* rx, int64_t nu, const double* ru);

/* A batch of independent plants in ONE call and ONE set of kernel launches (latency regime: the README plant's 59 columns fill
 * a quarter of the CUs; four of them take the time of one).  The reference's counterpart is a loop of SLS_𝓗₂ calls
 * (src/synthesis.jl:11), one per plant.  The plants are solved as the block-diagonal composite plant — column c of plant i has
 * exactly the index sets, masks and constraints it has alone, so every per-column result is the one the single call returns —
 * with default groups (one per column).  All plants share T, index_base and flags (dims[i].T etc. must agree).
 *   dims[nplants], P[nplants];  Sx[i], Su[i]: the T masks of plant i;  phix_vals[i][t], phiu_vals[i][t] as in
 *   sls_h2_sf_solve;  col_status: NULL or col_status[i] = NULL / array of dims[i].Nx.  Returns like sls_h2_sf_solve. */
int sls_h2_sf_solve_batch(sls_ctx* ctx, int nplants, const sls_dims* dims, const sls_plant* P,
                          const sls_csc_bool* const* Sx, const sls_csc_bool* const* Su,
                          double* const* const* phix_vals, double* const* const* phiu_vals,
                          int32_t* const* col_status, sls_stats* stats);

/* ---- the same path split into plan / execute ------------------------------------
 * A plan = symbolic pass + everything resident in HBM on ONE device of the context
 * (shared operator A,B2 in CSR; per-subproblem index sets, masks, destination
 * table, factor workspace).  It owns the subproblems of groups
 * [group_begin, group_end) — the shard of this rank (src/synthesis.jl:16 static
 * contiguous chunking; here the caller chooses the cut, see sls_shard_groups).
 * sls_plan_execute is the hot path proper: device-resident in, device-resident out. */
typedef struct sls_plan_info {
  int64_t n_subproblems;       /* owned by this plan                                */
  int64_t n_values;            /* length of the full value array: n_values_x+n_values_u */
  int64_t n_values_x, n_values_u;
  int64_t n_packed;            /* # values this plan writes (its free variables)     */
  int64_t workspace_bytes;     /* device bytes held by the plan                      */
  int32_t max_nx, max_nu, T;
  int32_t device;              /* HIP ordinal                                        */
  double  flops_alg, bytes_alg;/* Σ over owned subproblems              */
  double  t_symbolic_s, t_upload_s;
} sls_plan_info;

int  sls_h2_sf_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P,
                    const sls_csc_bool* Sx, const sls_csc_bool* Su,
                    int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                    int64_t group_begin, int64_t group_end, sls_plan** plan_out);
int  sls_plan_get_info(const sls_plan* plan, sls_plan_info* info);

/* Value-array layout ("mask order"): [t=0..T-1: nnz(𝓢x[t]) doubles] then
 * [t=0..T-1: nnz(𝓢u[t]) doubles].  sls_plan_value_offsets fills off_x[T+1], off_u[T+1]
 * (offsets of each t's slice in that array; off_x[T] = n_values_x = off_u[0]).       */
int  sls_plan_value_offsets(const sls_plan* plan, int64_t* off_x, int64_t* off_u);

/* Run the solve on `hip_stream` (a hipStream_t cast to void*; NULL = HIP's null stream,
 * which is also torch's default stream).  d_values: DEVICE pointer.
 *   packed == 0: d_values has n_values doubles; the plan writes only its own entries
 *                (caller zero-fills once; entries of other shards are untouched).
 *   packed == 1: d_values has n_packed doubles; entry k goes to mask-order position
 *                dest[k] (sls_plan_packed_dest) — the layout the RCCL all-gather moves.
 * Asynchronous w.r.t. the host: returns after enqueueing.  Status/residuals stay on
 * the device until sls_plan_fetch_status.                                           */
int  sls_plan_execute(sls_plan* plan, void* hip_stream, double* d_values, int packed);
/* Several resident plans of one device in one call: plan 0 runs on `hip_stream`, the others on their plan-owned streams, which
 * first wait for everything enqueued on `hip_stream` before the call (fork edge) and are joined back into `hip_stream` by an
 * event each: work enqueued on `hip_stream` BEFORE the call has finished with d_values[i] when a plan overwrites it, work
 * enqueued AFTERWARDS sees all results; the host is never blocked.  (SLS_BATCH_FORK=0 in the environment drops the fork
 * edge: then the caller must guarantee that nothing still pending on `hip_stream` reads or writes any d_values[i], i >= 1.)
 * Measured (4 README plans): 0.27 ms per call against 0.48 ms for four calls in a row — a cross-queue event wait costs
 * ≈0.1 ms on this stack; a caller that can merge its plants up front should use sls_h2_sf_solve_batch (one launch, 0.126 ms
 * for the same four).  d_values[i] / packed as above; no plan may appear twice. */
int  sls_plan_execute_batch(sls_plan* const* plans, int nplans, void* hip_stream, double* const* d_values, int packed);
int  sls_plan_synchronize(sls_plan* plan, void* hip_stream);
int  sls_plan_packed_dest(const sls_plan* plan, int64_t* dest /* n_packed, host */);
/* col_status / residual / iters: NULL or arrays of n_subproblems (host). Synchronises. */
int  sls_plan_fetch_status(sls_plan* plan, int32_t* col_status, double* residual, int32_t* iters);
/* Refinement for the resident path (sls_h2_sf_solve does this by itself).  After an execute: reads the statuses, and for the
 * groups whose one-wave / twisted columns stopped between 1e-11 and the acceptance level after four or more passes, ended
 * NOTCONV, or were called infeasible at a small residual (by a twisted kernel: at any residual, after three or more passes) — the
 * signature of a near-singular constraint matrix, where Φ is
 * only determined to residual/σ_min — builds a second plan on the tile kernel (minimal-residual multiplier iteration, 1e-13),
 * runs it on `hip_stream` into `d_values` (layout `packed` as in sls_plan_execute: the refinement numbers its free variables
 * where `plan` put them, so it writes either layout in place) and ATTACHES it to `plan`: every later sls_plan_execute runs it
 * after the main launches, sls_plan_fetch_status reports the refined outcome, and sls_plan_destroy frees it.  The plan does
 * not keep its inputs: pass the same dims / P / masks / group list it was built from.  Waits for the device;
 * *n_refined = subproblems re-solved (0: nothing qualified, nothing attached).  𝓗₂ objective only.                       */
int  sls_plan_refine(sls_plan* plan, const sls_dims* dims, const sls_plant* P,
                     const sls_csc_bool* Sx, const sls_csc_bool* Su,
                     int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                     void* hip_stream, double* d_values, int packed, int64_t* n_refined);
/* ---- new values of A and B2 for a live plan (same non-zero pattern: no rebuild) ---------------------------------------------
 * Masks, index sets, destinations, launch list and workspace depend on the pattern of (A≠0), (B2≠0) alone; only the plan's copy
 * of the operator (and the four-wave kernel's prepared records, gathered from it) holds numbers.  sls_plan_update_plant rewrites
 * those on `hip_stream`; the next sls_plan_execute solves the new plant.
 *   A_nzval [nnz(A)], B2_nzval [nnz(B2)]: the CSC nzval arrays, in the order of the matrices the plan was built from.  Either may
 *     be NULL (unchanged); both NULL is a no-op that returns 0.
 *   on_device = 0: HOST arrays, not kept after return.  on_device = 1: DEVICE pointers on the plan's device, read on `hip_stream`
 *     (they must stay valid and unchanged until the update has run there).
 * Ordering: the call enqueues on `hip_stream` and returns, like sls_plan_execute (host arrays up to 8 MiB go through the
 * context's pinned buffer; larger ones are copied synchronously).  sls_plan_execute joins its auxiliary streams back into the
 * caller's stream before it ends, so an update enqueued on the same stream after an execute runs behind all of that execute's
 * launches, and an execute enqueued after the update sees the new values.  Executes of this plan on OTHER streams are the
 * caller's to order against the update (sls_plan_synchronize, or an event).
 * The zero rule: kernel selection sized the kernels' LDS lists from the NON-ZERO counts at plan time, and the gathers skip zeros
 * at run time.  A non-zero entry may therefore take any finite value, 0.0 included; an entry that was exactly 0.0 when the plan
 * was built must stay 0.0 (a gather could overrun its list otherwise); non-finite values are refused too.
 *   host path:   checked before anything is enqueued — SLS_EINVAL, the message names the matrix and the nzval position, the
 *                plan is untouched.
 *   device path: the kernel checks each entry; an offending entry is not written and is counted.  sls_plan_update_result waits
 *                for the last update and returns the count (0 = applied in full; always 0 after a host-path update).  A non-zero
 *                count means the operator is a mix of old and new values — safe (the capacities hold), but the caller repeats
 *                the update with valid values.
 * Equivalence: when the new values have the non-zero pattern of the plan-time values, the plan is equivalent to one built from
 * the new plant.  When an entry goes to 0.0 the plan keeps its plan-time index sets — a superset of what the reference would now
 * compute (src/reduction.jl:14 reads (A≠0) by value), whose extra rows are still constrained — so the results may differ from a
 * fresh plan's.
 * Only A and B2 change: B1, C1, D11, D12 and the ridge term stay plan constants, and sls_plan_objective (which reads neither A
 * nor B2) stays correct.  Which columns are near-singular depends on the values: an update detaches and frees a refinement
 * attached by sls_plan_refine (waiting for the plan's last execute first); run sls_plan_refine again with the new plant.  Works
 * for every plan kind (sls_h2_sf_plan, sls_h2_sf_plan_localized, both objectives, either layout).  A closed-loop simulator
 * (sls_closed_loop_plan) keeps its own copy of the plant; to run the new Φ against another plant than the design model, step
 * the stand-alone controller (sls_controller_*), which holds no plant.                                                          */
int  sls_plan_update_plant(sls_plan* plan, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device);
int  sls_plan_update_result(sls_plan* plan, int64_t* n_rejected);
/* The operator values the plan holds now, as CSC nzval arrays in the plan's order (HOST outputs of nnz(A) / nnz(B2) doubles,
 * either may be NULL): what the updates so far left on the device, refused entries of the device path at their old values.
 * Like sls_plan_update_result it waits for the plan's last update and for nothing else on the device (the copy runs on the
 * plan's own stream behind that update).  A caller that updates from device memory and later needs the plant on the host — to
 * pass it to sls_plan_refine — reads it here instead of keeping its own copies.  Like every call on a context, the update
 * entry points are for one thread at a time per context (they share the context's pinned staging buffer).                    */
int  sls_plan_fetch_plant(sls_plan* plan, double* A_nzval, double* B2_nzval);
/* ---- new LQR weights for a live plan (no rebuild) ----------------------------------------------------------------------------
 * For a plan built with SLS_PLAN_WEIGHTS_UPDATABLE in sls_dims.flags.  The flag requires the LQR shape: C1 and D12 are each NULL
 * (identity) or hold exactly one stored entry per column on that column's own z-row — C1 = [diag(q); 0], D12 = [0; diag(r)];
 * D11 is NULL or has no non-zero on a z-row a column selects (sls_h2_sf_plan_localized: no non-zero at all); no coupled column
 * group (non-diagonal B1[c_j, c_j]); either objective.  SLS_EUNSUPPORTED with the reason otherwise.  Masks, index sets,
 * destinations, launch list and workspaces do not depend on a weight value; what does is the per-column record
 * 1 / (B1[c,c]²·v² + ridge) and the four-wave kernel's plan-time tables, and sls_plan_update_weights rewrites those on
 * `hip_stream`; the next sls_plan_execute solves the re-weighted problem, sls_plan_objective values it.
 *   c1_diag [Nx]: c1_diag[i] is the stored value C1[i, i]; d12_diag [Nu]: d12_diag[j] is D12[Nx + j, j].  NULL: that half keeps its
 *     values; both NULL is SLS_EINVAL, and so is a plan built without the flag.
 *   on_device, ordering, staging and the one-thread-per-context rule: as sls_plan_update_plant.  Nothing is allocated and the
 *     device is never waited for.
 * The value rule: a value is accepted when it is finite and B1[c,c]²·v² + ridge > 0 in every column that holds the variable
 * (the plan-time rule: a singular Hessian is refused; the sign of v does not matter, 0.0 needs a positive ridge).
 *   host path:   checked before anything is enqueued — SLS_EINVAL, the message names the matrix and the position, the plan is
 *                untouched.
 *   device path: the kernel skips an offending value — every record keeps its old value for that variable — and counts it.
 *                sls_plan_update_weights_result waits for the plan's last update and returns the count of the last weights
 *                update (0 = applied in full).
 * A value whose variable lies in no solved column's index sets is only kept (sls_plan_fetch_weights returns it).
 * Equivalence: the records are rewritten to the bits a plan built from the re-weighted plant with the flag holds, so the next
 * execute gives that plan's Φ.  An attached refinement is detached and freed as by sls_plan_update_plant; with
 * sls_plan_track_changes on, the subproblems in which at least one record value changed bits are marked dirty.  B1, the ridge
 * term, D11 and the shape stay plan constants.
 * sls_plan_fetch_weights: the diagonals the plan holds now (HOST outputs, either may be NULL): the plan-time values, then what the
 * updates left, refused values of the device path at their old values.  Waits like sls_plan_fetch_plant.                      */
int  sls_plan_update_weights(sls_plan* plan, void* hip_stream, const double* c1_diag, const double* d12_diag, int on_device);
int  sls_plan_update_weights_result(sls_plan* plan, int64_t* n_rejected);
int  sls_plan_fetch_weights(sls_plan* plan, double* c1_diag, double* d12_diag);
/* ---- re-solve only some columns of a resident plan ---------------------------------------------------------------------------
 * Subproblem q reads the plant only through A[s_x(q), s_x(q)] and B2[s_x(q), s_u(q)], so a change of A[i,j] can move it only if
 * i and j lie in s_x(q), and a change of B2[i,k] only if i lies in s_x(q) and k in s_u(q); every other column would be solved
 * again to the same bits.  The index sets are plan-time (the zero rule above keeps them), so the rule is exact for the plan as
 * it runs.
 * sls_plan_execute_columns runs the listed subproblems only: `subs` [nsubs] are positions in col_status order, 0-based, strictly
 *   ascending, in HOST memory (SLS_EINVAL otherwise).  Same kernels, LDS plans, workspaces and launch parameters as
 *   sls_plan_execute, each launch over the listed columns it owns (none: skipped).  Entries of d_values, and status / residual /
 *   iteration words, of other subproblems are not written.  A coupled group (non-diagonal B1[c_j,c_j]) is solved as a whole when
 *   any of its columns is listed.  *n_solved (nullable): subproblems solved.  nsubs = 0 returns 0 and enqueues nothing.
 * sls_plan_track_changes(plan, 1): every later sls_plan_update_plant (either path) also marks, in one "dirty" byte per
 *   subproblem on the device, the subproblems touched by the entries it actually changes: accepted, and the bits of the new
 *   value differ from the plan's current value (0.0 → −0.0 counts; a refused entry does not).  Marks accumulate over updates;
 *   turning tracking on clears them (and makes the feature's device buffers, which are not part of workspace_bytes).
 *   sls_plan_track_changes(plan, 0): later updates mark nothing; existing marks stay.
 * sls_plan_execute_dirty runs sls_plan_execute_columns on the marked set, then clears the marks on the same stream.  0 solved and
 *   nothing enqueued when tracking was never on.
 * THE HOST WAIT: grids and skipped launches are decided on the host, so sls_plan_execute_columns and sls_plan_execute_dirty build
 *   the launch lists on `hip_stream`, then wait for that stream — for everything enqueued on it before the call — and copy two
 *   int32 per launch to the host before they enqueue the solve.  The solve itself is asynchronous like sls_plan_execute.
 * A full sls_plan_execute neither reads nor clears the marks.  SLS_EUNSUPPORTED while a refinement is attached (sls_plan_refine).
 * sls_plan_fetch_dirty copies the marks to dirty[n_subproblems] (HOST); it waits for the plan's last execute and last update,
 *   like sls_plan_update_result.  sls_plan_clear_dirty clears them on `hip_stream`.                                            */
int  sls_plan_execute_columns(sls_plan* plan, void* hip_stream, double* d_values, int packed, const int64_t* subs, int64_t nsubs,
                              int64_t* n_solved);
int  sls_plan_track_changes(sls_plan* plan, int on);
int  sls_plan_execute_dirty(sls_plan* plan, void* hip_stream, double* d_values, int packed, int64_t* n_solved);
int  sls_plan_fetch_dirty(sls_plan* plan, uint8_t* dirty);
int  sls_plan_clear_dirty(sls_plan* plan, void* hip_stream);
/* ---- objective value of every column, evaluated on the device from the written Φ ------------------------------------------
 * The number the reference's JuMP model calls objective_value(problem) (src/synthesis.jl:52): per subproblem the cost it
 * minimised, at the point that was written — Σₜ‖[C̃1 D̃12]Φ̃[t]B̃1 + D̃11‖²_F for the 𝓗₂ objective (the ridge term of
 * sls_set_ridge included: it is part of what the column minimised), Σₜ‖[C̃1 D̃12]Φ̃[t]B̃1‖₂ for SLS_SOLVE_SUM_OF_NORMS — and
 * their sum, the squared 𝓗₂ norm of the closed loop.  A pass of its own over the value array (csrc/sls_objective.hip), so it
 * reports whatever was written last, an attached refinement included.  Conventions:
 *  - a coupled group (non-diagonal B1[c_j,c_j]) has ONE joint value: its first column carries it, its other columns report
 *    0.0, so the array always sums to the total;
 *  - columns that are not SLS_COL_OK are evaluated like any other, at the least-squares point that was written;
 *    SLS_COL_TRIVIAL gives the constant T·‖D̃11[:,c]‖²;
 *  - a column with B1[c,c] = 0 has a constant cost; the engine returns its minimum-norm point and reports that norm
 *    (Σz²) plus the constant — the objective it minimised;
 *  - bit-identical from call to call and between the two layouts (fixed summation order, no floating-point atomics).
 * sls_plan_objective: enqueue on hip_stream after the execute that wrote d_values (layout `packed` as in sls_plan_execute);
 *   DEVICE outputs d_col_objective[n_subproblems] and d_total[1], either may be NULL.  Asynchronous like sls_plan_execute.
 * sls_plan_fetch_objective: the same on the plan's stream (which first waits for the plan's last execute) into plan-owned
 *   buffers, waits, copies to the HOST arrays col_objective[n_subproblems] / total (each nullable).                        */
int  sls_plan_objective(sls_plan* plan, void* hip_stream, const double* d_values, int packed,
                        double* d_col_objective, double* d_total);
int  sls_plan_fetch_objective(sls_plan* plan, const double* d_values, int packed, double* col_objective, double* total);
/* ---- achievability residual of every column against the FULL plant, evaluated on the device from the written Φ -------------
 * sls_plan_fetch_status reports ‖Ez − f‖∞ of the reduced problem: the constraints restricted to the rows of s_x.  This is the
 * defect of the system-level identities Φx[1] = I, Φx[t+1] = A·Φx[t] + B2·Φu[t], 0 = A·Φx[T] + B2·Φu[T] on ALL rows of the plant,
 * per subproblem (global column c, 0-based t), against the values of A and B2 the plan holds NOW (sls_plan_update_plant):
 *     Δ[0] = Φx[0][:,c] − e_c,   Δ[t+1] = Φx[t+1][:,c] − A·Φx[t][:,c] − B2·Φu[t][:,c]  (t = 0 … T−2),
 *     Δ[T] = −A·Φx[T−1][:,c] − B2·Φu[T−1][:,c].
 * Φ is read through the subproblem's mask and destination table, like sls_plan_objective (a stored-false mask entry reads as
 * 0.0).  Rows of s_x are the LOCAL part; the HALO H(q) is the set of rows r ∉ s_x with A[r,j] stored for some j ∈ s_x or B2[r,k]
 * stored for some k ∈ s_u (by pattern, like the index sets) — rows the reduced problem never constrained: a mask wider at an
 * earlier step than at the last, or an actuator whose B2 column leaves s_x, puts a defect there that the status cannot show.
 * Row c belongs to H(q) when c ∉ s_x, so a SLS_COL_TRIVIAL column (Φ = 0) reports 1.0: against the full system that is its defect.
 * Per subproblem, in col_status order (a coupled or multi-column group reports one value per column, each a column of Φ):
 *     res_inf  = max |Δ[t][r]| over local and halo rows;   halo_inf = the same over halo rows only (exactly 0.0: H(q) empty);
 *     res_l1   = Σ_t Σ_r |Δ[t][r]|;
 * totals[0] = max res_inf, totals[1] = max res_l1 — the 𝓔₁ norm of Δ; robust SLS needs it below 1 to use the Φ of infeasible
 * (least-squares) columns.  Both objectives.  A NaN in Φ gives +inf.  Bit-identical from call to call and between the two
 * layouts (fixed summation order, no floating-point atomics).  A read-only pass of its own (csrc/sls_residual.hip): it reports
 * whatever was written last, an attached refinement included; a shard plan reports its own subproblems.  Plans of
 * sls_h2_sf_plan_localized are supported.  SLS_EINVAL for a NULL d_values.
 * sls_plan_residual: enqueue on hip_stream behind whatever wrote d_values and whatever sls_plan_update_plant enqueued there
 *   (layout `packed` as in sls_plan_execute); DEVICE outputs d_res_inf / d_halo_inf / d_res_l1 [n_subproblems] and d_totals[2],
 *   each may be NULL.  Asynchronous like sls_plan_execute, EXCEPT on first use per plan: the halo lists are built once on the host
 *   from the plan's index sets (read back from the device) and uploaded — synchronous copies; their buffers are the feature's
 *   own and not part of workspace_bytes.
 * sls_plan_fetch_residual: the same on the plan's stream (which first waits for the plan's last execute AND last update) into
 *   plan-owned buffers, waits, copies to the HOST arrays res_inf / halo_inf / res_l1 [n_subproblems] / totals[2] (each nullable). */
int  sls_plan_residual(sls_plan* plan, void* hip_stream, const double* d_values, int packed,
                       double* d_res_inf, double* d_halo_inf, double* d_res_l1, double* d_totals);
int  sls_plan_fetch_residual(sls_plan* plan, const double* d_values, int packed,
                             double* res_inf, double* halo_inf, double* res_l1, double* totals);
/* ---- gradient of the 𝓗₂ cost in the stored entries of A and B2 (plans built with SLS_PLAN_MULTIPLIERS) ---------
 * J = Σ_j c_j·J_j with J_j the number sls_plan_objective reports for subproblem j and c_j a caller-supplied column weight
 * (default 1).  With μ_j the multiplier of subproblem j's achievability constraints (E_jᵀμ_j = ∇_z J_j on its free variables;
 * block row 0 is x₀ = e, block row k is x_k − Ãx_{k−1} − B̃u_{k−1}; the kernel's iteration from λ = 0 gives the minimum-norm one
 * where E_j is rank deficient) the envelope theorem gives, for stored entries, in the CSC order of sls_plan_update_plant:
 *     ∂J/∂A[a,b]  = Σ_j c_j·[a ∈ s_x(j), b ∈ s_x(j)]·Σ_{k=1..T} μ_{j,k}[a]·x_{j,k−1}[b]
 *     ∂J/∂B2[a,m] = Σ_j c_j·[a ∈ s_x(j), m ∈ s_u(j)]·Σ_{k=1..T} μ_{j,k}[a]·u_{j,k−1}[m]
 * and, for a plan that also has SLS_PLAN_WEIGHTS_UPDATABLE, in the diagonals the plan holds now (sls_plan_fetch_weights):
 *     ∂J/∂c1[i] = 2·c1[i]·Σ_j c_j·b_j²·Σ_t x_{j,t}[i]²,   ∂J/∂d12[m] = 2·d12[m]·Σ_j c_j·b_j²·Σ_t u_{j,t}[m]²      (b_j = B1[c_j,c_j]).
 * x, u are read from d_values through the mask and the destination table (a fixed variable reads 0.0), μ from the buffer the
 * LAST execute wrote: d_values must be what that execute (full or partial) produced.  A subproblem whose status is neither
 * SLS_COL_OK nor SLS_COL_TRIVIAL contributes 0 (sls_plan_fetch_gradient counts them); so does a column with B1[c,c] = 0, whose cost
 * is constant.  Every sum runs in a fixed order (k ascending, then subproblems ascending; no floating-point atomics): the result
 * is bit-identical from call to call, between the two layouts, and whether the multipliers came from a full or a partial execute.
 * sls_plan_gradient: enqueue on hip_stream behind the execute that wrote d_values and the plan's last update (the stream waits
 *   for both); DEVICE outputs d_gA[nnz(A)], d_gB2[nnz(B2)], d_gc1[Nx], d_gd12[Nu], each may be NULL; d_col_weight: DEVICE
 *   n_subproblems values or NULL.  Asynchronous like sls_plan_objective, EXCEPT on first use per plan: the entry tables are built
 *   on the host from the index sets (read back from the device) and uploaded; their buffers and the multiplier buffer
 *   ((T+1)·32 doubles per subproblem) are the feature's own and not part of workspace_bytes.
 *   SLS_EINVAL without the flag, before the plan's first execute, and for d_gc1 / d_gd12 without SLS_PLAN_WEIGHTS_UPDATABLE.
 * sls_plan_fetch_gradient: the same on the plan's stream with HOST arrays (col_weight included; each nullable), waits;
 *   *n_skipped (nullable) = subproblems that contributed 0 because of their status.
 * sls_plan_fetch_multipliers: μ of subproblem `sub` (col_status order) as the last execute left it, to the HOST array
 *   mu[(T+1)·ñx], block-row major, rows in s_x order; len must be (T+1)·ñx.  mu = NULL with len = 0 is the size query: the
 *   call returns (T+1)·ñx (positive; every error code is negative) and copies nothing.                                        */
int  sls_plan_gradient(sls_plan* plan, void* hip_stream, const double* d_values, int packed, const double* d_col_weight,
                       double* d_gA, double* d_gB2, double* d_gc1, double* d_gd12);
int  sls_plan_fetch_gradient(sls_plan* plan, const double* d_values, int packed, const double* col_weight,
                             double* gA, double* gB2, double* gc1, double* gd12, int64_t* n_skipped);
int  sls_plan_fetch_multipliers(sls_plan* plan, int64_t sub, double* mu, int64_t len);
/* One-shot calls: opt in per context (default off: the one-shot calls do exactly what they do today).  With the option on,
 * sls_h2_sf_solve, sls_h2_sf_solve_batch (composite order: plant 0's columns, then plant 1's, …) and
 * sls_h2_sf_solve_localized evaluate on each device after the last launch (refinement included) and before the download.
 * sls_ctx_last_objective returns the values of the last such call in col_status order (n = its number of subproblems;
 * col_objective nullable).  SLS_EUNSUPPORTED after a call whose group list had overlapping groups (that Φ is a sum of
 * layers: no single objective belongs to a column); SLS_EINVAL when no solve has run with the option on, or n is wrong.   */
int  sls_ctx_want_objective(sls_ctx* ctx, int on);
int  sls_ctx_last_objective(sls_ctx* ctx, double* col_objective, int64_t n, double* total);
/* average device time of the solve over the timed sls_plan_execute calls since the last call, from HIP events on the launch
 * stream.  A plan that executes as one launch (sls_plan_describe lists one kernel, no refinement is attached) has the events
 * bound to that kernel's dispatch whenever its previous execute is still in flight: the average is then the dispatch's own
 * begin -> end, the interval a kernel trace reports, and no marker is queued around the kernel.  Every other plan
 * (size classes on forked streams, an attached refinement, the tile kernel behind its counter memset), an execute behind one
 * that has already finished and an execute on a capturing stream record the two events around the execute's work: the average
 * is the interval between the two stream markers, as before, which on one launch reads a few microseconds more.              */
int  sls_plan_kernel_time_ms(sls_plan* plan, double* avg_ms, int64_t* n_launches);
/* Human-readable list of the kernels one sls_plan_execute launches ("name nsub= grid= block= lds=;" per launch). */
int  sls_plan_describe(const sls_plan* plan, char* buf, int64_t buflen);
/* convenience for non-torch callers: device buffer management on the plan's device.  */
int  sls_plan_alloc_values(sls_plan* plan, int packed, double** d_values_out);
int  sls_plan_free_values(sls_plan* plan, double* d_values);
int  sls_plan_download(sls_plan* plan, const double* d_values /* mask order */,
                       double* const* phix_vals, double* const* phiu_vals);
void sls_plan_destroy(sls_plan* plan);

/* d_dst[idx[k]] = d_src[k], k < n  — unpack of the all-gathered packed shards.       */
int  sls_scatter_f64(sls_ctx* ctx, int dev_slot, void* hip_stream,
                     const double* d_src, const int64_t* d_idx, int64_t n, double* d_dst);

/* Cost-balanced contiguous cut of the groups into `nshards` ranges (cost model
 * Σ (T+1)·ñx³).  Fills cuts[nshards+1].  Pure host; needs no device.     */
int  sls_shard_groups(const sls_dims* dims, const sls_plant* P,
                      const sls_csc_bool* Sx, const sls_csc_bool* Su,
                      int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                      int nshards, int64_t* cuts);

/* Host-only symbolic pass for groups [group_begin, group_end): how many values the shard
 * produces (n_packed), the length of the full value array (n_values) and, when dest !=
 * NULL, the mask-order destination of every packed value (dest[n_packed]) — identical to
 * what a plan over the same range reports.  info (nullable) receives the symbolic part of
 * sls_plan_info (device = -1).  Needs no device: lets every rank know every other rank's
 * layout without communication, and lets the N>1 gather path be tested on CPU ranks.  */
int  sls_h2_sf_packed_layout(const sls_dims* dims, const sls_plant* P,
                             const sls_csc_bool* Sx, const sls_csc_bool* Su,
                             int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                             int64_t group_begin, int64_t group_end,
                             int64_t* n_packed, int64_t* n_values, int64_t* dest, sls_plan_info* info);

/* ---- (d,T)-localization masks: the README recipe (reference README.md:52-54), not part of the package itself -------
 *     𝓢x[t] = (A.≠0)^min(d,  ⌊α(t−1)⌋) .≠ 0                    t = 1..T   (Nx×Nx)
 *     𝓢u[t] = (B₂'.≠0)·(A.≠0)^min(d+1,⌊α(t−1)⌋) .≠ 0           t = 1..T   (Nu×Nx)
 * computed per column as level sets of exact k-step walks (= Boolean matrix powers), on host threads.  Two-call
 * protocol: with rowval_x == NULL only the counts are returned — nnz_x[t], nnz_u[t] (T entries each); the caller then
 * allocates, for every t, colptr_x[t] (Nx+1), rowval_x[t] (nnz_x[t]), colptr_u[t] (Nx+1), rowval_u[t] (nnz_u[t]) and
 * calls again.  Indices follow dims->index_base; rows ascend inside a column (a valid SparseMatrixCSC{Bool,Int} pattern,
 * every stored value true).  Only dims->Nx, Nu, T and index_base are read.  Pure host; needs no device.               */
int  sls_localization_masks(const sls_dims* dims, const sls_csc_f64* A, const sls_csc_f64* B2, int64_t d, double alpha,
                            int64_t* nnz_x, int64_t* nnz_u,
                            int64_t* const* colptr_x, int64_t* const* rowval_x,
                            int64_t* const* colptr_u, int64_t* const* rowval_u);

/* The same recipe computed on the device: one wave per column expands the level sets of A's pattern with an
 * LDS bitmap, in a count launch and a fill launch (csrc/sls_masks.hip); only A's and B2's patterns go up and only the Int64 row
 * indices come down.  Same arguments and two-call protocol as sls_localization_masks, bit-identical output; SLS_EUNSUPPORTED
 * when the state bitmap or a level set does not fit LDS (then use the host version). */
int  sls_localization_masks_device(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_f64* A, const sls_csc_f64* B2,
                                   int64_t d, double alpha, int64_t* nnz_x, int64_t* nnz_u,
                                   int64_t* const* colptr_x, int64_t* const* rowval_x,
                                   int64_t* const* colptr_u, int64_t* const* rowval_u);

/* ---- the same solve with the masks never leaving the device (SURVEY §8 row f1 on the solve path) --------------------------
 * For callers whose masks ARE the README recipe (reference README.md:52-54: 𝓢x[t] = (A.≠0)^min(d,⌊α(t−1)⌋), 𝓢u[t] =
 * (B₂'.≠0)(A.≠0)^min(d+1,⌊α(t−1)⌋)): the plan is built from (A, B₂, d, α, T) alone.  Level sets, index sets
 * (src/reduction.jl:14), the per-column mask slices (src/synthesis.jl:57-60) and the destinations (src/synthesis.jl:65-67) are
 * computed by device kernels (csrc/sls_masks.hip: column_tables_kernel) and stay in HBM; no mask array crosses PCIe in either
 * direction.  The value arrays come back in the CSC order of exactly the masks sls_localization_masks[_device] returns for the
 * same (d, α, T) — a caller that wants Φ as sparse matrices fetches the patterns with that call, a caller that feeds
 * sls_closed_loop_* or its own device code needs no pattern at all.
 * Restrictions (SLS_EUNSUPPORTED otherwise; pass the masks to sls_h2_sf_plan / sls_h2_sf_solve then): default groups [[i] for
 * i in 1:Nx]; the 3-argument Plant's cost ([C1 D12] = I, D11 = 0; C1/D11/D12 NULL or equal to that by value); no ridge term;
 * every mask row inside its column's index set (holds whenever A has a full diagonal, as every README-style plant has);
 * d + 2 ≤ 62; the whole plant on ONE device (the plan covers all columns; mask-order output only, packed = 0).
 * dims->T is the horizon; dims->flags selects the objective as usual.  Plans built this way are executed, queried and
 * destroyed like any other (sls_plan_execute with packed = 0, sls_plan_fetch_status, sls_plan_download, sls_plan_destroy). */
int  sls_h2_sf_plan_localized(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, int64_t d, double alpha,
                              sls_plan** plan_out);
/* One-shot form on device slot 0: plan (as above) + solve + download.  phix_vals[t] / phiu_vals[t], col_status, stats and the
 * return value as in sls_h2_sf_solve. */
int  sls_h2_sf_solve_localized(sls_ctx* ctx, const sls_dims* dims, const sls_plant* P, int64_t d, double alpha,
                               double* const* phix_vals, double* const* phiu_vals, int32_t* col_status, sls_stats* stats);

/* ---- closed-loop simulation with an on-device Φ (reference README.md:62-72; a user script there, not package code) ----
 *     β[:,t+1] = Σ_{τ=1..min(t,T−1)} Φx[τ+1]·(x[:,t+1−τ] − β[:,t+1−τ])
 *     u[:,t]   = Σ_{τ=1..min(t,T)}   Φu[τ]  ·(x[:,t+1−τ] − β[:,t+1−τ])
 *     x[:,t+1] = A·x[:,t] + B₁·w(t) + B₂·u[:,t]              t = 1..steps−1,   x[:,1] = β[:,1] = 0
 * for `nscen` disturbance scenarios at once.  sls_closed_loop_plan builds the row-oriented FIR operator from the masks
 * (P->A, B1, B2 are read; Φx must be square: Sx[t] is Nx×Nx) on device `dev_slot` of the context.
 * sls_closed_loop_run: d_values = Φ in the mask-order value array a plan's sls_plan_execute(packed = 0) fills (DEVICE);
 *   d_w [steps][Nw][nscen] (DEVICE; NULL = no disturbance; w(steps) is never read),
 *   d_x [steps][Nx][nscen], d_u [steps][Nu][nscen] (DEVICE, written; time-major, scenario innermost; x[0] = 0, u[steps−1] = 0
 *   as in the README's arrays).  Enqueues on `hip_stream` (NULL = null stream) and returns; steps−1 kernels replayed
 *   from a hipGraph that is cached while (d_w, d_x, d_u, steps, nscen) stay the same.
 * sls_closed_loop_run_host: same with HOST w/x/u (staged through device buffers; d_values stays a device pointer). */
typedef struct sls_loop sls_loop;
int  sls_closed_loop_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P,
                          const sls_csc_bool* Sx, const sls_csc_bool* Su, sls_loop** loop_out);
int  sls_closed_loop_run(sls_loop* loop, void* hip_stream, const double* d_values, const double* d_w,
                         int64_t steps, int64_t nscen, double* d_x, double* d_u);
int  sls_closed_loop_run_host(sls_loop* loop, const double* d_values, const double* h_w,
                              int64_t steps, int64_t nscen, double* h_x, double* h_u);
/* device time of the last sls_closed_loop_run (HIP events on its stream); synchronises on it */
int  sls_closed_loop_last_ms(sls_loop* loop, double* ms);
/* stored-true Φ entries one time step reads (12 B each: the HBM traffic model of the step kernel) */
int  sls_closed_loop_entries(const sls_loop* loop, int64_t* n_entries);
void sls_closed_loop_destroy(sls_loop* loop);

/* ---- stand-alone controller: one step from a measured state to u (csrc/sls_controller.hip) ----
 * What an SLS user deploys.  sls_closed_loop_* fuses the controller with ONE fixed linear plant; here the state comes from
 * outside, so the plant may differ from the design model, be non-linear or simulated elsewhere, or be measured, and Φ may be
 * swapped under a running controller (gain scheduling: sls_plan_update_plant, sls_plan_execute, sls_controller_load, next step).
 * Steps are numbered k = 0, 1, … since the last reset; step k takes x_k of `nscen` scenarios and gives
 *     ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
 *     u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
 *     β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}
 * (τ and the Φ indices 1-based as in the reference README.md:62-72; row k of the simulator's x, u arrays is step k here; a
 * non-zero x_0 acts as a disturbance at time 0, the SLS meaning of an initial condition; Φx[1] is not part of the operator and
 * stored-false mask entries are never read, as in the simulator).  Fed the x of a simulator run, the steps return that run's u
 * bit for bit in rows 0 … steps−2 (the simulator's last u row is the README's never-assigned zero; the controller computes it).
 * sls_controller_plan: masks only — Nx, Nu, T, index_base of dims are read; Sx[t] is Nx×Nx, Su[t] Nu×Nx.  nscen is fixed here
 *   and every buffer is allocated here: the row-ordered Φ, β (two copies) and the history of ŵ (a ring of 2^⌈log₂T⌉ slots, each
 *   stored twice); the controller starts in the reset state.  SLS_EUNSUPPORTED when (T+1)·Nx exceeds int32 (an entry's history
 *   offset is an int32) or nscen exceeds 65535·64.
 * sls_controller_load: d_values = Φ in the mask-order value array sls_plan_execute(packed = 0) fills (DEVICE), gathered into
 *   row order; β, the history and the step counter are NOT touched.
 * sls_controller_reset: β = 0, history = 0, k = 0.
 * sls_controller_step: d_x [Nx][nscen] (DEVICE), d_u [Nu][nscen] (DEVICE, written; may be NULL when Nu = 0), d_what [Nx][nscen]
 *   (DEVICE, written: ŵ_k) or NULL; scenario innermost, like the simulator's arrays.  One kernel launch.
 * load, reset and step allocate nothing and never wait for the device: they enqueue on `hip_stream` (NULL = null stream) and
 * return, like sls_plan_execute.  The step counter lives on the host and advances at enqueue; the caller issues the calls of
 * one controller on one stream or orders them with events.  SLS_EINVAL: a step before the first load, a null d_x, a null d_u
 * with Nu > 0, nscen < 1, a dev_slot out of range; the controller stays usable.  A step on a stream that is being captured
 * (hipStreamIsCapturing) returns SLS_EUNSUPPORTED: the ring position is a launch argument and a graph would freeze it.
 * sls_controller_info (each output nullable): stored-true Φ entries one step reads (12 B each), steps enqueued since the
 * last reset, and the device bytes of β and the history (what a reset clears). */
typedef struct sls_controller sls_controller;
int  sls_controller_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                         int64_t nscen, sls_controller** out);
int  sls_controller_load(sls_controller* ctl, void* hip_stream, const double* d_values);
int  sls_controller_reset(sls_controller* ctl, void* hip_stream);
int  sls_controller_step(sls_controller* ctl, void* hip_stream, const double* d_x, double* d_u, double* d_what);
int  sls_controller_info(const sls_controller* ctl, int64_t* n_entries, int64_t* steps_done, int64_t* state_bytes);
void sls_controller_destroy(sls_controller* ctl);

/* ---- closed-loop rollout of a resident Φ against an ensemble of plants (csrc/sls_rollout.hip, csrc/sls_rollout.h) ----
 * How a Φ behaves on plants that are NOT the design model.  Every one of `nscen` scenarios has its own VALUES of A and B2 on the
 * patterns given at plan time; B1 and Φ are shared.  Steps are numbered as for the controller; step k of scenario s is
 *     ŵ_k     = x_k − β_k                                   (β_0 = 0; ŵ_j = 0 for j < 0)
 *     u_k     = Σ_{τ=1..T}   Φu[τ]   · ŵ_{k+1−τ}
 *     β_{k+1} = Σ_{τ=1..T−1} Φx[τ+1] · ŵ_{k+1−τ}
 *     x_{k+1} = A⁽ˢ⁾·x_k + B1·w_k + B2⁽ˢ⁾·u_k
 *     J⁽ˢ⁾   += Σ_i (q_i·x_k[i])² + Σ_j (r_j·u_k[j])²        peak_x⁽ˢ⁾ = max(peak_x⁽ˢ⁾, max_i |x_k[i]|), peak_u likewise
 * x_0 comes from the reset (default 0; a non-zero x_0 acts as a disturbance at time 0: ŵ_0 = x_0).  After K steps in total J and
 * the peaks cover k = 0 … K−1; the current state x_K is not counted yet.  With the design plant, x_0 = 0 and one run, the recorded
 * x, u are rows 0 … steps−1 of sls_closed_loop_run bit for bit (the simulator's step restated on the controller's ring).  Device
 * memory does not depend on the number of steps.  Cost and peaks are accumulated per row by exactly one owner each and reduced in
 * a fixed order (sls_rollout.h): no floating-point atomics, bit-identical from run to run and however the steps are split into calls.
 * sls_rollout_plan: dims, P->A, P->B1, P->B2 (patterns and initial values) and the masks are read.  Everything is allocated here: Φ
 *   in row order, the mirrored ŵ ring of the controller, x and β (two copies each), the plant values per scenario in CSR order,
 *   scenario innermost ([nnz(A)][nscen], [nnz(B2)][nscen], every scenario initialised from P), a staging buffer of
 *   max(nnz(A), nnz(B2))·nscen doubles for the host path of set_plant, the weights q = 1, r = 1 and the per-row accumulators.  The
 *   object starts in the reset state.  Limits and codes as sls_controller_plan: SLS_EUNSUPPORTED when (T+1)·Nx exceeds int32 or
 *   nscen exceeds 65535·64; SLS_EINVAL for nscen < 1 or a dev_slot out of range.
 * sls_rollout_load: d_values = Φ in the mask-order value array sls_plan_execute(packed = 0) fills (DEVICE), as sls_controller_load;
 *   state, accumulators and the step counter are NOT touched, so Φ may be swapped in the middle of a rollout.
 * sls_rollout_set_plant: new plant values, in the caller's CSC nzval order — the convention of sls_plan_update_plant and
 *   sls_plan_fetch_plant, so a plan's current values pass straight through.  NULL keeps what is there.  per_scenario = 0: one
 *   array of nnz values, broadcast to all scenarios; per_scenario = 1: [nnz][nscen], scenario innermost.  on_device = 1: DEVICE
 *   arrays, read by a gather kernel on the stream (they must stay valid until it has run); on_device = 0: HOST arrays, copied to the
 *   staging buffer first — this path waits for the stream until the copy is done.  THE VALUES ARE NOT VALIDATED: no finite rule and
 *   no zero rule apply (a rollout has no kernel selection that depends on them); a NaN or an unstable plant simply shows in x, u
 *   and the cost.
 * sls_rollout_set_weights: q [Nx], rr [Nu] (NULL keeps; HOST or DEVICE by on_device; the host path waits for its copy) — the
 *   arrays of sls_plan_fetch_weights can be passed as they are.  Takes effect from the next step on; what is accumulated stays.
 * sls_rollout_reset: clears the ring, β, x, the accumulators and the step count; d_x0 [Nx][nscen] (DEVICE) or NULL for x_0 = 0.
 * sls_rollout_run: `steps` steps from the current state.  d_w [steps][Nw][nscen] (DEVICE) or NULL; d_x [steps][Nx][nscen] and
 *   d_u [steps][Nu][nscen] (DEVICE, each nullable) record x_k, u_k of the steps run — with both NULL only cost and peaks accumulate.
 *   One kernel launch per step; the call enqueues on `hip_stream` (NULL = null stream) and returns, allocates nothing and never
 *   waits.  steps = 0 is a no-op.  SLS_EINVAL before the first load or for steps < 0; SLS_EUNSUPPORTED on a stream that is being
 *   captured (the ring slot and the buffer parity are launch arguments); the object stays usable.
 * sls_rollout_stats: d_cost, d_peak_x, d_peak_u [nscen] each (DEVICE, nullable), of the steps run since the last reset; enqueued.
 * sls_rollout_fetch: the same into HOST arrays (nullable) plus x_now [Nx][nscen], the current state x_K; waits for the stream.
 * sls_rollout_info (each output nullable): stored-true Φ entries a step reads (12 B each), steps enqueued since the last reset,
 *   device bytes of the state (what a reset clears) and of the per-scenario plant values (a step reads them once: 8·nnz·nscen B).
 * The caller issues the calls of one object on one stream or orders them with events. */
typedef struct sls_rollout sls_rollout;
int  sls_rollout_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                      const sls_csc_bool* Su, int64_t nscen, sls_rollout** out);
int  sls_rollout_load(sls_rollout* r, void* hip_stream, const double* d_values);
int  sls_rollout_set_plant(sls_rollout* r, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device,
                           int per_scenario);
int  sls_rollout_set_weights(sls_rollout* r, void* hip_stream, const double* q, const double* rr, int on_device);
int  sls_rollout_reset(sls_rollout* r, void* hip_stream, const double* d_x0);
int  sls_rollout_run(sls_rollout* r, void* hip_stream, const double* d_w, int64_t steps, double* d_x, double* d_u);
int  sls_rollout_stats(sls_rollout* r, void* hip_stream, double* d_cost, double* d_peak_x, double* d_peak_u);
int  sls_rollout_fetch(sls_rollout* r, void* hip_stream, double* x_now, double* cost, double* peak_x, double* peak_u);
int  sls_rollout_info(const sls_rollout* r, int64_t* n_entries, int64_t* steps_done, int64_t* state_bytes, int64_t* plant_bytes);
void sls_rollout_destroy(sls_rollout* r);

/* ---- robust-stability margins of a resident Φ for an ensemble of plants (csrc/sls_margin.hip, csrc/sls_margin.h) ----
 * For which plants of an ensemble is the loop GUARANTEED stable, and how much can it amplify a bounded disturbance?  A finite
 * rollout cannot say; the defect of the achievability constraint can.  The controller of sls_controller_* on plant s,
 * x_{k+1} = A⁽ˢ⁾·x_k + B2⁽ˢ⁾·u_k + w̃_k, reconstructs a disturbance that obeys exactly
 *     ŵ_{k+1} = w̃_k − Σ_{τ=0..T−1} D⁽ˢ⁾[τ]·ŵ_{k−τ}
 *     D⁽ˢ⁾[τ] = Φx[τ+1] − A⁽ˢ⁾·Φx[τ] − B2⁽ˢ⁾·Φu[τ]           (0-based slices; Φx[0] := I, Φx[T] := 0)
 * and x = Φx ∗ ŵ, u = Φu ∗ ŵ.  The loop on plant s is internally stable when ‖D⁽ˢ⁾‖ < 1 in an induced norm,
 *     ‖D‖_𝓛₁ = max_i Σ_τ Σ_j |D[τ][i,j]|       ‖D‖_𝓔₁ = max_j Σ_τ Σ_i |D[τ][i,j]|,
 * and then ‖ŵ‖∞ ≤ ‖w̃‖∞ / (1 − ‖D‖_𝓛₁): every 𝓛₁ bound of sls_norms_l1 degrades by at most that factor.  A stored-false mask
 * entry is 0 and is never read; no value of Sx[0] is ever read.  D has a pattern that depends on the non-zero patterns only
 * (sls_margin.h); an entry's value is one fma chain over CSR row i of A⁽ˢ⁾, then of B2⁽ˢ⁾, in ascending position.
 * sls_margin_plan: dims, P->A, P->B2 (patterns and initial values; P->B1 is checked and not used) and the masks are read.
 *   Everything is allocated here: Φ by columns, the defect pattern by columns and by rows, the plant values per scenario as in
 *   sls_rollout_plan (every scenario initialised from P) with the staging buffer of set_plant, a scratch of 8·n_defect·nscen B
 *   that holds |D| of every pattern entry, and the result buffer of the fetch.  Codes and limits as sls_rollout_plan:
 *   SLS_EUNSUPPORTED when (T+1)·Nx exceeds int32, nscen exceeds 65535·64 or the defect pattern exceeds int32; SLS_EINVAL for
 *   nscen < 1 or a dev_slot out of range.
 * sls_margin_load: d_values = Φ in the mask-order value array sls_plan_execute(packed = 0) fills (DEVICE), gathered by columns.
 * sls_margin_set_plant: exactly the contract of sls_rollout_set_plant (CSC nzval order, NULL keeps, on_device, per_scenario; the
 *   host path waits for its copy; THE VALUES ARE NOT VALIDATED).
 * sls_margin_run: outputs on the DEVICE, each may be NULL, scenario innermost: d_row_l1 [Nx][nscen] = Σ_τ Σ_j |D⁽ˢ⁾[τ][i,j]|,
 *   d_col_l1 [Nx][nscen] = Σ_τ Σ_i |D⁽ˢ⁾[τ][i,j]|, d_totals [2][nscen] = ‖D⁽ˢ⁾‖_𝓛₁ then ‖D⁽ˢ⁾‖_𝓔₁.  Three launches; the call
 *   enqueues on `hip_stream` (NULL = null stream), allocates nothing and never waits.  A row or column without a pattern entry
 *   reports exactly 0.0.  A NaN in Φ or in a scenario's plant values gives +inf in the sums it reaches in that scenario and
 *   nothing elsewhere.  Every sum has one fixed order and one owner, no floating-point atomics: bit-identical from call to call,
 *   and the numbers of scenario s do not depend on nscen, on the scenario's position, on the other scenarios' values or on how
 *   the values arrived (shared or per scenario, host or device).  SLS_EINVAL before the first load; the object stays usable.
 * sls_margin_fetch: the same passes into the object's buffer, copied to HOST arrays (each nullable); waits for the stream.
 * sls_margin_info (each output nullable): stored-true Φ entries outside Sx[0], pattern entries of D, all device bytes of the
 *   object (the scratch included) and those of the per-scenario plant values.
 * The caller issues the calls of one object on one stream or orders them with events. */
typedef struct sls_margin sls_margin;
int  sls_margin_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                     const sls_csc_bool* Su, int64_t nscen, sls_margin** out);
int  sls_margin_load(sls_margin* m, void* hip_stream, const double* d_values);
int  sls_margin_set_plant(sls_margin* m, void* hip_stream, const double* A_nzval, const double* B2_nzval, int on_device,
                          int per_scenario);
int  sls_margin_run(sls_margin* m, void* hip_stream, double* d_row_l1, double* d_col_l1, double* d_totals);
int  sls_margin_fetch(sls_margin* m, void* hip_stream, double* row_l1, double* col_l1, double* totals);
int  sls_margin_info(const sls_margin* m, int64_t* n_entries, int64_t* n_defect, int64_t* device_bytes, int64_t* plant_bytes);
void sls_margin_destroy(sls_margin* m);

/* ---- worst-case 𝓛₁ margin over a box of plants (csrc/sls_margin_box.h, csrc/sls_margin_box.hip), on the same object ----
 * Every stored A[i,k], B2[i,m] of scenario s is known to ± a radius round the centre sls_margin_set_plant set.  Rows of D
 * decouple and a row's absolute sum is convex in the row's coefficients, so max over the box of ‖D‖_𝓛₁ = max_i max_σ f_i(σ) over
 * the 2^b_i sign patterns σ of the row's b_i uncertain coefficients: exact, and the plant that takes every row's arg-max vertex
 * attains all of them at once.  The ACTIVE LIST of row i: its CSR entries of A, then of B2, whose radius is > 0 in at least one
 * scenario; bit b of a vertex code set means centre + radius.  A row with more than 10 active coefficients reports the triangle
 * bound Σ|d⁰| + Σ_b ρ_b·Σ|φ_b| (an upper bound; exact = 0, vertex −1).
 * sls_margin_fetch_plant: the plant values as they are on the device — the centres of the box — to HOST arrays [nnz][nscen] in the
 *   CSC nzval order (each nullable); waits for the stream.
 * sls_margin_set_radius: HOST arrays in the CSC nzval order of A / B2, NULL = zeros, [nnz] or [nnz][nscen] by per_scenario.  A
 *   radius that is negative or not finite: SLS_EINVAL, the object unchanged.  A setup call: builds the active lists on the host,
 *   allocates (the first time) and waits for the device.  SLS_EUNSUPPORTED when Nx·nscen exceeds int32.
 * sls_margin_box_run: outputs on the DEVICE, each may be NULL, scenario innermost: d_row_wc [Nx][nscen] = the row's largest
 *   vertex sum, d_row_vertex [Nx][nscen] = its code (ties: the lowest; −1 for a bound row), d_totals [nscen] = max_i d_row_wc =
 *   the worst ‖D‖_𝓛₁ of the box.  Two launches; enqueues on `hip_stream`, allocates nothing and never waits.  Sums in the one
 *   order of sls_margin_run: with every radius 0, d_row_wc is its d_row_l1 bit for bit.  The numbers of scenario s do not depend
 *   on nscen, its position, the other scenarios or the call (the codes do, through the shared active lists; so does which rows
 *   are exact).  NaN as in sls_margin_run.  SLS_EINVAL before the first load or the first set_radius; the object stays usable.
 * sls_margin_box_fetch: the same pass into the object's buffer, copied to HOST arrays (each nullable); row_exact [Nx].  Waits.
 * sls_margin_box_worst_plant: box_fetch, then HOST arrays [nnz][nscen] in CSC nzval order (each nullable): centre ± radius by
 *   every row's vertex, centre + radius in a bound row.  Fit for sls_margin_set_plant / sls_rollout_set_plant (per_scenario).
 * sls_margin_box_info (each nullable; SLS_EINVAL before a set_radius): the longest active list, the rows on the bound path, the
 *   vertex sums one scenario evaluates (Σ 2^b_i over the exact rows), the device bytes set_radius allocated. */
int  sls_margin_fetch_plant(sls_margin* m, void* hip_stream, double* A_nzval, double* B2_nzval);
int  sls_margin_set_radius(sls_margin* m, const double* A_rad, const double* B2_rad, int per_scenario);
int  sls_margin_box_run(sls_margin* m, void* hip_stream, double* d_row_wc, int64_t* d_row_vertex, double* d_totals);
int  sls_margin_box_fetch(sls_margin* m, void* hip_stream, double* row_wc, int64_t* row_vertex, uint8_t* row_exact, double* totals);
int  sls_margin_box_worst_plant(sls_margin* m, void* hip_stream, double* A_nzval, double* B2_nzval);
int  sls_margin_box_info(const sls_margin* m, int64_t* max_bits, int64_t* n_inexact_rows, int64_t* n_vertex_sums,
                         int64_t* device_bytes);

/* ---- closed-loop 𝓛₁ and 𝓗∞ norms of a resident Φ (csrc/sls_norms.hip) ----
 * The two norms SLS designs are judged by beside the 𝓗₂ cost.  Built from the masks alone, like the controller.  Rows are the Nx
 * state rows followed by the Nu input rows, N = Nx + Nu; for t = 0 … T−1 (0-based)
 *     G[t] = diag(cz) · [Φx[t]; Φu[t]] · diag(b)        N × Nx, real          G(ω) = Σ_t G[t] · e^{−iωt}
 * cz [N] and b [Nx] are HOST vectors, NULL = all ones.  Unlike the controller, Φx[0] IS part of the operator (the identity block
 * of the closed-loop response); a stored-false mask entry is not, and is never read.  With cz the diagonal of [C1 D12], b the
 * diagonal of B1 and D11 = 0, G is the closed-loop map w → z; with both NULL it is Φ itself (the norms of the robust-SLS bounds).
 * Non-diagonal weights are not supported.
 * sls_norms_plan: Nx, Nu, T, index_base of dims are read.  Builds the entries twice — by rows (key t·Nx + col) and by columns
 *   (key t·N + row), each with a permutation into the mask-order value array — and allocates every buffer: both value orders,
 *   the work vectors of max_freq frequencies and the result buffer of the fetch calls.  SLS_EUNSUPPORTED when T·N exceeds int32
 *   (the keys are int32) or max_freq exceeds 65535·64; SLS_EINVAL for max_freq < 1, a non-finite weight, a dev_slot out of range.
 * sls_norms_load: d_values = Φ in the mask-order value array sls_plan_execute(packed = 0) fills (DEVICE); one gather launch
 *   fills both value orders, the weights folded in: the stored entry is Φ·(cz[row]·b[col]).
 * sls_norms_l1: outputs on the DEVICE, each may be NULL.  row_l1[i] = Σ_t Σ_j |G[t][i,j]| (N), col_l1[j] = Σ_t Σ_i |G[t][i,j]|
 *   (Nx), totals[0] = max_i row_l1 — the 𝓛₁ norm, the induced ℓ∞ → ℓ∞ gain — and totals[1] = max_j col_l1, the 𝓔₁ norm (the
 *   norm sls_plan_residual reports of Δ).  One wave per row or column, a fixed summation order, no floating-point atomics:
 *   bit-identical from call to call.  A NaN in Φ gives +inf in its row and its column.
 * sls_norms_hinf: omega = HOST array of nfreq ≤ max_freq angles in radians per sample.  cos(ω·t), sin(ω·t) are computed on the
 *   host and copied up through the context's pinned buffer, ordered on the stream.  For every frequency f, independently,
 *       v₀[j] = 1 + (uint32)(j·2654435761u)·2⁻³²            (then normalised)
 *       repeat iters times:   y = G(ω_f)·v ;   v ← G(ω_f)ᴴ·y ;   v ← v/‖v‖₂
 *       sigma[f] = ‖G(ω_f)·v‖₂
 *   d_sigma [nfreq] and d_peak [2] on the DEVICE, each may be NULL.  sigma[f] is a LOWER bound of σ_max(G(ω_f)) that does not
 *   decrease as iters grows (how fast it closes depends on the gap between the two largest singular values); the sigma of a
 *   frequency does not depend on the other frequencies of the call.  peak[0] = max_f sigma[f], peak[1] = the index of the first
 *   frequency that attains it, as a double.  THE PEAK IS A LOWER BOUND OF THE 𝓗∞ NORM ON THE CALLER'S GRID ONLY: a resonance
 *   between two grid points is not seen, and refining the grid is the caller's business.  SLS_EINVAL: nfreq < 1 or > max_freq,
 *   iters < 1, a non-finite ω, a call before the first load; the object stays usable.
 * load, l1 and hinf allocate nothing and enqueue on `hip_stream` (NULL = null stream); hinf waits only for an earlier twiddle
 * upload that still reads the pinned buffer.  The caller issues the calls of one object on one stream or orders them with events.
 * sls_norms_fetch_l1 / sls_norms_fetch_hinf: the same passes into the plan-owned buffer on `hip_stream`, waited for and copied
 *   to HOST arrays (each nullable), like sls_plan_fetch_objective.
 * sls_norms_info (each output nullable): stored-true entries (a pass reads 12 B each), device bytes held, max_freq.
 *
 * 𝓗₂ shares and covariance.  Under unit white w the steady-state covariance of z is Σ = Σ_{t<T} G[t]·G[t]ᵀ — exact for the FIR
 * closed loop from step T on.
 * sls_norms_h2: outputs on the DEVICE, each may be NULL.  row_h2[i] = Σ_t Σ_j G[t][i,j]² (N) is the variance of z_i, its square
 *   root the RMS of that state or actuator; col_h2[j] = Σ_t Σ_i G[t][i,j]² (Nx) is the share of disturbance j — with cz / b from
 *   the plant and D11 = 0 the number sls_plan_objective reports for column j; totals[0] = Σ_i row_h2[i], the squared 𝓗₂ norm,
 *   totals[1] = max_i row_h2[i].  The 𝓛₁ pass with fma(v, v, ·) per entry: a fixed order, no floating-point atomics, bit-identical
 *   from call to call; a sum that comes out NaN is reported as +inf.  Asynchronous on `hip_stream`, allocates nothing.  The
 *   plan-owned copy of the result takes the place of the 𝓛₁ one (a fetch call always makes its own pass first).
 * sls_norms_cov_pattern: the entries of Σ the caller wants, pair_i[p], pair_j[p] in HOST memory (index_base of the plan's dims
 *   applies): any order, duplicates and i == j allowed.  SLS_EINVAL for an index outside the N rows (the message names p) or
 *   npairs < 0, SLS_EUNSUPPORTED for npairs > 2³¹ − 1; the pattern in place is kept then.  Uploads the list and allocates it and
 *   a result buffer (16 B per pair, counted in sls_norms_info's device_bytes from then on); a second call replaces the first
 *   after the device is idle; npairs = 0 clears the pattern.  Waits; may be called before or after sls_norms_load.
 * sls_norms_cov: d_cov [npairs] on the DEVICE: cov[p] = Σ_t Σ_k G[t][i_p,k]·G[t][j_p,k], the sum over the keys the two row lists
 *   share, one wave per pair.  Bit-identical from call to call; (i,j) and (j,i) give the same bits; the value of a pair does not
 *   depend on the other pairs of the list or on its place in it; a pair without a shared key gives exactly 0.0; a NaN in a
 *   shared entry reaches that pair and no other.  SLS_EINVAL before the first load, without a pattern, for a NULL output (all
 *   refused before anything is enqueued).  Asynchronous, allocates nothing.
 * sls_norms_fetch_h2 / sls_norms_fetch_cov: the same passes into object-owned buffers, waited for and copied to HOST arrays
 *   (each nullable). */
typedef struct sls_norms sls_norms;
int  sls_norms_plan(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                    const double* cz, const double* b, int64_t max_freq, sls_norms** out);
int  sls_norms_load(sls_norms* norms, void* hip_stream, const double* d_values);
int  sls_norms_l1(sls_norms* norms, void* hip_stream, double* d_row_l1, double* d_col_l1, double* d_totals);
int  sls_norms_hinf(sls_norms* norms, void* hip_stream, const double* omega, int64_t nfreq, int64_t iters, double* d_sigma,
                    double* d_peak);
int  sls_norms_fetch_l1(sls_norms* norms, void* hip_stream, double* row_l1, double* col_l1, double* totals);
int  sls_norms_fetch_hinf(sls_norms* norms, void* hip_stream, const double* omega, int64_t nfreq, int64_t iters, double* sigma,
                          double* peak);
int  sls_norms_h2(sls_norms* norms, void* hip_stream, double* d_row_h2, double* d_col_h2, double* d_totals);
int  sls_norms_fetch_h2(sls_norms* norms, void* hip_stream, double* row_h2, double* col_h2, double* totals);
int  sls_norms_cov_pattern(sls_norms* norms, int64_t npairs, const int64_t* pair_i, const int64_t* pair_j);
int  sls_norms_cov(sls_norms* norms, void* hip_stream, double* d_cov);
int  sls_norms_fetch_cov(sls_norms* norms, void* hip_stream, double* cov);
int  sls_norms_info(const sls_norms* norms, int64_t* n_entries, int64_t* device_bytes, int64_t* max_freq);
void sls_norms_destroy(sls_norms* norms);

/* Symbolic pass only (replaces reference src/reduction.jl:11-27 for one group):
 * fills s_x / s_u (index_base of dims), returns their lengths.  Pure host.           */
int  sls_sparsity_dim_reduction(const sls_dims* dims, const sls_csc_f64* A,
                                const sls_csc_bool* Sx_last, const sls_csc_bool* Su_last,
                                const int64_t* cj, int64_t ncj,
                                int64_t* sx_out, int64_t* nsx, int64_t* su_out, int64_t* nsu);

/* The same sets for EVERY single-column subproblem c = 0..Nx-1 at once, on the device (one wave per
 * column, LDS bitmap union of the last masks' columns — csrc/sls_masks.hip).  CSR-style output: s_x(c) = sx_idx[sx_ptr[c]-b ..
 * sx_ptr[c+1]-b), ascending (the order the destination tables use; the reference's unique(findnz) order is the same set),
 * b = dims->index_base; likewise s_u.  Two-call protocol: with sx_idx == NULL only sx_ptr / su_ptr (Nx+1 each) are filled;
 * the caller allocates sx_idx (sx_ptr[Nx]-b entries) and su_idx and calls again.  SLS_EUNSUPPORTED when the state bitmap
 * does not fit LDS.                                                                                                    */
int  sls_index_sets_device(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_f64* A,
                           const sls_csc_bool* Sx_last, const sls_csc_bool* Su_last,
                           int64_t* sx_ptr, int64_t* sx_idx, int64_t* su_ptr, int64_t* su_idx);

#ifdef __cplusplus
}
#endif
#endif /* SLS_MI355X_H */
