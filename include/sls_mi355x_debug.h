/* sls_mi355x_debug.h — DIAGNOSTIC entry points of libsls_mi355x.so.
 *
 * Not part of the drop-in boundary (include/sls_mi355x.h): nothing here replaces a reference interface.  These are the
 * hooks the test-suite and the measurement scripts under tools/ use to look inside a plan — kernel phase counters, the
 * factor workspace, the per-column tables, the MFMA tile inversion on its own.  They are declared so that the shared
 * library exports nothing a header does not name (tests/test_host.py checks both directions); a host program has no
 * reason to call them and their signatures may change between rounds without an ABI version bump.
 */
#ifndef SLS_MI355X_DEBUG_H
#define SLS_MI355X_DEBUG_H

#include "sls_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-subproblem phase cycle counters (s_memtime) of the last execute: out[n_subproblems * 8].  Only when the plan was
 * built with SLS_PHASE_TIMERS=1..5 in the environment (tools/phase_breakdown*.py explain the slots); SLS_EINVAL otherwise. */
int sls_plan_debug_phase_cycles(sls_plan* plan, unsigned long long* out);

/* Copy `count` doubles of the plan's factor workspace (the pivot blocks P_k as the kernels left them), starting at
 * `offset`, to the host (tools/tile_check_factor.py). */
int sls_plan_debug_read_workspace(sls_plan* plan, int64_t offset, int64_t count, double* out);

/* The prepared records of the four-wave twisted kernel (one per column of a four-wave launch, built once at plan time by
 * twisted4_prepare_kernel), in col_status order.  *n_columns: their number; caps[4]: the list capacities (rows of Ã, of Ãᵀ,
 * of B̃2, of B̃2ᵀ); with E = 32·(caps[0] + caps[1] + caps[2]) + 64·caps[3] entries per column: columns[n] (col_status index),
 * counts[n][4] (longest list of each kind), indices[n][E] / values[n][E] (the lists arow [caps[0]][32], acol [caps[1]][32],
 * brow [caps[2]][32], bcol [caps[3]][64], zero padded; local indices / gathered operator values), bits[n][2] (mask-repeat
 * bits of the upward and the downward helper).  Every output but n_columns may be NULL.  SLS_EINVAL when the plan has no
 * four-wave launch. */
int sls_plan_debug_twisted4_tables(sls_plan* plan, int64_t* n_columns, int32_t* caps, int64_t* columns, int32_t* counts,
                                   int32_t* indices, double* values, uint64_t* bits);

/* The plan-time static blocks of the same columns (the second thing twisted4_prepare_kernel builds), in col_status order.
 * Block k of a column's block-tridiagonal Schur system has the static part
 *     S_k = δ·I + Wx_k + B̃·Wu_{k−1}·B̃ᵀ + Ã·Wx_{k−1}·Ãᵀ                          (no factor P in it: fixed by the plan),
 * slot k = 1 … T of the column's pool holds S_k, slot 0 the upward helper's first block: S_1 with δ·w/(δ + w) in the place of
 * Wx_0.  *n_columns: the columns; *n_slots = T + 1; delta[n]: the column's shift δ; valid[n][T + 1]: 1 where the kernel
 * filled the slot — exactly the slots a helper wave reads (the others are reused from a neighbour while the masks repeat, or
 * lie on the other side of the meeting block) — unfilled slots hold zeros; offsets[n + 1]: column i's doubles are
 * blocks[offsets[i] … offsets[i + 1]).  A column's pool is [T + 1][TQ][64] doubles, TQ = (offsets[i + 1] − offsets[i]) / (64·(T + 1))
 * = TR·(TR + 1)/2 with TR = 3 tile rows in the classes <32,10>, <32,12> and 4 in <32,14>, <32,16>: lane 8·a + b of the
 * helper's 8×8 lane grid owns the entries (a + 8·ri, b + 8·cj) of the block, 0 ≤ ri, cj < TR, and stores those with ri ≤ cj in
 * the order q = (0,0), (0,1), … (0,TR−1), (1,1), … — the upper block triangle of the symmetric S_k, rows and columns beyond ñx
 * included (δ on their diagonal).  Every output but n_columns may be NULL.  SLS_EINVAL when the plan has no four-wave launch
 * or keeps no pool (SLS_T4_PRESTATIC=0 in lab mode, or a pool beyond the plan's byte budget). */
/* The setup images of the same columns (the third thing twisted4_prepare_kernel builds, kept exactly when the static blocks
 * are), in col_status order: per column first the dense image of Ã the launch holds in LDS — ad_doubles[i] = 8·TR·40 doubles, row
 * i of Ã at [40·i … 40·i + ñx), zero elsewhere — then the weight table Wx, (T + 1) rows of 32: row k holds mask_k ⊙ H⁻¹ on the
 * column's ñx state rows, zero beyond them and in row T.  offsets[n + 1]: column i's doubles are images[offsets[i] … offsets[i + 1]).
 * Every output but n_columns may be NULL.  SLS_EINVAL when the plan has no four-wave launch or keeps no pool. */
int sls_plan_debug_twisted4_images(sls_plan* plan, int64_t* n_columns, int64_t* offsets, int32_t* ad_doubles, double* images);

int sls_plan_debug_twisted4_static(sls_plan* plan, int64_t* n_columns, int32_t* n_slots, int64_t* offsets, double* delta,
                                   uint8_t* valid, double* blocks);

/* Invert one dense SPD matrix (host, n×n row-major) with the tile kernel's blocked symmetric FP64-MFMA sweep — the unit
 * test of the MFMA operand / result lane maps (tests/test_gpu_tile.py).  mlds != 0: block resident in LDS. */
int sls_debug_tile_invert(sls_ctx* ctx, int dev_slot, int n, const double* h_A, double* h_out, int mlds);

/* The mask / destination tables of a one-device plan as the solve kernels see them, built on the host (host_tables = 1)
 * or expanded on the device from the compact form (0).  Null outputs: only *md_total (the tables' length) is returned.
 * *was_compact reports whether the device expansion actually ran (0 when some column is not regular). */
int sls_debug_plan_tables(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                          const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                          int host_tables, int64_t* md_total, uint8_t* mask_out, int32_t* dest_out, int32_t* was_compact);

/* The same tables (and the concatenated index sets s_x, s_u of all columns, 0-based: *n_idx entries) of a plan built by the
 * device-resident symbolic route (sls_h2_sf_plan_localized), for the bit-for-bit comparison with the host route. */
int sls_debug_plan_tables_localized(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, int64_t d, double alpha,
                                    int64_t* md_total, uint8_t* mask_out, int32_t* dest_out, int64_t* n_idx, int32_t* idx_out);

/* The text sls_plan_describe gives for the plan sls_h2_sf_plan would build from these inputs on a device with `ncu` compute
 * units: the host symbolic pass and kernel selection only — no context, no device (tests/test_host.py compares it with the
 * launch lists recorded in tests/golden/launch_lists.json). */
int sls_debug_describe_launches(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                                int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t group_begin,
                                int64_t group_end, int ncu, char* buf, int64_t buflen);

/* Host twin of sls_plan_objective (csrc/sls_objective.cpp): the host symbolic pass with explicit tables over all groups, then
 * the same formulas from HOST value arrays (phix_vals[t] / phiu_vals[t] as sls_h2_sf_solve fills them) in one serial loop.
 * Needs no device.  ridge_x / ridge_u: the weights of sls_set_ridge (Nx / Nu, NULL = none).  Outputs, each nullable:
 * col_objective[n_subproblems] in col_status order, *total, and per column the number of products its value sums
 * (col_terms) and the sum of their absolute values (col_abs) — what a bound on the summation order needs. */
int sls_debug_objective_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                             int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, const double* ridge_x,
                             const double* ridge_u, const double* const* phix_vals, const double* const* phiu_vals,
                             double* col_objective, double* total, int64_t* col_terms, double* col_abs);

/* Host twin of sls_plan_residual (csrc/sls_residual.cpp): the host symbolic pass with explicit tables over all groups, then
 * the same formulas from HOST value arrays (phix_vals[t] / phiu_vals[t] as sls_h2_sf_solve fills them) against P's A and B2 in
 * one serial loop, accumulated in long double.  Needs no device.  Outputs, each nullable, [n_subproblems] in col_status order
 * unless noted: res_inf, halo_inf, res_l1, totals[2]; what a summation-order bound 2·N·2⁻⁵³·S needs — ent_terms / ent_abs: the
 * largest N and the largest S over the entries Δ[t][r] of the column (bounds res_inf and halo_inf), l1_terms / l1_abs: N and S
 * of res_l1; halo_ptr[n_subproblems + 1] and halo_rows[halo_ptr[n_subproblems]] (halo_cap: its capacity; 0-based, ascending per
 * subproblem): H(q).  Call with halo_rows = NULL first for the length. */
int sls_debug_residual_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                            int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, const double* const* phix_vals,
                            const double* const* phiu_vals, double* res_inf, double* halo_inf, double* res_l1, double* totals,
                            int64_t* ent_terms, double* ent_abs, int64_t* l1_terms, double* l1_abs, int64_t* halo_ptr,
                            int32_t* halo_rows, int64_t halo_cap);

/* Host twin of sls_plan_update_plant (csrc/sls_symbolic.cpp: apply_operator_update): the four operator value arrays a plan of
 * (A, B2) holds — A_val / B_val in row order, At_val / Bt_val in the CSC order — after an update with A_nzval / B2_nzval
 * (either NULL = unchanged), plus the value map row_pos[nnz(A) + nnz(B2)] and the plan-time-zero marks.  Needs no device.
 * Every output is nullable and is filled even when the update is refused (SLS_EINVAL: the arrays then hold the plan-time
 * values, untouched). */
int sls_debug_operator_update_host(const sls_dims* dims, const sls_csc_f64* A, const sls_csc_f64* B2, const double* A_nzval,
                                   const double* B2_nzval, double* A_val, double* At_val, double* B_val, double* Bt_val,
                                   int32_t* row_pos, uint8_t* zero);

/* Host twin of the marks sls_plan_track_changes keeps (csrc/sls_symbolic.cpp: mark_affected_host): the host symbolic pass over
 * all groups, then dirty[n_subproblems] in col_status order — 1 where a flagged entry can move the subproblem (A[i,j] with i and j
 * in its s_x; B2[i,k] with i in s_x and k in s_u), 0 elsewhere.  changed_A[nnz(A)] / changed_B2[nnz(B2)]: one flag per CSC
 * position, either NULL = none.  Needs no device. */
int sls_debug_affected_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t ngroups,
                            const int64_t* group_ptr, const int64_t* group_cols, const uint8_t* changed_A, const uint8_t* changed_B2,
                            uint8_t* dirty);

/* The shape rule of SLS_PLAN_WEIGHTS_UPDATABLE that needs no index set (csrc/sls_weights.h: weights_shape_check): 0 and the
 * Nx + Nu diagonal values (C1's, then D12's; nullable) when C1 and D12 are each NULL or hold one stored entry per column on the
 * column's own z-row, SLS_EUNSUPPORTED with the reason otherwise.  dims and P are validated first.  Needs no device. */
int sls_debug_weights_shape_check(const sls_dims* dims, const sls_plant* P, double* diag);

/* The weight records of the host symbolic pass over all groups, and the host twin of sls_plan_update_weights
 * (csrc/sls_weights.cpp: weight_records_host).  dims->flags decides whether the pass is an updatable one
 * (SLS_PLAN_WEIGHTS_UPDATABLE); ridge_x / ridge_u: the weights of sls_set_ridge (NULL = none).  With c1_diag [Nx] and / or
 * d12_diag [Nu] given (updatable pass only, SLS_EINVAL otherwise) the update is then applied to the pass's records: strict = 1 as
 * the host path does (every value checked first; SLS_EINVAL and nothing written on a refusal), strict = 0 as the device kernel does
 * (refused values skipped and counted in *n_rejected).  Outputs, each nullable, [n_subproblems] in col_status order unless
 * noted: *n_w (doubles in the weight pool), has_w, off_w, n_x / n_u (ñx, ñu), w_pool [*n_w], obj_pool [2·n_subproblems],
 * b2 (B1[c,c]² of an updatable pass, else zeros), diag [Nx + Nu] (the diagonals after the update; updatable pass only),
 * dirty (1 where the update changed the bits of a record value).  Call with w_pool = NULL first for *n_w.  Needs no device. */
int sls_debug_weights_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t ngroups,
                           const int64_t* group_ptr, const int64_t* group_cols, const double* ridge_x, const double* ridge_u,
                           const double* c1_diag, const double* d12_diag, int strict, int64_t* n_w, int32_t* has_w, int64_t* off_w,
                           int32_t* n_x, int32_t* n_u, double* w_pool, double* obj_pool, double* b2, double* diag, uint8_t* dirty,
                           int64_t* n_rejected);

/* The tables of the stand-alone controller (sls_controller_plan) from the masks (dims: Nx, Nu, T, index_base are read), built
 * on the host by the routine the plan uses (csrc/sls_symbolic.cpp: build_controller_operator).  *n_entries: stored-true entries of
 * Sx[1..T−1] and Su[0..T−1]; row_ptr[Nx + Nu + 1]: the Nx β rows, then the Nu u rows; per entry, ascending in (lag, col) inside a
 * row: lag[e] = τ (1-based: Φx[τ+1] in a β row, Φu[τ] in a u row), col[e] (0-based), perm[e] = its index in the mask-order value
 * array.  Every output is nullable: call with only n_entries first for the length.  Needs no device. */
int sls_debug_controller_tables(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries,
                                int32_t* row_ptr, int32_t* lag, int32_t* col, int32_t* perm);

/* Host twin of sls_controller_step (csrc/sls_controller.cpp): `steps` steps from the reset state in one serial loop through the
 * same tables, the same mirrored ring and β double buffer (csrc/sls_controller.h), rows accumulated in long double and rounded
 * to double where the device stores one.  values: Φ in mask order (HOST); x [steps][Nx][nscen] (HOST); outputs, each nullable:
 * u [steps][Nu][nscen], what [steps][Nx][nscen] (ŵ).  Needs no device. */
int sls_debug_controller_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                              int64_t nscen, int64_t steps, const double* x, double* u, double* what);

/* Both tables of the closed-loop norm passes (sls_norms_plan) from the masks (dims: Nx, Nu, T, index_base are read), built on the
 * host by the routine the plan uses (csrc/sls_symbolic.cpp: build_norms_operator).  *n_entries: stored-true entries of Sx[0..T−1]
 * and Su[0..T−1].  Rows (N = Nx + Nu: state rows, then input rows): row_ptr[N + 1], row_key[e] = t·Nx + col ascending inside a
 * row; columns: col_ptr[Nx + 1], col_key[e] = t·N + row ascending inside a column; row_perm / col_perm: the entry's index in the
 * mask-order value array.  Every output is nullable: call with only n_entries first for the length.  Needs no device. */
int sls_debug_norms_tables(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries, int32_t* row_ptr,
                           int32_t* row_key, int32_t* row_perm, int32_t* col_ptr, int32_t* col_key, int32_t* col_perm);

/* Host twin of sls_norms_load + sls_norms_l1 + sls_norms_hinf (csrc/sls_norms.cpp): the same tables, twiddles and per-entry
 * operations in a plain loop order, in double.  values: Φ in mask order (HOST); cz [N], b [Nx]: NULL = ones.  Outputs, each
 * nullable: row_l1 [N], col_l1 [Nx], totals [2], sigma [nfreq], peak [2]; omega, nfreq and iters are read only when sigma or peak
 * is asked for.  Needs no device. */
int sls_debug_norms_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values, const double* cz,
                         const double* b, const double* omega, int64_t nfreq, int64_t iters, double* row_l1, double* col_l1,
                         double* totals, double* sigma, double* peak);

/* Host twin of sls_norms_load + sls_norms_h2 (csrc/sls_norms.cpp): fma(v, v, ·) per entry over the same tables, rows and entries
 * ascending, in double.  Outputs, each nullable: row_h2 [N], col_h2 [Nx], totals [2] (Σ row_h2, max row_h2).  Needs no device. */
int sls_debug_norms_h2_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values, const double* cz,
                            const double* b, double* row_h2, double* col_h2, double* totals);

/* Host twin of sls_norms_load + sls_norms_cov_pattern + sls_norms_cov (csrc/sls_norms.cpp): cov[p] = Σ over the keys rows
 * pair_i[p] and pair_j[p] share (index_base of dims applies) of fma(v_i, v_j, ·), by a two-pointer merge of the two row lists.
 * SLS_EINVAL for an index out of range (the message names p) or npairs < 0.  Needs no device. */
int sls_debug_norms_cov_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values, const double* cz,
                             const double* b, int64_t npairs, const int64_t* pair_i, const int64_t* pair_j, double* cov);

/* The plan-time tables of the ensemble rollout (sls_rollout_plan; csrc/sls_rollout.cpp: build_rollout_tables) beyond the
 * controller's: A and B2 by rows (A_ptr / B2_ptr [Nx + 1], A_idx / B2_idx column per CSR entry, ascending inside a row), A_src /
 * B2_src — the position in the caller's CSC nzval array the gather of sls_rollout_set_plant reads for each CSR entry — B2_owner
 * (1 where the entry's state row is the first, ascending, that stores the entry's column: that wave counts u_j in cost and
 * peak) and the orphan actuators (empty B2 column; counted by a wave of their own), ascending.  *n_entries: stored-true Φ
 * entries; *n_orphan.  Every output is nullable.  Needs no device. */
int sls_debug_rollout_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries,
                             int64_t* n_orphan, int32_t* A_ptr, int32_t* A_idx, int32_t* A_src, int32_t* B2_ptr, int32_t* B2_idx,
                             int32_t* B2_src, uint8_t* B2_owner, int32_t* orphan);

/* Host twin of a whole rollout (csrc/sls_rollout.cpp: RolloutHost — the tables, the mirrored ring, the double buffers, the owner
 * flags and the stats reduction of the device object in serial loops, rows accumulated in long double and rounded to double
 * where the device stores one): plan with P, load `values` (Φ in mask order, HOST), set_plant(A_nzval, B2_nzval, per_scenario)
 * (CSC order, NULL keeps P's), set_weights(q, rr) (NULL = ones), reset(x0) (NULL = 0), then `steps` steps with w
 * [steps][Nw][nscen] or NULL — as ONE run when nchunks = 0, else as nchunks runs of chunks[c] steps (they must add up to steps).
 * values2 non-NULL: that Φ is loaded before step switch_step, state kept.  Outputs, each nullable: x [steps][Nx][nscen],
 * u [steps][Nu][nscen], x_end [Nx][nscen] (the state after the last step), cost, peak_x, peak_u [nscen].  Needs no device. */
int sls_debug_rollout_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                           int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario, const double* q,
                           const double* rr, const double* x0, const double* w, int64_t steps, const int64_t* chunks, int64_t nchunks,
                           const double* values2, int64_t switch_step, double* x, double* u, double* x_end, double* cost,
                           double* peak_x, double* peak_u);

/* The plan-time tables of the robust-stability margins (sls_margin_plan; csrc/sls_margin.cpp: build_margin_tables).  Φ by
 * columns WITHOUT Sx[0]: phi_seg[Nx·T + 1] — column j, slice τ (0-based) is the segment [phi_seg[j·T + τ], phi_seg[j·T + τ + 1]) —
 * phi_row (state row i, or Nx + m for input row m; ascending inside a segment) and phi_perm (the entry's index in the mask-order
 * value array).  The defect pattern by columns: def_ptr[Nx + 1], def_key[d] = τ·Nx + i ascending inside a column, def_start[d] =
 * the position of Φx[τ+1][i,j] in the Φ list or −1; by rows: row_ptr[Nx + 1] and row_perm, the positions d of row i's entries,
 * ascending.  The plant by rows with the gather's source positions as in sls_debug_rollout_tables.  *n_entries: stored-true Φ
 * entries outside Sx[0]; *n_defect.  Every output is nullable: call with the two counts first for the lengths.  Needs no device. */
int sls_debug_margin_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries,
                            int64_t* n_defect, int32_t* phi_seg, int32_t* phi_row, int32_t* phi_perm, int32_t* def_ptr, int32_t* def_key,
                            int32_t* def_start, int32_t* row_ptr, int32_t* row_perm, int32_t* A_ptr, int32_t* A_idx, int32_t* A_src,
                            int32_t* B2_ptr, int32_t* B2_idx, int32_t* B2_src);

/* Host twin of sls_margin_plan + load + set_plant + run (csrc/sls_margin.cpp: margin_host — the same tables, the same fma chain
 * per entry (csrc/sls_margin.h: margin_entry), the sums in long double rounded once).  values: Φ in mask order (HOST); A_nzval /
 * B2_nzval: CSC order, NULL keeps P's, [nnz] or [nnz][nscen] by per_scenario.  Outputs, each nullable: row_l1, col_l1
 * [Nx][nscen], totals [2][nscen]; and the error model of each: row_n / col_n [Nx] = the number N of terms (start values and
 * products) that went into the output, row_s / col_s [Nx][nscen] = the sum S of their absolute values; tot_n [2], tot_s
 * [2][nscen] = the maxima over rows / columns.  A double evaluation in any order lies within 2·N·2⁻⁵³·S of the exact value.
 * Needs no device. */
int sls_debug_margin_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                          int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario, double* row_l1, double* col_l1,
                          double* totals, int64_t* row_n, int64_t* col_n, int64_t* tot_n, double* row_s, double* col_s, double* tot_s);

/* Host twin of sls_margin_plan + load + set_plant + set_radius + box_run (csrc/sls_margin_box.cpp: margin_box_host — the same
 * tables and active lists, d⁰ by margin_entry_signed, every vertex in long double rounded once).  Plant values as above; A_rad /
 * B2_rad: CSC order, NULL = zeros, [nnz] or [nnz][nscen] by rad_per_scenario (SLS_EINVAL for a negative or non-finite radius).
 * Outputs, each nullable: row_wc, row_vertex [Nx][nscen], row_exact [Nx], totals [nscen], the worst plant A_worst / B2_worst
 * [nnz][nscen] (CSC order), the active lists act_ptr [Nx + 1] and act_ent [≤ nnz(A) + nnz(B2)] (coefficient c < nnz(A): CSR entry
 * c of A, else CSR entry c − nnz(A) of B2), and the error model of row_wc: row_n [Nx] = the number N of terms (start values, centre
 * products, ρ·φ products), row_s [Nx][nscen] = the sum S of their absolute values; a double evaluation of a vertex sum or of the
 * triangle bound lies within 2·N·2⁻⁵³·S of its exact value.  Needs no device. */
int sls_debug_margin_box_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                              int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario, const double* A_rad,
                              const double* B2_rad, int rad_per_scenario, double* row_wc, int64_t* row_vertex, uint8_t* row_exact,
                              double* totals, int64_t* row_n, double* row_s, double* A_worst, double* B2_worst, int32_t* act_ptr,
                              int32_t* act_ent);
/* fabs(margin_entry_signed) against margin_entry (csrc/sls_margin_box.h, csrc/sls_margin.h) on every pattern entry and scenario of
 * the plant given as above: *n_entries = the entries compared, *n_mismatch = those whose 64 bits differ, *n_negative = those whose
 * signed value is below 0 (so that the comparison is not empty).  Needs no device. */
int sls_debug_margin_entry_signed(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                                  const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario,
                                  int64_t* n_entries, int64_t* n_mismatch, int64_t* n_negative);

/* The entry tables of sls_plan_gradient and its host twin (csrc/sls_gradient.cpp) for the plan sls_h2_sf_plan would build from
 * these inputs.  Call with every output NULL but n_slots to size the arrays.  Tables, each nullable: *n_slots = listed entries
 * over all subproblems; ent_ptr [n_subproblems + 1]; ent [3·n_slots] = (position, local row, local column) per listed entry —
 * position: CSC position in A's nzval, or nnz(A) + that in B2's; inv_ptr [nnz(A) + nnz(B2) + 1]; inv_slot / inv_sub [n_slots]:
 * per stored entry its slots and their subproblems, ascending.  Twin, when mu is given: mu holds (T+1)·ñx doubles per
 * subproblem, concatenated in col_status order, block-row major (what sls_plan_fetch_multipliers returns); phix_vals /
 * phiu_vals as sls_plan_download gives them; col_status / col_weight nullable.  Accumulates in long double in the device's
 * order: gA / gB2, per entry abs_A / abs_B2 = Σ|terms| and terms_A / terms_B2 = the number N of products — a double evaluation
 * in any order lies within N·2⁻⁵³·Σ|terms| (first order) of the exact sum.  Needs no device. */
int sls_debug_gradient_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                            int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t* n_slots,
                            int64_t* ent_ptr, int32_t* ent, int64_t* inv_ptr, int64_t* inv_slot, int32_t* inv_sub,
                            const double* mu, const double* const* phix_vals, const double* const* phiu_vals,
                            const int32_t* col_status, const double* col_weight, double* gA, double* gB2, double* abs_A,
                            double* abs_B2, int64_t* terms_A, int64_t* terms_B2);

#ifdef __cplusplus
}
#endif
#endif /* SLS_MI355X_DEBUG_H */
