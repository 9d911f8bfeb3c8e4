// sls_debug.cpp — the exports of include/sls_mi355x_debug.h that look into a plan or run a host twin: diagnostics for the tests
// and the tools, not part of the drop-in ABI.  (sls_debug_controller_* live with the controller, sls_controller.hip; the
// tables and the 𝓛₁ / 𝓗∞ twin of the norms with sls_norms.hip.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "../../include/sls_mi355x_debug.h"
#include "sls_gradient.h"
#include "sls_margin.h"
#include "sls_margin_box.h"
#include "sls_norms.h"
#include "sls_objective.h"
#include "sls_plan.h"
#include "sls_residual.h"
#include "sls_routing.h"
#include "sls_symbolic.h"
#include "sls_weights.h"

using namespace sls;

extern "C" {

/* diagnostics (include/sls_mi355x_debug.h): the tables of a plan built by the device-resident route, for the bit-for-bit
   comparison with the host route's (sls_debug_plan_tables) */
int sls_debug_plan_tables_localized(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, int64_t d, double alpha,
                                    int64_t* md_total, uint8_t* mask_out, int32_t* dest_out, int64_t* n_idx, int32_t* idx_out) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  sls_plan* pl = nullptr;
  int rc = sls_h2_sf_plan_localized(ctx, dev_slot, dims, P, d, alpha, &pl);
  if (rc) return rc;
  const int64_t n = pl->sym.md_total;
  int64_t ni = 0;
  for (const SubDesc& sd : pl->sym.subs) ni += sd.n + sd.m;
  if (md_total) *md_total = n;
  if (n_idx) *n_idx = ni;
  hipError_t e = hipSuccess;
  if (n > 0 && mask_out) e = hipMemcpy(mask_out, pl->kp.mask_pool, (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && n > 0 && dest_out) e = hipMemcpy(dest_out, pl->d_dest, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && ni > 0 && idx_out) e = hipMemcpy(idx_out, pl->kp.idx_pool, (size_t)ni * sizeof(int32_t), hipMemcpyDeviceToHost);
  sls_plan_destroy(pl);
  if (e != hipSuccess) return hipfail(ctx, e, "hipMemcpy D2H (tables)");
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the host twin of the device evaluation — symbolic pass with explicit tables, then
   the same formulas from host arrays in one serial loop (csrc/sls_objective.cpp).  Needs no device. */
int sls_debug_objective_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                             int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, const double* ridge_x,
                             const double* ridge_u, const double* const* phix_vals, const double* const* phiu_vals,
                             double* col_objective, double* total, int64_t* col_terms, double* col_abs) {
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  if (!phix_vals || !phiu_vals) return fail(nullptr, SLS_EINVAL, "null value arrays");
  in.reg_x = ridge_x; in.reg_u = ridge_u;
  Symbolic S;
  S.want_packed = false; S.compact = false;
  std::vector<int64_t> gptr, gcols;
  normalise_groups(in, gptr, gcols);
  rc = build_symbolic(in, 0, (int64_t)gptr.size() - 1, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  std::vector<double> vals((size_t)std::max<int64_t>(S.n_values, 1), 0.0);
  for (int64_t t = 0; t < S.T; ++t) {
    const int64_t nx = S.off_x[t + 1] - S.off_x[t], nu = S.off_u[t + 1] - S.off_u[t];
    if ((nx > 0 && !phix_vals[t]) || (nu > 0 && !phiu_vals[t])) return fail(nullptr, SLS_EINVAL, "null phix_vals[t]/phiu_vals[t]");
    if (nx > 0) std::copy(phix_vals[t], phix_vals[t] + nx, vals.begin() + S.off_x[t]);
    if (nu > 0) std::copy(phiu_vals[t], phiu_vals[t] + nu, vals.begin() + S.off_u[t]);
  }
  rc = objective_host(S, (dims->flags & SLS_SOLVE_SUM_OF_NORMS) ? 1 : 0, vals.data(), col_objective, total, col_terms, col_abs, msg);
  if (rc) return fail(nullptr, rc, msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the host twin of sls_plan_residual — symbolic pass with explicit tables, then the
   same formulas from host arrays in one serial loop (csrc/sls_residual.cpp).  Needs no device. */
int sls_debug_residual_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                            int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, const double* const* phix_vals,
                            const double* const* phiu_vals, double* res_inf, double* halo_inf, double* res_l1, double* totals,
                            int64_t* ent_terms, double* ent_abs, int64_t* l1_terms, double* l1_abs, int64_t* halo_ptr,
                            int32_t* halo_rows, int64_t halo_cap) {
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  if (!phix_vals || !phiu_vals) return fail(nullptr, SLS_EINVAL, "null value arrays");
  Symbolic S;
  S.want_packed = false; S.compact = false;
  std::vector<int64_t> gptr, gcols;
  normalise_groups(in, gptr, gcols);
  rc = build_symbolic(in, 0, (int64_t)gptr.size() - 1, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  std::vector<double> vals((size_t)std::max<int64_t>(S.n_values, 1), 0.0);
  for (int64_t t = 0; t < S.T; ++t) {
    const int64_t nx = S.off_x[t + 1] - S.off_x[t], nu = S.off_u[t + 1] - S.off_u[t];
    if ((nx > 0 && !phix_vals[t]) || (nu > 0 && !phiu_vals[t])) return fail(nullptr, SLS_EINVAL, "null phix_vals[t]/phiu_vals[t]");
    if (nx > 0) std::copy(phix_vals[t], phix_vals[t] + nx, vals.begin() + S.off_x[t]);
    if (nu > 0) std::copy(phiu_vals[t], phiu_vals[t] + nu, vals.begin() + S.off_u[t]);
  }
  std::vector<int64_t> hp;
  std::vector<int32_t> hr;
  rc = residual_host(S, vals.data(), res_inf, halo_inf, res_l1, totals, ent_terms, ent_abs, l1_terms, l1_abs, &hp, &hr, msg);
  if (rc) return fail(nullptr, rc, msg);
  if (halo_ptr) std::copy(hp.begin(), hp.end(), halo_ptr);
  if (halo_rows) {
    if (halo_cap < (int64_t)hr.size()) return fail(nullptr, SLS_EINVAL, "sls_debug_residual_host: halo_rows is shorter than halo_ptr[n_subproblems]");
    std::copy(hr.begin(), hr.end(), halo_rows);
  }
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the host twin of sls_plan_update_plant — the operator arrays of a plan of (A, B2),
   the value map and zero marks, then apply_operator_update with the new nzval arrays.  Needs no device. */
int sls_debug_operator_update_host(const sls_dims* dims, const sls_csc_f64* A, const sls_csc_f64* B2, const double* A_nzval,
                                   const double* B2_nzval, double* A_val, double* At_val, double* B_val, double* Bt_val,
                                   int32_t* row_pos, uint8_t* zero) {
  Symbolic S;
  std::string msg;
  int rc = operator_csr_checked(dims, A, B2, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  OperatorValueMap M;
  build_operator_value_map(S, M);
  rc = apply_operator_update(S, M, A_nzval, B2_nzval, msg);
  if (A_val) std::copy(S.A_csr.val.begin(), S.A_csr.val.end(), A_val);
  if (At_val) std::copy(S.At_csr.val.begin(), S.At_csr.val.end(), At_val);
  if (B_val) std::copy(S.B_csr.val.begin(), S.B_csr.val.end(), B_val);
  if (Bt_val) std::copy(S.Bt_csr.val.begin(), S.Bt_csr.val.end(), Bt_val);
  if (row_pos) std::copy(M.row_pos.begin(), M.row_pos.end(), row_pos);
  if (zero) std::copy(M.zero.begin(), M.zero.end(), zero);
  if (rc) return fail(nullptr, rc, msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the host twin of the marks sls_plan_track_changes keeps — the host symbolic pass
   over all groups, then mark_affected_host with the caller's changed flags.  Needs no device. */
int sls_debug_affected_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t ngroups,
                            const int64_t* group_ptr, const int64_t* group_cols, const uint8_t* changed_A, const uint8_t* changed_B2,
                            uint8_t* dirty) {
  if (!dirty) return fail(nullptr, SLS_EINVAL, "null argument");
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  std::vector<int64_t> gptr, gcols;
  normalise_groups(in, gptr, gcols);
  Symbolic S;
  S.want_packed = false; S.compact = false;
  rc = build_symbolic(in, 0, (int64_t)gptr.size() - 1, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  OperatorValueMap M;
  build_operator_value_map(S, M);
  std::fill(dirty, dirty + S.subs.size(), (uint8_t)0);
  rc = mark_affected_host(S, M, changed_A, changed_B2, dirty, msg);
  if (rc) return fail(nullptr, rc, msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the index-set-free part of the updatable shape rule.  Needs no device. */
int sls_debug_weights_shape_check(const sls_dims* dims, const sls_plant* P, double* diag) {
  Inputs in{dims, P, nullptr, nullptr, 0, nullptr, nullptr};
  std::string msg;
  if (!dims || !P) return fail(nullptr, SLS_EINVAL, "null dims/plant");
  sls_dims d0 = *dims; d0.T = 1;                       // the masks are not looked at: validate the plant alone
  {
    // validate_inputs wants masks; an empty Nx×Nx / Nu×Nx pair of one time step serves
    std::vector<int64_t> cp((size_t)dims->Nx + 1, dims->index_base);
    sls_csc_bool sx{dims->Nx, dims->Nx, cp.data(), nullptr, nullptr}, su{dims->Nu, dims->Nx, cp.data(), nullptr, nullptr};
    in.dims = &d0; in.Sx = &sx; in.Su = &su;
    int rc = validate_inputs(in, msg);
    if (rc) return fail(nullptr, rc, msg);
  }
  std::vector<double> dg;
  int rc = weights_shape_check(dims, P, dg, msg);
  if (rc) return fail(nullptr, rc, msg);
  if (diag) std::copy(dg.begin(), dg.end(), diag);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the weight records of the host symbolic pass and the host twin of
   sls_plan_update_weights on them.  Needs no device. */
int sls_debug_weights_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t ngroups,
                           const int64_t* group_ptr, const int64_t* group_cols, const double* ridge_x, const double* ridge_u,
                           const double* c1_diag, const double* d12_diag, int strict, int64_t* n_w, int32_t* has_w, int64_t* off_w,
                           int32_t* n_x, int32_t* n_u, double* w_pool, double* obj_pool, double* b2, double* diag, uint8_t* dirty,
                           int64_t* n_rejected) {
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  in.reg_x = ridge_x; in.reg_u = ridge_u;
  std::vector<int64_t> gptr, gcols;
  normalise_groups(in, gptr, gcols);
  Symbolic S;
  S.want_packed = false; S.compact = false;
  rc = build_symbolic(in, 0, (int64_t)gptr.size() - 1, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  const size_t ns = S.subs.size();
  if (n_rejected) *n_rejected = 0;
  if (dirty) std::fill(dirty, dirty + ns, (uint8_t)0);
  int rcu = 0;
  if (c1_diag || d12_diag) {
    if (!S.wu.updatable) return fail(nullptr, SLS_EINVAL, "weights update: the symbolic pass was not made with SLS_PLAN_WEIGHTS_UPDATABLE");
    if (strict) rcu = check_weights_update(S.wu, S.Nx, S.Nu, c1_diag, d12_diag, msg);
    if (!rcu) rcu = weight_records_host(S, c1_diag, d12_diag, S.w_pool.data(), S.wu.diag.data(), dirty, n_rejected, msg);
  }
  if (n_w) *n_w = (int64_t)S.w_pool.size();
  for (size_t q = 0; q < ns; ++q) {
    if (has_w) has_w[q] = S.subs[q].has_w;
    if (off_w) off_w[q] = S.subs[q].off_w;
    if (n_x) n_x[q] = S.subs[q].n;
    if (n_u) n_u[q] = S.subs[q].m;
    if (b2) b2[q] = S.wu.updatable ? S.wu.b2[q] : 0.0;
  }
  if (w_pool) std::copy(S.w_pool.begin(), S.w_pool.end(), w_pool);
  if (obj_pool) std::copy(S.obj_pool.begin(), S.obj_pool.end(), obj_pool);
  if (diag && S.wu.updatable) std::copy(S.wu.diag.begin(), S.wu.diag.end(), diag);
  if (rcu) return fail(nullptr, rcu, msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the launch list sls_plan_describe would print for a plan of these inputs on a
 * device with `ncu` compute units — symbolic pass + kernel selection on the host, no context, no device */
int sls_debug_describe_launches(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                                int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t group_begin,
                                int64_t group_end, int ncu, char* buf, int64_t buflen) {
  if (!buf || buflen <= 0 || ncu <= 0) return fail(nullptr, SLS_EINVAL, "bad argument");
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  Symbolic S;
  rc = build_symbolic(in, group_begin, group_end, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  RoutingResult route;
  rc = build_launch_list(S, (int)S.T, (dims->flags & SLS_SOLVE_SUM_OF_NORMS) ? 1 : 0, ncu, false, RoutingKnobs::from_env(), route, msg);
  if (rc) return fail(nullptr, rc, msg);
  std::string d;
  for (const LaunchSpec& L : route.launches) d += describe_launch(L);
  std::snprintf(buf, (size_t)buflen, "%s", d.c_str());
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): per-subproblem phase cycle counters when SLS_PHASE_TIMERS is set */
int sls_plan_debug_phase_cycles(sls_plan* plan, unsigned long long* out /* n_subproblems*8 */) {
  if (!plan || !out) return fail(nullptr, SLS_EINVAL, "null argument");
  if (!plan->kp.dbg) return fail(plan->ctx, SLS_EINVAL, "phase timers are off (set SLS_PHASE_TIMERS=1 before planning)");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = wait_plan_done(plan)) return rc;
  HIPCHK(plan->ctx, hipMemcpy(out, plan->kp.dbg, (size_t)plan->kp.nsub * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): invert one dense SPD matrix (host, n×n row-major) with the tile kernel's blocked
 * symmetric MFMA sweep — the unit test of the FP64 MFMA operand / result lane maps (tests/test_gpu_tile.py) */
int sls_debug_tile_invert(sls_ctx* ctx, int dev_slot, int n, const double* h_A, double* h_out, int mlds) {
  if (!ctx || !h_A || !h_out || n <= 0) return fail(ctx, SLS_EINVAL, "bad argument");
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "dev_slot out of range");
  HIPCHK(ctx, hipSetDevice(ctx->devs[dev_slot]));
  const size_t nn = (size_t)n * n, wsd = (size_t)tile_ht(tile_nt(n)) * 256;
  double *dA = nullptr, *dO = nullptr, *dW = nullptr;
  HIPCHK(ctx, hipMalloc(&dA, nn * 8));
  hipError_t e = hipMalloc(&dO, nn * 8);
  if (e == hipSuccess) e = hipMalloc(&dW, wsd * 8);
  if (e == hipSuccess) e = hipMemcpy(dA, h_A, nn * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_tile_invert(dA, n, dW, dO, mlds != 0, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(h_out, dO, nn * 8, hipMemcpyDeviceToHost);
  (void)hipFree(dA); (void)hipFree(dO); (void)hipFree(dW);
  if (e != hipSuccess) return hipfail(ctx, e, "sls_debug_tile_invert");
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the mask / destination tables of a one-device plan as the solve kernels see them,
   built on the host (host_tables = 1) or expanded on the device from the compact form (0).  Call with null outputs for the
   length.  `was_compact` reports whether the device expansion actually ran (0 when some column is not regular). */
int sls_debug_plan_tables(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                          const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                          int host_tables, int64_t* md_total, uint8_t* mask_out, int32_t* dest_out, int32_t* was_compact) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  sls_plan* pl = nullptr;
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::vector<int64_t> gptr, gcols;
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(ctx, rc, msg);
  normalise_groups(in, gptr, gcols);
  PlanOpts opt; opt.host_tables = host_tables ? 1 : 0;
  rc = plan_create(ctx, dev_slot, dims, P, Sx, Su, ngroups, group_ptr, group_cols, 0, (int64_t)gptr.size() - 1, false, opt, &pl);
  if (rc) return rc;
  const int64_t n = pl->sym.md_total;
  if (md_total) *md_total = n;
  if (was_compact) *was_compact = pl->sym.compact ? 1 : 0;
  hipError_t e = hipSuccess;
  if (n > 0 && mask_out) e = hipMemcpy(mask_out, pl->kp.mask_pool, (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && n > 0 && dest_out) e = hipMemcpy(dest_out, pl->d_dest, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
  sls_plan_destroy(pl);
  if (e != hipSuccess) return hipfail(ctx, e, "hipMemcpy D2H (tables)");
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): copy `count` doubles of the factor workspace, starting at `offset`, to the host */
int sls_plan_debug_read_workspace(sls_plan* plan, int64_t offset, int64_t count, double* out) {
  if (!plan || !out || offset < 0 || count < 0) return fail(nullptr, SLS_EINVAL, "bad argument");
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  if (int rc = wait_plan_done(plan)) return rc;
  HIPCHK(plan->ctx, hipMemcpy(out, plan->kp.fac_ws + offset, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the prepared records of the four-wave columns, in col_status order */
int sls_plan_debug_twisted4_tables(sls_plan* plan, int64_t* n_columns, int32_t* caps, int64_t* columns, int32_t* counts,
                                   int32_t* indices, double* values, uint64_t* bits) {
  if (!plan || !n_columns) return fail(nullptr, SLS_EINVAL, "null argument");
  if (!plan->t4_records) return fail(plan->ctx, SLS_EINVAL, "this plan has no four-wave launch");
  const KernelParams& kp = plan->kp;
  *n_columns = plan->t4_records;
  if (caps) { caps[0] = kp.w_nzA; caps[1] = kp.w_nzAc; caps[2] = kp.w_nzB; caps[3] = kp.w_nzBc; }
  if (!columns && !counts && !indices && !values && !bits) return 0;
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  std::vector<unsigned char> host((size_t)(plan->t4_records * plan->t4_stride));
  HIPCHK(plan->ctx, hipMemcpy(host.data(), plan->d_t4, host.size(), hipMemcpyDeviceToHost));
  std::vector<std::pair<int64_t, int64_t>> by_col;          // (col_status index, record)
  for (const auto& L : plan->launches) {
    if (!(L.kind == LaunchKind::Twisted && L.four)) continue;
    for (int s = 0; s < L.nsub; ++s)
      by_col.emplace_back(plan->sym.subs[(size_t)plan->sym.order[(size_t)L.order_off + s]].out_index, L.t4_off + s);
  }
  std::sort(by_col.begin(), by_col.end());
  const size_t ne = (size_t)twisted4_record_entries(kp.w_nzA, kp.w_nzAc, kp.w_nzB, kp.w_nzBc);
  for (size_t i = 0; i < by_col.size(); ++i) {
    const unsigned char* rec = host.data() + (size_t)by_col[i].second * plan->t4_stride;
    if (columns) columns[i] = by_col[i].first;
    if (bits) std::memcpy(bits + 2 * i, rec, 16);
    if (counts) std::memcpy(counts + 4 * i, rec + 16, 16);
    if (values) std::memcpy(values + ne * i, rec + kT4RecHeader, ne * 8);
    if (indices) std::memcpy(indices + ne * i, rec + kT4RecHeader + ne * 8, ne * 4);
  }
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): δ, slot flags and static blocks of the four-wave columns, in col_status order */
int sls_plan_debug_twisted4_static(sls_plan* plan, int64_t* n_columns, int32_t* n_slots, int64_t* offsets, double* delta,
                                   uint8_t* valid, double* blocks) {
  if (!plan || !n_columns) return fail(nullptr, SLS_EINVAL, "null argument");
  if (!plan->t4_records) return fail(plan->ctx, SLS_EINVAL, "this plan has no four-wave launch");
  if (!plan->d_t4s) return fail(plan->ctx, SLS_EINVAL, "this plan keeps no static blocks (its launches rebuild them)");
  const KernelParams& kp = plan->kp;
  const int64_t slots = kp.T + 1;
  *n_columns = plan->t4_records;
  if (n_slots) *n_slots = (int32_t)slots;
  struct Col { int64_t out_index, record, first, doubles; };
  std::vector<Col> by_col;
  for (const auto& L : plan->launches) {
    if (!(L.kind == LaunchKind::Twisted && L.four)) continue;
    for (int s = 0; s < L.nsub; ++s)
      by_col.push_back({plan->sym.subs[(size_t)plan->sym.order[(size_t)L.order_off + s]].out_index, L.t4_off + s,
                        L.t4s_off + s * L.t4s_stride, L.t4s_stride});
  }
  std::sort(by_col.begin(), by_col.end(), [](const Col& a, const Col& b) { return a.out_index < b.out_index; });
  if (offsets) {
    int64_t o = 0;
    for (size_t i = 0; i < by_col.size(); ++i) { offsets[i] = o; o += by_col[i].doubles; }
    offsets[by_col.size()] = o;
  }
  if (!delta && !valid && !blocks) return 0;
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  HIPCHK(plan->ctx, hipDeviceSynchronize());      // a plant update may still be rewriting the pool on the caller's stream
  if (delta || valid) {
    std::vector<unsigned char> host((size_t)(plan->t4_records * plan->t4_stride));
    HIPCHK(plan->ctx, hipMemcpy(host.data(), plan->d_t4, host.size(), hipMemcpyDeviceToHost));
    const size_t tail = (size_t)twisted4_record_tail(kp.w_nzA, kp.w_nzAc, kp.w_nzB, kp.w_nzBc);
    for (size_t i = 0; i < by_col.size(); ++i) {
      const unsigned char* rec = host.data() + (size_t)by_col[i].record * plan->t4_stride + tail;
      if (delta) std::memcpy(delta + i, rec, 8);
      if (valid) std::memcpy(valid + (size_t)slots * i, rec + 8, (size_t)slots);
    }
  }
  if (blocks) {
    std::vector<double> host((size_t)plan->t4s_doubles);
    HIPCHK(plan->ctx, hipMemcpy(host.data(), plan->d_t4s, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    int64_t o = 0;
    for (size_t i = 0; i < by_col.size(); ++i) {
      std::memcpy(blocks + o, host.data() + by_col[i].first, (size_t)by_col[i].doubles * sizeof(double));
      o += by_col[i].doubles;
    }
  }
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the setup images (Ã's dense image, then the weight table Wx) of the four-wave columns, in col_status order */
int sls_plan_debug_twisted4_images(sls_plan* plan, int64_t* n_columns, int64_t* offsets, int32_t* ad_doubles, double* images) {
  if (!plan || !n_columns) return fail(nullptr, SLS_EINVAL, "null argument");
  if (!plan->t4_records) return fail(plan->ctx, SLS_EINVAL, "this plan has no four-wave launch");
  if (!plan->d_t4s || !plan->d_t4i) return fail(plan->ctx, SLS_EINVAL, "this plan keeps no setup images (its launches build them)");
  *n_columns = plan->t4_records;
  struct Col { int64_t out_index, first, doubles; int32_t ad; };
  std::vector<Col> by_col;
  for (const auto& L : plan->launches) {
    if (!(L.kind == LaunchKind::Twisted && L.four)) continue;
    for (int s = 0; s < L.nsub; ++s)
      by_col.push_back({plan->sym.subs[(size_t)plan->sym.order[(size_t)L.order_off + s]].out_index, L.t4i_off + s * L.t4i_stride,
                        L.t4i_stride, (int32_t)twisted4_image_ad_doubles(twisted4_tile_rows(L.cls))});
  }
  std::sort(by_col.begin(), by_col.end(), [](const Col& a, const Col& b) { return a.out_index < b.out_index; });
  int64_t o = 0;
  for (size_t i = 0; i < by_col.size(); ++i) {
    if (offsets) offsets[i] = o;
    if (ad_doubles) ad_doubles[i] = by_col[i].ad;
    o += by_col[i].doubles;
  }
  if (offsets) offsets[by_col.size()] = o;
  if (!images) return 0;
  HIPCHK(plan->ctx, hipSetDevice(plan->dev));
  HIPCHK(plan->ctx, hipDeviceSynchronize());      // a plant update may still be rewriting the pool on the caller's stream
  std::vector<double> host((size_t)plan->t4i_doubles);
  HIPCHK(plan->ctx, hipMemcpy(host.data(), plan->d_t4i, host.size() * sizeof(double), hipMemcpyDeviceToHost));
  o = 0;
  for (size_t i = 0; i < by_col.size(); ++i) {
    std::memcpy(images + o, host.data() + by_col[i].first, (size_t)by_col[i].doubles * sizeof(double));
    o += by_col[i].doubles;
  }
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of load + h2 (csrc/sls_norms.cpp).  Needs no device. */
int sls_debug_norms_h2_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values, const double* cz,
                            const double* b, double* row_h2, double* col_h2, double* totals) {
  NormsOperator Op;
  std::string msg;
  int rc = build_norms_operator(dims, Sx, Su, Op, msg);
  if (!rc) rc = norms_h2_host(Op, values, cz, b, row_h2, col_h2, totals, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_norms_h2_host: " + msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of load + cov_pattern + cov (csrc/sls_norms.cpp).  Needs no device. */
int sls_debug_norms_cov_host(const sls_dims* dims, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values, const double* cz,
                             const double* b, int64_t npairs, const int64_t* pair_i, const int64_t* pair_j, double* cov) {
  NormsOperator Op;
  std::string msg;
  int rc = build_norms_operator(dims, Sx, Su, Op, msg);
  if (!rc) rc = norms_cov_host(Op, values, cz, b, dims->index_base, npairs, pair_i, pair_j, cov, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_norms_cov_host: " + msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the plan-time tables of sls_margin_plan (csrc/sls_margin.cpp).  Needs no device. */
int sls_debug_margin_tables(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t* n_entries,
                            int64_t* n_defect, int32_t* phi_seg, int32_t* phi_row, int32_t* phi_perm, int32_t* def_ptr, int32_t* def_key,
                            int32_t* def_start, int32_t* row_ptr, int32_t* row_perm, int32_t* A_ptr, int32_t* A_idx, int32_t* A_src,
                            int32_t* B2_ptr, int32_t* B2_idx, int32_t* B2_src) {
  MarginTables Tb;
  std::string msg;
  int rc = build_margin_tables(dims, P, Sx, Su, Tb, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_margin_tables: " + msg);
  if (n_entries) *n_entries = (int64_t)Tb.phi_perm.size();
  if (n_defect) *n_defect = (int64_t)Tb.def_key.size();
  auto put = [](const std::vector<int32_t>& v, int32_t* o) { if (o) std::copy(v.begin(), v.end(), o); };
  put(Tb.phi_seg, phi_seg); put(Tb.phi_row, phi_row); put(Tb.phi_perm, phi_perm);
  put(Tb.def_ptr, def_ptr); put(Tb.def_key, def_key); put(Tb.def_start, def_start); put(Tb.row_ptr, row_ptr); put(Tb.row_perm, row_perm);
  const FirOperator& F = Tb.R.F;
  put(F.A.ptr, A_ptr); put(F.A.idx, A_idx); put(Tb.R.A_src, A_src); put(F.B2.ptr, B2_ptr); put(F.B2.idx, B2_idx); put(Tb.R.B2_src, B2_src);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of plan + load + set_plant + run (csrc/sls_margin.cpp).  Needs no device. */
int sls_debug_margin_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                          int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario, double* row_l1, double* col_l1,
                          double* totals, int64_t* row_n, int64_t* col_n, int64_t* tot_n, double* row_s, double* col_s, double* tot_s) {
  MarginTables Tb;
  std::string msg;
  int rc = build_margin_tables(dims, P, Sx, Su, Tb, msg);
  if (!rc) rc = margin_host(Tb, values, nscen, A_nzval, B2_nzval, per_scenario != 0, row_l1, col_l1, totals, row_n, col_n, tot_n, row_s, col_s,
                            tot_s, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_margin_host: " + msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): host twin of plan + load + set_plant + set_radius + box_run (csrc/sls_margin_box.cpp).
   Needs no device. */
int sls_debug_margin_box_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, const double* values,
                              int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario, const double* A_rad,
                              const double* B2_rad, int rad_per_scenario, double* row_wc, int64_t* row_vertex, uint8_t* row_exact,
                              double* totals, int64_t* row_n, double* row_s, double* A_worst, double* B2_worst, int32_t* act_ptr,
                              int32_t* act_ent) {
  MarginTables Tb;
  std::string msg;
  int rc = build_margin_tables(dims, P, Sx, Su, Tb, msg);
  if (!rc) rc = margin_box_host(Tb, values, nscen, A_nzval, B2_nzval, per_scenario != 0, A_rad, B2_rad, rad_per_scenario != 0, row_wc, row_vertex,
                                row_exact, totals, row_n, row_s, A_worst, B2_worst, msg);
  if (!rc && (act_ptr || act_ent)) {
    MarginBoxLists L;
    rc = build_margin_box_lists(Tb.R.F.A.ptr, Tb.R.A_src, Tb.R.F.B2.ptr, Tb.R.B2_src, nscen, A_rad, B2_rad, rad_per_scenario != 0, L, msg);
    if (!rc && act_ptr) std::copy(L.act_ptr.begin(), L.act_ptr.end(), act_ptr);
    if (!rc && act_ent) std::copy(L.act_ent.begin(), L.act_ent.end(), act_ent);
  }
  if (rc) return fail(nullptr, rc, "sls_debug_margin_box_host: " + msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): fabs(margin_entry_signed) against margin_entry, bit for bit.  Needs no device. */
int sls_debug_margin_entry_signed(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                                  const double* values, int64_t nscen, const double* A_nzval, const double* B2_nzval, int per_scenario,
                                  int64_t* n_entries, int64_t* n_mismatch, int64_t* n_negative) {
  MarginTables Tb;
  std::string msg;
  int rc = build_margin_tables(dims, P, Sx, Su, Tb, msg);
  if (!rc) rc = margin_entry_signed_check(Tb, values, nscen, A_nzval, B2_nzval, per_scenario != 0, n_entries, n_mismatch, n_negative, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_margin_entry_signed: " + msg);
  return 0;
}

/* diagnostics (include/sls_mi355x_debug.h): the entry tables of sls_plan_gradient and the host twin of its two kernels
   (csrc/sls_gradient.cpp).  Needs no device. */
int sls_debug_gradient_host(const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su,
                            int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols, int64_t* n_slots,
                            int64_t* ent_ptr, int32_t* ent, int64_t* inv_ptr, int64_t* inv_slot, int32_t* inv_sub,
                            const double* mu, const double* const* phix_vals, const double* const* phiu_vals,
                            const int32_t* col_status, const double* col_weight, double* gA, double* gB2, double* abs_A,
                            double* abs_B2, int64_t* terms_A, int64_t* terms_B2) {
  Inputs in{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  std::string msg;
  int rc = validate_inputs(in, msg);
  if (rc) return fail(nullptr, rc, msg);
  Symbolic S;
  S.want_packed = false; S.compact = false;
  std::vector<int64_t> gptr, gcols;
  normalise_groups(in, gptr, gcols);
  rc = build_symbolic(in, 0, (int64_t)gptr.size() - 1, S, msg);
  if (rc) return fail(nullptr, rc, msg);
  GradientTables G;
  build_gradient_tables(S.At_csr, S.Bt_csr, S.subs.data(), (int64_t)S.subs.size(), S.idx_pool.data(), G);
  if (n_slots) *n_slots = G.ent_ptr.back();
  if (ent_ptr) std::copy(G.ent_ptr.begin(), G.ent_ptr.end(), ent_ptr);
  if (ent) std::copy(G.ent.begin(), G.ent.end(), ent);
  if (inv_ptr) std::copy(G.inv_ptr.begin(), G.inv_ptr.end(), inv_ptr);
  if (inv_slot) std::copy(G.inv_slot.begin(), G.inv_slot.end(), inv_slot);
  if (inv_sub) std::copy(G.inv_sub.begin(), G.inv_sub.end(), inv_sub);
  if (!mu) return 0;
  if (!phix_vals || !phiu_vals) return fail(nullptr, SLS_EINVAL, "null value arrays");
  std::vector<double> vals((size_t)std::max<int64_t>(S.n_values, 1), 0.0);
  for (int64_t t = 0; t < S.T; ++t) {
    const int64_t nx = S.off_x[t + 1] - S.off_x[t], nu = S.off_u[t + 1] - S.off_u[t];
    if ((nx > 0 && !phix_vals[t]) || (nu > 0 && !phiu_vals[t])) return fail(nullptr, SLS_EINVAL, "null phix_vals[t]/phiu_vals[t]");
    if (nx > 0) std::copy(phix_vals[t], phix_vals[t] + nx, vals.begin() + S.off_x[t]);
    if (nu > 0) std::copy(phiu_vals[t], phiu_vals[t] + nu, vals.begin() + S.off_u[t]);
  }
  rc = gradient_host(S, G, mu, vals.data(), col_status, col_weight, S.b_zero.data(), gA, gB2, abs_A, abs_B2, terms_A, terms_B2, msg);
  if (rc) return fail(nullptr, rc, "sls_debug_gradient_host: " + msg);
  return 0;
}

}  // extern "C"
