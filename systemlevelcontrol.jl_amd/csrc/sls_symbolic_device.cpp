// sls_symbolic_device.cpp — host drivers of the three device symbolic passes (kernels: sls_masks.hip; LDS list plans:
// sls_symbolic_device.h): sls_localization_masks_device (mask_levels_kernel), sls_index_sets_device (index_sets_kernel) and
// sls_h2_sf_plan_localized (column_tables_kernel, level_prefix_kernel), which ends in plan_finish (sls_plan_build.cpp).  Each is a count
// pass, repeated with a doubled list capacity while a list overflows (count_with_retry), exclusive prefixes of the sizes, and
// a fill pass with the same grid and LDS.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "sls_object.h"
#include "sls_plan.h"
#include "sls_symbolic_device.h"
#include "sls_weights.h"

using namespace sls;

namespace {

// The count pass at growing capacities: cap0, then doubled up to cap_limit while it overflows.  Every round clears the two flag
// words at d_flags (default stream) and calls count(launch, &overflow), which launches the pass and reads the overflow word back
// however its route does.  `ll` is left as the fill pass needs it.
template <class Count>
int count_with_retry(sls_ctx* ctx, const ListPlan& lp, int ncu, int64_t Nx, int32_t* d_flags, ListLaunch& ll, Count&& count,
                     const char* what, const char* refusal) {
  for (int cap = lp.cap0;; cap = std::min(lp.cap_limit, 2 * cap)) {
    ll = list_launch(lp, cap, ncu, Nx);
    int32_t overflow = 0;
    hipError_t e = hipMemsetAsync(d_flags, 0, 8, nullptr);
    if (e == hipSuccess) e = count(ll, &overflow);
    if (e != hipSuccess) return hipfail(ctx, e, what);
    if (!overflow) return 0;
    if (cap >= lp.cap_limit) return fail(ctx, SLS_EUNSUPPORTED, refusal);
  }
}

struct TempArena : Arena {       // an arena for the length of a call: its allocation is freed on leaving the scope
  void* p = nullptr;
  ~TempArena() { if (p) (void)hipFree(p); }
};

// What sls_h2_sf_plan_localized holds until plan_finish takes the plan over: the plan itself, and the two arenas where they came
// from hipMalloc and not from the slot's caches.  Released here, on every return.
struct LocalizedHold {
  sls_plan* pl = nullptr;
  void *own1 = nullptr, *own2 = nullptr;
  void drop1() { if (own1) (void)hipFree(own1); own1 = nullptr; }
  ~LocalizedHold() { drop1(); if (own2) (void)hipFree(own2); delete pl; }
};

}  // namespace

extern "C" {

int sls_localization_masks_device(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_f64* A, const sls_csc_f64* B2,
                                  int64_t d, double alpha, int64_t* nnz_x, int64_t* nnz_u, int64_t* const* colptr_x,
                                  int64_t* const* rowval_x, int64_t* const* colptr_u, int64_t* const* rowval_u) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (!dims || !A || !B2 || !nnz_x || !nnz_u) return fail(ctx, SLS_EINVAL, "null argument");
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "dev_slot out of range");
  std::vector<int32_t> kx, ku, a_cp, a_ri, b_rp, b_ci;
  int kmax = 0;
  std::string msg;
  int rc = mask_recipe_inputs(dims, A, B2, d, alpha, kx, ku, kmax, a_cp, a_ri, b_rp, b_ci, msg);
  if (rc) return fail(ctx, rc, msg);
  const bool fill = rowval_x != nullptr;
  if (fill && (!colptr_x || !colptr_u || !rowval_u)) return fail(ctx, SLS_EINVAL, "null output arrays");
  const int64_t Nx = dims->Nx, Nu = dims->Nu, T = dims->T;
  const int base = dims->index_base, K1 = kmax + 1;
  const ListPlan lp = mask_list_plan(Nx, Nu);
  if (!lp.fits()) return fail(ctx, SLS_EUNSUPPORTED, "device mask recipe: the state bitmap does not fit LDS (Nx > ≈7e5); use sls_localization_masks");
  HIPCHK(ctx, hipSetDevice(ctx->devs[dev_slot]));
  MaskParams mp{};
  mp.Nx = (int32_t)Nx; mp.Nu = (int32_t)Nu; mp.T = (int32_t)T; mp.kmax = kmax; mp.base = base;
  TempArena a, a2;
  a.table(a_cp, &mp.A_cp); a.table(a_ri, &mp.A_ri); a.table(b_rp, &mp.B_rp); a.table(b_ci, &mp.B_ci);
  a.table(kx, &mp.kx); a.table(ku, &mp.ku);
  a.buffer((size_t)Nx * K1, &mp.cntx); a.buffer((size_t)Nx * K1, &mp.cntu); a.buffer(2, &mp.overflow);
  if ((rc = a.commit(ctx, &a.p, "hipMalloc (mask recipe tables)", "H2D of the plant pattern failed"))) return rc;
  ListLaunch ll{};
  rc = count_with_retry(ctx, lp, ctx->ncu[dev_slot], Nx, mp.overflow, ll, [&](const ListLaunch& l, int32_t* overflow) {
    mp.cap = l.cap;
    hipError_t e = launch_mask_levels(mp, false, l.grid, l.lds, nullptr);
    return e != hipSuccess ? e : hipMemcpy(overflow, mp.overflow, 4, hipMemcpyDeviceToHost);
  }, "device mask recipe (count pass)", "device mask recipe: a level set does not fit the LDS list; use sls_localization_masks");
  if (rc) return rc;
  std::vector<int32_t> cntx((size_t)Nx * K1), cntu((size_t)Nx * K1);
  hipError_t e = hipMemcpy(cntx.data(), mp.cntx, cntx.size() * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cntu.data(), mp.cntu, cntu.size() * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hipfail(ctx, e, "device mask recipe (level sizes)");
  // prefix sums over the columns, per level; sizes per time step
  std::vector<int64_t> prex((size_t)K1 * Nx), preu((size_t)K1 * Nx), totx(K1, 0), totu(K1, 0);
  for (int k = 0; k < K1; ++k) {
    int64_t sx = 0, su = 0;
    for (int64_t c = 0; c < Nx; ++c) { prex[(size_t)k * Nx + c] = sx; preu[(size_t)k * Nx + c] = su; sx += cntx[(size_t)c * K1 + k]; su += cntu[(size_t)c * K1 + k]; }
    totx[k] = sx; totu[k] = su;
  }
  std::vector<int64_t> offx(T + 1, 0), offu(T + 1, 0);
  for (int64_t t = 0; t < T; ++t) { nnz_x[t] = totx[kx[t]]; nnz_u[t] = totu[ku[t]]; offx[t + 1] = offx[t] + nnz_x[t]; offu[t + 1] = offu[t] + nnz_u[t]; }
  if (!fill) return 0;
  for (int64_t t = 0; t < T; ++t) {
    if (!colptr_x[t] || !colptr_u[t] || (nnz_x[t] && !rowval_x[t]) || (nnz_u[t] && !rowval_u[t])) return fail(ctx, SLS_EINVAL, "null output array for some t");
    const int64_t* px = prex.data() + (size_t)kx[t] * Nx; const int64_t* pu = preu.data() + (size_t)ku[t] * Nx;
    for (int64_t c = 0; c < Nx; ++c) { colptr_x[t][c] = px[c] + base; colptr_u[t][c] = pu[c] + base; }
    colptr_x[t][Nx] = nnz_x[t] + base; colptr_u[t][Nx] = nnz_u[t] + base;
  }
  a2.table(prex, &mp.prex); a2.table(preu, &mp.preu); a2.table(offx, &mp.offx); a2.table(offu, &mp.offu);
  a2.buffer((size_t)(offx[T] + offu[T]), &mp.rowx);
  if ((rc = a2.commit(ctx, &a2.p, "hipMalloc (mask row indices)", "H2D of the prefix tables failed"))) return rc;
  mp.rowu = mp.rowx + offx[T];
  e = launch_mask_levels(mp, true, ll.grid, ll.lds, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) return hipfail(ctx, e, "device mask recipe (fill pass)");
  // row indices → the caller's 2T arrays
  std::vector<int64_t> beg(2 * T + 1);
  std::vector<void*> ptrs(2 * T);
  for (int64_t t = 0; t < T; ++t) { beg[t] = offx[t]; ptrs[t] = rowval_x[t]; beg[T + t] = offx[T] + offu[t]; ptrs[T + t] = rowval_u[t]; }
  beg[2 * T] = offx[T] + offu[T];
  rc = pinned_download(ctx, dev_slot, ctx->devs[dev_slot], mp.rowx, beg, ptrs);
  if (rc > 0) {
    rc = 0;
    for (int64_t s2 = 0; s2 < 2 * T && e == hipSuccess; ++s2)
      if (beg[s2 + 1] > beg[s2]) e = hipMemcpy(ptrs[s2], mp.rowx + beg[s2], (size_t)(beg[s2 + 1] - beg[s2]) * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = hipfail(ctx, e, "hipMemcpy D2H (mask row indices)");
  }
  return rc;
}

int sls_index_sets_device(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_csc_f64* A, const sls_csc_bool* Sx_last,
                          const sls_csc_bool* Su_last, int64_t* sx_ptr, int64_t* sx_idx, int64_t* su_ptr, int64_t* su_idx) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (!dims || !A || !Sx_last || !Su_last || !sx_ptr || !su_ptr) return fail(ctx, SLS_EINVAL, "null argument");
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "dev_slot out of range");
  const bool fill = sx_idx != nullptr;
  if (fill && !su_idx) return fail(ctx, SLS_EINVAL, "null output arrays");
  std::vector<int32_t> a_cp, a_ri, sx_cp, sx_ri, su_cp, su_ri;
  std::string msg;
  int rc = index_set_inputs(dims, A, Sx_last, Su_last, a_cp, a_ri, sx_cp, sx_ri, su_cp, su_ri, msg);
  if (rc) return fail(ctx, rc, msg);
  const int64_t Nx = dims->Nx, Nu = dims->Nu;
  const int base = dims->index_base;
  const ListPlan lp = index_list_plan(Nx, Nu);
  if (!lp.fits()) return fail(ctx, SLS_EUNSUPPORTED, "device index sets: the state bitmap does not fit LDS (Nx > ≈7e5); use sls_sparsity_dim_reduction");
  HIPCHK(ctx, hipSetDevice(ctx->devs[dev_slot]));
  IndexSetParams ip{};
  ip.Nx = (int32_t)Nx; ip.Nu = (int32_t)Nu; ip.base = base;
  TempArena a, a2;
  a.table(a_cp, &ip.A_cp); a.table(a_ri, &ip.A_ri); a.table(sx_cp, &ip.Sx_cp); a.table(sx_ri, &ip.Sx_ri);
  a.table(su_cp, &ip.Su_cp); a.table(su_ri, &ip.Su_ri);
  a.buffer((size_t)Nx, &ip.cntx); a.buffer((size_t)Nx, &ip.cntu); a.buffer(2, &ip.overflow);
  if ((rc = a.commit(ctx, &a.p, "hipMalloc (index set tables)", "H2D of the patterns failed"))) return rc;
  ListLaunch ll{};
  rc = count_with_retry(ctx, lp, ctx->ncu[dev_slot], Nx, ip.overflow, ll, [&](const ListLaunch& l, int32_t* overflow) {
    ip.cap = l.cap;
    hipError_t e = launch_index_sets(ip, false, l.grid, l.lds, nullptr);
    return e != hipSuccess ? e : hipMemcpy(overflow, ip.overflow, 4, hipMemcpyDeviceToHost);
  }, "device index sets (count pass)", "device index sets: an index set does not fit the LDS list");
  if (rc) return rc;
  std::vector<int32_t> cntx(Nx), cntu(Nx);
  hipError_t e = hipMemcpy(cntx.data(), ip.cntx, (size_t)Nx * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cntu.data(), ip.cntu, (size_t)Nx * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hipfail(ctx, e, "device index sets (sizes)");
  std::vector<int64_t> px(Nx + 1, 0), pu(Nx + 1, 0);
  for (int64_t c = 0; c < Nx; ++c) { px[c + 1] = px[c] + cntx[c]; pu[c + 1] = pu[c] + cntu[c]; }
  for (int64_t c = 0; c <= Nx; ++c) { sx_ptr[c] = px[c] + base; su_ptr[c] = pu[c] + base; }
  if (!fill) return 0;
  a2.table(px, &ip.ptrx); a2.table(pu, &ip.ptru);
  a2.buffer((size_t)(px[Nx] + pu[Nx]), &ip.outx);
  if ((rc = a2.commit(ctx, &a2.p, "hipMalloc (index sets)", "device index sets (fill pass)"))) return rc;
  ip.outu = ip.outx + px[Nx];
  e = launch_index_sets(ip, true, ll.grid, ll.lds, nullptr);
  if (e == hipSuccess && px[Nx]) e = hipMemcpy(sx_idx, ip.outx, (size_t)px[Nx] * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && pu[Nx]) e = hipMemcpy(su_idx, ip.outu, (size_t)pu[Nx] * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hipfail(ctx, e, "device index sets (fill pass)");
  return 0;
}

// ---- device-resident symbolic route (SURVEY §8 row f1 on the solve path; reference README.md:52-54 + src/reduction.jl:14) ----
// The README's masks are a function of (A, B2, d, α, T).  Instead of receiving them as 2T host arrays (8 B per entry over
// PCIe, read once by the host pass), this route derives everything a plan needs from the plant pattern ON THE DEVICE: level
// sets per column (count pass), exclusive prefixes over the columns (the CSC positions), then index sets, compact bit masks
// and first destinations (fill pass), expanded into the kernels' tables by the same expand_tables_kernel as the host route.
// Over PCIe: the plant (KBs), 24 B per column of sizes coming back, 64 B per column of descriptors going up.
int sls_h2_sf_plan_localized(sls_ctx* ctx, int dev_slot, const sls_dims* dims, const sls_plant* P, int64_t d, double alpha,
                             sls_plan** plan_out) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (!plan_out) return fail(ctx, SLS_EINVAL, "null plan_out");
  *plan_out = nullptr;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return fail(ctx, SLS_EINVAL, "dev_slot out of range");
  if (!ctx->ridge_x.empty() || !ctx->ridge_u.empty())
    return fail(ctx, SLS_EUNSUPPORTED, "the device-resident symbolic route does not carry the ridge term of sls_set_ridge; pass the masks to sls_h2_sf_plan");
  LocalizedHold hold;
  sls_plan* pl = hold.pl = new (std::nothrow) sls_plan();
  if (!pl) return fail(ctx, SLS_ENOMEM, "out of memory");
  pl->ctx = ctx; pl->dev = ctx->devs[dev_slot]; pl->slot = dev_slot;
  const double t0 = now_s();
  Symbolic& S = pl->sym;
  S.want_packed = false; S.compact = true;
  LocalizedHost L;
  std::string msg;
  int rc = localized_prepare(dims, P, d, alpha, S, L, msg);
  if (rc) return fail(ctx, rc, msg);
  const int64_t Nx = dims->Nx, Nu = dims->Nu, T = dims->T;
  pl->gbeg = 0; pl->gend = Nx; pl->ngroups_in = 0;
  DebugTicker tick("sls localized", 34);
  tick("host: checks, pattern, operator CSR");
  hipError_t e = hipSetDevice(pl->dev);
  if (e != hipSuccess) return hipfail(ctx, e, "hipSetDevice");

  const int K1 = L.kmax + 1;
  ColumnTableParams cp{};
  cp.Nx = (int32_t)Nx; cp.Nu = (int32_t)Nu; cp.T = (int32_t)T; cp.kmax = L.kmax;
  cp.qx1 = L.kx[T - 1] + 1; cp.qu1 = L.ku[T - 1] + 1;
  cp.KL = std::max(L.kmax, std::max(cp.qx1, cp.qu1));
  // ---- arena 1 (temporary): patterns, schedule, operator rows for the nnz counts, count-pass outputs, prefixes ----
  Arena A1;
  int64_t *d_prex, *d_preu, *d_totx, *d_totu;
  A1.table(L.a_cp, &cp.A_cp); A1.table(L.a_ri, &cp.A_ri); A1.table(L.b_rp, &cp.B_rp); A1.table(L.b_ci, &cp.B_ci);
  A1.table(S.A_csr.ptr, &cp.A_rowptr); A1.table(S.A_csr.idx, &cp.A_colidx); A1.table(S.A_csr.val, &cp.A_val);
  A1.table(S.B_csr.ptr, &cp.B_rowptr); A1.table(S.B_csr.idx, &cp.B_colidx); A1.table(S.B_csr.val, &cp.B_val);
  A1.table(L.kx, &cp.kx); A1.table(L.ku, &cp.ku);
  A1.buffer((size_t)Nx * K1, &cp.cntx); A1.buffer((size_t)Nx * K1, &cp.cntu); A1.buffer((size_t)K1 * Nx, &d_prex); A1.buffer((size_t)K1 * Nx, &d_preu);
  // what comes back to the host in ONE copy, adjacent in the arena: flags (256 B), level totals, per-column sizes
  A1.buffer(64, &cp.flags); A1.buffer((size_t)K1, &d_totx); A1.buffer((size_t)K1, &d_totu); A1.buffer((size_t)Nx * 6, &cp.col_info);
  const size_t sz_tot = Arena::al((size_t)K1 * 8), back_bytes = 256 + 2 * sz_tot + (size_t)Nx * 6 * 4;
  const ListPlan lp = tables_list_plan(Nx, Nu, T);
  if (!lp.fits()) return fail(ctx, SLS_EUNSUPPORTED, "device symbolic route: the state bitmap does not fit LDS (Nx > ≈7e5); pass the masks to sls_h2_sf_plan");
  // the temporary arena comes from the slot's cached scratch workspace when that is free and large enough (a hipMalloc +
  // hipFree pair per call costs ≈0.3 ms); the plan borrows the same scratch only after this arena is done with
  sls_ctx::Slot& sl = ctx->slots[dev_slot];
  void* a1 = (!sl.scratch_in_use && sl.scratch_bytes >= A1.bytes()) ? sl.scratch : nullptr;
  if (!a1) {
    e = hipMalloc(&a1, A1.bytes());
    if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc (symbolic arena)");
    hold.own1 = a1;
  }
  if ((rc = A1.commit_in(ctx, a1, "hipMemcpy H2D (plant pattern)"))) return rc;
  std::vector<unsigned char> back(back_bytes);
  ListLaunch ll{};
  rc = count_with_retry(ctx, lp, ctx->ncu[dev_slot], Nx, cp.flags, ll, [&](const ListLaunch& l, int32_t* overflow) {
    cp.cap = l.cap;
    hipError_t ec = launch_column_tables(cp, false, l.grid, l.lds, nullptr);
    if (ec == hipSuccess) ec = launch_level_prefix(cp.cntx, cp.cntu, (int)Nx, K1, d_prex, d_preu, d_totx, d_totu, nullptr);
    if (ec == hipSuccess) ec = hipMemcpy(back.data(), cp.flags, back_bytes, hipMemcpyDeviceToHost);
    if (ec == hipSuccess) *overflow = reinterpret_cast<const int32_t*>(back.data())[0];
    return ec;
  }, "device symbolic route (count pass)", "device symbolic route: a column's level sets do not fit LDS; pass the masks to sls_h2_sf_plan");
  if (rc) return rc;
  tick("device: count pass + prefixes + D2H");

  // ---- host: value-array offsets, per-column placement, descriptors, solve order ----
  LocalizedLayout lay;
  rc = localized_layout(dims, P->B1, L, reinterpret_cast<const int64_t*>(back.data() + 256),
                        reinterpret_cast<const int64_t*>(back.data() + 256 + sz_tot),
                        reinterpret_cast<const int32_t*>(back.data() + 256 + 2 * sz_tot), S, lay, msg);
  if (rc) return fail(ctx, rc, msg);
  tick("host: offsets + descriptors");

  // ---- arena 2 (kept by the plan): the fill pass's own inputs (one staged copy); index sets, compact masks, bases ----
  Arena A2;
  A2.table(lay.cw_off, &cp.cw_off); A2.table(lay.idx_off, &cp.idx_off); A2.table(S.off_x, &cp.offx); A2.table(S.off_u, &cp.offu);
  A2.buffer((size_t)lay.idx_total, &cp.idx_pool); A2.buffer((size_t)lay.cw_total, &cp.cmask); A2.buffer((size_t)2 * T * Nx, &cp.cbase);
  const size_t a2_bytes = A2.bytes();
  // a one-shot call builds and drops a plan per call, so the slot caches one such buffer (as for the plan arena)
  const bool a2_borrowed = !sl.ltab_in_use;
  void* a2 = nullptr;
  if (a2_borrowed && (sl.ltab_bytes < a2_bytes || sl.ltab_bytes > 4 * a2_bytes + (64u << 20))) {
    if (sl.ltab) (void)hipFree(sl.ltab);
    sl.ltab = nullptr; sl.ltab_bytes = 0;
  }
  if (a2_borrowed && sl.ltab) a2 = sl.ltab;
  else {
    e = hipMalloc(&a2, a2_bytes);
    if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc (device tables)");
    if (a2_borrowed) { sl.ltab = a2; sl.ltab_bytes = a2_bytes; } else hold.own2 = a2;
  }
  if ((rc = A2.commit_in(ctx, a2, "device symbolic route (fill pass)"))) return rc;
  cp.prex = d_prex; cp.preu = d_preu;
  e = launch_column_tables(cp, true, ll.grid, ll.lds, nullptr);
  int32_t fl[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpy(fl, cp.flags, 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hipfail(ctx, e, "device symbolic route (fill pass)");
  if (fl[1]) return fail(ctx, SLS_EUNSUPPORTED, "device symbolic route: a mask row lies outside its column's index set (A without a full diagonal); pass the masks to sls_h2_sf_plan");
  tick("device: fill pass");
  if (S.wu.updatable) {
    // updatable weights on this route: a record for every column with B1[c,c] ≠ 0, filled on the host by the update's own twin
    // from the plan-time diagonals.  The index sets exist on the device only, so they come back once (4 B per local variable,
    // flagged plans only); plan_finish drops the host copy again.
    S.idx_pool.resize((size_t)lay.idx_total);
    e = lay.idx_total ? hipMemcpy(S.idx_pool.data(), cp.idx_pool, (size_t)lay.idx_total * sizeof(int32_t), hipMemcpyDeviceToHost) : hipSuccess;
    if (e != hipSuccess) return hipfail(ctx, e, "hipMemcpy D2H (index sets)");
    if ((rc = localized_weight_records(dims, P->B1, lay, S, msg))) return fail(ctx, rc, msg);
  }
  hold.drop1();
  // arena 2 becomes the plan's, and the plan plan_finish's (which destroys it on failure)
  if (a2_borrowed) { sl.ltab_in_use = true; pl->ltab_borrowed = true; }
  else pl->dev_allocs.push_back(a2);
  hold.own2 = nullptr; hold.pl = nullptr;
  const DeviceTables dt{cp.idx_pool, cp.cmask, cp.cbase, cp.cw_off};
  PlanOpts opt;
  opt.multipliers = (dims->flags & SLS_PLAN_MULTIPLIERS) != 0;
  return plan_finish(ctx, dev_slot, dims, pl, t0, false, opt, &dt, plan_out);
}

}  // extern "C"
