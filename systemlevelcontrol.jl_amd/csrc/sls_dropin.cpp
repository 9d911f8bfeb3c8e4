// sls_dropin.cpp — the one-shot calls of include/sls_mi355x.h, clients of the resident-plan API (sls_plan_build.cpp, sls_api.cpp):
//   sls_h2_sf_solve            ≙ SLS_𝓗₂(P, 𝓢; 𝓘)                    (src/synthesis.jl:11-32)
//   sls_h2_sf_solve_batch        several plants as one block-diagonal solve
//   sls_h2_sf_solve_localized    masks built on the device from (d, α)
// Their index arithmetic is in sls_dropin_host.cpp (no HIP, tested on its own).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_dropin_host.h"
#include "sls_plan.h"

using namespace sls;

namespace {

struct GroupList {            // what a refinement needs to see of the caller's arguments
  const sls_dims* dims; const sls_plant* P; const sls_csc_bool* Sx; const sls_csc_bool* Su;
  int64_t ngroups; const int64_t* group_ptr; const int64_t* group_cols;
};

// Shared tail of the solve calls, over one plan per device slot (dvals[i]: its value array; packed layout with several
// devices): execute, each device on its own stream → synchronise → refinement (`refine` != NULL) → objective into the context →
// download → status → stats.  The caller owns plans and value arrays, also when this fails.
int run_plans(sls_ctx* ctx, const std::vector<sls_plan*>& plans, const std::vector<double*>& dvals, const GroupList* refine,
              double* const* phix_vals, double* const* phiu_vals, int32_t* col_status, sls_stats& st) {
  const int ndev = (int)plans.size();
  const int packed = ndev == 1 ? 0 : 1;
  const Symbolic& S0 = plans[0]->sym;
  const int64_t T = S0.T;
  int rc = 0;
  const double t0 = now_s();
  for (int i = 0; i < ndev; ++i)
    if ((rc = sls_plan_execute(plans[i], plans[i]->stream, dvals[i], packed))) return rc;
  for (int i = 0; i < ndev; ++i)
    if ((rc = sls_plan_synchronize(plans[i], plans[i]->stream))) return rc;
  // refinement (select_refinement_groups): into the same device array, before anything is downloaded
  std::vector<std::vector<int32_t>> stt_d(ndev), its_d(ndev); std::vector<std::vector<double>> res_d(ndev);
  if (refine) {
    for (int i = 0; i < ndev; ++i) {
      int64_t nr = 0;
      rc = attach_refinement(plans[i], refine->dims, refine->P, refine->Sx, refine->Su, refine->ngroups, refine->group_ptr,
                             refine->group_cols, plans[i]->stream, dvals[i], &nr, stt_d[i], res_d[i], its_d[i], packed);
      if (rc) return rc;
      st.n_refined += nr;
    }
  }
  const double t1 = now_s();
  st.t_solve_s = t1 - t0;
  if (ctx->want_objective) {
    // after the last launch (refinement included), before the download: every device evaluates its shard, in col_status order
    ctx->obj_state = 0;
    ctx->last_objective.assign((size_t)S0.n_total_subproblems, 0.0);
    double tot = 0.0;
    for (int i = 0; i < ndev; ++i) {
      double ti = 0.0;
      rc = sls_plan_fetch_objective(plans[i], dvals[i], packed, ctx->last_objective.data() + plans[i]->sym.first_sub_index, &ti);
      if (rc) return rc;
      tot += ti;
    }
    ctx->last_total = tot; ctx->obj_state = 1;
  }
  // one device: the mask-order array comes down as it is; several: D2H of each shard's packed values + host scatter into the per-t arrays
  st.n_values_x = S0.off_x[T]; st.n_values_u = S0.n_values - S0.off_x[T];
  std::vector<double> stage;
  std::vector<int32_t> slice_of;
  for (int i = 0; i < ndev; ++i) {
    sls_plan* pl = plans[i];
    const Symbolic& S = pl->sym;
    if (ndev == 1) {
      if ((rc = sls_plan_download(pl, dvals[i], phix_vals, phiu_vals))) return rc;
    } else if (S.n_packed > 0) {
      stage.resize((size_t)S.n_packed);
      hipError_t e = hipSetDevice(pl->dev);
      if (e == hipSuccess) e = hipMemcpy(stage.data(), dvals[i], (size_t)S.n_packed * sizeof(double), hipMemcpyDeviceToHost);
      if (e != hipSuccess) return hipfail(ctx, e, "hipMemcpy D2H");
      unpack_packed_shard(T, S.off_x.data(), S.off_u.data(), S.n_values, S.packed_to_final.data(), S.n_packed, stage.data(), slice_of,
                          phix_vals, phiu_vals);
    }
    const int64_t ns = pl->info.n_subproblems;
    if (!refine) {
      stt_d[i].resize(ns); its_d[i].resize(ns); res_d[i].resize(ns);
      if ((rc = sls_plan_fetch_status(pl, stt_d[i].data(), res_d[i].data(), its_d[i].data()))) return rc;
    }
    fold_column_status(stt_d[i].data(), res_d[i].data(), its_d[i].data(), ns, col_status ? col_status + S.first_sub_index : nullptr, st);
    st.n_subproblems += ns; st.n_free += S.n_packed;
    st.max_nx = std::max(st.max_nx, S.max_n); st.max_nu = std::max(st.max_nu, S.max_m);
    st.flops_alg += S.flops_alg; st.bytes_alg += S.bytes_alg;
  }
  st.t_download_s = now_s() - t1;
  return 0;
}

// A group list that names a column more than once (assign_group_layers): the layers are solved one after the other and summed
// on the host — layer 0 in place, the later ones added in layer order.  Returns the result of the whole call.
int solve_layers(sls_ctx* ctx, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx, const sls_csc_bool* Su, int64_t ngroups,
                 const int64_t* group_ptr, const int64_t* group_cols, const std::vector<int32_t>& layer_of, int nlayers,
                 double* const* phix_vals, double* const* phiu_vals, int32_t* col_status, sls_stats* stats) {
  const int64_t Nx = dims->Nx, T = dims->T; const int b = dims->index_base;
  std::vector<int64_t> nnzx(T), nnzu(T);
  for (int64_t t = 0; t < T; ++t) { nnzx[t] = Sx[t].colptr[Nx] - b; nnzu[t] = Su[t].colptr[Nx] - b; }
  sls_stats tot{};
  std::vector<std::vector<double>> tx(T), tu(T);
  std::vector<double*> px(T), pu(T);
  std::vector<int64_t> lptr, lcols, lstat_pos;
  for (int lay = 0; lay < nlayers; ++lay) {
    layer_group_list(lay, layer_of, group_ptr, group_cols, lptr, lcols, lstat_pos);
    double* const* ox = phix_vals; double* const* ou = phiu_vals;
    if (lay > 0) {
      for (int64_t t = 0; t < T; ++t) {
        tx[t].assign((size_t)std::max<int64_t>(nnzx[t], 1), 0.0); tu[t].assign((size_t)std::max<int64_t>(nnzu[t], 1), 0.0);
        px[t] = tx[t].data(); pu[t] = tu[t].data();
      }
      ox = px.data(); ou = pu.data();
    }
    std::vector<int32_t> lst(lcols.size(), 0);
    sls_stats ls{};
    const int rc = sls_h2_sf_solve(ctx, dims, P, Sx, Su, (int64_t)lptr.size() - 1, lptr.data(), lcols.data(), ox, ou, lst.data(), &ls);
    if (rc < 0) return rc;
    if (lay > 0)
      for (int64_t t = 0; t < T; ++t) {
        for (int64_t i = 0; i < nnzx[t]; ++i) phix_vals[t][i] += tx[t][(size_t)i];
        for (int64_t i = 0; i < nnzu[t]; ++i) phiu_vals[t][i] += tu[t][(size_t)i];
      }
    if (col_status) for (size_t q = 0; q < lst.size(); ++q) col_status[lstat_pos[q]] = lst[q];
    accumulate_layer_stats(tot, ls);
  }
  if (stats) *stats = tot;
  return (int)std::min<int64_t>(tot.n_not_ok, 0x7fffffff);
}

}  // namespace

extern "C" {

int sls_h2_sf_solve(sls_ctx* ctx, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* Sx,
                    const sls_csc_bool* Su, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                    double* const* phix_vals, double* const* phiu_vals, int32_t* col_status, sls_stats* stats) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (!phix_vals || !phiu_vals) return fail(ctx, SLS_EINVAL, "null output arrays");
  if (dims && (dims->flags & SLS_PLAN_MULTIPLIERS)) return fail(ctx, SLS_EUNSUPPORTED, "SLS_PLAN_MULTIPLIERS: a one-shot call keeps no plan; build one with sls_h2_sf_plan");
  // anything else that is missing or malformed is left to the regular path to report
  if (dims && ngroups > 0 && group_ptr && group_cols && Sx && Su && dims->Nx > 0 && dims->T > 0) {
    std::vector<int32_t> layer_of;
    int nlayers = 1;
    bool masks = true;
    for (int64_t t = 0; t < dims->T; ++t) masks = masks && Sx[t].colptr && Su[t].colptr;
    if (assign_group_layers(dims->Nx, dims->index_base, ngroups, group_ptr, group_cols, layer_of, nlayers) == GroupLayering::Layered && masks) {
      const int lrc = solve_layers(ctx, dims, P, Sx, Su, ngroups, group_ptr, group_cols, layer_of, nlayers, phix_vals, phiu_vals, col_status, stats);
      if (ctx->want_objective) { ctx->obj_state = lrc >= 0 ? 2 : 0; ctx->last_objective.clear(); }   // a sum of layers: no per-column objective
      return lrc;
    }
  }
  const int ndev = (int)ctx->devs.size();
  std::vector<int64_t> cuts(ndev + 1, 0);
  int rc = sls_shard_groups(dims, P, Sx, Su, ngroups, group_ptr, group_cols, ndev, cuts.data());
  if (rc) { ctx->err = sls_last_error(nullptr); return rc; }

  sls_stats st{};
  st.n_devices = ndev;
  std::vector<sls_plan*> plans(ndev, nullptr);
  std::vector<double*> dvals(ndev, nullptr);
  auto cleanup = [&]() {
    for (int i = 0; i < ndev; ++i) {
      if (plans[i]) { if (dvals[i]) sls_plan_free_values(plans[i], dvals[i]); sls_plan_destroy(plans[i]); }
    }
  };
  for (int i = 0; i < ndev; ++i) {
    rc = plan_create(ctx, i, dims, P, Sx, Su, ngroups, group_ptr, group_cols, cuts[i], cuts[i + 1], ndev > 1, PlanOpts{}, &plans[i]);
    if (rc) { cleanup(); return rc; }
    st.t_symbolic_s += plans[i]->info.t_symbolic_s;
    st.t_upload_s += plans[i]->info.t_upload_s;
    // one device: the kernels write straight into the mask-order array (no unpack on the host); several devices: each
    // shard comes back packed and is scattered into the caller's arrays
    rc = sls_plan_alloc_values(plans[i], ndev == 1 ? 0 : 1, &dvals[i]);
    if (rc) { cleanup(); return rc; }
  }
  const Symbolic& S0 = plans[0]->sym;
  // zero the caller's arrays (columns outside every group, masked-but-unowned entries)
  for (int64_t t = 0; t < S0.T; ++t) {
    const int64_t nx = S0.off_x[t + 1] - S0.off_x[t], nu = S0.off_u[t + 1] - S0.off_u[t];
    if ((nx > 0 && !phix_vals[t]) || (nu > 0 && !phiu_vals[t])) { cleanup(); return fail(ctx, SLS_EINVAL, "null phix_vals[t]/phiu_vals[t]"); }
    if (ndev == 1) continue;        // one device: the whole (zero-initialised) device array is copied over them
    if (nx > 0) std::memset(phix_vals[t], 0, (size_t)nx * sizeof(double));
    if (nu > 0) std::memset(phiu_vals[t], 0, (size_t)nu * sizeof(double));
  }
  const char* refine_env = sls_knob("SLS_REFINE");
  const GroupList gl{dims, P, Sx, Su, ngroups, group_ptr, group_cols};
  const bool refine = !(refine_env && refine_env[0] == '0') && !(dims->flags & SLS_SOLVE_SUM_OF_NORMS);
  rc = run_plans(ctx, plans, dvals, refine ? &gl : nullptr, phix_vals, phiu_vals, col_status, st);
  cleanup();
  if (rc) return rc;
  if (stats) *stats = st;
  return (int)std::min<int64_t>(st.n_not_ok, 0x7fffffff);
}

int sls_h2_sf_solve_localized(sls_ctx* ctx, const sls_dims* dims, const sls_plant* P, int64_t d, double alpha,
                              double* const* phix_vals, double* const* phiu_vals, int32_t* col_status, sls_stats* stats) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (!phix_vals || !phiu_vals) return fail(ctx, SLS_EINVAL, "null output arrays");
  if (dims && (dims->flags & SLS_PLAN_MULTIPLIERS)) return fail(ctx, SLS_EUNSUPPORTED, "SLS_PLAN_MULTIPLIERS: a one-shot call keeps no plan; build one with sls_h2_sf_plan_localized");
  std::vector<sls_plan*> plans(1, nullptr);
  std::vector<double*> dvals(1, nullptr);
  int rc = sls_h2_sf_plan_localized(ctx, 0, dims, P, d, alpha, &plans[0]);
  if (rc) return rc;
  sls_stats st{};
  st.n_devices = 1;
  st.t_symbolic_s = plans[0]->info.t_symbolic_s; st.t_upload_s = plans[0]->info.t_upload_s;
  rc = sls_plan_alloc_values(plans[0], 0, &dvals[0]);
  if (rc == 0) rc = run_plans(ctx, plans, dvals, nullptr, phix_vals, phiu_vals, col_status, st);
  if (dvals[0]) sls_plan_free_values(plans[0], dvals[0]);
  sls_plan_destroy(plans[0]);
  if (rc) return rc;
  if (stats) *stats = st;
  return (int)std::min<int64_t>(st.n_not_ok, 0x7fffffff);
}

int sls_h2_sf_solve_batch(sls_ctx* ctx, int nplants, const sls_dims* dims, const sls_plant* P, const sls_csc_bool* const* Sx,
                          const sls_csc_bool* const* Su, double* const* const* phix_vals, double* const* const* phiu_vals,
                          int32_t* const* col_status, sls_stats* stats) {
  if (!ctx) return fail(nullptr, SLS_EINVAL, "null context");
  if (nplants <= 0 || !dims || !P || !Sx || !Su || !phix_vals || !phiu_vals) return fail(ctx, SLS_EINVAL, "null argument");
  for (int i = 0; i < nplants; ++i)
    if (dims[i].flags & SLS_PLAN_MULTIPLIERS) return fail(ctx, SLS_EUNSUPPORTED, "SLS_PLAN_MULTIPLIERS: a one-shot call keeps no plan; build one with sls_h2_sf_plan");
  if (nplants == 1) return sls_h2_sf_solve(ctx, &dims[0], &P[0], Sx[0], Su[0], 0, nullptr, nullptr, phix_vals[0], phiu_vals[0],
                                           col_status ? col_status[0] : nullptr, stats);
  BatchComposite C;
  std::string msg;
  if (int rc = C.build(nplants, dims, P, Sx, Su, phix_vals, phiu_vals, msg)) return fail(ctx, rc, msg);
  struct RidgeGuard {
    sls_ctx* c; std::vector<double> rx, ru; bool on = false;
    ~RidgeGuard() { if (on) { c->ridge_x.swap(rx); c->ridge_u.swap(ru); } }
  } rg{ctx, {}, {}, false};
  if (!ctx->ridge_x.empty() || !ctx->ridge_u.empty()) {
    for (int i = 0; i < nplants; ++i)
      if ((!ctx->ridge_x.empty() && (int64_t)ctx->ridge_x.size() != dims[i].Nx) || (!ctx->ridge_u.empty() && (int64_t)ctx->ridge_u.size() != dims[i].Nu))
        return fail(ctx, SLS_EINVAL, "sls_set_ridge: the weights' lengths do not match Nx / Nu of plant " + std::to_string(i) + " of the batch");
    rg.rx = ctx->ridge_x; rg.ru = ctx->ridge_u; rg.on = true;
    std::vector<double> cx, cu;
    C.tile_ridge(rg.rx, rg.ru, cx, cu);
    ctx->ridge_x.swap(cx); ctx->ridge_u.swap(cu);
  }
  const int rc = sls_h2_sf_solve(ctx, &C.dims, &C.plant, C.Sx.data(), C.Su.data(), 0, nullptr, nullptr, C.px.data(), C.pu.data(), C.status.data(), stats);
  if (rc < 0) return rc;
  if (int src = C.split(phix_vals, phiu_vals, col_status, msg)) return fail(ctx, src, msg);
  return rc;
}

}  // extern "C"
