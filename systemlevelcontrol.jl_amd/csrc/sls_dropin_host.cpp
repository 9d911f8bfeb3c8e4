// sls_dropin_host.cpp — see sls_dropin_host.h.  No HIP, no context, no plan.
#include "sls_dropin_host.h"

#include <algorithm>
#include <cstring>

namespace sls {

GroupLayering assign_group_layers(int64_t Nx, int index_base, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                                  std::vector<int32_t>& layer_of, int& nlayers) {
  const int b = index_base;
  std::vector<int32_t> next_layer((size_t)Nx, 0);
  layer_of.assign((size_t)ngroups, 0);
  nlayers = 1;
  for (int64_t g = 0; g < ngroups; ++g) {
    if (group_ptr[g + 1] < group_ptr[g]) return GroupLayering::Malformed;
    int32_t lay = 0;
    for (int64_t k = group_ptr[g]; k < group_ptr[g + 1]; ++k) {
      const int64_t c = group_cols[k] - b;
      if (c < 0 || c >= Nx) return GroupLayering::Malformed;
      lay = std::max(lay, next_layer[(size_t)c]);
    }
    for (int64_t k = group_ptr[g]; k < group_ptr[g + 1]; ++k) next_layer[(size_t)(group_cols[k] - b)] = lay + 1;
    layer_of[(size_t)g] = lay; nlayers = std::max(nlayers, lay + 1);
  }
  return nlayers == 1 ? GroupLayering::None : GroupLayering::Layered;
}

void layer_group_list(int lay, const std::vector<int32_t>& layer_of, const int64_t* group_ptr, const int64_t* group_cols,
                      std::vector<int64_t>& lptr, std::vector<int64_t>& lcols, std::vector<int64_t>& lstat_pos) {
  lptr.assign(1, 0); lcols.clear(); lstat_pos.clear();
  for (int64_t g = 0; g < (int64_t)layer_of.size(); ++g) {
    if (layer_of[(size_t)g] != lay) continue;
    for (int64_t k = group_ptr[g]; k < group_ptr[g + 1]; ++k) { lcols.push_back(group_cols[k]); lstat_pos.push_back(k); }
    lptr.push_back((int64_t)lcols.size());
  }
}

void accumulate_layer_stats(sls_stats& tot, const sls_stats& ls) {
  tot.n_subproblems += ls.n_subproblems; tot.n_not_ok += ls.n_not_ok; tot.n_free += ls.n_free; tot.n_refined += ls.n_refined;
  tot.n_values_x = ls.n_values_x; tot.n_values_u = ls.n_values_u; tot.n_devices = ls.n_devices;
  tot.max_nx = std::max(tot.max_nx, ls.max_nx); tot.max_nu = std::max(tot.max_nu, ls.max_nu); tot.max_iters = std::max(tot.max_iters, ls.max_iters);
  tot.max_residual = std::max(tot.max_residual, ls.max_residual);
  tot.flops_alg += ls.flops_alg; tot.bytes_alg += ls.bytes_alg; tot.t_symbolic_s += ls.t_symbolic_s; tot.t_upload_s += ls.t_upload_s;
  tot.t_solve_s += ls.t_solve_s; tot.t_download_s += ls.t_download_s;
}

void balanced_cuts(const std::vector<double>& cost, int nshards, int64_t* cuts) {
  const int64_t ng = (int64_t)cost.size();
  double total = 0; for (double c : cost) total += c;
  cuts[0] = 0;
  double acc = 0; int64_t g = 0;
  for (int s = 1; s < nshards; ++s) {
    const double target = total * s / nshards;
    while (g < ng && acc + 0.5 * cost[g] < target) { acc += cost[g]; ++g; }
    // leave at least one group for every remaining shard when possible
    const int64_t max_g = ng - (nshards - s) > 0 ? ng - (nshards - s) : 0;
    if (g > max_g) g = max_g;
    if (g < cuts[s - 1]) g = cuts[s - 1];
    cuts[s] = g;
    acc = 0; for (int64_t q = 0; q < g; ++q) acc += cost[q];
  }
  cuts[nshards] = ng;
}

void select_refinement_groups(int64_t gbeg, int64_t gend, const std::vector<int64_t>& gptr, const std::vector<int64_t>& gcols,
                              int index_base, const int32_t* cls, const char* on_twisted, const int32_t* stt, const int32_t* its,
                              const double* res, std::vector<int64_t>& rg_ptr, std::vector<int64_t>& rg_cols,
                              std::vector<int64_t>& rg_dst) {
  rg_ptr.assign(1, 0); rg_cols.clear(); rg_dst.clear();
  const int64_t q0 = gptr[gbeg];
  // on_twisted — columns of the twisted kernels (latency regime: at most one per CU): the two-ended elimination meets a
  // near-singular direction in its middle block, where the multiplier iteration contracts worse than in the one-ended kernels
  // (tools/fuzz_h2.py seed 235, column 52: residual 0.4–0.7 after six passes against 5e-9 in the one-wave kernel and 4e-10 in the
  // tile kernel) — a column they flag infeasible gets the tile kernel's verdict
  for (int64_t g = gbeg; g < gend; ++g) {
    bool want = false;
    for (int64_t q = gptr[g] - q0; q < gptr[g + 1] - q0; ++q) {
      if (cls[q] < 0) continue;                                  // solved by the tile kernel already: nothing to gain
      want = want || (stt[q] == SLS_COL_NOTCONV) || (stt[q] == SLS_COL_OK && its[q] >= 4 && res[q] > 1e-11) ||
             (stt[q] == SLS_COL_INFEASIBLE && its[q] >= 3 && (res[q] < 1e-6 || on_twisted[q]));      // (flagged at the second pass: the residual did not move at all — a plain infeasible column, on any kernel)
    }
    if (!want) continue;
    for (int64_t q = gptr[g]; q < gptr[g + 1]; ++q) { rg_cols.push_back(gcols[q] + index_base); rg_dst.push_back(q - q0); }
    rg_ptr.push_back((int64_t)rg_cols.size());
  }
}

void fold_column_status(const int32_t* stt, const double* res, const int32_t* its, int64_t ns, int32_t* col_status, sls_stats& st) {
  for (int64_t q = 0; q < ns; ++q) {
    if (col_status) col_status[q] = stt[q];
    if (stt[q] != SLS_COL_OK && stt[q] != SLS_COL_TRIVIAL) st.n_not_ok++;
    else st.max_residual = std::max(st.max_residual, res[q]);
    st.max_iters = std::max(st.max_iters, its[q]);
  }
}

void unpack_packed_shard(int64_t T, const int64_t* off_x, const int64_t* off_u, int64_t n_values, const int64_t* packed_to_final,
                         int64_t n_packed, const double* stage, std::vector<int32_t>& slice_of, double* const* phix_vals,
                         double* const* phiu_vals) {
  if (slice_of.empty()) {
    slice_of.resize((size_t)n_values);
    for (int64_t t = 0; t < T; ++t) {
      std::fill(slice_of.begin() + off_x[t], slice_of.begin() + off_x[t + 1], (int32_t)t);
      std::fill(slice_of.begin() + off_u[t], slice_of.begin() + off_u[t + 1], (int32_t)(T + t));
    }
  }
  for (int64_t k = 0; k < n_packed; ++k) {
    const int64_t f = packed_to_final[k];
    const int32_t sl = slice_of[(size_t)f];
    if (sl < T) phix_vals[sl][f - off_x[sl]] = stage[k];
    else phiu_vals[sl - T][f - off_u[sl - T]] = stage[k];
  }
}

int BatchComposite::build(int nplants_in, const sls_dims* d, const sls_plant* P, const sls_csc_bool* const* Sx_in,
                          const sls_csc_bool* const* Su_in, double* const* const* phix_vals, double* const* const* phiu_vals,
                          std::string& msg) {
  nplants = nplants_in;
  T = d[0].T;
  base = d[0].index_base;
  xo.assign(nplants + 1, 0); uo.assign(nplants + 1, 0);
  for (int i = 0; i < nplants; ++i) {
    if (d[i].T != T || d[i].index_base != base || d[i].flags != d[0].flags) {
      msg = "plants of one batch must share T, index_base and flags"; return SLS_EINVAL;
    }
    if (!Sx_in[i] || !Su_in[i] || !phix_vals[i] || !phiu_vals[i]) { msg = "null per-plant argument"; return SLS_EINVAL; }
    if (d[i].Nz != d[i].Nx + d[i].Nu) { msg = "Nz must equal Nx + Nu (state feedback with z = [x; u] rows)"; return SLS_ENOTSF; }
    // each plant is validated as the single call would, so that an error names the plant and not a composite row
    Inputs in{&d[i], &P[i], Sx_in[i], Su_in[i], 0, nullptr, nullptr};
    std::string m;
    if (int rc = validate_inputs(in, m)) { msg = "plant " + std::to_string(i) + ": " + m; return rc; }
    xo[i + 1] = xo[i] + d[i].Nx; uo[i + 1] = uo[i] + d[i].Nu;
  }
  const int64_t NX = xo[nplants], NU = uo[nplants];
  auto cat_f64 = [&](const sls_csc_f64* sls_plant::*pick, const std::vector<int64_t>& coff, int kind /*0: x rows, 1: z rows*/, Csc& out,
                     sls_csc_f64& view, int64_t nrows) {
    const int64_t ncols = coff[nplants];
    out.colptr.assign(ncols + 1, base);
    int64_t nnz = 0;
    for (int i = 0; i < nplants; ++i) { const sls_csc_f64* M = P[i].*pick; if (M) nnz += M->colptr[M->ncols] - base; }
    out.rowval.resize(nnz); out.val.resize(nnz);
    int64_t k = 0;
    for (int i = 0; i < nplants; ++i) {
      const sls_csc_f64* M = P[i].*pick;
      const int64_t nc = coff[i + 1] - coff[i];
      for (int64_t c = 0; c < nc; ++c) {
        if (M)
          for (int64_t e = M->colptr[c] - base; e < M->colptr[c + 1] - base; ++e) {
            const int64_t r = M->rowval[e] - base;
            out.rowval[k] = base + (kind == 0 ? xo[i] + r : (r < d[i].Nx ? xo[i] + r : NX + uo[i] + (r - d[i].Nx)));
            out.val[k] = M->nzval ? M->nzval[e] : 1.0;
            ++k;
          }
        out.colptr[coff[i] + c + 1] = base + k;
      }
    }
    view = sls_csc_f64{nrows, ncols, out.colptr.data(), out.rowval.data(), out.val.data()};
  };
  // NULL C1 / D12 = the default weights [C1 D12] = I (src/types/GeneralizedPlant.jl:105-110): all plants or none
  int n_defw = 0;
  for (int i = 0; i < nplants; ++i) {
    if ((P[i].C1 == nullptr) != (P[i].D12 == nullptr)) { msg = "C1 and D12 must be given together"; return SLS_EINVAL; }
    if (!P[i].C1) ++n_defw;
  }
  if (n_defw != 0 && n_defw != nplants) { msg = "plants of one batch must all give C1, D12 or all leave them NULL"; return SLS_EINVAL; }
  cat_f64(&sls_plant::A, xo, 0, cA, vA, NX);
  // B1 / D11: the path only ever reads column c of plant i for c < Nx_i (the default groups 1:Nx, src/synthesis.jl:15,42), and
  // the symbolic pass addresses it as composite column xo[i] + c — so plant i's first Nx_i columns sit at xo[i]; surplus
  // disturbance channels (Nw_i > Nx_i) belong to no subproblem and are left out
  cat_f64(&sls_plant::B1, xo, 0, cB1, vB1, NX);
  cat_f64(&sls_plant::B2, uo, 0, cB2, vB2, NX);
  cat_f64(&sls_plant::C1, xo, 1, cC1, vC1, NX + NU);
  cat_f64(&sls_plant::D11, xo, 1, cD11, vD11, NX + NU);
  cat_f64(&sls_plant::D12, uo, 1, cD12, vD12, NX + NU);
  plant = sls_plant{&vA, &vB1, &vB2, n_defw ? nullptr : &vC1, &vD11, n_defw ? nullptr : &vD12};
  mx.assign(T, Csc{}); mu.assign(T, Csc{});
  Sx.resize(T); Su.resize(T);
  auto cat_bool = [&](const sls_csc_bool* const* Ms, int64_t t, const std::vector<int64_t>& roff, int64_t nrows, Csc& out, sls_csc_bool& view) {
    out.colptr.assign(NX + 1, base);
    int64_t nnz = 0;
    for (int i = 0; i < nplants; ++i) nnz += Ms[i][t].colptr[d[i].Nx] - base;
    out.rowval.resize(nnz); out.bval.resize(nnz);
    int64_t k = 0;
    for (int i = 0; i < nplants; ++i) {
      const sls_csc_bool& M = Ms[i][t];
      for (int64_t c = 0; c < d[i].Nx; ++c) {
        for (int64_t e = M.colptr[c] - base; e < M.colptr[c + 1] - base; ++e) {
          out.rowval[k] = base + roff[i] + (M.rowval[e] - base);
          out.bval[k] = M.nzval ? M.nzval[e] : 1;
          ++k;
        }
        out.colptr[xo[i] + c + 1] = base + k;
      }
    }
    view = sls_csc_bool{nrows, NX, out.colptr.data(), out.rowval.data(), out.bval.data()};
  };
  for (int64_t t = 0; t < T; ++t) { cat_bool(Sx_in, t, xo, NX, mx[t], Sx[t]); cat_bool(Su_in, t, uo, NU, mu[t], Su[t]); }
  dims = d[0];
  dims.Nx = NX; dims.Nu = NU; dims.Nw = NX; dims.Nz = NX + NU;
  bx.assign(T, {}); bu.assign(T, {});
  px.resize(T); pu.resize(T);
  for (int64_t t = 0; t < T; ++t) {
    bx[t].resize((size_t)std::max<int64_t>(1, (int64_t)mx[t].rowval.size())); bu[t].resize((size_t)std::max<int64_t>(1, (int64_t)mu[t].rowval.size()));
    px[t] = bx[t].data(); pu[t] = bu[t].data();
  }
  status.assign((size_t)NX, 0);
  return 0;
}

void BatchComposite::tile_ridge(const std::vector<double>& rx, const std::vector<double>& ru, std::vector<double>& cx,
                                std::vector<double>& cu) const {
  cx.clear(); cu.clear();
  for (int i = 0; i < nplants; ++i) { cx.insert(cx.end(), rx.begin(), rx.end()); cu.insert(cu.end(), ru.begin(), ru.end()); }
}

int BatchComposite::split(double* const* const* phix_vals, double* const* const* phiu_vals, int32_t* const* col_status,
                          std::string& msg) const {
  for (int64_t t = 0; t < T; ++t) {
    for (int i = 0; i < nplants; ++i) {
      const int64_t x0 = mx[t].colptr[xo[i]] - base, x1 = mx[t].colptr[xo[i + 1]] - base;
      const int64_t u0 = mu[t].colptr[xo[i]] - base, u1 = mu[t].colptr[xo[i + 1]] - base;
      if (x1 > x0) { if (!phix_vals[i][t]) { msg = "null phix_vals[i][t]"; return SLS_EINVAL; } std::memcpy(phix_vals[i][t], bx[t].data() + x0, (size_t)(x1 - x0) * sizeof(double)); }
      if (u1 > u0) { if (!phiu_vals[i][t]) { msg = "null phiu_vals[i][t]"; return SLS_EINVAL; } std::memcpy(phiu_vals[i][t], bu[t].data() + u0, (size_t)(u1 - u0) * sizeof(double)); }
    }
  }
  if (col_status)
    for (int i = 0; i < nplants; ++i)
      if (col_status[i]) std::copy(status.begin() + xo[i], status.begin() + xo[i + 1], col_status[i]);
  return 0;
}

}  // namespace sls
