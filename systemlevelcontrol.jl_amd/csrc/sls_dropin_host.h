// sls_dropin_host.h — the index arithmetic of the one-shot calls (sls_dropin.cpp) and of the shard cuts, pure C++ with no HIP:
// plain arrays in and out, a message string for errors, no context and no plan.  tests/host_sanitize/sanitize_dropin.cpp runs
// it under AddressSanitizer + UndefinedBehaviorSanitizer.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sls_mi355x.h"
#include "sls_symbolic.h"

namespace sls {

// A column listed in several groups: the reference solves it once per group, each time with that group's index sets, and ADDS
// the contributions (Φ̃ += [Φₓ Φᵤ] per group and the (+) fold, src/synthesis.jl:24,67).  A plan gives every subproblem its own
// destinations, so the drop-in call cuts such a group list into LAYERS in which every column appears at most once (a group
// goes to the first layer none of its columns has been used in), solves the layers one after the other and sums them on the
// host.
enum class GroupLayering {
  None,        // no column is listed twice: one solve of the whole list
  Layered,     // layer_of / nlayers are valid, nlayers ≥ 2
  Malformed,   // descending group_ptr or a column out of range: the regular path reports it
};
GroupLayering assign_group_layers(int64_t Nx, int index_base, int64_t ngroups, const int64_t* group_ptr, const int64_t* group_cols,
                                  std::vector<int32_t>& layer_of, int& nlayers);
// the group list of one layer, columns as the caller gave them; lstat_pos: position of each of its columns in the caller's flat list
void layer_group_list(int lay, const std::vector<int32_t>& layer_of, const int64_t* group_ptr, const int64_t* group_cols,
                      std::vector<int64_t>& lptr, std::vector<int64_t>& lcols, std::vector<int64_t>& lstat_pos);
// what a layer's solve adds to the stats of the whole call
void accumulate_layer_stats(sls_stats& tot, const sls_stats& ls);

// cuts[0 .. nshards]: contiguous runs of groups of about equal predicted cost (sls_shard_groups)
void balanced_cuts(const std::vector<double>& cost, int nshards, int64_t* cuts);

// Refinement: columns the one-wave / twisted kernels left at a residual between 1e-11 and the acceptance level after four or
// more passes sit on a near-singular constraint matrix — their plain multiplier iteration contracts slowly there, and Φ is
// only determined to residual/σ_min (fuzz seed 77: residual 4e-10, σ_min 2e-6, |ΔΦ| 2e-4 with status OK).  The tile kernel's
// minimal-residual iteration takes the same columns to 1e-13: their groups are solved once more on it.  This picks them: of the
// groups [gbeg, gend) of the normalised list (gptr, gcols; 0-based columns), every group with a qualifying member, whole.
// cls / on_twisted / stt / its / res are per subproblem of the shard (subproblem 0 = first column of group gbeg); rg_cols comes
// back in the caller's index base, rg_dst relative to the shard.
void select_refinement_groups(int64_t gbeg, int64_t gend, const std::vector<int64_t>& gptr, const std::vector<int64_t>& gcols,
                              int index_base, const int32_t* cls, const char* on_twisted, const int32_t* stt, const int32_t* its,
                              const double* res, std::vector<int64_t>& rg_ptr, std::vector<int64_t>& rg_cols,
                              std::vector<int64_t>& rg_dst);

// col_status[q] = stt[q] (col_status nullable) and what the ns columns add to st: n_not_ok, max_residual over the OK / TRIVIAL
// columns only, max_iters over all
void fold_column_status(const int32_t* stt, const double* res, const int32_t* its, int64_t ns, int32_t* col_status, sls_stats& st);

// One shard's packed values (stage[k] belongs at value index packed_to_final[k]) into the caller's per-t arrays.  slice_of —
// value index → slice (t for Φx[t], T+t for Φu[t]) as a flat table, one lookup per value (a binary search per value cost more
// than the solve) — is built by the first call and reused by the following shards.
void unpack_packed_shard(int64_t T, const int64_t* off_x, const int64_t* off_u, int64_t n_values, const int64_t* packed_to_final,
                         int64_t n_packed, const double* stage, std::vector<int32_t>& slice_of, double* const* phix_vals,
                         double* const* phiu_vals);

// The block-diagonal composite of a batch of plants (sls_h2_sf_solve_batch), in the callers' own index base.  Column blocks are
// laid side by side, rows shifted per plant; the z rows of C1 / D11 / D12 are [x of all plants; u of all plants] so that
// Nz = Nx + Nu keeps its meaning.  The views point into the object's own storage: it is neither copied nor moved.
struct BatchComposite {
  BatchComposite() = default;
  BatchComposite(const BatchComposite&) = delete;
  BatchComposite& operator=(const BatchComposite&) = delete;

  int nplants = 0;
  int64_t T = 0;
  int base = 0;
  std::vector<int64_t> xo, uo;             // nplants+1: first state / input of each plant in the composite
  sls_dims dims{};
  sls_plant plant{};
  std::vector<sls_csc_bool> Sx, Su;        // T views
  std::vector<double*> px, pu;             // T composite value arrays: plant i's values of slice t are one contiguous run (its columns are adjacent)
  std::vector<int32_t> status;             // NX

  // 0, or an error code and its message; phix_vals / phiu_vals are only checked for NULL per-plant arrays here
  int build(int nplants_in, const sls_dims* d, const sls_plant* P, const sls_csc_bool* const* Sx_in, const sls_csc_bool* const* Su_in,
            double* const* const* phix_vals, double* const* const* phiu_vals, std::string& msg);
  // the ridge term of sls_set_ridge has per-plant length: every plant of the batch gets it (concatenated for the composite)
  void tile_ridge(const std::vector<double>& rx, const std::vector<double>& ru, std::vector<double>& cx, std::vector<double>& cu) const;
  // px / pu / status back into the callers' per-plant arrays (col_status and its entries nullable)
  int split(double* const* const* phix_vals, double* const* const* phiu_vals, int32_t* const* col_status, std::string& msg) const;

 private:
  struct Csc { std::vector<int64_t> colptr, rowval; std::vector<double> val; std::vector<uint8_t> bval; };
  Csc cA, cB1, cB2, cC1, cD11, cD12;
  sls_csc_f64 vA{}, vB1{}, vB2{}, vC1{}, vD11{}, vD12{};
  std::vector<Csc> mx, mu;
  std::vector<std::vector<double>> bx, bu;
};

}  // namespace sls
