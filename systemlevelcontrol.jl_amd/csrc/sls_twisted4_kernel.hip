// sls_twisted4_kernel.hip — LATENCY regime of the H2 column solve, round 3: FOUR waves per subproblem (gfx950).
//
// The two-wave twisted kernel (sls_wave_kernel.hip) halves the serial chain over the T+1 block rows: wave 0 eliminates
// upwards from block 0, wave 1 downwards from block T.  What is left on each wave's chain per block is
//     build D'_k from P_{k∓1} (two sparse products through an LDS image: ≈4.8 k cycles)  →  Gauss–Jordan (≈7.0 k)  →  fused sweep,
// strictly one after the other, on ONE of the CU's four SIMDs while two stand idle (README chain: 59 columns on 256 CUs).
//
// Here each direction gets a HELPER wave on its own SIMD that takes the build off the chain.  With
//     S_k = δI + W_k + B̃ Wu_{k−1} B̃ᵀ + Ã W_{k−1} Ãᵀ            (the diagonal block of E H⁻¹ Eᵀ + δI: static, no P in it)
//     upward:    D'_k = S_k − X P_{k−1} Xᵀ,   X = Ã W_{k−1}        downward:  G_k = S_k − X P_{k+1} Xᵀ,   X = W_k Ãᵀ
// the next block is the Schur complement of the bordered matrix [[G, Xᵀ], [X, S]] on G = the block being inverted RIGHT NOW:
// eliminating G's pivots from the border produces S − X G⁻¹ Xᵀ in place of S.  The chain wave inverts G by the same tiled
// Gauss–Jordan as before and, per pivot, drops the pivot row (its pre-update values, times 1/pivot) and 1/pivot into LDS — the
// lanes that own the row publish it one pivot ahead, and the chain wave itself reads its copy of the scaled row from that record
// (two DS reads) instead of fetching the row lane by lane and scaling it again; the helper —
// one or two pivots behind — applies that pivot to its own tiles of X and S (6 ds_swizzle, column p of X as a row through one
// narrow LDS record, 18 FMA, no reciprocal chain).  When the chain wave has finished block k (store + fused
// sweep), block k+1 is waiting for it in LDS in exactly the lane layout its Gauss–Jordan starts from.  Chain per block:
// Gauss–Jordan + store + sweep; the sparse products are gone (the helper never forms P·anything: same flops as the explicit
// products, but off the chain).  The middle block takes both helpers' contributions.
// The elimination form is as stable as the explicit one: for a PSD bordered matrix the border lies in range(G), so along a
// (near-)null direction of G + δI the border column is O(eps) and enters the update as (eps)²/δ — the same quadratic
// term the explicit form has through Q = W − W P W.
// Hand-offs go through LDS flags (monotone sequence numbers; DS operations of one wave execute in program order, so a
// flag written after the data is seen after the data): chain → helper per pivot, helper → chain per block.  All four waves
// of the workgroup are resident (one workgroup per CU), every wait is on a wave that never waits for the waiter.
// Everything else — setup, residual passes, output — is split four ways instead of two; the order of the sweeps' vector operations,
// the middle block, the multiplier iteration and the status words are those of the two-wave kernel.  The mat-vec inside the
// sweeps is not, in the three-tile classes (<32,10>, <32,12>): P_k stays in the tile layout the Gauss–Jordan leaves it in —
// in registers, in the workspace (nine rows of 64 per block) and in all four sweeps (matvec_tiles: Pᵀ·v, reduced over the
// lane-grid rows by VALU cross-lane moves) — and the input vector of a block's fused sweep step, which has no P_k in it, is
// formed one block ahead, before that block's elimination starts.  Same entries, same products; the additions come in another
// order than in the two-wave kernel.  The four-tile classes keep its column layout and its mat-vec.
// The symbolic part of the setup — the gather of Ã, Ãᵀ, B̃, B̃ᵀ from the shared CSR operator into row lists of local indices
// and values (a binary search in the index set per entry), the list lengths, and which blocks repeat their predecessor's
// masks — depends only on what a plan fixes.  twisted4_prepare_kernel (below) does it once per plan, one record per column in a
// plan-owned pool; a launch copies the record into LDS with coalesced loads and builds its dense images from there.
// The static parts S_k themselves (and δ) are plan constants too: the same kernel builds them into a second pool, in the helper's
// register layout, and the helpers load them (h2_column_twisted4_kernel<…, PRE = true>); the instantiation with PRE = false
// still rebuilds them per launch, for plans whose pool would be too large and for SLS_T4_PRESTATIC=0.  With the blocks go the two
// setup images that depend on the plan alone — the dense image of Ã and the weight table Wx — in a third pool: the PRE
// instantiation copies them, the other one builds them in a second setup stage.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "sls_device.h"
#include "sls_launch.h"
#include "sls_wave_util.h"
#include "sls_column_ops.h"

namespace sls {

#ifndef SLS_T4_EXP
#define SLS_T4_EXP 0          // timing experiment (WRONG results on purpose): 1 = helper does not eliminate
#endif

// meeting block.  The upward side carries the mask ramp (its helper needs a fresh static part for every block while the
// masks still grow — loaded from the plan's pool, or rebuilt: in the three-tile classes from Ã / B̃ values gathered once per
// column into registers, so a rebuild reads weights only — the downward side's masks repeat) and the middle block's own
// inversion: it gets the shorter half.
#ifndef SLS_T4_MIDDLE_SHIFT
#define SLS_T4_MIDDLE_SHIFT 0
#endif
static inline __host__ __device__ int twisted4_middle(int T) { return T >= 7 ? (T + 1) / 2 - SLS_T4_MIDDLE_SHIFT : (T - 1) / 2; }

// LDS flags between the waves of one workgroup: RELAXED workgroup-scope atomics are plain ds_read/ds_write (a `volatile` access
// makes the backend wait for every outstanding LDS and global operation after it — ≈250 cycles per pivot on the chain wave,
// measured); ordering comes from the hardware (DS operations of one wave execute in program order) plus compiler barriers.
__device__ __forceinline__ int flag_load(const int* f) {
  return __builtin_amdgcn_readfirstlane(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
__device__ __forceinline__ void flag_store(int* f, int v) {
  asm volatile("" ::: "memory");
  __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void wait_flag(const int* f, int target) {
  for (;;) {
    if (flag_load(f) >= target) break;
    __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
}

// Broadcast inside each 8-lane group of the lane grid (lane = 8·a + b → the value of lane (a, QA)) WITHOUT the LDS crossbar:
// two DPP row_newbcast moves per 32-bit half, one per half of the 16-lane DPP row (bank masks 0x3 / 0xc).  ds_swizzle does the
// same in one DS instruction per half.  Measured SLOWER (README launch 0.1174 → 0.1239 ms): the waves are bound by instruction
// issue, and four VALU moves per value cost more issue slots than two ds_swizzle; kept as an A/B switch.
// ISA markers for tools/isa_mix.py (-DSLS_ISA_MARKS=1, assembly listings only): an assembler comment at a point every pivot
// already passes through a sched_barrier, so the listing is cut into one span per pivot without moving anything across it.
#if defined(SLS_ISA_MARKS) && SLS_ISA_MARKS
#define SLS_ISA_MARK(name) asm volatile("; isa-mark " name)
#else
#define SLS_ISA_MARK(name) ((void)0)
#endif

// Per-pivot phase stamps (SLS_PHASE_TIMERS = 2 / 3: chain waves' / helper waves' shares, tools/t4_phases.py) are compiled in only
// with -DSLS_T4_PHASES=1: the shipped kernel carries no s_memtime pair around the helper's wait and no dbg_level branch per block.
#ifndef SLS_T4_PHASES
#define SLS_T4_PHASES 0
#endif
#ifndef SLS_T4_SAME
#define SLS_T4_SAME 1          // reuse of the static part of a block while the masks repeat (0: always rebuilt; diagnostics)
#endif
#ifndef SLS_T4_DPP
#define SLS_T4_DPP 0
#endif
template <int QA>
__device__ __forceinline__ double bcast8(double v) {
  if constexpr (SLS_T4_DPP != 0) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    int l2 = __builtin_amdgcn_update_dpp(0, lo, 0x150 + QA, 0xf, 0x3, false);
    l2 = __builtin_amdgcn_update_dpp(l2, lo, 0x150 + 8 + QA, 0xf, 0xc, false);
    int h2 = __builtin_amdgcn_update_dpp(0, hi, 0x150 + QA, 0xf, 0x3, false);
    h2 = __builtin_amdgcn_update_dpp(h2, hi, 0x150 + 8 + QA, 0xf, 0xc, false);
    return __hiloint2double(h2, l2);
  } else {
    constexpr int pattern = 0x18 | (QA << 5);
    return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), pattern), __builtin_amdgcn_ds_swizzle(__double2loint(v), pattern));
  }
}

// LDS byte address of a pointer into the workgroup's LDS (the low half of the flat address)
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)p; }

// Stores by EIGHT lanes of the wave without a divergent region: EXEC is set by two scalar moves around the DS instructions
// (the eight lanes are known at compile time) and restored to all lanes — the code around these calls runs with every lane
// active.  A compiler-generated `if (lane ∈ set) store` cost the chain wave ≈150 cycles per pivot (v_cmp → s_and_saveexec →
// branch), 64-lane stores to junk addresses loaded the LDS pipe that all four waves' cross-lane traffic shares.
// s_lshl_b64 writes SCC, hence the "scc" clobber.  The compiler does not count these DS operations in its s_waitcnt bookkeeping; LDS operations complete in order, so every
// wait it emits for its own operations only becomes stricter.
// Lanes 8·A … 8·A+7 (one row of the lane grid): TR doubles to addr + off0 + 64·q, one more to addr_d + offd, a flag word.
typedef double d2_t __attribute__((ext_vector_type(2)));
// Packed layout of a published pivot: per lane-grid column b a record of SB doubles at rowbuf[pv·RS + SB·b]:
//   TR = 3: {row·d [b], row·d [b+8], row·d [b+16], d}        (SB = 4: two ds_write_b128)
//   TR = 4: {row·d [b], [b+8], [b+16], [b+24], d, –}          (SB = 6: two ds_write_b128 + one ds_write_b64)
// then the flag word: three (four) DS instructions per pivot instead of five (six) — each costs a lone wave ≈ 12 issue cycles.
// The eight lanes are switched by a wave-uniform mask m (0xff: store, 0: the DS instructions issue with no lane active and write
// nothing): a pivot that may not be published costs no branch, and no register merges behind one.
template <int A, int O0>
__device__ __forceinline__ void store_row8_3(unsigned long long m, unsigned addr, double v0, double v1, double v2, double d, unsigned addr_flag, int flagval) {
  const d2_t q0 = {v0, v1}, q1 = {v2, d};
  asm volatile("s_lshl_b64 exec, %[m], %[sh]\n\t"
               "ds_write_b128 %[a], %[q0] offset:%[o0]\n\tds_write_b128 %[a], %[q1] offset:%[o1]\n\t"
               "ds_write_b32 %[af], %[vf]\n\ts_mov_b64 exec, -1"
               :: [m] "s"(m), [sh] "n"(8 * A), [a] "v"(addr), [q0] "v"(q0), [q1] "v"(q1), [af] "v"(addr_flag), [vf] "v"(flagval),
                  [o0] "n"(O0), [o1] "n"(O0 + 16) : "memory", "scc");
}
template <int A, int O0>
__device__ __forceinline__ void store_row8_4(unsigned long long m, unsigned addr, double v0, double v1, double v2, double v3, double d, unsigned addr_flag, int flagval) {
  const d2_t q0 = {v0, v1}, q1 = {v2, v3};
  asm volatile("s_lshl_b64 exec, %[m], %[sh]\n\t"
               "ds_write_b128 %[a], %[q0] offset:%[o0]\n\tds_write_b128 %[a], %[q1] offset:%[o1]\n\tds_write_b64 %[a], %[vd] offset:%[o2]\n\t"
               "ds_write_b32 %[af], %[vf]\n\ts_mov_b64 exec, -1"
               :: [m] "s"(m), [sh] "n"(8 * A), [a] "v"(addr), [q0] "v"(q0), [q1] "v"(q1), [vd] "v"(d), [af] "v"(addr_flag), [vf] "v"(flagval),
                  [o0] "n"(O0), [o1] "n"(O0 + 16), [o2] "n"(O0 + 32) : "memory", "scc");
}
// Lanes 0, 8, 16, … 56 (column 0 of the lane grid): TR doubles to addr + O0 + 64·q
template <int O0>
__device__ __forceinline__ void store_col8_3(unsigned addr, double v0, double v1, double v2) {
  asm volatile("s_mov_b32 exec_lo, 0x01010101\n\ts_mov_b32 exec_hi, 0x01010101\n\t"
               "ds_write_b64 %[a], %[v0] offset:%[o0]\n\tds_write_b64 %[a], %[v1] offset:%[o1]\n\tds_write_b64 %[a], %[v2] offset:%[o2]\n\t"
               "s_mov_b64 exec, -1"
               :: [a] "v"(addr), [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [o0] "n"(O0), [o1] "n"(O0 + 64), [o2] "n"(O0 + 128) : "memory");
}
template <int O0>
__device__ __forceinline__ void store_col8_4(unsigned addr, double v0, double v1, double v2, double v3) {
  asm volatile("s_mov_b32 exec_lo, 0x01010101\n\ts_mov_b32 exec_hi, 0x01010101\n\t"
               "ds_write_b64 %[a], %[v0] offset:%[o0]\n\tds_write_b64 %[a], %[v1] offset:%[o1]\n\tds_write_b64 %[a], %[v2] offset:%[o2]\n\tds_write_b64 %[a], %[v3] offset:%[o3]\n\t"
               "s_mov_b64 exec, -1"
               :: [a] "v"(addr), [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3), [o0] "n"(O0), [o1] "n"(O0 + 64), [o2] "n"(O0 + 128), [o3] "n"(O0 + 192) : "memory");
}

// Lanes QA, QA + 8, … QA + 56 (column QA of the lane grid): TR doubles to addr + O0 (one 32-byte record per lane-grid row)
template <int QA, int O0>
__device__ __forceinline__ void store_xcol8_3(unsigned addr, double v0, double v1, double v2) {
  const d2_t q0 = {v0, v1};
  asm volatile("s_mov_b32 exec_lo, %[m]\n\ts_mov_b32 exec_hi, %[m]\n\t"
               "ds_write_b128 %[a], %[q0] offset:%[o0]\n\tds_write_b64 %[a], %[v2] offset:%[o1]\n\t"
               "s_mov_b64 exec, -1"
               :: [m] "n"((int)(0x01010101u << QA)), [a] "v"(addr), [q0] "v"(q0), [v2] "v"(v2), [o0] "n"(O0), [o1] "n"(O0 + 16) : "memory");
}
template <int QA, int O0>
__device__ __forceinline__ void store_xcol8_4(unsigned addr, double v0, double v1, double v2, double v3) {
  const d2_t q0 = {v0, v1}, q1 = {v2, v3};
  asm volatile("s_mov_b32 exec_lo, %[m]\n\ts_mov_b32 exec_hi, %[m]\n\t"
               "ds_write_b128 %[a], %[q0] offset:%[o0]\n\tds_write_b128 %[a], %[q1] offset:%[o1]\n\t"
               "s_mov_b64 exec, -1"
               :: [m] "n"((int)(0x01010101u << QA)), [a] "v"(addr), [q0] "v"(q0), [q1] "v"(q1), [o0] "n"(O0), [o1] "n"(O0 + 16) : "memory");
}

// Tiled Gauss–Jordan of the chain wave on the 8×8 lane grid (lane (a, b) holds {rows a + 8·ri} × {columns b + 8·cj}), in place
// on the tiles, publishing every pivot's row and reciprocal for the helper wave: rowbuf[pv] = eight packed records (RS doubles per pivot, see store_row8_*), then *flag = seqbase + pv + 1.
// The chain wave takes its own copy of the scaled pivot row from that record.  The owner lanes of pivot p + 1 (lane-grid row
// (p + 1) mod 8) hold row p + 1 in their tiles; as soon as the FMAs of pivot p that touch it are done they multiply it with the
// predicted reciprocal and publish it, flag included, and every lane reads the record of its grid column back: two DS reads
// where 2·TR ds_bpermute and TR multiplies used to fetch and scale the row a second time.  Same operands, same product, formed by
// the lane that owns the row.  The reads follow the stores in the program of ONE wave, whose DS operations execute in order, and
// every pivot has a slot of its own: a read can see neither an older nor a newer record than its pivot's.  A flag value is only
// ever raised earlier than before (record p + 1 while pivot p is still being eliminated), which the helper's rule — flag ≥
// seqbase + p + 1 ⇒ record p is valid — does not notice, except that its speculative read succeeds more often.
template <int NP, int TR, int RS>
__device__ __forceinline__ void gj_tiles_publish(double (&Tt)[TR * TR], const int lane, const int n, double* rowbuf, int* flag,
                                                 const int seqbase) {
  int ta = lane >> 3, tb = lane & 7, nn = __builtin_amdgcn_readfirstlane(n);
  asm volatile("" : "+v"(ta), "+v"(tb), "+s"(nn));
  double dnext = fast_rcp(readlane_f64(Tt[0], 0));
  constexpr int SB = (TR == 3) ? 4 : 6;                   // doubles per published record (see store_row8_*)
  static_assert(RS == 8 * SB, "row stride = eight records");
  static_assert(TR == 3 || TR == 4, "store_row8_* are written for three or four tile columns");
  const unsigned pub_addr = lds_addr(rowbuf + SB * tb), flag_addr = lds_addr(flag);
  const double* row_rec = rowbuf + SB * tb;               // the record of this lane's grid column
  double col[TR], tj[TR];
  // Pivot q for the helper and for this wave: the row as it is BEFORE the update of pivot q, times 1/pivot (what an LU step uses),
  // 1/pivot, then the flag — every lane multiplies, the eight owner lanes (a = q mod 8) store (m = 0xff; m = 0: nobody does).
  auto publish = [&](auto q_c, const double xr, const unsigned long long m) {
    constexpr int q = decltype(q_c)::value;
    constexpr int qs = q / 8;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int cj = 0; cj < TR; ++cj) t[cj] = Tt[qs * TR + cj] * xr;
    if constexpr (TR == 3) store_row8_3<q % 8, q * RS * 8>(m, pub_addr, t[0], t[1], t[2], xr, flag_addr, seqbase + q + 1);
    else store_row8_4<q % 8, q * RS * 8>(m, pub_addr, t[0], t[1], t[2], t[3], xr, flag_addr, seqbase + q + 1);
  };
  // Column q by ds_swizzle inside the 8-lane group; the scaled row q from the record published just before: two DS reads (1/pivot,
  // the fourth double of a three-tile record and the fifth of a four-tile one, is wave-uniform here already and is not read)
  auto fetch = [&](auto q_c) {
    constexpr int q = decltype(q_c)::value;
    constexpr int qa = q % 8, qs = q / 8;
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      col[ri] = bcast8<qa>(Tt[ri * TR + qs]);
    }
    const double* rec = row_rec + q * RS;
    const d2_t r0 = *reinterpret_cast<const d2_t*>(rec);
    tj[0] = r0[0]; tj[1] = r0[1];
    if constexpr (TR == 3) tj[2] = rec[2];
    else { const d2_t r1 = *reinterpret_cast<const d2_t*>(rec + 2); tj[2] = r1[0]; tj[TR - 1] = r1[1]; }
  };
  // pivot 0 is published here: the caller's receive() has seen the helper's hand-over, so the previous block's records are consumed
  publish(std::integral_constant<int, 0>{}, dnext, 0xffull);
  fetch(std::integral_constant<int, 0>{});
  static_for<NP>([&](auto pv_c) {
    constexpr int pv = decltype(pv_c)::value;
    constexpr int pa = pv % 8, ps = pv / 8;
    if (pv < nn) {
      const double d = dnext;
      constexpr bool have_next = pv + 1 < NP;
      constexpr int na = (pv + 1) % 8, ns = have_next ? (pv + 1) / 8 : ps;
      double xr = 0.0;
      if constexpr (have_next) {
        const double a_nn = readlane_f64(Tt[ns * TR + ns], na * 8 + na);
        const double a_pn = readlane_f64(Tt[ps * TR + ns], pa * 8 + na);
        const double pn = __builtin_fma(-(a_pn * d), a_pn, a_nn);
        xr = __builtin_amdgcn_rcp(pn);
        if (SLS_GJ_NR >= 1) xr = __builtin_fma(__builtin_fma(-pn, xr, 1.0), xr, xr);
        if (SLS_GJ_NR >= 2) xr = __builtin_fma(__builtin_fma(-pn, xr, 1.0), xr, xr);
      }
      double c0[TR], t0[TR], tfix[TR];
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) c0[ri] = col[ri];
#pragma unroll
      for (int cj = 0; cj < TR; ++cj) {
        t0[cj] = tj[cj];
        tfix[cj] = (cj == ps && tb == pa) ? (1.0 + d) : t0[cj];
      }
      __builtin_amdgcn_sched_barrier(0);
      SLS_ISA_MARK("chain-pivot");
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
        for (int cj = 0; cj < TR; ++cj)
          if (ri == ns || cj == ns || ri == ps) Tt[ri * TR + cj] = __builtin_fma(-c0[ri], tfix[cj], Tt[ri * TR + cj]);
      }
      const bool own = ta == pa;
#pragma unroll
      for (int cj = 0; cj < TR; ++cj) {                     // (selects, not a branch: a register write inside a divergent region made the
        const double nv = (cj == ps && tb == pa) ? d : t0[cj];   //  allocator copy the whole tile array around it, ≈30 v_mov per pivot)
        Tt[ps * TR + cj] = own ? nv : Tt[ps * TR + cj];
      }
      if constexpr (have_next) {
        // Row pv + 1 is final once the FMAs above have touched tile row ns: publish it now, with the predicted reciprocal, and read it
        // back behind the rest of this pivot's FMAs.  Not for a pivot that is not eliminated (pv + 1 = nn): no record, no flag —
        // the stores then run with no lane active, and what the reads return is never used.
        __builtin_amdgcn_sched_barrier(0);
        publish(std::integral_constant<int, have_next ? pv + 1 : 0>{}, xr, (pv + 1 < nn) ? 0xffull : 0ull);
        __builtin_amdgcn_sched_barrier(0);
        fetch(std::integral_constant<int, have_next ? pv + 1 : 0>{});
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
        for (int cj = 0; cj < TR; ++cj)
          if (!(ri == ns || cj == ns || ri == ps)) Tt[ri * TR + cj] = __builtin_fma(-c0[ri], tfix[cj], Tt[ri * TR + cj]);
      }
      if constexpr (have_next) dnext = xr;
    }
  });
}

// Pᵀ·v on the tiles where the Gauss–Jordan left them (three-tile classes): lane (a, b) multiplies its 3×3 tiles with the vector
// entries of its tile ROWS, v_q = v[a + 8·q], and the three partial sums — entries b, b + 8, b + 16 of the product — are added
// over a by VALU cross-lane moves only: no LDS image of the matrix, no LDS round trip in the reduction.  The waves are bound
// by instruction issue, so the three sums share their moves (pairsum32 / pairsum16: one pair of swaps reduces two values, each
// into one half): bit 2 of a for entries b and b + 8 together and for b + 16 alone, bit 1 for that pair, bit 0 by DPP — 14
// instructions, where three separate three-stage sums take 39.  The complete sums land by a:
//   a = 0, 1: entry b        a = 4, 5: entry b + 8        a = 2, 3, 6, 7: entry b + 16
// and the caller's lanes a = 0, 4, 2 (twisted4_tile_slot) store the vector with one DS write by 24 lanes.
// The sum runs over rows, as the column-layout mat-vec's does: the same entries of the computed inverse meet the same
// entries of v, only the order of the additions differs.
__device__ __forceinline__ double matvec_tiles(const double (&Tt)[9], const double v0, const double v1, const double v2) {
  double r[3];
#pragma unroll
  for (int cj = 0; cj < 3; ++cj) r[cj] = __builtin_fma(Tt[6 + cj], v2, __builtin_fma(Tt[3 + cj], v1, Tt[cj] * v0));
  return xsum8(pairsum16(pairsum32(r[0], r[1]), xsum32(r[2])));
}
// which third of the product (tile column cj) the lanes of lane-grid row a hold after matvec_tiles; the writers are a = 0, 4, 2
__device__ __forceinline__ int twisted4_tile_slot(int ta) { return (ta & 2) ? 2 : (ta >> 2); }

// The helper wave's side of the same elimination: X ← X − X[:,p]·(d·g[p,:]),  S ← S − (X[:,p]·d)·X[:,p]ᵀ for every pivot p the chain
// wave has published (same lane grid; column p of X by ds_swizzle inside the 8-lane group, the same column as a row through the
// LDS record `xbuf`).  Columns ≤ p of X are dead after pivot p and are left to whatever the update makes of them.
template <int NP, int TR, int RS>
__device__ __forceinline__ void helper_eliminate(double (&Xw)[TR * TR], double (&Sw)[TR * TR], const int lane, const int n,
                                                 const double* rowbuf, const int* flag, const int seqbase, double* xbuf,
                                                 unsigned long long& wait_cycles) {
  int ta = lane >> 3, tb = lane & 7, nn = __builtin_amdgcn_readfirstlane(n);
  asm volatile("" : "+v"(ta), "+v"(tb), "+s"(nn));
  int ready = 0;
  // Column q of X in both index forms, fetched one pivot ahead (as the chain wave does with its pivot row and column): only the
  // entries of the NEXT pivot's column slot have to be up to date before its cross-lane reads issue, the other FMAs of the
  // step run in their shadow.  Two register sets, alternating by pivot parity (no copies).
  // Row form: the eight lanes that hold column q (b = q mod 8) write their TR entries as one 32-byte record per lane-grid row a,
  // every lane reads back record b (rows b + 8·cj): two DS writes by eight lanes + two reads instead of 2·TR ds_bpermute.  The
  // slot is reused by the next pivot without a wait: DS operations of one wave execute in program order, the read of pivot q is
  // done before the write of pivot q + 1.  Only the S update (phase B) uses the row form, off the step's dependent chain.
  // The column form stays a broadcast inside the 8-lane group: read from record a of the same buffer it costs four DS instructions
  // less, and the launch was SLOWER (the helper's busy time fell, the chain wave's Gauss–Jordan grew).
  double xc[2][TR], xrw[2][TR];
  const unsigned xw_addr = lds_addr(xbuf + 4 * ta);
  const double* xr_rec = xbuf + 4 * tb;
  auto fetchX = [&](auto q_c) {
    constexpr int q = decltype(q_c)::value;
    constexpr int qa = q % 8, qs = q / 8, par = q & 1;
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      xc[par][ri] = bcast8<qa>(Xw[ri * TR + qs]);
    }
    static_assert(TR == 3 || TR == 4, "store_xcol8_* are written for three or four tile rows");
    if constexpr (TR == 3) store_xcol8_3<qa, 0>(xw_addr, Xw[qs], Xw[TR + qs], Xw[2 * TR + qs]);
    else store_xcol8_4<qa, 0>(xw_addr, Xw[qs], Xw[TR + qs], Xw[2 * TR + qs], Xw[3 * TR + qs]);
    const d2_t r0 = *reinterpret_cast<const d2_t*>(xr_rec);
    xrw[par][0] = r0[0]; xrw[par][1] = r0[1];
    if constexpr (TR == 3) xrw[par][2] = xr_rec[2];
    else { const d2_t r1 = *reinterpret_cast<const d2_t*>(xr_rec + 2); xrw[par][2] = r1[0]; xrw[par][3] = r1[1]; }
  };
  fetchX(std::integral_constant<int, 0>{});
  // The published row of the NEXT pivot is read speculatively one step ahead, flag first (DS operations execute in order: a
  // flag value that covers the pivot makes the data read after it valid); only when the chain wave had not got there yet
  // does the step poll and read again.  Takes two LDS round trips per pivot off the helper's chain.
  double dn[2] = {0.0, 0.0}, gn[2][TR];
  int fnext = 0;
  constexpr int SB = (TR == 3) ? 4 : 6;
  static_assert(RS == 8 * SB, "row stride = eight records");
  auto read_row = [&](int q, int par) {                   // the record of this lane's grid column: two ds_read_b128 (+ one b64)
    const double* rec = rowbuf + q * RS + SB * tb;
    const d2_t q0 = *reinterpret_cast<const d2_t*>(rec), q1 = *reinterpret_cast<const d2_t*>(rec + 2);
    gn[par][0] = q0[0]; gn[par][1] = q0[1]; gn[par][2] = q1[0];
    if constexpr (TR == 3) dn[par] = q1[1];
    else { gn[par][TR - 1] = q1[1]; dn[par] = rec[4]; }
  };
  auto prefetch_row = [&](auto q_c) {
    constexpr int q = decltype(q_c)::value, par = q & 1;
    fnext = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
    read_row(q, par);
  };
  prefetch_row(std::integral_constant<int, 0>{});
  static_for<NP>([&](auto pv_c) {
    constexpr int pv = decltype(pv_c)::value;
    if (pv < nn) {
      constexpr bool have_next = pv + 1 < NP;
      constexpr int ps = pv / 8, ns = have_next ? (pv + 1) / 8 : pv / 8, par = pv & 1;
      const int target = seqbase + pv + 1;
      ready = max(ready, __builtin_amdgcn_readfirstlane(fnext));
      if (ready < target) {
        unsigned long long w0 = 0;
        if constexpr (SLS_T4_PHASES != 0) w0 = __builtin_amdgcn_s_memtime();
        while (ready < target) {
          ready = flag_load(flag);
          if (ready < target) __builtin_amdgcn_s_sleep(1);
        }
        if constexpr (SLS_T4_PHASES != 0) wait_cycles += __builtin_amdgcn_s_memtime() - w0;
        asm volatile("" ::: "memory");
        read_row(pv, par);
      }
      if constexpr (have_next) prefetch_row(std::integral_constant<int, have_next ? pv + 1 : 0>{});
      const double d = dn[par];
      double m[TR];
      const double (&grow)[TR] = gn[par];
      __builtin_amdgcn_sched_barrier(0);
      SLS_ISA_MARK("helper-pivot");
      // phase A: the next pivot's column slot of X
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) Xw[ri * TR + ns] = __builtin_fma(-xc[par][ri], grow[ns], Xw[ri * TR + ns]);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (have_next) fetchX(std::integral_constant<int, have_next ? pv + 1 : 0>{});
      __builtin_amdgcn_sched_barrier(0);
      // phase B: the live rest of X (column slots below the pivot's are dead), the stored half of S (tiles ri ≤ cj)
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) m[ri] = xc[par][ri] * d;
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
        for (int cj = 0; cj < TR; ++cj) {
          if (cj != ns && cj >= ps) Xw[ri * TR + cj] = __builtin_fma(-xc[par][ri], grow[cj], Xw[ri * TR + cj]);      // grow = g[p,:]·d as published
          if (ri <= cj) Sw[ri * TR + cj] = __builtin_fma(-m[ri], xrw[par][cj], Sw[ri * TR + cj]);
        }
      }
      // Every tile is updated at this pivot, not later: without the pin the compiler sinks the updates of column slots whose
      // pivots are still 8–16 steps away into one batch there, keeps every postponed pivot's column and row alive until then and
      // spills them to AGPRs (≈ 290 accvgpr copies over the <32,12> helper loop; 28 with the pin, tools/isa_mix.py).
#pragma unroll
      for (int q = 0; q < TR * TR; ++q) asm volatile("" : "+v"(Xw[q]), "+v"(Sw[q]));
    }
  });
}

// Static part of block k on the lane grid, S_k = δI + W_k + Ã W_{k−1} Ãᵀ + B̃ Wu_{k−1} B̃ᵀ (stored half, tiles ri ≤ cj): the ONE text
// of this arithmetic.  twisted4_prepare_kernel runs it once per plan into the column's pool; the rebuild instantiation of the
// solve kernel runs it per launch.  Both must give the same bits, so the order is fixed: the diagonal δ + wc[i], then the Ã
// entries in list order (the first KH from registers, padding included, then the tail up to the longest list), then B̃'s.
// wc / wp: Wx_k / Wx_{k−1} rows of the weight table, wu: Wu_{k−1}; fold0: δ·w/(δ + w) in the place of Wx_0 (upward block 1).
// HOIST: the second factors come from GA / GB (the values the LDS gathers below would read, held in registers).
template <int TR, bool HOIST, int KH, int KB, int NPL, int LDT>
__device__ __forceinline__ void twisted4_static_block(double (&Sw)[TR * TR], const double delta, const double* wc_, const double* wp_,
                                                      const double* wu_, const bool fold0, const int ta, const int tb,
                                                      const int nzA, const int nzB, const int MC,
                                                      const int (&hac)[TR][KH], const double (&hav)[TR][KH],
                                                      const int (&hbc)[TR][KB], const double (&hbv)[TR][KB],
                                                      const double (&GA)[KH][TR][TR], const double (&GB)[KB][TR][TR],
                                                      const int32_t* arow_c, const double* arow_v, const int32_t* brow_c,
                                                      const double* brow_v, const double* Ad, const double* Bd) {
#pragma unroll
  for (int ri = 0; ri < TR; ++ri) {
    const int i = ta + 8 * ri;
    const double di = delta + wc_[i];
#pragma unroll
    for (int cj = 0; cj < TR; ++cj) Sw[ri * TR + cj] = (i == tb + 8 * cj) ? di : 0.0;
  }
#pragma unroll
  for (int e = 0; e < KH; ++e) {
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      const int cc = hac[ri][e];
      const double w0 = wp_[cc];
      const double v = hav[ri][e] * (fold0 ? delta * w0 / (delta + w0) : w0);
#pragma unroll
      for (int cj = ri; cj < TR; ++cj) {
        double g;
        if constexpr (HOIST) g = GA[e][ri][cj]; else g = Ad[(tb + 8 * cj) * LDT + cc];
        Sw[ri * TR + cj] = __builtin_fma(v, g, Sw[ri * TR + cj]);
      }
    }
  }
  for (int e = KH; e < nzA; ++e) {
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      const int i = ta + 8 * ri;
      const int cc = arow_c[e * NPL + i];
      const double w0 = wp_[cc];
      const double v = arow_v[e * NPL + i] * (fold0 ? delta * w0 / (delta + w0) : w0);
#pragma unroll
      for (int cj = ri; cj < TR; ++cj) Sw[ri * TR + cj] = __builtin_fma(v, Ad[(tb + 8 * cj) * LDT + cc], Sw[ri * TR + cj]);
    }
  }
#pragma unroll
  for (int e = 0; e < KB; ++e) {
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      const int cc = hbc[ri][e];
      const double v = hbv[ri][e] * wu_[cc];
#pragma unroll
      for (int cj = ri; cj < TR; ++cj) {
        double g;
        if constexpr (HOIST) g = GB[e][ri][cj]; else g = Bd[(tb + 8 * cj) * MC + cc];
        Sw[ri * TR + cj] = __builtin_fma(v, g, Sw[ri * TR + cj]);
      }
    }
  }
  for (int e = KB; e < nzB; ++e) {
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      const int i = ta + 8 * ri;
      const int cc = brow_c[e * NPL + i];
      const double v = brow_v[e * NPL + i] * wu_[cc];
#pragma unroll
      for (int cj = ri; cj < TR; ++cj) Sw[ri * TR + cj] = __builtin_fma(v, Bd[(tb + 8 * cj) * MC + cc], Sw[ri * TR + cj]);
    }
  }
}

// Which slots of a column's pool the helpers read (c = twisted4_middle(T); bits: the mask-repeat words of the record, taken as
// 0 when the reuse is compiled out).  The upward helper produces blocks 1 … c: block 1 from slot 0, block 2 always from slot 2,
// a later block k from slot k unless k < 64 and bit k of bits[0] lets it reuse its predecessor's.  The downward helper
// produces blocks T … c + 1 (its contribution to the middle block c is zeros): block T always from slot T, a later block k
// from slot k unless k < 64 and bit k of bits[1] is set.  The solve kernel's helper loop follows the same rule.
static inline __host__ __device__ bool twisted4_slot_read(int slot, int T, int c, unsigned long long up, unsigned long long down) {
  if (slot == 0) return c >= 1;
  const bool rep_up = slot < 64 && ((up >> slot) & 1ull), rep_down = slot < 64 && ((down >> slot) & 1ull);
  const bool by_up = slot >= 2 && slot <= c && (slot == 2 || !rep_up);
  const bool by_down = slot >= c + 1 && slot <= T && (slot == T || !rep_down);
  return by_up || by_down;
}

template <int NPL, int RPL, bool PRE>
__device__ __forceinline__ void twisted4_solve_column(const KernelParams& p, const SubDesc& sd, const unsigned char* __restrict__ rec,
                                                      const double* __restrict__ spool, const double* __restrict__ images,
                                                      double* __restrict__ fac, unsigned char* lds_raw) {
  static_assert(NPL == 32, "written for the NPL = 32 classes (8×8 lane grid)");
  constexpr int HS = 64 / NPL, NP = HS * RPL;
  constexpr int TR = (NP + 7) / 8, NR = 8 * TR, TT = TR * TR;
  constexpr int LDT = 40;                                 // leading dimension of the tile images (8·a + b: no bank conflict)
  constexpr int RS = (TR == 3) ? 32 : 48;                 // doubles per published pivot: eight packed records (store_row8_*)
  constexpr int PRIVC = NR * LDT + 2 * NPL;               // chain wave: mat, tmp, tmp2
  constexpr int PRIVH = 32;                               // helper wave: the row form of column p of X (eight 32-byte records)
  constexpr int DIRSZ = NR * RS + NR * LDT + 2;           // per direction: published rows, hand-off tiles, two flags
  const int wv = threadIdx.x >> 6;                        // 0/1: chain waves (up / down), 2/3: their helpers
  const int dir = wv & 1, helper = wv >> 1;
  const int lane = threadIdx.x & 63;
  const int h = lane / NPL, j = lane % NPL;
  const int ta = lane >> 3, tb = lane & 7;
  const int n = sd.n, m = sd.m, nm = n + m, T = p.T;
  const int MC = p.w_mcap;
  const int capA = p.w_nzA, capAc = p.w_nzAc, capB = p.w_nzB, capBc = p.w_nzBc;
  const int c = twisted4_middle(T);

  // ---- LDS carve (must match twisted4_kernel_lds_bytes: the private part, then the walk of column_carve, sls_device.h) ----
  static_assert(2 * PRIVC + 2 * PRIVH + 2 * DIRSZ + NR * LDT == twisted4_kernel_private_doubles(NPL, RPL), "the private part twisted4_kernel_lds_bytes counts");
  double* dp = reinterpret_cast<double*>(lds_raw);
  double* privc = dp + dir * PRIVC; dp += 2 * PRIVC;
  double* mat = privc; double* tmp = mat + NR * LDT; double* tmp2 = tmp + NPL;
  double* xbuf = dp + dir * PRIVH; dp += 2 * PRIVH;
  double* dirb = dp + dir * DIRSZ;
  double* dirb_other = dp + (1 - dir) * DIRSZ; dp += 2 * DIRSZ;
  double* rowbuf = dirb; double* hand = rowbuf + NR * RS;
  int* flagA = reinterpret_cast<int*>(hand + NR * LDT);   // chain → helper: rows published (sequence number)
  int* flagB = flagA + 2;                                  // helper → chain: tiles of step s are in `hand`
  double* hand_other = dirb_other + NR * RS;
  int* flagB_other = reinterpret_cast<int*>(hand_other + NR * LDT) + 2;
  double* Ad = dp;     dp += NR * LDT;                    // dense image of Ã (zero padded; leading dimension 40: 8·a + b conflict-free)
  double* hx = dp;     dp += NPL;
  double* gx = dp;     dp += NPL;
  double* hu = dp;     dp += 64;
  double* gu = dp;     dp += 64;
  double* red = dp;    dp += 8;                           // [0..3] per-wave maxima, [4] δ, [5..6] mask-repeat bits (up, down)
  unsigned long long* samew = reinterpret_cast<unsigned long long*>(red + 5);
  int32_t* nzs = reinterpret_cast<int32_t*>(dp) + NPL + 64;   // nzA, nzAc, nzB, nzBc (behind the NPL + 64 words that held s_x, s_u before the prepared records)
  dp += (NPL + 64 + 8) / 2;
  double* lam = dp;    dp += (T + 1) * NPL;
  double* rq = dp;     dp += (T + 1) * NPL;
  double* xs = dp;     dp += (T + 1) * NPL;
  double* Bd = dp;     dp += NPL * MC;
  double* us = dp;     dp += T * MC;
  double* wxt = dp;    dp += (T + 1) * NPL;                // Wx_k[j] for every block k (row T = 0): mask ⊙ H⁻¹ expanded once
  double* wut = dp;    dp += T * MC;                       // Wu_k[q]
  double* arow_v = dp; dp += capA * NPL;
  double* acol_v = dp; dp += capAc * NPL;
  double* brow_v = dp; dp += capB * NPL;
  double* bcol_v = dp; dp += capBc * 64;
  int32_t* ip = reinterpret_cast<int32_t*>(dp);
  int32_t* arow_c = ip; ip += capA * NPL;
  int32_t* acol_c = ip; ip += capAc * NPL;
  int32_t* brow_c = ip; ip += capB * NPL;
  int32_t* bcol_c = ip; ip += capBc * 64;
  uint8_t* mask = reinterpret_cast<uint8_t*>(ip);
  const int32_t* dest = p.dest_pool + sd.off_dest;
  unsigned long long tc[4] = {0, 0, 0, 0};
  unsigned long long tlast = __builtin_amdgcn_s_memtime();
  auto lap = [&](int slot) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tc[slot] += now - tlast; tlast = now; };

  __syncthreads();
  // Plan-time blocks: each helper asks for the static block of its first step (upward: slot 0, downward: slot T) before anything
  // else — step s = 1 has no elimination beside it to hide the load behind, and the chain wave waits for its hand-over.
  constexpr int TQ0 = TR * (TR + 1) / 2;
  double Sl0[TQ0];
  if constexpr (PRE) {
    if (helper) {
      const double* src = spool + (int64_t)(dir == 0 ? 0 : T) * (TQ0 * 64) + lane;
#pragma unroll
      for (int q = 0; q < TQ0; ++q) Sl0[q] = src[q * 64];
    }
  }
  // ---- setup, split over the four waves ----
  // The row lists of Ã, Ãᵀ, B̃, B̃ᵀ, their lengths and the mask-repeat bits come from the column's prepared record
  // (twisted4_prepare_kernel, once per plan): one coalesced copy onto the list images, which lie in the record in LDS order.
  {
    const int nw = (int)(twisted4_record_entries(capA, capAc, capB, capBc) * 3 / 2);          // 64-bit words: values, then indices
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(rec + kT4RecHeader);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(arow_v);
    for (int i = threadIdx.x; i < nw; i += 256) dst[i] = src[i];
    // … and with plan-time blocks the two images of the setup, which lie in the column's pool as the launch would build them
    if constexpr (PRE) {
      for (int i = threadIdx.x; i < NR * LDT; i += 256) Ad[i] = images[i];
      for (int i = threadIdx.x; i < (T + 1) * NPL; i += 256) wxt[i] = images[NR * LDT + i];
    }
  }
  if (wv == 0) {
    if (lane < NPL) {
      hx[lane] = (lane < n) ? (sd.has_w ? p.w_pool[sd.off_w + lane] : 1.0) : 0.0;
      gx[lane] = (lane < n && sd.has_w) ? p.w_pool[sd.off_w + nm + lane] : 0.0;
    }
    hu[lane] = (lane < m) ? (sd.has_w ? p.w_pool[sd.off_w + n + lane] : 1.0) : 0.0;
    gu[lane] = (lane < m && sd.has_w) ? p.w_pool[sd.off_w + nm + n + lane] : 0.0;
  } else if (wv == 1) {
    for (int i = lane; i < T * nm; i += 64) mask[i] = p.mask_pool[sd.off_mask + i];
  } else if (wv == 2) {
    if constexpr (!PRE) {
      for (int i = lane; i < NR * LDT; i += 64) Ad[i] = 0.0;
      for (int i = lane; i < NPL * MC; i += 64) Bd[i] = 0.0;
    }
  } else {
    if (lane < 4) nzs[lane] = reinterpret_cast<const int32_t*>(rec + 16)[lane];
    // δ depends on the weights and the row lists only: with the plan-time blocks it comes from the record, like them
    if constexpr (PRE) { if (lane == 4) red[4] = *reinterpret_cast<const double*>(rec + twisted4_record_tail(capA, capAc, capB, capBc)); }
    if (lane < 2) samew[lane] = reinterpret_cast<const unsigned long long*>(rec)[lane];
    for (int i = lane; i < (T + 1) * NPL; i += 64) { lam[i] = 0.0; rq[i] = 0.0; xs[i] = 0.0; }
  }
  if (helper == 0) {
    if (lane < NPL) { tmp[lane] = 0.0; tmp2[lane] = 0.0; }
  } else if (lane < 4) {
    flagA[lane] = 0;                                      // flagA[0..1], flagB[0..1] of this direction
  }
  __syncthreads();
  // LDS only from here: no global chain, no search.  With plan-time blocks this stage and its barrier do not exist: no δ
  // reduction, no dense B̃ (the regions stay in the carve, unused), and the images of Ã and Wx were copied above.
  if constexpr (!PRE) {
  if (wv == 0) {
    const int a0 = nzs[0], a2 = nzs[2];
    double sc = 0.0;
    if (lane < n) {
      sc = hx[lane];
      for (int e = 0; e < a0; ++e) { const double v = arow_v[e * NPL + lane]; sc = __builtin_fma(v * v, hx[arow_c[e * NPL + lane]], sc); }
      for (int e = 0; e < a2; ++e) { const double v = brow_v[e * NPL + lane]; sc = __builtin_fma(v * v, hu[brow_c[e * NPL + lane]], sc); }
    }
    const double dl_ = p.delta_rel * wave_max_f64(sc);
    if (lane == 0) red[4] = dl_;
  } else if (wv == 1) {
    // dense image of B̃ (a list entry is a stored non-zero, the padding is 0.0)
    const int a2 = nzs[2];
    if (lane < n) {
      for (int e = 0; e < a2; ++e) {
        const double v = brow_v[e * NPL + lane];
        if (v != 0.0) Bd[lane * MC + brow_c[e * NPL + lane]] = v;
      }
    }
  } else if (wv == 2) {
    // dense image of Ã for the helpers (row i, column loc): the second factor of Ã W Ãᵀ and the border blocks X
    const int a0 = nzs[0];
    if (lane < n) {
      for (int e = 0; e < a0; ++e) {
        const double v = arow_v[e * NPL + lane];
        if (v != 0.0) Ad[lane * LDT + arow_c[e * NPL + lane]] += v;
      }
    }
  } else {
    // weight tables for the helpers: one LDS read per weight later instead of mask → weight → select chains per block
    for (int i = lane; i < (T + 1) * NPL; i += 64) {
      const int k = i / NPL, jj = i % NPL;
      wxt[i] = (k < T && jj < n && mask[k * nm + jj]) ? hx[jj] : 0.0;
    }
    for (int i = lane; i < T * MC; i += 64) {
      const int k = i / MC, q = i % MC;
      wut[i] = (q < m && mask[k * nm + n + q]) ? hu[q] : 0.0;
    }
  }
  __syncthreads();
  }
  const int nzA = nzs[0], nzAc = nzs[1], nzB = nzs[2], nzBc = nzs[3];
  const double delta = red[4];
  lap(0);

  constexpr int KR = 4;
  int arc[KR], acc_[KR];
  double arv[KR], acv[KR];
#pragma unroll
  for (int e = 0; e < KR; ++e) {
    const bool okr = e < capA, okc = e < capAc;
    arc[e] = okr ? arow_c[e * NPL + j] : 0;  arv[e] = okr ? arow_v[e * NPL + j] : 0.0;
    acc_[e] = okc ? acol_c[e * NPL + j] : 0; acv[e] = okc ? acol_v[e * NPL + j] : 0.0;
  }
  auto dotA_row = [&](const double* vec) -> double {
    static_assert(KR == 4, "written for four cached entries");
    const double v0 = vec[arc[0]], v1 = vec[arc[1]], v2 = vec[arc[2]], v3 = vec[arc[3]];
    double a = __builtin_fma(arv[1], v1, arv[0] * v0) + __builtin_fma(arv[3], v3, arv[2] * v2);
    for (int e = KR; e < nzA; ++e) a = __builtin_fma(arow_v[e * NPL + j], vec[arow_c[e * NPL + j]], a);
    return a;
  };
  auto dotA_col = [&](const double* vec) -> double {
    static_assert(KR == 4, "written for four cached entries");
    const double v0 = vec[acc_[0]], v1 = vec[acc_[1]], v2 = vec[acc_[2]], v3 = vec[acc_[3]];
    double a = __builtin_fma(acv[1], v1, acv[0] * v0) + __builtin_fma(acv[3], v3, acv[2] * v2);
    for (int e = KR; e < nzAc; ++e) a = __builtin_fma(acol_v[e * NPL + j], vec[acol_c[e * NPL + j]], a);
    return a;
  };
  auto wx_of = [&](int k) -> double { return (k >= 0 && k <= T - 1 && j < n && mask[k * nm + j]) ? hx[j] : 0.0; };

  // The three-tile classes keep P_k in the Gauss–Jordan's tile layout (lane (a, b): Pk[ri·TR + cj] = P[a + 8·ri][b + 8·cj]) — in
  // registers, in the workspace (nine rows of 64 in the block's RPL·64 slot) and in every sweep: no conversion anywhere.  The
  // four-tile classes keep the two-wave kernel's column layout (lane (h, j): rows HS·r + h of column j) — sixteen tiles would
  // not fit the slot.  Either way the mat-vec reads its vector from tmp2 and gives entry `wi` of Pᵀ·tmp2 to the lanes `wr`, which
  // write it back: lanes 0 … NPL − 1 with wi = lane in the column layout; 24 lanes in the tile layout (matvec_tiles).  The
  // weight of entry wi comes from the table there (wxt[k·NPL + i] is wx_of(k) of lane i).
  constexpr bool TILE = (TR == 3);
  constexpr int PN = TILE ? TT : RPL;                      // registers (and workspace rows) per block
  const int wi = TILE ? tb + 8 * twisted4_tile_slot(ta) : lane;
  const bool wr = TILE ? ((0x15u >> ta) & 1u) != 0 : (lane < NPL);        // a = 0, 2, 4 (a shift, not three compares: no branches)
  auto wk_arg = [&](int k) -> double {                     // the sweeps' weight argument: only the column layout reads it
    if constexpr (TILE) return 0.0; else return wx_of(k);
  };
  auto matvec = [&](const double (&Pk)[PN]) -> double {
    if constexpr (TILE) {
      return matvec_tiles(Pk, tmp2[ta], tmp2[ta + 8], tmp2[ta + 16]);
    } else {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        const double y = tmp2[HS * r + h];
        if ((r & 3) == 0) a0 = __builtin_fma(Pk[r], y, a0);
        else if ((r & 3) == 1) a1 = __builtin_fma(Pk[r], y, a1);
        else if ((r & 3) == 2) a2 = __builtin_fma(Pk[r], y, a2);
        else a3 = __builtin_fma(Pk[r], y, a3);
      }
      double part = (a0 + a1) + (a2 + a3);
      if (HS >= 2) part = xsum32(part);
      return part;
    }
  };
  auto load_P = [&](int k, double (&Pk)[PN]) {
#pragma unroll
    for (int r = 0; r < PN; ++r) Pk[r] = fac[((int64_t)k * RPL + r) * 64 + lane];
  };
  auto store_P = [&](int k, const double (&Pk)[PN]) {
#pragma unroll
    for (int r = 0; r < PN; ++r) fac[((int64_t)k * RPL + r) * 64 + lane] = Pk[r];
  };

  // r = f − E z(λ): x_t, u_t first (any order), then r_t = f_t − x_t + Ãx_{t−1} + B̃u_{t−1}; 4·HS time steps per round
  auto x_of = [&](int t) -> double {
    const double l0 = lam[t * NPL + j];
    const uint8_t mk = mask[t * nm + j];
    const double a = dotA_col(lam + (t + 1) * NPL);
    const double v = hx[j] * (l0 - a - gx[j]);
    return mk ? v : 0.0;
  };
  int lgMP = 0;
  while ((1 << lgMP) < m) ++lgMP;
  const int uq = lane & ((1 << lgMP) - 1), uts = lane >> lgMP, NTS = 64 >> lgMP;
  auto u_of = [&](int t) -> double {
    const double* l1 = lam + (t + 1) * NPL;
    double a = 0.0;
    for (int e = 0; e < nzBc; ++e) a = __builtin_fma(bcol_v[e * 64 + uq], l1[bcol_c[e * 64 + uq]], a);
    return mask[t * nm + n + uq] ? hu[uq] * (-a - gu[uq]) : 0.0;
  };
  constexpr int G = 4 * HS;
  const int gid = wv * HS + h;
  bool xu_valid = false;
  auto residual_pass = [&]() -> double {       // all 256 threads; contains workgroup barriers
    const bool live = j < n;
    xu_valid = true;
    const int nit = (T + G) / G;
#pragma unroll 2
    for (int it = 0; it < nit; ++it) {
      const int t = gid + it * G;
      const double v = (t < T && live) ? x_of(min(t, T - 1)) : 0.0;
      if (t <= T) xs[t * NPL + j] = v;
    }
    if (uq < m) {
#pragma unroll 2
      for (int t = wv * NTS + uts; t < T; t += 4 * NTS) us[t * MC + uq] = u_of(t);
    }
    __syncthreads();
    double rmax = 0.0;
#pragma unroll 2
    for (int it = 0; it < nit; ++it) {
      const int t = gid + it * G;
      const int tc_ = min(t, T), tp = max(tc_ - 1, 0);
      double a = (t == 0 && j == sd.pos) ? 1.0 : 0.0;
      a -= xs[tc_ * NPL + j];
      double b = dotA_row(xs + tp * NPL);
      const double* up = us + tp * MC;
      for (int e = 0; e < nzB; ++e) b = __builtin_fma(brow_v[e * NPL + j], up[brow_c[e * NPL + j]], b);
      if (t >= 1) a += b;
      if (live && t <= T) {
        rmax = resid_max(rmax, a);
        rq[t * NPL + j] = a;
      }
    }
    rmax = wave_max_f64(rmax);
    if (lane == 0) red[wv] = rmax;
    __syncthreads();
    const double r2 = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r2;
  };
  auto output_pass = [&]() {
    constexpr int CH = 8;
    if (j < n) {
      for (int t0 = gid; t0 < T; t0 += G * CH) {
        int dd[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) { const int t = t0 + q * G; dd[q] = (t < T && mask[t * nm + j]) ? dest[t * nm + j] : -1; }
#pragma unroll
        for (int q = 0; q < CH; ++q) { const int t = t0 + q * G; if (dd[q] >= 0) p.out[dd[q]] = xu_valid ? xs[t * NPL + j] : 0.0; }
      }
    }
    if (uq < m) {
      for (int t0 = wv * NTS + uts; t0 < T; t0 += 4 * NTS * CH) {
        int dd[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) { const int t = t0 + q * 4 * NTS; dd[q] = (t < T && mask[t * nm + n + uq]) ? dest[t * nm + n + uq] : -1; }
#pragma unroll
        for (int q = 0; q < CH; ++q) { const int t = t0 + q * 4 * NTS; if (dd[q] >= 0) p.out[dd[q]] = xu_valid ? us[t * MC + uq] : 0.0; }
      }
    }
  };

  double resid;
  if (sd.has_w) {
    resid = residual_pass();
  } else {
    if (threadIdx.x == 0 && sd.pos >= 0) rq[sd.pos] = 1.0;
    __syncthreads();
    resid = (sd.pos >= 0) ? 1.0 : 0.0;
  }
  int iters = 0, status = 0;

  // ---- sweep steps of the later passes (the two-wave kernel's order of operations; the mat-vec is this kernel's own) ----
  auto elim_up = [&](int k, const double (&Pk)[PN], double wk) {
    if (lane < NPL) {
      double a = rq[k * NPL + lane];
      if (k >= 1) a += dotA_row(tmp);                        // tmp = Wx_{k−1} q_{k−1}
      tmp2[lane] = (lane < n) ? a : 0.0;
    }
    WSYNC();
    const double q = matvec(Pk);
    if (wr) { rq[k * NPL + wi] = q; tmp[wi] = (TILE ? wxt[k * NPL + wi] : wk) * q; }
    WSYNC();
  };
  auto elim_down = [&](int k, const double (&Pk)[PN], double wk) {
    if (lane < NPL) {
      double a = rq[k * NPL + lane];
      if (k < T) a += (TILE ? wxt[k * NPL + lane] : wk) * dotA_col(tmp);      // tmp = q_{k+1}
      tmp2[lane] = (lane < n) ? a : 0.0;
    }
    WSYNC();
    const double q = matvec(Pk);
    if (wr) { rq[k * NPL + wi] = q; tmp[wi] = q; }
    WSYNC();
  };
  auto middle = [&](const double (&Pc)[PN]) {
    if (lane < NPL) {
      double a = rq[c * NPL + lane];
      if (c >= 1) a += dotA_row(tmp);
      a += (TILE ? wxt[c * NPL + lane] : wx_of(c)) * dotA_col(rq + (c + 1) * NPL);
      tmp2[lane] = (lane < n) ? a : 0.0;
    }
    WSYNC();
    const double dl = matvec(Pc);
    if (wr) { rq[c * NPL + wi] = dl; lam[c * NPL + wi] += dl; }
    WSYNC();
  };
  auto outward = [&]() {
    double Pk[PN];
    if (wv == 0) {
      for (int k = c - 1; k >= 0; --k) {
        load_P(k, Pk);
        if (lane < NPL) {
          double a = 0.0;
          if (lane < n && mask[k * nm + lane]) a = hx[lane] * dotA_col(rq + (k + 1) * NPL);
          tmp2[lane] = a;
        }
        WSYNC();
        const double dl = matvec(Pk) + (wr ? rq[k * NPL + wi] : 0.0);
        if (wr) { rq[k * NPL + wi] = dl; lam[k * NPL + wi] += dl; }
        WSYNC();
      }
    } else if (wv == 1) {
      for (int k = c + 1; k <= T; ++k) {
        load_P(k, Pk);
        // tmp = Wx_{k−1} Δλ_{k−1}.  Three-tile classes: the step before wrote it together with rq[k − 1] (as elim_up does); only
        // the first step, whose predecessor is wave 0's `middle`, forms it here.  Entries 24 … 31 are written by that first step
        // alone (zeros: wxt is 0 beyond ñx) and no dot product reads them.
        if (!TILE || k == c + 1) {
          if (lane < NPL) tmp[lane] = (TILE ? wxt[(k - 1) * NPL + lane] : wx_of(k - 1)) * rq[(k - 1) * NPL + lane];
          WSYNC();
        }
        if (lane < NPL) tmp2[lane] = (lane < n) ? dotA_row(tmp) : 0.0;
        WSYNC();
        const double dl = matvec(Pk) + (wr ? rq[k * NPL + wi] : 0.0);
        if (wr) {
          rq[k * NPL + wi] = dl; lam[k * NPL + wi] += dl;
          if constexpr (TILE) tmp[wi] = wxt[k * NPL + wi] * dl;
        }
        WSYNC();
      }
    }
  };

  // SLS_PHASE_TIMERS = 4 (-DSLS_T4_PHASES=1 builds only): what follows lap(1), per wave — 0 residual passes, 1 inward sweeps of the
  // later passes, 2 middle (wave 1: waiting for it), 3 outward sweeps (stamped BEFORE the barrier: the slower wave shows),
  // 4 output pass, 5 the barriers behind the factor half and behind the sweeps
  unsigned long long p4[6] = {0, 0, 0, 0, 0, 0}, t4last = 0;
  auto stamp4 = [&](int slot) {
    if constexpr (SLS_T4_PHASES != 0) {
      if (p.dbg_level == 4) { const unsigned long long now = __builtin_amdgcn_s_memtime(); p4[slot] += now - t4last; t4last = now; }
    }
  };
  unsigned long long ph[4] = {0, 0, 0, 0};      // diagnostics (SLS_PHASE_TIMERS ≥ 2): chain wave: hand-off waits / Gauss–Jordan / store + sweep; helper: static + border / elimination / of which waiting
  if (resid > p.tol) {
    double M[PN];
    if (helper == 0) {
      // =================== chain wave: Gauss–Jordan + store + fused sweep per block; blocks arrive from the helper ===================
      // the helper hands over the stored half (tiles ri ≤ cj of every lane); the other half is read at the mirror position
      auto receive = [&](double (&Tt)[TT], int s, bool mid) {
        wait_flag(flagB, s);
#pragma unroll
        for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
          for (int cj = 0; cj < TR; ++cj)
            Tt[ri * TR + cj] = (ri <= cj) ? hand[(ta + 8 * ri) * LDT + tb + 8 * cj] : hand[(tb + 8 * cj) * LDT + ta + 8 * ri];
        }
        if (mid) {
          wait_flag(flagB_other, T - c + 1);
#pragma unroll
          for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
            for (int cj = 0; cj < TR; ++cj)
              Tt[ri * TR + cj] += (ri <= cj) ? hand_other[(ta + 8 * ri) * LDT + tb + 8 * cj] : hand_other[(tb + 8 * cj) * LDT + ta + 8 * ri];
          }
        }
      };
      const int s_end = (dir == 0) ? c : T - c;
      if constexpr (TILE) {
        // The sweep step of block k multiplies P_k with  rq[k] + Ã·(Wx_{k−1} q_{k−1})  (downward: rq[k] + Wx_k·Ãᵀ q_{k+1}), which has no
        // P_k in it: it is formed and laid out in tmp2 at the end of the step BEFORE, and this lane's three entries of it (its tile
        // rows) wait in registers through the Gauss–Jordan.  After the last pivot the tiles are used where they are: nine FMAs, the
        // reduction over the lane-grid rows (matvec_tiles), one write — and the nine global stores, which nothing waits for.
        double v[TR];
        auto sweep_input = [&](int kn) {                    // elim_up's / elim_down's first half, for block kn
          if (lane < NPL) {
            double a = rq[kn * NPL + lane];
            if (dir == 0) { if (kn >= 1) a += dotA_row(tmp); }                  // tmp = Wx_{kn−1} q_{kn−1}
            else if (kn < T) a += wxt[kn * NPL + lane] * dotA_col(tmp);          // tmp = q_{kn+1}; the table's wx_of(kn)
            tmp2[lane] = (lane < n) ? a : 0.0;
          }
          WSYNC();
#pragma unroll
          for (int q = 0; q < TR; ++q) v[q] = tmp2[ta + 8 * q];
        };
        auto sweep = [&](int k, double wk) {                // … and their second half; wk = Wx_k[wi]
          const double q = matvec_tiles(M, v[0], v[1], v[2]);
          if (wr) { rq[k * NPL + wi] = q; tmp[wi] = (dir == 0) ? wk * q : q; }
          WSYNC();
        };
        sweep_input((dir == 0) ? 0 : T);                    // the first block of either chain has no predecessor
        if (dir == 0) {
          // block 0 is diagonal (δ + Wx_0): its inverse needs no elimination, and the helper folds it into block 1's weights
#pragma unroll
          for (int ri = 0; ri < TR; ++ri) {
            const int i = ta + 8 * ri;
            const double di = 1.0 / (delta + wxt[i]);       // wxt[i] = Wx_0[i]
#pragma unroll
            for (int cj = 0; cj < TR; ++cj) M[ri * TR + cj] = (i == tb + 8 * cj && i < n) ? di : 0.0;
          }
          store_P(0, M);
          sweep(0, wxt[wi]);
          if (c > 1) sweep_input(1);                        // (block c is the middle block: no fused step)
        }
        for (int s = 1; s <= s_end; ++s) {
          const int k = (dir == 0) ? s : T - s + 1;
          const bool mid = (dir == 0) && (s == c);
          const bool more = (dir == 0) ? (s + 1 < c) : (s < s_end);      // the next block has a fused step
          const double wk = wxt[k * NPL + wi];             // (the table: one read, no mask → weight chain)
          unsigned long long q0 = (SLS_T4_PHASES != 0) ? __builtin_amdgcn_s_memtime() : 0;
          receive(M, s, mid);
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[0] += q1 - q0; q0 = q1; }
          gj_tiles_publish<NP, TR, RS>(M, lane, n, rowbuf, flagA, s * 64);
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { __builtin_amdgcn_sched_barrier(0); asm volatile("" :: "v"(M[0])); const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[1] += q1 - q0; q0 = q1; }
          SLS_ISA_MARK("chain-tail");
          store_P(k, M);
          if (!mid) {
            sweep(k, wk);
            if (more) sweep_input((dir == 0) ? k + 1 : k - 1);
          }
          SLS_ISA_MARK("chain-tail-end");
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[2] += q1 - q0; q0 = q1; }
        }
      } else {
        if (dir == 0) {
          // block 0 is diagonal (δ + Wx_0): its inverse needs no elimination, and the helper folds it into block 1's weights
          const double w0 = wx_of(0);
#pragma unroll
          for (int r = 0; r < RPL; ++r) M[r] = (HS * r + h == j && j < n) ? 1.0 / (delta + w0) : 0.0;
          store_P(0, M);
          elim_up(0, M, w0);
        }
        for (int s = 1; s <= s_end; ++s) {
          const int k = (dir == 0) ? s : T - s + 1;
          const bool mid = (dir == 0) && (s == c);
          unsigned long long q0 = (SLS_T4_PHASES != 0) ? __builtin_amdgcn_s_memtime() : 0;
          double Tt[TT];
          receive(Tt, s, mid);
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[0] += q1 - q0; q0 = q1; }
          gj_tiles_publish<NP, TR, RS>(Tt, lane, n, rowbuf, flagA, s * 64);
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { __builtin_amdgcn_sched_barrier(0); asm volatile("" :: "v"(Tt[0])); const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[1] += q1 - q0; q0 = q1; }
          SLS_ISA_MARK("chain-tail");
          // tiles → column layout (lane (h, j): rows HS·r + h of column j) through the private image
#pragma unroll
          for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
            for (int cj = 0; cj < TR; ++cj) mat[(ta + 8 * ri) * LDT + tb + 8 * cj] = Tt[ri * TR + cj];
          }
          WSYNC();
#pragma unroll
          for (int r = 0; r < RPL; ++r) M[r] = mat[(HS * r + h) * LDT + j];
          WSYNC();
          store_P(k, M);
          if (!mid) { if (dir == 0) elim_up(k, M, wx_of(k)); else elim_down(k, M, wx_of(k)); }
          SLS_ISA_MARK("chain-tail-end");
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[2] += q1 - q0; q0 = q1; }
        }
      }
    } else {
      // =================== helper wave: static part S_k, border X, elimination behind the chain wave's pivots ===================
      // row lists of Ã and B̃ for this lane's tile rows a + 8·ri: first KH / KB entries in registers for the whole column
      // (rebuild instantiation only: with plan-time blocks the helper reads no list at all)
      constexpr int KH = 4, KB = 2, TQ = TR * (TR + 1) / 2;
      int hac[TR][KH], hbc[TR][KB];
      double hav[TR][KH], hbv[TR][KB];
#pragma unroll
      for (int ri = 0; ri < TR && !PRE; ++ri) {
        const int i = ta + 8 * ri;
#pragma unroll
        for (int e = 0; e < KH; ++e) { const bool ok = e < capA; hac[ri][e] = ok ? arow_c[e * NPL + i] : 0; hav[ri][e] = ok ? arow_v[e * NPL + i] : 0.0; }
#pragma unroll
        for (int e = 0; e < KB; ++e) { const bool ok = e < capB; hbc[ri][e] = ok ? brow_c[e * NPL + i] : 0; hbv[ri][e] = ok ? brow_v[e * NPL + i] : 0.0; }
      }
      // The three-tile classes also keep, for the whole column, what the static build gathers through those lists — Ã[b + 8·cj, hac]
      // and B̃[b + 8·cj, hbc] for the stored half cj ≥ ri — and the nine Ã values of this direction's border: addresses and values
      // do not depend on the block, only the weights do.  A rebuild is then weight reads + FMAs, no dependent LDS address chain.
      // The four-tile classes have no registers to spare (they spill already) and gather from LDS per block as before.
      constexpr bool HOIST = (TR == 3);
      double GA[KH][TR][TR], GB[KB][TR][TR], XA[TT];
      if constexpr (HOIST) {
#pragma unroll
        for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
          for (int cj = ri; cj < TR; ++cj) {
            if constexpr (!PRE) {
#pragma unroll
              for (int e = 0; e < KH; ++e) GA[e][ri][cj] = Ad[(tb + 8 * cj) * LDT + hac[ri][e]];
#pragma unroll
              for (int e = 0; e < KB; ++e) GB[e][ri][cj] = Bd[(tb + 8 * cj) * MC + hbc[ri][e]];
            }
          }
#pragma unroll
          for (int cj = 0; cj < TR; ++cj) {
            const int i = ta + 8 * ri, l = tb + 8 * cj;
            XA[ri * TR + cj] = (dir == 0) ? Ad[i * LDT + l] : Ad[l * LDT + i];
          }
        }
      }
      // which blocks can reuse the previous step's static part: masks of (k, k−1) equal those of the block produced before
      // (upward: k−1; downward: k+1 — never block T, whose Wx is 0): one bit per block, from the prepared record
      const unsigned long long samebits = (SLS_T4_SAME != 0) ? samew[dir] : 0ull;
      double Sc[TT];                         // cached static part (stored half) while the masks repeat
      bool have_S = false;
      const int s_end = (dir == 0) ? c : T - c + 1;
      auto load_border = [&](int k, double (&Xn)[TT]) {     // X of block k: upward Ã·Wx_{k−1}, downward Wx_k·Ãᵀ
        const double* wrow = wxt + ((dir == 0) ? k - 1 : k) * NPL;
        if constexpr (HOIST) {                              // three weights of this lane's tile columns (rows), nine multiplies
          double wr[TR];
#pragma unroll
          for (int q = 0; q < TR; ++q) wr[q] = wrow[((dir == 0) ? tb : ta) + 8 * q];
#pragma unroll
          for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
            for (int cj = 0; cj < TR; ++cj) Xn[ri * TR + cj] = (dir == 0) ? XA[ri * TR + cj] * wr[cj] : wr[ri] * XA[ri * TR + cj];
          }
        } else {
#pragma unroll
          for (int ri = 0; ri < TR; ++ri) {
            const int i = ta + 8 * ri;
#pragma unroll
            for (int cj = 0; cj < TR; ++cj) {
              const int l = tb + 8 * cj;
              Xn[ri * TR + cj] = (dir == 0) ? Ad[i * LDT + l] * wrow[l] : wrow[i] * Ad[l * LDT + i];
            }
          }
        }
      };
      double Xn[TT];
      if (s_end >= 2) load_border((dir == 0) ? 2 : T - 1, Xn);
      if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { __builtin_amdgcn_sched_barrier(0); ph[3] = __builtin_amdgcn_s_memtime() - tlast; }   // pre-loop: lap(0) → first block
      // What step s starts from: 0 = zeros (the downward helper's share of the middle block), 1 = the cached static part of the
      // step before (masks repeat), 2 = a fresh static part — rebuilt here, or read from the column's plan-time pool
      // (twisted4_slot_read states the same rule per slot).  `have`: a cached part exists (any fresh block but the upward first).
      auto step_kind = [&](int s, bool have) -> int {
        const int k = (dir == 0) ? s : T - s + 1;
        if (dir == 1 && k == c) return 0;
        return (have && k < 64 && ((samebits >> k) & 1ull) && !(dir == 0 && s == 2)) ? 1 : 2;
      };
      // Plan-time blocks: the step that needs a fresh block loads this lane's TQ doubles of it and waits for them — one memory
      // latency (≈ 1.7 k cycles) where the rebuild took 2.8 k.  Loading a step ahead, behind the previous block's elimination,
      // hides that latency too and was measured SLOWER: a helper that is never late runs in lock step
      // with its chain wave, whose Gauss–Jordan then loses more than the hand-off waits gain.
      auto load_slot = [&](int s, double (&Sl)[TQ]) {
        const int slot = (dir == 0 && s == 1) ? 0 : ((dir == 0) ? s : T - s + 1);
        const double* src = spool + (int64_t)slot * (TQ * 64) + lane;
#pragma unroll
        for (int q = 0; q < TQ; ++q) Sl[q] = src[q * 64];
      };
      auto hand_over = [&](const double (&Sw)[TT], int s) {
#pragma unroll
        for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
          for (int cj = ri; cj < TR; ++cj) hand[(ta + 8 * ri) * LDT + tb + 8 * cj] = Sw[ri * TR + cj];
        }
        if (lane == 0) flag_store(flagB, s);
        WSYNC();
      };
      for (int s = 1; s <= s_end; ++s) {
        unsigned long long q0 = (SLS_T4_PHASES != 0) ? __builtin_amdgcn_s_memtime() : 0;
        const int k = (dir == 0) ? s : T - s + 1;           // block being produced (downward helper's last step: k = c, the middle)
        const int kind = step_kind(s, have_S);
        const bool fold0 = (dir == 0) && (s == 1);           // upward, block 1: P_0 = (δ + Wx_0)⁻¹ is diagonal, W − W P_0 W = δ·w/(δ + w) takes the place of Wx_0
        double Sw[TT];
        if (kind == 0) {
#pragma unroll
          for (int q = 0; q < TT; ++q) Sw[q] = 0.0;
        } else if (kind == 1) {
#pragma unroll
          for (int q = 0; q < TT; ++q) Sw[q] = Sc[q];
        } else {
          if constexpr (PRE) {
            double Sl[TQ];
            if (s == 1) {                                    // requested in the setup
#pragma unroll
              for (int q = 0; q < TQ; ++q) Sl[q] = Sl0[q];
            } else {
              load_slot(s, Sl);
            }
            int q = 0;
#pragma unroll
            for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
              for (int cj = 0; cj < TR; ++cj) Sw[ri * TR + cj] = (ri <= cj) ? Sl[q++] : 0.0;      // the half below is never read
            }
          } else {
            twisted4_static_block<TR, HOIST, KH, KB, NPL, LDT>(Sw, delta, wxt + k * NPL, wxt + (k - 1) * NPL, wut + (k - 1) * MC, fold0,
                                                               ta, tb, nzA, nzB, MC, hac, hav, hbc, hbv, GA, GB,
                                                               arow_c, arow_v, brow_c, brow_v, Ad, Bd);
          }
          if (!fold0) {
#pragma unroll
            for (int q = 0; q < TT; ++q) Sc[q] = Sw[q];
            have_S = true;
          }
        }
        if (s >= 2) {
          double Xw[TT];
#pragma unroll
          for (int q = 0; q < TT; ++q) Xw[q] = Xn[q];
          if (s + 1 <= s_end) load_border((dir == 0) ? s + 1 : T - s, Xn);      // next step's border: its loads fly during this elimination
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[0] += q1 - q0; q0 = q1; }
          if (SLS_T4_EXP != 1) helper_eliminate<NP, TR, RS>(Xw, Sw, lane, n, rowbuf, flagA, (s - 1) * 64, xbuf, ph[2]);
          if (SLS_T4_PHASES != 0 && p.dbg_level >= 2) { __builtin_amdgcn_sched_barrier(0); asm volatile("" :: "v"(Sw[0])); const unsigned long long q1 = __builtin_amdgcn_s_memtime(); ph[1] += q1 - q0; q0 = q1; }
        }
        hand_over(Sw, s);
      }
    }
    lap(1);                        // own half of the factorisation
    if constexpr (SLS_T4_PHASES != 0) t4last = tlast;
    __syncthreads();
    lap(2);                        // waiting for the other waves
    stamp4(5);
    if (wv == 0) middle(M);        // M = P_c
    __syncthreads();
    stamp4(2);
    outward();
    stamp4(3);
    __syncthreads();
    stamp4(5);
    lap(3);

    // ---------------- multiplier iteration ----------------
    double prev = resid, prev2 = resid;
    int itmax = p.max_iters;
    for (int it = 1; it <= itmax; ++it) {
      iters = it;
      if (it > 1) {
        double Pk[PN];
        if (wv == 0) {
          for (int k = 0; k < c; ++k) { load_P(k, Pk); elim_up(k, Pk, wk_arg(k)); }
        } else if (wv == 1) {
          for (int k = T; k > c; --k) { load_P(k, Pk); elim_down(k, Pk, wk_arg(k)); }
        }
        stamp4(1);
        __syncthreads();
        stamp4(5);
        if (wv == 0) { load_P(c, Pk); middle(Pk); }
        __syncthreads();
        stamp4(2);
        outward();
        stamp4(3);
        __syncthreads();
        stamp4(5);
      }
      resid = residual_pass();
      stamp4(0);
      if (resid <= p.tol) break;
      if (it >= 2 && resid > p.stag * prev) {          // (still_contracting: sls_device.h)
        if (!(p.max_iters_slow > 0 && (resid > p.tol_ok || itmax > p.max_iters) && still_contracting(it >= 3 ? prev2 : prev, prev, resid))) { status = 1; break; }
        itmax = max(itmax, p.max_iters_slow);
      }
      prev2 = prev; prev = resid;
    }
    if (resid <= p.tol_ok) status = 0;
    else if (status == 0) status = 2;
  }
  if constexpr (SLS_T4_PHASES != 0) { if (t4last == 0) t4last = __builtin_amdgcn_s_memtime(); }      // (a column that needed no pass)
  output_pass();
  stamp4(4);
  if (p.dbg && lane == 0) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    if (p.dbg_level <= 1 && wv < 2) {
      for (int q = 0; q < 3; ++q) p.dbg[sd.out_index * 8 + wv * 4 + q] = tc[q];
      p.dbg[sd.out_index * 8 + wv * 4 + 3] = (tc[3] << 32) | ((now - tlast) & 0xffffffffull);
    } else if ((p.dbg_level == 2 && wv < 2) || (p.dbg_level == 3 && wv >= 2)) {       // 2: chain waves' shares, 3: helper waves'
      for (int q = 0; q < 3; ++q) p.dbg[sd.out_index * 8 + dir * 4 + q] = ph[q];
      p.dbg[sd.out_index * 8 + dir * 4 + 3] = tc[1];
      if (SLS_T4_PHASES != 0 && p.dbg_level == 3) {       // helper waves: + the setup lap and the pre-loop stamp in the high halves (tools/t4_phases.py)
        p.dbg[sd.out_index * 8 + dir * 4 + 2] = (ph[2] & 0xffffffffull) | (tc[0] << 32);
        p.dbg[sd.out_index * 8 + dir * 4 + 3] = (tc[1] & 0xffffffffull) | (ph[3] << 32);
      }
    } else if (SLS_T4_PHASES != 0 && p.dbg_level == 4 && wv < 2) {       // 4: the chain waves' time after the factor half, two shares per slot
      for (int q = 0; q < 3; ++q) p.dbg[sd.out_index * 8 + wv * 4 + q] = (p4[2 * q] & 0xffffffffull) | (p4[2 * q + 1] << 32);
      p.dbg[sd.out_index * 8 + wv * 4 + 3] = tc[1];
    }
  }
  if (sd.pos < 0 && status == 0) status = 3;
  if (threadIdx.x == 0) {
    p.status[sd.out_index] = status;
    p.resid[sd.out_index] = resid;
    p.iters[sd.out_index] = iters;
  }
}

// PRE: the helpers read the static blocks from the plan's pool (p.t4_static); otherwise they rebuild them in the launch.  A
// template flag, not a branch: the rebuild's gather registers must not stay live in the instantiation that never rebuilds.
template <int NPL, int RPL, bool PRE>
__global__ __launch_bounds__(256, 1) void h2_column_twisted4_kernel(const KernelParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double* fac = p.fac_ws + (int64_t)blockIdx.x * p.fac_stride;
  for (int s = blockIdx.x; s < p.nsub; s += gridDim.x) {
    const SubDesc sd = p.subs[p.order[p.order_off + s]];
    const int rs = p.t4_pos ? p.t4_pos[s] : s;      // a selected run: the record (and the pool) of the column's place in the full launch
    const double* spool = PRE ? p.t4_static + (int64_t)rs * p.t4_static_stride : nullptr;
    const double* images = PRE ? p.t4_images + (int64_t)rs * p.t4_images_stride : nullptr;
    twisted4_solve_column<NPL, RPL, PRE>(p, sd, p.t4_rec + (int64_t)rs * p.t4_stride, spool, images, fac, lds_raw);
  }
}

// Plan time, once: the symbolic part of a four-wave column's setup — everything that depends only on what a plan fixes (index
// sets, masks, the plan's own copy of A / B2).  One wave per column of the launch, record s ↔ order[order_off + s]; layout:
// sls_device.h (twisted4_record_bytes).  The lists follow CSR order, skip entries outside the index set and stored zeros, and
// are never cut: the capacities are the structural row maxima.  Every lane writes its own column of every list, padding
// included, so the record needs no clear.
// With a pool (p.t4_static, TR = the class's tile rows; TR = 0: none) the kernel then builds what else a launch would rebuild from
// the same inputs every time: δ (into the record's tail) and the static blocks S_k the helpers read (twisted4_slot_read), in the
// helper's register layout (sls_device.h: twisted4_static_doubles), with the launch's own arithmetic (twisted4_static_block).
// Wave 0 does the symbolic part while waves 1 … 3 lay out weights and weight tables; the slots are dealt round over the four waves.
template <int TR>
__global__ __launch_bounds__(256) void twisted4_prepare_kernel(const KernelParams p, unsigned char* __restrict__ pool) {
  constexpr int NPL = 32;
  constexpr int LDT = 40, NR = TR > 0 ? 8 * TR : 8, TT = TR > 0 ? TR * TR : 1, TQ = TR * (TR + 1) / 2;
  __shared__ int32_t sx[NPL];
  __shared__ int32_t su[64];
  __shared__ unsigned long long sbits[2];
  __shared__ int32_t snz[4];
  __shared__ double sdelta;
  extern __shared__ __attribute__((aligned(16))) unsigned char prep_lds[];
  const int wv = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const SubDesc sd = p.subs[p.order[p.order_off + blockIdx.x]];
  const int n = sd.n, m = sd.m, nm = n + m, T = p.T;
  const int MC = p.w_mcap;
  const int capA = p.w_nzA, capAc = p.w_nzAc, capB = p.w_nzB, capBc = p.w_nzBc;
  unsigned char* rec = pool + (int64_t)blockIdx.x * p.t4_stride;
  double* arow_v = reinterpret_cast<double*>(rec + kT4RecHeader);
  double* acol_v = arow_v + capA * NPL;
  double* brow_v = acol_v + capAc * NPL;
  double* bcol_v = brow_v + capB * NPL;
  int32_t* arow_c = reinterpret_cast<int32_t*>(bcol_v + capBc * 64);
  int32_t* acol_c = arow_c + capA * NPL;
  int32_t* brow_c = acol_c + capAc * NPL;
  int32_t* bcol_c = brow_c + capB * NPL;
  const uint8_t* mask = p.mask_pool + sd.off_mask;
  // dynamic LDS (twisted4_prepare_lds_bytes; only with a pool): the images the static build reads, as the launch lays them out
  double* Ad = reinterpret_cast<double*>(prep_lds);
  double* Bd = Ad + NR * LDT;
  double* wxt = Bd + NPL * MC;
  double* wut = wxt + (T + 1) * NPL;
  double* hx = wut + T * MC;
  double* hu = hx + NPL;
  if (wv == 0) {
    if (lane < NPL) sx[lane] = (lane < n) ? p.idx_pool[sd.off_sx + lane] : 0x7fffffff;
    su[lane] = (lane < m) ? p.idx_pool[sd.off_su + lane] : 0x7fffffff;
    WSYNC();
    int cntA = 0, cntB = 0, cntAc = 0, cntBc = 0;
    if (lane < n) {
      const int g = sx[lane];
      cntA = gather_list(p.A_rowptr, p.A_colidx, p.A_val, g, sx, n, capA, NPL, lane, arow_c, arow_v);
      cntB = gather_list(p.B_rowptr, p.B_colidx, p.B_val, g, su, m, capB, NPL, lane, brow_c, brow_v);
      cntAc = gather_list(p.At_rowptr, p.At_colidx, p.At_val, g, sx, n, capAc, NPL, lane, acol_c, acol_v);
    }
    if (lane < m) cntBc = gather_list(p.Bt_rowptr, p.Bt_colidx, p.Bt_val, su[lane], sx, n, capBc, 64, lane, bcol_c, bcol_v);
    if (lane < NPL) {
      for (int e = cntA; e < capA; ++e) { arow_c[e * NPL + lane] = 0; arow_v[e * NPL + lane] = 0.0; }
      for (int e = cntB; e < capB; ++e) { brow_c[e * NPL + lane] = 0; brow_v[e * NPL + lane] = 0.0; }
      for (int e = cntAc; e < capAc; ++e) { acol_c[e * NPL + lane] = 0; acol_v[e * NPL + lane] = 0.0; }
    }
    for (int e = cntBc; e < capBc; ++e) { bcol_c[e * 64 + lane] = 0; bcol_v[e * 64 + lane] = 0.0; }
    const int a0 = wave_max_i32(cntA), a1 = wave_max_i32(cntAc), a2 = wave_max_i32(cntB), a3 = wave_max_i32(cntBc);
    // mask-repeat bits: block k (2 ≤ k ≤ T−1, k < 64) may reuse the static part of the block produced before it — ko = k−1 upward,
    // k+1 downward, ko ≤ T−1 — when the masks of (k, k−1) equal those of (ko, ko−1) on all n + m rows.  Every lane walks its rows
    // down the time steps once (independent loads): d1 bit k = steps k and k−1 agree, d2 bit k = steps k+1 and k agree (bit 0 of
    // either word is scratch); then upward = d1[k] ∧ d1[k−1], downward = d2[k] ∧ d1[k].
    unsigned long long d1 = ~0ull, d2 = ~0ull;
    const int klast = min(T - 1, 64);
    for (int r = lane; r < nm; r += 64) {
      uint8_t prev = mask[r];
#pragma unroll 8
      for (int k = 1; k <= klast; ++k) {
        const uint8_t cur = mask[k * nm + r];
        const unsigned long long ne = (cur != prev) ? 1ull : 0ull;
        d1 &= ~(ne << (k & 63));
        d2 &= ~(ne << (k - 1));
        prev = cur;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { d1 &= __shfl_xor(d1, off); d2 &= __shfl_xor(d2, off); }
    auto bit_range = [](int lo, int hi) -> unsigned long long {            // bits lo … hi, hi ≤ 63
      return hi < lo ? 0ull : ((hi >= 63 ? ~0ull : ((1ull << (hi + 1)) - 1)) & ~((1ull << lo) - 1));
    };
    unsigned long long bits[2];
    bits[0] = d1 & (d1 << 1) & bit_range(2, min(T - 1, 63));
    bits[1] = d2 & d1 & bit_range(2, min(T - 2, 63));
    if (lane == 0) {
      reinterpret_cast<unsigned long long*>(rec)[0] = bits[0];
      reinterpret_cast<unsigned long long*>(rec)[1] = bits[1];
      int32_t* cnt = reinterpret_cast<int32_t*>(rec + 16);
      cnt[0] = a0; cnt[1] = a1; cnt[2] = a2; cnt[3] = a3;
      sbits[0] = bits[0]; sbits[1] = bits[1];
      snz[0] = a0; snz[1] = a1; snz[2] = a2; snz[3] = a3;
    }
  } else if constexpr (TR > 0) {
    // weights and weight tables exactly as the launch's setup makes them; the dense images start from zero
    if (wv == 1) {
      if (lane < NPL) hx[lane] = (lane < n) ? (sd.has_w ? p.w_pool[sd.off_w + lane] : 1.0) : 0.0;
      hu[lane] = (lane < m) ? (sd.has_w ? p.w_pool[sd.off_w + n + lane] : 1.0) : 0.0;
      WSYNC();
      for (int i = lane; i < (T + 1) * NPL; i += 64) {
        const int k = i / NPL, jj = i % NPL;
        wxt[i] = (k < T && jj < n && mask[k * nm + jj]) ? hx[jj] : 0.0;
      }
      for (int i = lane; i < T * MC; i += 64) {
        const int k = i / MC, q = i % MC;
        wut[i] = (q < m && mask[k * nm + n + q]) ? hu[q] : 0.0;
      }
    } else if (wv == 2) {
      for (int i = lane; i < NR * LDT; i += 64) Ad[i] = 0.0;
    } else {
      for (int i = lane; i < NPL * MC; i += 64) Bd[i] = 0.0;
    }
  }
  if constexpr (TR > 0) {
    __syncthreads();              // the record (written by wave 0) is read back below by all four waves
    const int nzA = snz[0], nzB = snz[2];
    if (wv == 0) {
      // δ: the launch's reduction, operation for operation (rebuild instantiation, setup)
      const double dl_ = p.delta_rel * wave_max_f64(tikhonov_scale<NPL>(lane, n, hx, hu, arow_c, arow_v, nzA, brow_c, brow_v, nzB));
      if (lane == 0) { sdelta = dl_; *reinterpret_cast<double*>(rec + twisted4_record_tail(capA, capAc, capB, capBc)) = dl_; }
    } else if (wv == 1) {
      if (lane < n) {
        for (int e = 0; e < nzB; ++e) {
          const double v = brow_v[e * NPL + lane];
          if (v != 0.0) Bd[lane * MC + brow_c[e * NPL + lane]] = v;
        }
      }
    } else if (wv == 2) {
      if (lane < n) {
        for (int e = 0; e < nzA; ++e) {
          const double v = arow_v[e * NPL + lane];
          if (v != 0.0) Ad[lane * LDT + arow_c[e * NPL + lane]] += v;
        }
      }
    }
    __syncthreads();
    // the two images a launch would build the same way (Ã: zero fill, then `+=` in list order; Wx: mask ⊙ H⁻¹), as they stand here
    if (p.t4_images) {
      double* img = p.t4_images + (int64_t)blockIdx.x * p.t4_images_stride;
      constexpr int NAD = NR * LDT;
      for (int i = threadIdx.x; i < NAD; i += 256) img[i] = Ad[i];
      for (int i = threadIdx.x; i < (T + 1) * NPL; i += 256) img[NAD + i] = wxt[i];
    }
    const double delta = sdelta;
    const int c = twisted4_middle(T);
    const unsigned long long up = (SLS_T4_SAME != 0) ? sbits[0] : 0ull, down = (SLS_T4_SAME != 0) ? sbits[1] : 0ull;
    uint8_t* valid = rec + twisted4_record_tail(capA, capAc, capB, capBc) + 8;
    for (int k = threadIdx.x; k <= T; k += 256) valid[k] = twisted4_slot_read(k, T, c, up, down) ? 1 : 0;
    // this lane's rows of the lists, as the helper holds them
    constexpr int KH = 4, KB = 2;
    const int ta = lane >> 3, tb = lane & 7;
    int hac[TR][KH], hbc[TR][KB];
    double hav[TR][KH], hbv[TR][KB];
#pragma unroll
    for (int ri = 0; ri < TR; ++ri) {
      const int i = ta + 8 * ri;
#pragma unroll
      for (int e = 0; e < KH; ++e) { const bool ok = e < capA; hac[ri][e] = ok ? arow_c[e * NPL + i] : 0; hav[ri][e] = ok ? arow_v[e * NPL + i] : 0.0; }
#pragma unroll
      for (int e = 0; e < KB; ++e) { const bool ok = e < capB; hbc[ri][e] = ok ? brow_c[e * NPL + i] : 0; hbv[ri][e] = ok ? brow_v[e * NPL + i] : 0.0; }
    }
    const double GA[KH][TR][TR] = {}, GB[KB][TR][TR] = {};      // (not read: the gathers come from the LDS images)
    double* col = p.t4_static + (int64_t)blockIdx.x * p.t4_static_stride;
    int turn = 0;
    for (int slot = 0; slot <= T; ++slot) {
      if (!twisted4_slot_read(slot, T, c, up, down)) continue;
      if ((turn++ & 3) != wv) continue;
      const int k = slot == 0 ? 1 : slot;
      double Sw[TT];
      twisted4_static_block<TR, false, KH, KB, NPL, LDT>(Sw, delta, wxt + k * NPL, wxt + (k - 1) * NPL, wut + (k - 1) * MC, slot == 0,
                                                         ta, tb, nzA, nzB, MC, hac, hav, hbc, hbv, GA, GB,
                                                         arow_c, arow_v, brow_c, brow_v, Ad, Bd);
      double* dst = col + (int64_t)slot * (TQ * 64) + lane;
      int q = 0;
#pragma unroll
      for (int ri = 0; ri < TR; ++ri) {
#pragma unroll
        for (int cj = ri; cj < TR; ++cj) dst[64 * q++] = Sw[ri * TR + cj];
      }
    }
  }
}

// dynamic LDS of twisted4_prepare_kernel<TR> with a pool: Ã and B̃ images, the two weight tables, hx, hu (less than the solve kernel's)
static inline size_t twisted4_prepare_lds_bytes(int TR, int T, int mcap) {
  return sizeof(double) * ((size_t)8 * TR * 40 + (size_t)32 * mcap + (size_t)(T + 1) * 32 + (size_t)T * mcap + 32 + 64);
}

template <int TR>
static hipError_t launch_one_twisted4_prepare(const KernelParams& p, unsigned char* pool, size_t lds, hipStream_t st) {
  if (lds > 32768) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&twisted4_prepare_kernel<TR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((twisted4_prepare_kernel<TR>), dim3(p.nsub), dim3(TR > 0 ? 256 : 64), lds, st, p, pool);
  return hipGetLastError();
}

// cls: the launch's size class (2 … 5); p.t4_static / p.t4_static_stride: the launch's part of the pool, or NULL for none
hipError_t launch_twisted4_prepare(int cls, const KernelParams& p, unsigned char* pool, hipStream_t st) {
  if (p.nsub <= 0) return hipSuccess;
  if (p.t4_static == nullptr) return launch_one_twisted4_prepare<0>(p, pool, 0, st);      // one wave: the symbolic part alone
  const int TR = twisted4_tile_rows(cls);
  const size_t lds = twisted4_prepare_lds_bytes(TR, p.T, p.w_mcap);
  return TR == 3 ? launch_one_twisted4_prepare<3>(p, pool, lds, st) : launch_one_twisted4_prepare<4>(p, pool, lds, st);
}

template <int NPL, int RPL>
static hipError_t launch_one_twisted4(const KernelParams& p, int grid, size_t lds, hipStream_t st, const LaunchEvents* ev) {
  if (p.t4_static == nullptr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&h2_column_twisted4_kernel<NPL, RPL, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (ev) hipExtLaunchKernelGGL((h2_column_twisted4_kernel<NPL, RPL, false>), dim3(grid), dim3(256), (uint32_t)lds, st, ev->start, ev->stop, 0, p);
    else hipLaunchKernelGGL((h2_column_twisted4_kernel<NPL, RPL, false>), dim3(grid), dim3(256), lds, st, p);
    return hipGetLastError();
  }
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&h2_column_twisted4_kernel<NPL, RPL, true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if (ev) hipExtLaunchKernelGGL((h2_column_twisted4_kernel<NPL, RPL, true>), dim3(grid), dim3(256), (uint32_t)lds, st, ev->start, ev->stop, 0, p);
  else hipLaunchKernelGGL((h2_column_twisted4_kernel<NPL, RPL, true>), dim3(grid), dim3(256), lds, st, p);
  return hipGetLastError();
}

hipError_t launch_twisted4(int cls, const KernelParams& p, int grid, size_t lds, hipStream_t st, const LaunchEvents* ev) {
  switch (cls) {
    case 2: return launch_one_twisted4<32, 10>(p, grid, lds, st, ev);
    case 3: return launch_one_twisted4<32, 12>(p, grid, lds, st, ev);
    case 4: return launch_one_twisted4<32, 14>(p, grid, lds, st, ev);
    case 5: return launch_one_twisted4<32, 16>(p, grid, lds, st, ev);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace sls
