// =============================================================================
// dq_rules.h -- the rules every output depends on, each stated once for the
// kernels, the host engine and a plain C++ test program.
//
// Part 1: the reference's arithmetic rules (DivQuantCluster.cpp): the cut of a
// cluster (:388-403), the split pass's integer threshold (:473), the FP64
// 2-means decision (:616-623), the proof that the first 2-means iteration is
// a fixed point, and the child boxes that proof allows.
// Part 2: the GPU design's record tiling, which the host and plan_kernel must
// agree on to the last tile.
//
// NOT here, on purpose: the mean / variance / TSE epilogues.  node_results
// and means_from_sums (dq_kernels.hip) scale the integer sums by data_weight;
// the weighted paths (dq_weighted.hip, dq_wsmall.hip) fold already weighted
// summands and scale nothing.  They are different operations and stay apart.
//
// Every translation unit is built with -ffp-contract=off: the expressions
// below must round like the reference's separate multiplies and adds.
// oracle/dq_oracle.cpp keeps its own statement of every rule (the tests
// compare against it) and does not include this header.
// Pinned on the CPU by tests/test_rules.py (tests/native/rules_check.cpp).
// =============================================================================
#pragma once
#include <math.h>

#include <cstdint>

#include "stl_order.h"   // DQ_HD

#if defined(DQ_CHECK)    // the engine's (dq_engine.h, included first)
#define DQ_RULES_PRE(cond) DQ_CHECK(cond, "dq_rules.h precondition")
#else
#include <cassert>
#define DQ_RULES_PRE(cond) assert(cond)
#endif

namespace dq {

// ---------------------------------------------------------------------------
// Part 1: arithmetic rules

// Split-pass threshold (:473): cut < v  <=>  v >= thr for integer v in [0, 255].
DQ_HD inline int32_t split_threshold(double cut) {
  if (!(cut == cut)) return 256;     // NaN: nothing moves
  if (cut < 0.0) return 0;
  if (cut >= 255.0) return 256;
  return (int32_t)floor(cut) + 1;
}

// The cut of a cluster (:388-403): the axis of the largest variance and the
// mean on it; on a tie or a NaN the earlier axis wins (comparisons and copies
// only).  The split pass's shift is 16 - 8 * axis.  Scalars, so that a caller
// holding the channels in registers (plan_child) indexes no array.
struct Cut {
  int axis;
  double pos;
};
DQ_HD inline Cut choose_cut(double m0, double m1, double m2, double v0, double v1, double v2) {
  double maxv = v0, cut = m0;
  int axis = 0;
  if (maxv < v1) { maxv = v1; axis = 1; cut = m1; }
  if (maxv < v2) { axis = 2; cut = m2; }
  return Cut{axis, cut};
}
DQ_HD inline Cut choose_cut(const double mean[3], const double var[3]) {
  return choose_cut(mean[0], mean[1], mean[2], var[0], var[1], var[2]);
}

// The 2-means decision from the halves' means (:616-623): a point stays old
// iff lhs < rr*R + rg*G + rb*B (:683).
struct Decision {
  double lhs, rr, rg, rb;
};
DQ_HD inline Decision decision_from_means(const double om[3], const double nm[3]) {
  Decision d;
  d.lhs = 0.5 * (om[0] * om[0] - nm[0] * nm[0] + om[1] * om[1] - nm[1] * nm[1] +
                 om[2] * om[2] - nm[2] * nm[2]);
  d.rr = om[0] - nm[0];
  d.rg = om[1] - nm[1];
  d.rb = om[2] - nm[2];
  return d;
}
// A bound on every term of the decision over the colour cube: the FP64
// evaluation's error is below 4 * 2^-53 * M.
DQ_HD inline double decision_scale(double lhs, double rr, double rg, double rb) {
  return (fabs(rr) + fabs(rg) + fabs(rb)) * 255.0 + fabs(lhs);
}

// A child's box on the cut's axis when the parent's halves are proven to be
// the cut's (v_axis < thr old | >= thr new).
DQ_HD inline int32_t clip_old_hi(int32_t hi, int32_t thr) { return hi < thr - 1 ? hi : thr - 1; }
DQ_HD inline int32_t clip_new_lo(int32_t lo, int32_t thr) { return lo > thr ? lo : thr; }

// Is the first 2-means iteration after the split a fixed point, for every
// point the node's box [box_lo, box_hi] can hold?  (lhs, rr, rg, rb) is that
// iteration's decision, the split sent v_axis >= thr new (:438-559).  The
// decision is checked at the corners of both halves of the cut: every point
// with v_axis >= thr must go new (max of the linear form <= lhs - margin) and
// every other point must stay old (min >= lhs + margin).  The margin 1e-12*M
// dwarfs the FP64 evaluation's error (decision_scale), so each point's exact
// outcome equals the cut's.  Then the iteration's halves -- hence its exact
// sums -- are the split's, the next decision is the same again, and the
// results are what the first 2-means epilogue would publish as a fixed point.
// A non-finite or tiny M (NaN / inf means of an empty half) proves nothing.
DQ_HD inline bool cut_is_fixed_point(const int32_t box_lo[3], const int32_t box_hi[3], int axis,
                                     int32_t thr, double lhs, double rr, double rg, double rb) {
  const double M = decision_scale(lhs, rr, rg, rb);
  if (!(M > 1e-30 && M < 1e30)) return false;
  const double mg = 1e-12 * M;
  const double c[3] = {rr, rg, rb};
  for (int side = 0; side < 2; ++side) {   // 0: the cut's old half, 1: its new half
    int32_t lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = box_lo[k]; hi[k] = box_hi[k]; }
    if (side) lo[axis] = clip_new_lo(lo[axis], thr);
    else hi[axis] = clip_old_hi(hi[axis], thr);
    if (lo[axis] > hi[axis]) continue;   // the box holds no point of this half
    double ext = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double a = c[k] * (double)lo[k], b = c[k] * (double)hi[k];
      ext += side ? fmax(a, b) : fmin(a, b);
    }
    if (side ? !(ext <= lhs - mg) : !(ext >= lhs + mg)) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------
// Part 2: record tiling.  A record of `len` points of a round with tile length
// tl gets tiles of roundup_4096(ceil(len / nt)) points clamped to [4096, tl]:
// whole 4096-point sweeps, at least nt (node_tiles) tiles per record while
// they last, and one empty tile for an empty record.  Stated on
// L = ceil(len / 4096) < 2^20 sweeps -- nested ceilings:
// ceil(ceil(len / nt) / 4096) = ceil(L / nt).  tl is a whole number of sweeps
// (Engine::round_tile_len, tile_max), 1 <= nt <= 65536 (Engine::apply_tune).
constexpr uint32_t kTileSweep = 4096;

// Exact a / b for a < 2^22, b >= 1.  On the device a float reciprocal (error
// < 0.75 on the quotient) and one correction each way: a generic 32-bit
// division is ~4x the code; the sharded plan inlines 30+ of them and outgrew
// the I-cache.  On the host a plain division under the same precondition.
DQ_HD inline uint32_t small_udiv(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t q = (uint32_t)((float)a * __builtin_amdgcn_rcpf((float)b));
  int32_t r = (int32_t)(a - q * b);
  if (r < 0) { q -= 1u; r += (int32_t)b; }
  if ((uint32_t)r >= b) q += 1u;
  return q;
#else
  DQ_RULES_PRE(a < (1u << 22) && b >= 1u);
  return a / b;
#endif
}

DQ_HD inline uint32_t tile_sweeps_of(uint32_t len, uint32_t tl, uint32_t nt) {
  const uint32_t L = (len >> 12) + ((len & (kTileSweep - 1)) != 0 ? 1u : 0u);
  const uint32_t m = small_udiv(L + nt - 1u, nt);
  const uint32_t cap = tl / kTileSweep;
  const uint32_t c = cap < m ? cap : m;
  return c > 1u ? c : 1u;
}

// Tile length of a record, in points.
DQ_HD inline uint32_t tile_len_of(uint32_t len, uint32_t tl, uint32_t nt) {
  return tile_sweeps_of(len, tl, nt) * kTileSweep;
}

// Tiles of a record: ceil(len / tile length) = ceil(L / m) (nested ceilings
// again); an empty record still gets one (empty) tile.
DQ_HD inline uint32_t ntiles_of(uint32_t len, uint32_t tl, uint32_t nt) {
  if (len == 0) return 1;
  const uint32_t L = (len >> 12) + ((len & (kTileSweep - 1)) != 0 ? 1u : 0u);
  const uint32_t m = tile_sweeps_of(len, tl, nt);
  return small_udiv(L + m - 1u, m);
}

}  // namespace dq
