// The per-step arithmetic of the model-based lookahead (include/drpo_hip.h, drpo_rollout_lookahead),
// written once for its two users: the every-k scan of csrc/lookahead.hip and the planner's
// k = H score of csrc/plan.hip, which must produce the same bits.
//
// The definition is ordered double arithmetic, one rounding per operation. The header's
// __dadd_rn / __dmul_rn are a plain + and * compiled under the default contraction, which
// stays with them when they are inlined: a multiply feeding an add became one v_fma_f64 (one
// rounding for two operations; measured: one float32 of 9,546 off by an ulp at H 128). So the
// two operations are written here, with contraction off from here to the end of the including
// file.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace drpo {

__device__ __forceinline__ double dadd(double a, double b) { return a + b; }   // round to nearest, never fused
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }

// the result as stored: rounded to float32 once, a NaN as the canonical quiet NaN, so that it
// does not depend on which NaN an operation produced
__device__ __forceinline__ float look_store(double x) {
  const float f = (float)x;
  return f != f ? __int_as_float(0x7FC00000) : f;
}

// torch.maximum on doubles: a NaN in either operand stays
__device__ __forceinline__ double look_max(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? b : a)); }

// the critics' training units (src/smbpo.py:260-270), in double from the float32 inputs
__device__ __forceinline__ double look_reward(float reward, double rs, double ab) {
  double r = (double)reward;
  if (rs != 0.0) r = dmul(r, rs);
  if (ab != 0.0) r = dadd(r, ab);
  return r;
}
__device__ __forceinline__ double look_hprime(float value, double cs, double co) {
  double h = dmul((double)value, cs);
  h = dadd(h, dmul(h > 0.0 ? 1.0 : 0.0, co));
  return h;
}

// one step of the constraint critic's backup (compute_cons_target, src/ssac.py:284-294) from the
// value x behind it; the done branch is a select, never a product with zero.
// reachability: a = (1 - g) * h', formed by the caller (off the chain)
__device__ __forceinline__ double look_reach_step(bool done, double h, double a, double g, double x) {
  return done ? h : dadd(a, dmul(g, look_max(h, x)));
}
// cost: bits = 1 done | 2 violation
__device__ __forceinline__ double look_cost_step(unsigned bits, double g, double x) {
  const double v = (bits & 2) ? 1.0 : 0.0;
  return (bits & 1) ? v : dadd(v, dmul(g, x));
}

}  // namespace drpo
