// The linear shield's candidate action (src/sampling.py:430-434), one definition for
// drpo_shield_mix (shield.hip) and the shield inside the fused rollout (rollout_persist.hpp).
#pragma once

namespace drpo {

// Candidate k of K: a_safe * r + a_perf * (1 - r), r = (K-1-k)/(K-1); k = 0 is a_safe,
// k = K-1 a_perf. PyTorch CPU fp32 arithmetic: the ratios are formed in double and rounded
// to float once (tensor * python float), the products and the sum are rounded separately
// (no FMA).
__device__ __forceinline__ float shield_mix_k(float a_safe, float a_perf, int K, int k) {
  const double r = (double)(K - 1 - k) / (double)(K - 1);
  const float rs = (float)r, rp = (float)(1.0 - r);
  return __fadd_rn(__fmul_rn(a_safe, rs), __fmul_rn(a_perf, rp));
}

}  // namespace drpo
