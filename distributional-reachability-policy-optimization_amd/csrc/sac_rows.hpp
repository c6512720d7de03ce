// Row formulas of the safe-SAC update that more than one kernel evaluates: the policy's
// log-std map and squashed-Gaussian head (src/policy.py:88-97), the constraint critic's
// max-C upper bound (src/ssac.py:64-92,588-600) and the MLPMultiplier output transform
// (src/ssac.py:107-111). Each is written once here; csrc/sac.hip (row-wise launches) and
// csrc/mlp.hip (the same math fused into the forward / backward launches) call it.
// critic_rows.hpp keeps what needs a drpo_critic_head_t (targets, certificate loss).
#pragma once
#include "critic_rows.hpp"

namespace drpo {

// ---- policy log-std: log_std = -6 + 10 * sigmoid(raw), std = exp(log_std) ----------
constexpr float PI_LOG_STD_MIN = -6.f, PI_LOG_STD_SPAN = 10.f;
// from sg = sigmoid(raw); the two flavours differ only in how sg is formed
__device__ __forceinline__ float pi_log_std_of(float sg) { return PI_LOG_STD_MIN + PI_LOG_STD_SPAN * sg; }
// libm (expf, IEEE division): the row-wise head and the squashed-Gaussian backward
__device__ __forceinline__ float pi_log_std(float raw) { return pi_log_std_of(sigmoidf(raw)); }
// hardware transcendentals (critic_rows.hpp, ~1e-6 relative): the fused forward head
__device__ __forceinline__ float pi_log_std_hw(float raw) { return pi_log_std_of(cr_rcp(1.f + cr_exp(-raw))); }
// g = dL/d std -> dL/d raw: g * std * 10 * sg * (1 - sg), multiplied in this order
__device__ __forceinline__ float pi_dstd_draw(float g, float sd, float sg) {
  return g * sd * PI_LOG_STD_SPAN * sg * (1.f - sg);
}

// squashed-Gaussian head of one row (src/policy.py:88-97; Independent(Tanh(Normal))
// log_prob at the cached pre-tanh u). mode 0 sample, 1 rsample, 2 mean only.
// raw = [mu | log-std pre-activation] (2A values, any stride source).
template <typename RawAt>
__device__ __forceinline__ void squashed_gaussian_row(RawAt raw_at, int64_t i, int A, int mode, const float* eps,
                                                      uint64_t seed, uint64_t ctr, uint32_t site, float* a_out,
                                                      float* logp, float* u_out, float* e_out, float* amean) {
  float lp = 0.f;
  for (int d = 0; d < A; ++d) {
    const float mu = raw_at(d);
    const float ls = pi_log_std(raw_at(A + d));
    const float sd = expf(ls) * 1.0f;
    if (amean) amean[i * A + d] = tanhf(mu);
    if (mode == 2) continue;
    const float e = normal_at(eps, i * A + d, seed, ctr, site);
    const float u = (mode == 0) ? e * sd + mu : mu + e * sd;
    if (a_out) a_out[i * A + d] = tanhf(u);
    if (u_out) u_out[i * A + d] = u;
    if (e_out) e_out[i * A + d] = e;
    const float ladj = 2.f * (0.69314718055994531f - u - softplusf(-2.f * u));
    const float base = -((u - mu) * (u - mu)) / (2.f * (sd * sd)) - logf(sd) - 0.91893853320467274f;
    lp += (0.f - ladj) + base;
  }
  if (logp && mode != 2) logp[i] = lp;
}

// ---- constraint bound of one row -------------------------------------------------
// max over the C constraints of mu_c + ratio * std(raw log-std_c) (dist) or of mu_c; the
// first maximum wins a tie. ls: the arg-max's raw log-std (0 when !dist). mu_at(c) /
// ls_at(c) read the row (global memory or an LDS tile); ls_at is not called when !dist.
struct CcBound {
  float best;
  int arg;
  float ls;
};
template <typename MuAt, typename LsAt>
__device__ __forceinline__ CcBound cc_bound_row(MuAt mu_at, LsAt ls_at, int C, bool dist, float ratio, float lmin,
                                                float lmax) {
  CcBound b{0.f, 0, 0.f};
  for (int c = 0; c < C; ++c) {
    float v = mu_at(c);
    const float l = dist ? ls_at(c) : 0.f;
    if (dist) v = v + ratio * cc_std(l, lmin, lmax);
    if (c == 0 || v > b.best) { b.best = v; b.arg = c; b.ls = l; }
  }
  return b;
}

// ---- MLPMultiplier.forward output transform: lam = ub/2 * (1 + tanh(2x/ub)) ---------
__device__ __forceinline__ float multiplier_tanh(float x, float ub) { return tanhf(x / ub * 2.f); }
__device__ __forceinline__ float multiplier_lam_of(float t, float ub) { return ub / 2.f * (1.f + t); }   // t: the tanh
__device__ __forceinline__ float multiplier_lam(float x, float ub) {
  return multiplier_lam_of(multiplier_tanh(x, ub), ub);
}

}  // namespace drpo
