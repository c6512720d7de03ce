// Fused elementwise kernels of the safe-SAC update (src/ssac.py, src/smbpo.py:251-279).
// All are HBM/latency bound row-wise epilogues around the MLP kernels (mlp.hip):
//
//  drpo_sample_batch      mixed real/virtual minibatch gather + reward / constraint
//                         preprocessing (src/smbpo.py:253-270, src/sampling.py:147-151)
//  drpo_policy_head       squashed-Gaussian sample / rsample / mean + log_prob
//                         (src/policy.py:89-97, torch TanhTransform / Normal)
//  drpo_cc_head           constraint-critic log-std soft clamp, quantile upper bound
//                         mu + std_ratio*std and its max over C (src/ssac.py:64-92,588-600)
//  drpo_cc_dist           ConstraintCritic.forward's per-constraint outputs (src/ssac.py:75-92)
//  drpo_multiplier_head   Lagrangian multiplier loss gradient (src/ssac.py:529-568)
//  drpo_multiplier_out    MLPMultiplier.forward output transform (src/ssac.py:107-111)
// The critic / certificate losses, the actor losses' output gradients, the
// squashed-Gaussian backward and the alpha gradient have no launch of their own: the
// backward launches of mlp.hip and drpo_optim_step form them (row formulas shared with
// these kernels: sac_rows.hpp, critic_rows.hpp).
// drpo_multiplier_head accumulates its (already scaled) loss with a float atomic into a
// caller-zeroed device scalar, so no host synchronisation is needed.
#include "common.hpp"
#include "sac_rows.hpp"

using namespace drpo;

namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  __syncthreads();
  return s;   // valid in thread 0
}


}  // namespace

// ---------------------------------------------------------------------------
// minibatch sampling
// ---------------------------------------------------------------------------

__global__ void sample_batch_kernel(drpo_buffer_view_t real, drpo_buffer_view_t virt, int n_real, int B, int S, int A,
                                    int C, const int64_t* idx_real, const int64_t* idx_virt, uint64_t seed,
                                    uint64_t ctr, float reward_scale, float alive_bonus, float cscale, float coffset,
                                    float* os, float* oa, float* os2, float* orw, uint8_t* od, uint8_t* ov, float* oh) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const bool isr = i < n_real;
  const drpo_buffer_view_t& bv = isr ? real : virt;
  const int j = isr ? i : i - n_real;
  int64_t len = bv.len;
  if (len < 0) {
    const int64_t p = *bv.ptr_dev;
    len = p < bv.cap ? p : bv.cap;
  }
  int64_t q;
  const int64_t* ix = isr ? idx_real : idx_virt;
  if (ix) {
    q = ix[j];
  } else {
    const u32x4 rr = philox({(uint32_t)j, isr ? 0u : 1u, 0x5a4d11u, (uint32_t)ctr}, (uint32_t)seed,
                            (uint32_t)(seed >> 32));
    q = (int64_t)(((uint64_t)rr.x * (uint64_t)len) >> 32);
  }
  // grid.y splits the row's components over 4 threads (more loads in flight)
  const int part = blockIdx.y;
  if (part == 0) {
    for (int k = 0; k < S; ++k) os[(int64_t)i * S + k] = bv.s[q * S + k];
  } else if (part == 1) {
    for (int k = 0; k < S; ++k) os2[(int64_t)i * S + k] = bv.s2[q * S + k];
  } else if (part == 2) {
    for (int k = 0; k < A; ++k) oa[(int64_t)i * A + k] = bv.a[q * A + k];
    float r = bv.r[q];
    if (reward_scale != 0.f) r = r * reward_scale;
    if (alive_bonus != 0.f) r = r + alive_bonus;
    orw[i] = r;
    od[i] = bv.d[q];
    ov[i] = bv.v[q];
  } else {
    for (int c = 0; c < C; ++c) {
      float hv = bv.h[q * C + c] * cscale;
      hv = hv + (hv > 0.f ? 1.f : 0.f) * coffset;
      oh[(int64_t)i * C + c] = hv;
    }
  }
}

DRPO_API int drpo_sample_batch(const drpo_buffer_view_t* real, const drpo_buffer_view_t* virt, int n_real, int B,
                               int S, int A, int C, const int64_t* idx_real, const int64_t* idx_virt, uint64_t seed,
                               uint64_t ctr, float reward_scale, float alive_bonus, float constraint_scale,
                               float constraint_offset, float* s, float* a, float* s2, float* r, uint8_t* d,
                               uint8_t* v, float* h, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(real && virt && B >= 0 && n_real >= 0 && n_real <= B, "drpo_sample_batch: bad sizes");
  if (B == 0) return DRPO_OK;
  sample_batch_kernel<<<dim3((B + 63) / 64, 4), 64, 0, stream>>>(*real, *virt, n_real, B, S, A, C, idx_real, idx_virt, seed,
                                                          ctr, reward_scale, alive_bonus, constraint_scale,
                                                          constraint_offset, s, a, s2, r, d, v, h);
  DRPO_LAUNCH_CHECK("sample_batch");
  return DRPO_OK;
}

// ---------------------------------------------------------------------------
// policy head
// ---------------------------------------------------------------------------
// raw [B][2A] = (mu, log-std pre-activation). mode 0: sample (Normal.sample: eps*std+mu),
// 1: rsample (mu + eps*std), 2: mean only. Outputs are optional.
__global__ void policy_head_kernel(const float* raw, int64_t B, int A, int mode, const float* eps, uint64_t seed,
                                   uint64_t ctr, uint32_t site, float* a_out, float* logp, float* u_out, float* e_out,
                                   float* amean) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float* r = raw + i * 2 * A;
  if (mode == 3) {   // distribution parameters (loc, scale) for distr()
    for (int d = 0; d < A; ++d) {
      const float mu = r[d];
      const float sd = expf(pi_log_std(r[A + d])) * 1.0f;
      if (amean) amean[i * A + d] = tanhf(mu);
      if (u_out) u_out[i * A + d] = mu;
      if (e_out) e_out[i * A + d] = sd;
    }
    return;
  }
  squashed_gaussian_row([&](int c) { return r[c]; }, i, A, mode, eps, seed, ctr, site, a_out, logp, u_out, e_out,
                        amean);
}

DRPO_API int drpo_policy_head(const float* raw, int64_t B, int A, int mode, const float* eps, uint64_t seed,
                              uint64_t ctr, uint32_t site, float* a, float* logp, float* u, float* e, float* amean,
                              drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(mode >= 0 && mode <= 3 && A >= 1, "drpo_policy_head: bad mode/A");
  if (B == 0) return DRPO_OK;
  policy_head_kernel<<<(unsigned)((B + 63) / 64), 64, 0, stream>>>(raw, B, A, mode, eps, seed, ctr, site, a, logp,
                                                                      u, e, amean);
  DRPO_LAUNCH_CHECK("policy_head");
  return DRPO_OK;
}

// ---------------------------------------------------------------------------
// constraint-critic head: ub = mu + ratio*std (distributional) or mu; max over C
// ---------------------------------------------------------------------------
__global__ void cc_head_kernel(const float* mu, const float* lsraw, int64_t B, int C, int dist, float ratio, float lmin,
                               float lmax, float* ubmax, int* argmax) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const CcBound b = cc_bound_row([&](int c) { return mu[i * C + c]; }, [&](int c) { return lsraw[i * C + c]; }, C,
                                 dist, ratio, lmin, lmax);
  if (ubmax) ubmax[i] = b.best;
  if (argmax) argmax[i] = b.arg;
}

DRPO_API int drpo_cc_head(const float* mu, const float* lsraw, int64_t B, int C, int distributional, float std_ratio,
                          float log_std_min, float log_std_max, float* ubmax, int* argmax, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return DRPO_OK;
  cc_head_kernel<<<(unsigned)((B + 63) / 64), 64, 0, stream>>>(mu, lsraw, B, C, distributional, std_ratio,
                                                                  log_std_min, log_std_max, ubmax, argmax);
  DRPO_LAUNCH_CHECK("cc_head");
  return DRPO_OK;
}

// ConstraintCritic.forward outputs per constraint (src/ssac.py:75-92): mode 0
// (uncertainty) q = mu + std_ratio*std; mode 1 (sample) std and
// q = mu + clamp(eps, -2, 2)*std. n = rows*C elements.
__global__ void cc_dist_kernel(const float* mu, const float* lsraw, int64_t n, int mode, float std_ratio, float lmin,
                               float lmax, const float* eps, uint64_t seed, uint64_t ctr, float* std_out, float* q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float sd = cc_std(lsraw[i], lmin, lmax);
  if (mode == 0) {
    q[i] = mu[i] + std_ratio * sd;
  } else {
    float e = normal_at(eps, i, seed, ctr, 0xcc01u);
    e = fminf(fmaxf(e, -2.f), 2.f);
    if (std_out) std_out[i] = sd;
    q[i] = mu[i] + e * sd;
  }
}

DRPO_API int drpo_cc_dist(const float* mu, const float* lsraw, int64_t n, int mode, float std_ratio,
                          float log_std_min, float log_std_max, const float* eps, uint64_t seed, uint64_t ctr,
                          float* std_out, float* q, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(mu && lsraw && q && n >= 0 && (mode == 0 || mode == 1), "drpo_cc_dist: bad arguments");
  if (n == 0) return DRPO_OK;
  cc_dist_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(mu, lsraw, n, mode, std_ratio, log_std_min,
                                                                  log_std_max, eps, seed, ctr, std_out, q);
  DRPO_LAUNCH_CHECK("cc_dist");
  return DRPO_OK;
}

// ---------------------------------------------------------------------------
// multiplier head (mlp multiplier)
// ---------------------------------------------------------------------------
// x: multiplier MLP output [B]; sqc: max_C safe constraint value; aqc: max_C actor Qc.
// lam = multiplier_lam(x, ub); loss = -0.5 mean([sqc<=0] lam pen) + mean(([sqc>0](lam - (ub-eps)))^2)
__global__ __launch_bounds__(256) void multiplier_head_kernel(int64_t B, const float* x, const float* sqc,
                                                              const float* aqc, float thr, float plb, float pub,
                                                              float ub, float lam_eps, float* gx, float* loss) {
  __shared__ float red[8];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float l = 0.f;
  if (i < B && !x) {
    // scalar multiplier: the penalty sum of -mean(softplus(m) * penalty)
    l = fminf(fmaxf(aqc[i] - thr, plb), pub);
  } else if (i < B) {
    const float t = multiplier_tanh(x[i], ub);
    const float lam = multiplier_lam_of(t, ub);
    const float pen = fminf(fmaxf(aqc[i] - thr, plb), pub);
    const float safe = sqc[i] <= 0.f ? 1.f : 0.f, unsafe = 1.f - safe;
    const float invB = 1.f / (float)B;
    const float lu = unsafe * lam, tu = unsafe * (ub - lam_eps);
    l = (-0.5f * safe * lam * pen + (lu - tu) * (lu - tu)) * invB;
    const float glam = (-0.5f * safe * pen + 2.f * (lu - tu) * unsafe) * invB;
    gx[i] = glam * (ub / 2.f) * (1.f - t * t) * (2.f / ub);
  }
  if (loss) {
    const float s = block_sum(l, red);
    if (threadIdx.x == 0) atomicAdd(loss, s);
  }
}

DRPO_API int drpo_multiplier_head(int64_t B, const float* x, const float* safe_qc, const float* actor_qc,
                                  float threshold, float penalty_lb, float penalty_ub, float upper_bound,
                                  float lam_epsilon, float* gx, float* loss, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return DRPO_OK;
  multiplier_head_kernel<<<(unsigned)((B + 63) / 64), 64, 0, stream>>>(
      B, x, safe_qc, actor_qc, threshold, penalty_lb, penalty_ub, upper_bound, lam_epsilon, gx, loss);
  DRPO_LAUNCH_CHECK("multiplier_head");
  return DRPO_OK;
}

// lam = multiplier_lam(x, ub) (sac_rows.hpp)
__global__ void multiplier_out_kernel(int64_t B, const float* x, float ub, float* lam) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) lam[i] = multiplier_lam(x[i], ub);
}

DRPO_API int drpo_multiplier_out(int64_t B, const float* x, float upper_bound, float* lam, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return DRPO_OK;
  multiplier_out_kernel<<<(unsigned)((B + 63) / 64), 64, 0, stream>>>(B, x, upper_bound, lam);
  DRPO_LAUNCH_CHECK("multiplier_out");
  return DRPO_OK;
}
