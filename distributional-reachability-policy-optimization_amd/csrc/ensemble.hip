// Row-wise kernels around the fused ensemble MLP (mlp.hip) for the dynamics
// ensemble API and its fit (src/dynamics.py:112-253):
//
//  drpo_ens_gather_steps  fit / holdout minibatches: chronological replay indices
//                   (recorded or Philox) -> raw states, actions and targets [s', r]
//                   (src/dynamics.py:156-166,175-177; SampleBuffer.get order,
//                   src/sampling.py:87-92)
//  drpo_ens_head    Gaussian head: mu = diff + [s, 0], the soft log-var clamp, and
//                   optionally a sample mu + sqrt(exp(lv)) * eps split into (s', r)
//                   (src/dynamics.py:112-134,198-234)
//  drpo_ens_spread  the statistics ACROSS members of an all-member forward on shared rows:
//                   mean prediction, std of the members' means, root mean predicted
//                   variance, largest pair distance (extends means / mean / elite_samples,
//                   src/dynamics.py:206-234, which leave the reduction to the caller)
//  drpo_ens_loss    heteroscedastic NLL per member + log-var bound term, and its
//                   gradients w.r.t. the head outputs and min/max_log_var
//                   (src/dynamics.py:143-153,236-253)
// All are HBM/latency-bound epilogues; the GEMM work is in mlp.hip.
#include "common.hpp"
#include "ens_nll.hpp"

using namespace drpo;

namespace {

__device__ __forceinline__ int64_t chrono_to_phys(int64_t j, int64_t ptr, int64_t cap) {
  // SampleBuffer._get1: when wrapped, chronological order starts at ptr % cap
  return ptr > cap ? (ptr % cap + j) % cap : j;
}

}  // namespace

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
// One thread per gathered ELEMENT (row x [s | a | s' | r] column): the replay rows
// are random, so the copy is latency-bound; spreading it over rows * (2S+A+1)
// threads (instead of one thread per row walking its 2S+A+1 columns) keeps the whole
// chip's memory pipes busy. Each thread derives its row's index itself (recorded,
// or the row's Philox draw -- the same value for every column of the row).
// steps > 1: the minibatches of `steps` consecutive fit steps in ONE launch (step k:
// rows [k*rows, (k+1)*rows) of every output, indices idx[k*rows ..] or Philox counter
// ctr + k), so the fit loop pays one latency-bound gather per chunk of steps instead
// of one per step (the replay is not written during a fit).
__global__ void ens_gather_kernel(const float* __restrict__ bs, const float* __restrict__ ba,
                                  const float* __restrict__ bs2, const float* __restrict__ br, int64_t ptr,
                                  const int64_t* ptr_dev, int64_t cap, int64_t rows, int64_t steps,
                                  const int64_t* idx, uint64_t seed, uint64_t ctr, int S, int A,
                                  float* __restrict__ xs, float* __restrict__ xa, float* __restrict__ xt) {
  const int W = 2 * S + A + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= steps * rows * W) return;
  const int64_t gi = e / W;                  // row over all steps
  const int c = (int)(e - gi * W);
  const int64_t st = gi / rows, i = gi - st * rows;
  const int64_t p = ptr_dev ? *ptr_dev : ptr;
  const int64_t n = p < cap ? p : cap;
  int64_t j;
  if (idx) {
    j = idx[gi];
  } else {
    const uint64_t cs = ctr + (uint64_t)st;
    const u32x4 r = philox({(uint32_t)i, (uint32_t)(i >> 32), 0xe5e3b1u, (uint32_t)cs}, (uint32_t)seed,
                           (uint32_t)(seed >> 32));
    j = (int64_t)((((uint64_t)r.y << 32) | r.x) % (uint64_t)n);
  }
  const int64_t q = chrono_to_phys(j, p, cap);
  if (c < S) {
    xs[gi * S + c] = bs[q * S + c];
  } else if (c < S + A) {
    xa[gi * A + (c - S)] = ba[q * A + (c - S)];
  } else if (c < 2 * S + A) {
    xt[gi * (S + 1) + (c - S - A)] = bs2[q * S + (c - S - A)];
  } else {
    xt[gi * (S + 1) + S] = br[q];
  }
}

DRPO_API int drpo_ens_gather_steps(const float* states, const float* actions, const float* next_states,
                                   const float* rewards, int64_t ptr, const int64_t* ptr_dev, int64_t cap,
                                   int64_t rows, int64_t steps, const int64_t* idx, uint64_t seed, uint64_t ctr,
                                   int S, int A, float* xs, float* xa, float* xt, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(states && actions && next_states && rewards && cap >= 1 && rows >= 0 && steps >= 0 && S >= 1 &&
                   A >= 1,
               "drpo_ens_gather_steps: bad arguments");
  DRPO_REQUIRE(ptr_dev || ptr >= 1, "drpo_ens_gather_steps: empty buffer");
  const int64_t elems = steps * rows * (2 * S + A + 1);
  if (elems == 0) return DRPO_OK;
  DRPO_REQUIRE((elems + 255) / 256 <= 0x7fffffff, "drpo_ens_gather_steps: %lld elements", (long long)elems);
  ens_gather_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, stream>>>(states, actions, next_states, rewards, ptr,
                                                                         ptr_dev, cap, rows, steps, idx, seed, ctr,
                                                                         S, A, xs, xa, xt);
  DRPO_LAUNCH_CHECK("ens_gather");
  return DRPO_OK;
}

// ---------------------------------------------------------------------------
// Gaussian head (forward)
// ---------------------------------------------------------------------------
// D, LV: [Z][n][S1] head outputs (member-major); s: raw states [*][n][S] with
// member stride s_zstride (0 when every member sees the same rows). zsel: optional
// output-member -> input-member map (elite_samples). Outputs [Zo][n][*].
__global__ void ens_head_kernel(const float* D, const float* LVR, const float* s, int64_t s_zstride, int64_t n,
                                int S, const float* minlv, const float* maxlv, const int* zsel, const float* eps,
                                uint64_t seed, uint64_t ctr, float* mu, float* lv, float* s2, float* r) {
  const int S1 = S + 1;
  const int zo = blockIdx.y;
  const int zi = zsel ? zsel[zo] : zo;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * S1) return;
  const int64_t row = e / S1;
  const int k = (int)(e - row * S1);
  const int64_t src = (int64_t)zi * n * S1 + e;
  const float m = D[src] + (k < S ? s[(int64_t)zi * s_zstride + row * S + k] : 0.f);
  const float l = lv_clamp(LVR[src], minlv[k], maxlv[k]);
  const int64_t dst = (int64_t)zo * n * S1 + e;
  if (mu) mu[dst] = m;
  if (lv) lv[dst] = l;
  if (s2 || r) {
    float z;
    if (eps) {
      z = eps[dst];
    } else {
      float zz[4];
      philox_normal4(seed, (uint32_t)(dst >> 2), (uint32_t)(dst >> 34), 0xe5a1u, (uint32_t)ctr, zz);
      z = zz[dst & 3];
    }
    const float x = m + sqrtf(expf(l)) * z;
    if (k < S) {
      if (s2) s2[((int64_t)zo * n + row) * S + k] = x;
    } else if (r) {
      r[(int64_t)zo * n + row] = x;
    }
  }
}

DRPO_API int drpo_ens_head(const float* D, const float* LVR, const float* s, int64_t s_zstride, int64_t n, int S,
                           int nz_out, const float* minlv, const float* maxlv, const int* zsel, const float* eps,
                           uint64_t seed, uint64_t ctr, float* mu, float* lv, float* s2, float* r,
                           drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(D && LVR && s && minlv && maxlv && n >= 0 && S >= 1 && nz_out >= 1, "drpo_ens_head: bad arguments");
  if (n == 0) return DRPO_OK;
  dim3 grid((unsigned)((n * (S + 1) + 255) / 256), nz_out);
  ens_head_kernel<<<grid, 256, 0, stream>>>(D, LVR, s, s_zstride, n, S, minlv, maxlv, zsel, eps, seed, ctr, mu, lv, s2,
                                            r);
  DRPO_LAUNCH_CHECK("ens_head");
  return DRPO_OK;
}

// ---------------------------------------------------------------------------
// Spread of the members' predictions (the reduction across members)
// ---------------------------------------------------------------------------
// The split of ens_loss_kernel: thread t owns column lane k = t % KP of row r0 + t / KP (KP =
// S+1 rounded up to a power of two in 16..256), so a block is 256 / KP whole rows and reads
// 256 / KP * (S+1) consecutive floats of each member. Per chunk of KP columns (one chunk
// unless S+1 > 256):
//   1. the column's M values go to LDS (xd[m][t]) and into a sum, in list order; a second
//      pass over the thread's own LDS slots forms the variance about their mean. Only D is
//      read: the residual s is common to the members and would cost the difference its bits
//      (s ~ 1e4, D ~ 1e-3). The mean predicted variance is a third loop, over LVR.
//   2. the M (M-1) / 2 member pairs of a row are dealt to the row's KP lanes. A lane walks
//      the columns of its pair in column order through LDS, so a pair's sum does not depend
//      on which lane took it or on the order of the two members: (a - b)^2 == (b - a)^2.
// The per-row sums and the pair maximum are then reduced over the row's lanes (shuffles, and
// through LDS in wave order where a row spans waves): shapes that depend on S alone, so a
// row's results do not depend on n or on the row's place in a block. No atomics and no
// hand-off between workgroups.
constexpr int SPREAD_MAX_M = 32;
constexpr int SPREAD_LDM = 257;   // xd member stride: the pair loop's lanes differ in member, 257 = 1 (mod 64) spreads them over banks

inline int spread_kp(int S1) { return S1 > 256 ? 256 : loss_kp(S1); }

namespace {

// sum / max of v over the KP lanes of a row; every thread of the block calls it
template <bool MAX>
__device__ __forceinline__ float spread_row_reduce(float v, int KP, float* red, int tid) {
  const int w = KP < 64 ? KP : 64;
  for (int o = w >> 1; o > 0; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = MAX ? fmaxf(v, u) : v + u;
  }
  if (KP <= 64) return v;
  __syncthreads();                      // red is free again
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const int nw = KP >> 6, w0 = (tid >> 6) & ~(nw - 1);   // the row's waves, in order
  float t = red[w0];
  for (int i = 1; i < nw; ++i) t = MAX ? fmaxf(t, red[w0 + i]) : t + red[w0 + i];
  return t;
}

}  // namespace

__global__ __launch_bounds__(256) void ens_spread_kernel(drpo_ens_spread_t a, int KP) {
  extern __shared__ float spread_lds[];
  const int M = a.M, S = a.S, S1 = S + 1;
  float* xd = spread_lds;               // [M][SPREAD_LDM]: this chunk's d, by member and thread
  float* wl = xd + M * SPREAD_LDM;      // [256]: this chunk's column weights
  float* red = wl + 256;                // [4]
  const int tid = threadIdx.x, lane = tid % KP, rl = tid / KP, RP = 256 / KP;
  const int64_t row = (int64_t)blockIdx.x * RP + rl;
  const int64_t zs = a.n * S1;          // member stride of D, LVR
  const bool live = row < a.n;
  const bool wide = S1 > KP;            // several chunks (KP == 256, one row per block)
  const int P = M * (M - 1) / 2;
  const float fM = (float)M;
  float epi = 0.f, ale = 0.f, best = 0.f;
  float acc0 = 0.f, acc1 = 0.f;         // wide: the sums of this lane's (at most two) pairs over the chunks so far
  for (int c0 = 0; c0 < S1; c0 += KP) {
    const int k = c0 + lane;
    const float wk = k < S1 ? (a.scale ? a.scale[k] : 1.f) : 0.f;
    if (c0 > 0) __syncthreads();        // the previous chunk's pair loop is through with xd, wl
    if (rl == 0) wl[lane] = wk;
    if (live && k < S1) {
      const int64_t o = row * S1 + k;
      float sum = 0.f;
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const float d = a.D[(int64_t)(a.zsel ? a.zsel[m] : m) * zs + o];
        xd[m * SPREAD_LDM + tid] = d;
        sum += d;
      }
      const float dbar = sum / fM;
      float var = 0.f;
      for (int m = 0; m < M; ++m) {
        const float c = xd[m * SPREAD_LDM + tid] - dbar;
        var += c * c;
      }
      var /= fM;
      if (a.mean) a.mean[o] = (k < S ? a.s[row * S + k] : 0.f) + dbar;
      if (a.epistemic_std) a.epistemic_std[o] = sqrtf(var);
      epi += wk * wk * var;
      if (a.aleatoric_std || a.aleatoric) {
        const float lo = a.minlv[k], hi = a.maxlv[k];
        float av = 0.f;
#pragma unroll 4
        for (int m = 0; m < M; ++m)
          av += expf(lv_clamp(a.LVR[(int64_t)(a.zsel ? a.zsel[m] : m) * zs + o], lo, hi));
        av /= fM;
        if (a.aleatoric_std) a.aleatoric_std[o] = sqrtf(av);
        ale += wk * wk * av;
      }
    }
    if (a.disagreement && P > 0) {
      __syncthreads();
      const int kc = min(KP, S1 - c0);
      if (live) {
        int j = 0;
        for (int p = lane; p < P; p += KP, ++j) {
          int m1 = 0, rem = p;          // pair p -> members m1 < m2 of the list
          while (rem >= M - 1 - m1) {
            rem -= M - 1 - m1;
            ++m1;
          }
          const float* x1 = xd + m1 * SPREAD_LDM + rl * KP;
          const float* x2 = xd + (m1 + 1 + rem) * SPREAD_LDM + rl * KP;
          float q = wide ? (j == 0 ? acc0 : acc1) : 0.f;
          for (int kk = 0; kk < kc; ++kk) {
            const float t = wl[kk] * (x1[kk] - x2[kk]);
            q += t * t;
          }
          if (!wide) best = fmaxf(best, q);
          else if (j == 0) acc0 = q;
          else acc1 = q;
        }
      }
    }
  }
  if (wide) best = fmaxf(acc0, acc1);
  // sqrt is monotone: the root of the largest squared distance is the largest distance
  if (a.disagreement) {
    best = spread_row_reduce<true>(best, KP, red, tid);
    if (live && lane == 0) a.disagreement[row] = sqrtf(best);
  }
  if (a.epistemic) {
    epi = spread_row_reduce<false>(epi, KP, red, tid);
    if (live && lane == 0) a.epistemic[row] = sqrtf(epi);
  }
  if (a.aleatoric) {
    ale = spread_row_reduce<false>(ale, KP, red, tid);
    if (live && lane == 0) a.aleatoric[row] = sqrtf(ale);
  }
}

DRPO_API int drpo_ens_spread(const drpo_ens_spread_t* a, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(a, "drpo_ens_spread: null descriptor");
  const bool alea = a->aleatoric_std || a->aleatoric;
  DRPO_REQUIRE(a->mean || a->epistemic_std || a->disagreement || a->epistemic || alea,
               "drpo_ens_spread: no output requested");
  DRPO_REQUIRE(a->D, "drpo_ens_spread: null D");
  DRPO_REQUIRE(a->s || !a->mean, "drpo_ens_spread: mean needs s");
  DRPO_REQUIRE(a->LVR || !alea, "drpo_ens_spread: an aleatoric output needs LVR");
  DRPO_REQUIRE((a->minlv && a->maxlv) || !alea, "drpo_ens_spread: an aleatoric output needs minlv and maxlv");
  DRPO_REQUIRE(a->n >= 0 && a->S >= 1 && a->Z >= 1, "drpo_ens_spread: n=%lld S=%d Z=%d out of range", (long long)a->n,
               a->S, a->Z);
  DRPO_REQUIRE(a->M >= 1 && a->M <= SPREAD_MAX_M, "drpo_ens_spread: members M outside 1..32");
  DRPO_REQUIRE(a->zsel || a->Z <= SPREAD_MAX_M, "drpo_ens_spread: zsel NULL with Z=%d > 32", a->Z);
  DRPO_REQUIRE(a->zsel || a->M == a->Z, "drpo_ens_spread: zsel NULL means members 0..Z-1: M=%d, Z=%d", a->M, a->Z);
  if (a->n == 0) return DRPO_OK;
  const int KP = spread_kp(a->S + 1), RP = 256 / KP;
  const int64_t nb = (a->n + RP - 1) / RP;
  DRPO_REQUIRE(nb <= 0x7fffffff, "drpo_ens_spread: %lld rows", (long long)a->n);
  const size_t lds = sizeof(float) * ((size_t)a->M * SPREAD_LDM + 256 + 4);
  ens_spread_kernel<<<(unsigned)nb, 256, lds, stream>>>(*a, KP);
  DRPO_LAUNCH_CHECK("ens_spread");
  return DRPO_OK;
}

// ---------------------------------------------------------------------------
// NLL loss + gradients
// ---------------------------------------------------------------------------
// grid (row blocks of 256 / KP rows, member). Thread t owns column k = t % KP of row
// r0 + t / KP (KP = S1 rounded up to a power of two >= 16): one row per thread, so a
// block waits one memory latency (64-row blocks looped 4 times: 9.2 us per launch at
// E=7, b=256; the per-column log-var-bound partials are reduced through LDS). Each
// block leaves its partial sums in the workspace and ens_loss_reduce_kernel (one
// block) sums them in a fixed order into the per-member NLL, the total loss and the
// bound gradients: deterministic, no memset, and no in-kernel cross-workgroup hand-
// off (a device-scope fence writes back the whole XCD L2 on gfx950: measured 22 us
// for a last-block variant of this kernel).

__global__ __launch_bounds__(256) void ens_loss_kernel(const float* __restrict__ D, const float* __restrict__ LVR,
                                                       const float* __restrict__ s, int64_t s_zstride,
                                                       const float* __restrict__ t, int64_t t_zstride, int64_t b,
                                                       int S, int Z, int KP, const float* __restrict__ minlv,
                                                       const float* __restrict__ maxlv, const float* gscale,
                                                       float* gD, float* gLVR, float* __restrict__ part) {
  __shared__ float red[4];
  __shared__ float rmin[256], rmax[256];
  const int S1 = S + 1;
  const int nbx = gridDim.x;
  const int z = blockIdx.y, bx = blockIdx.x;
  const int tid = threadIdx.x;
  const bool grads = gD != nullptr;
  const int k = tid % KP, rl = tid / KP, RP = 256 / KP;
  const float inv_n = 1.f / (float)(b * S1);
  const float g = grads ? (gscale ? *gscale : 1.f) * inv_n : 0.f;
  const int64_t r0 = (int64_t)bx * RP;     // one row per thread (launcher: 256 / KP rows)
  const int64_t r1 = min(b, r0 + RP);
  float acc = 0.f, cmin = 0.f, cmax = 0.f;
  if (k < S1) {
    const float hi = maxlv[k], lo = minlv[k];
    for (int64_t row = r0 + rl; row < r1; row += RP) {
      const int64_t o = ((int64_t)z * b + row) * S1 + k;
      // nll_element (ens_nll.hpp) with sp_grad_exact for sp_grad, written out: through the helper
      // (templated on the flavour, the gradients behind a flag) this kernel took 801 instructions
      // and 51 VGPRs against 795 and 44 (profiles/fit_refactor)
      const float raw = LVR[o];
      const float l1 = hi - softplusf(hi - raw);
      const float l = lo + softplusf(l1 - lo);
      const float m = D[o] + (k < S ? s[(int64_t)z * s_zstride + row * S + k] : 0.f);
      const float diff = t[(int64_t)z * t_zstride + row * S1 + k] - m;
      const float iv = expf(-l);
      acc += diff * diff * iv + l;
      if (grads) {
        const float dl = (1.f - diff * diff * iv) * g;
        const float s1 = sp_grad_exact(l1 - lo), s2 = sp_grad_exact(hi - raw);
        gD[o] = -2.f * diff * iv * g;
        gLVR[o] = dl * s1 * s2;
        cmin += dl * (1.f - s1);
        cmax += dl * s1 * (1.f - s2);
      }
    }
  }
  const EnsPartials<float> P(part, Z, nbx, S1);
  float v = acc * inv_n;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  rmin[tid] = cmin;
  rmax[tid] = cmax;
  __syncthreads();
  const size_t pb = (size_t)z * nbx + bx;
  if (tid == 0) P.mse[pb] = red[0] + red[1] + red[2] + red[3];
  if (grads && tid < S1) {
    float a0 = 0.f, a1 = 0.f;
    for (int q = 0; q < RP; ++q) {
      a0 += rmin[q * KP + tid];
      a1 += rmax[q * KP + tid];
    }
    P.min[pb * S1 + tid] = a0;
    P.max[pb * S1 + tid] = a1;
  }
}

// per-member NLL, total loss, bound gradients from the block partials
// (ens_nll.hpp; also run as the last block of a drpo_mlp_wgrad_reduce launch)
__global__ __launch_bounds__(256) void ens_loss_reduce_kernel(drpo_ens_reduce_t r) {
  ens_loss_reduce_block(r, (const drpo_wgrad_adam_t*)nullptr);
}

DRPO_API size_t drpo_ens_loss_workspace_size(int64_t b, int S, int Z) {
  const int rows = loss_rows(S + 1);
  return EnsPartials<float>::bytes(Z, (size_t)((b + rows - 1) / rows), S + 1);
}

DRPO_API int drpo_ens_loss(const drpo_ens_upstream_t* up, const drpo_ens_reduce_t* red_in, float* gD, float* gLVR,
                           drpo_ens_reduce_t* reduce_out, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (const int e = ens_upstream_check("drpo_ens_loss", up)) return e;
  DRPO_REQUIRE(red_in, "drpo_ens_loss: null red_in");
  DRPO_REQUIRE(!gD == !gLVR && !gD == !red_in->gmin && !gD == !red_in->gmax,
               "drpo_ens_loss: gradient outputs (gD, gLVR, gmin, gmax) all or none");
  const int S1 = up->S + 1, rows = loss_rows(S1);
  const int nbx = (int)((up->b + rows - 1) / rows);
  const drpo_ens_reduce_t r = ens_reduce_from(*up, *red_in, nbx);
  if (const int e = ens_reduce_check("drpo_ens_loss", &r)) return e;
  ens_loss_kernel<<<dim3((unsigned)nbx, up->Z), 256, 0, stream>>>(up->D, up->LVR, up->s, up->s_zstride, up->t,
                                                                  up->t_zstride, up->b, up->S, up->Z, loss_kp(S1),
                                                                  up->minlv, up->maxlv, up->gscale, gD, gLVR,
                                                                  up->part);
  DRPO_LAUNCH_CHECK("ens_loss");
  if (reduce_out) {
    *reduce_out = r;   // deferred: the caller runs it (drpo_mlp_wgrad_reduce, drpo_ens_loss_reduce)
    return DRPO_OK;
  }
  ens_loss_reduce_kernel<<<1, 256, 0, stream>>>(r);
  DRPO_LAUNCH_CHECK("ens_loss_reduce");
  return DRPO_OK;
}

DRPO_API int drpo_ens_loss_reduce(const drpo_ens_reduce_t* red, drpo_stream_t stream) {
  if (const int e = ens_reduce_check("drpo_ens_loss_reduce", red)) return e;
  ens_loss_reduce_kernel<<<1, 256, 0, (hipStream_t)stream>>>(*red);
  DRPO_LAUNCH_CHECK("ens_loss_reduce");
  return DRPO_OK;
}
