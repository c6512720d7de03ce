// The model fit's heteroscedastic NLL (BatchedGaussianEnsemble.compute_loss,
// src/dynamics.py:136-153,236-253), the pieces its three sites share -- ens_loss_kernel
// (csrc/ensemble.hip), ens_upstream (csrc/mlp.hip) and fit_fb_body (csrc/fit.hip):
//   lv_clamp / nll_element / sp_grad_exact   one element's loss term and gradients
//   EnsPartials              the layout of the loss-partials workspace
//   ens_tile_partials        a 16-row tile's partial write-out (the fused kernels)
//   ens_loss_reduce_block    the fixed-order reduction of the partials, one 256-thread
//                            block: ens_loss_reduce_kernel, or the extra last block of a
//                            weight-gradient launch (one launch fewer per fit step)
//   ens_upstream_check / ens_reduce_check / ens_reduce_from   the host side of
//                            drpo_ens_upstream_t and drpo_ens_reduce_t
#pragma once
#include "common.hpp"

namespace drpo {
constexpr int LOSS_MAXS1 = 256;
constexpr int LOSS_MAXZ = 256;

// torch softplus backward, libm: x > 20 ? 1 : e^x / (e^x + 1) with expf and an IEEE divide
// (the hardware flavour is sp_grad, common.hpp)
__device__ __forceinline__ float sp_grad_exact(float x) {
  if (x > 20.f) return 1.f;
  const float z = expf(x);
  return z / (z + 1.f);
}

// the soft log-var clamp: lo + softplus(hi - softplus(hi - raw) - lo)
__device__ __forceinline__ float lv_clamp(float raw, float lo, float hi) {
  const float l1 = hi - softplusf(hi - raw);
  return lo + softplusf(l1 - lo);
}

// One NLL element: diff-head output D, raw log-var, state s (0 for the reward column),
// target t, the column's log-var bounds and the gradient scale g. Returns the loss term
// diff^2 exp(-l) + l; gd / gl: d / d(D, raw); cmn / cmx: the element's share of
// d / d(min_log_var, max_log_var). The clamp, exp(-l) and the loss term are libm (expf /
// log1pf); the softplus derivatives are the hardware sp_grad. The fused kernels (ens_upstream,
// fit_fb_body) call it; ens_loss_kernel is the same text with sp_grad_exact, written out
// (csrc/ensemble.hip says why).
__device__ __forceinline__ float nll_element(float D, float raw, float s, float t, float lo, float hi, float g,
                                             float& gd, float& gl, float& cmn, float& cmx) {
  const float l1 = hi - softplusf(hi - raw);
  const float l = lo + softplusf(l1 - lo);
  const float m = D + s;
  const float diff = t - m;
  const float iv = expf(-l);
  const float dl = (1.f - diff * diff * iv) * g;
  const float s1 = sp_grad(l1 - lo), s2 = sp_grad(hi - raw);
  gd = -2.f * diff * iv * g;
  gl = dl * s1 * s2;
  cmn = dl * (1.f - s1);
  cmx = dl * s1 * (1.f - s2);
  return diff * diff * iv + l;
}

// The loss-partials workspace: per (member z, row block bx) one mse partial, then per
// column the min- and the max-log-var bound gradient partials: part_mse [Z][nbx] |
// part_min [Z][nbx][S1] | part_max [Z][nbx][S1]. F: float or const float.
template <typename F>
struct EnsPartials {
  F *mse, *min, *max;
  __host__ __device__ EnsPartials(F* part, int Z, int nbx, int S1)
      : mse(part), min(part + (size_t)Z * nbx), max(part + (size_t)Z * nbx + (size_t)Z * nbx * S1) {}
  static __host__ __device__ size_t bytes(int Z, size_t nbx, int S1) {
    return sizeof(float) * (size_t)Z * nbx * (1 + 2 * (size_t)S1);
  }
};

// Row tilings. ens_loss_kernel takes 256 / KP rows per block with KP = S1 rounded up to a
// power of two >= 16, so at most 16; the fused kernels take ENS_TILE_ROWS. The workspace is
// sized for the loss kernel's tiling (drpo_ens_loss_workspace_size), which therefore has at
// least as many row blocks as the fused kernels write.
constexpr int LOSS_KP_MIN = 16;
constexpr int ENS_TILE_ROWS = 16;
static_assert(256 / LOSS_KP_MIN <= ENS_TILE_ROWS, "a workspace sized for ens_loss_kernel must cover the 16-row tiles");

inline int loss_kp(int S1) {
  int kp = LOSS_KP_MIN;
  while (kp < S1) kp <<= 1;
  return kp;
}
// rows per loss workgroup: one row per thread (256 / KP rows of KP column lanes)
inline int loss_rows(int S1) { return 256 / loss_kp(S1); }
__host__ __device__ inline int ens_tile_nbx(int64_t b) { return (int)((b + ENS_TILE_ROWS - 1) / ENS_TILE_ROWS); }

// A fused kernel's tile write-out at partial block pb = z * nbx + bx: the per-wave mse sums
// (s_mse[NW]) added in wave order by thread 0, and per column the sums over the tile's 16
// LDS rows of the bound-gradient shares (Cm / Cx, row stride ld). writes: whether this
// workgroup is the one that writes (one head's workgroup of a split-heads launch).
template <int NW>
__device__ __forceinline__ void ens_tile_partials(const EnsPartials<float>& P, size_t pb, int S1, const float* s_mse,
                                                  const float* Cm, const float* Cx, int ld, bool writes) {
  const int tid = threadIdx.x;
  if (!writes) return;
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < NW; ++w) t += s_mse[w];
    P.mse[pb] = t;
  }
  if (tid < S1) {
    float a0 = 0.f, a1 = 0.f;
    for (int r = 0; r < ENS_TILE_ROWS; ++r) {
      a0 += Cm[r * ld + tid];
      a1 += Cx[r * ld + tid];
    }
    P.min[pb * S1 + tid] = a0;
    P.max[pb * S1 + tid] = a1;
  }
}

// ---- host side of the two descriptors ------------------------------------------------
// heads: the launch reads up->D / up->LVR (drpo_ens_fit_fb forms them itself)
inline int ens_upstream_check(const char* who, const drpo_ens_upstream_t* up, bool heads = true) {
  DRPO_REQUIRE(up && (!heads || (up->D && up->LVR)) && up->s && up->t && up->minlv && up->maxlv,
               "%s: bad upstream (null D / LVR / s / t / minlv / maxlv)", who);
  DRPO_REQUIRE(up->part, "%s: bad upstream (no loss workspace)", who);
  DRPO_REQUIRE(up->b >= 1 && up->b <= ((int64_t)1 << 30), "%s: bad upstream (b = %lld rows)", who, (long long)up->b);
  DRPO_REQUIRE(up->S >= 1 && up->S + 1 <= LOSS_MAXS1, "%s: bad upstream (S + 1 = %d, at most %d)", who, up->S + 1,
               LOSS_MAXS1);
  DRPO_REQUIRE(up->Z >= 1 && up->Z <= LOSS_MAXZ, "%s: bad upstream (Z = %d members, 1..%d)", who, up->Z, LOSS_MAXZ);
  return DRPO_OK;
}

inline int ens_reduce_check(const char* who, const drpo_ens_reduce_t* red) {
  DRPO_REQUIRE(red && red->part && red->mse && red->minlv && red->maxlv,
               "%s: bad reduction (null part / mse / minlv / maxlv)", who);
  DRPO_REQUIRE(!red->gmin == !red->gmax, "%s: bad reduction (gmin and gmax: both or neither)", who);
  DRPO_REQUIRE(red->Z >= 1 && red->Z <= LOSS_MAXZ && red->S1 >= 1 && red->S1 <= LOSS_MAXS1 && red->nbx >= 1,
               "%s: bad reduction (Z = %d of 1..%d, S + 1 = %d of 1..%d, %d row blocks)", who, red->Z, LOSS_MAXZ,
               red->S1, LOSS_MAXS1, red->nbx);
  return DRPO_OK;
}

// the deferred reduction of a launch that wrote nbx row blocks of partials for `up`:
// mse / loss / gmin / gmax / weight from red_in, everything else from the launch
inline drpo_ens_reduce_t ens_reduce_from(const drpo_ens_upstream_t& up, const drpo_ens_reduce_t& red_in, int nbx) {
  drpo_ens_reduce_t r = red_in;
  r.part = up.part;
  r.nbx = nbx;
  r.Z = up.Z;
  r.S1 = up.S + 1;
  r.minlv = up.minlv;
  r.maxlv = up.maxlv;
  r.gscale = up.gscale;
  return r;
}

// per-member NLL, total loss, bound gradients from the block partials. Every sum is
// spread over 16 lanes (strided partials, then a fixed xor tree), so the kernel waits
// a couple of memory latencies instead of one per partial; the order is fixed, so the
// result is deterministic.
// Reduce: drpo_ens_reduce_t, in generic memory or read in place from a kernarg segment.
// adam (drpo_wgrad_adam_t, may be NULL): the log-var bounds take their Adam step here
// (the weight-gradient launch's fused step) instead of accumulating into gmin / gmax.
template <typename Reduce, typename AdamT>
__device__ __forceinline__ void ens_loss_reduce_block(Reduce& rd, AdamT* adam) {
  const float* __restrict__ part = rd.part;
  const int nbx = rd.nbx, Z = rd.Z, S1 = rd.S1;
  const float* __restrict__ minlv = rd.minlv;
  const float* __restrict__ maxlv = rd.maxlv;
  const float weight = rd.weight;
  const float* gscale = rd.gscale;
  float *mse = rd.mse, *loss = rd.loss, *gmin = rd.gmin, *gmax = rd.gmax;
  __shared__ float red[256], smx[LOSS_MAXS1], smn[LOSS_MAXS1];
  const int tid = threadIdx.x;
  const int grp = tid >> 4, l16 = tid & 15;
  const EnsPartials<const float> P(part, Z, nbx, S1);
  const float *part_mse = P.mse, *part_min = P.min, *part_max = P.max;
  for (int z = grp; z < Z; z += 16) {
    float m = 0.f;
    for (int q = l16; q < nbx; q += 16) m += part_mse[(size_t)z * nbx + q];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m += __shfl_xor(m, o, 16);
    if (l16 == 0) {
      mse[z] = m;
      red[z] = m;
    }
  }
  const size_t Q = (size_t)Z * nbx;
  const float gw = gmin ? (gscale ? *gscale : 1.f) * weight : 0.f;
  for (int c = grp; c < S1; c += 16) {
    // the bounds' values for the loss term below, read before any fused step moves them
    if (l16 == 0) {
      smx[c] = maxlv[c];
      smn[c] = minlv[c];
    }
    if (gmin) {
      float a0 = 0.f, a1 = 0.f;
      for (size_t q = l16; q < Q; q += 16) {
        a0 += part_min[q * S1 + c];
        a1 += part_max[q * S1 + c];
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o, 16);
        a1 += __shfl_xor(a1, o, 16);
      }
      if (l16 == 0) {
        if (adam) {
          // the bound's finished gradient -> Adam on the bound itself (fused step)
          const float g0 = gmin[c], g1 = gmax[c];
          const int64_t e0 = (gmin + c) - adam->g, e1 = (gmax + c) - adam->g;
          float p0 = adam->p[e0], m0 = adam->m[e0], v0 = adam->v[e0];
          float p1 = adam->p[e1], m1 = adam->m[e1], v1 = adam->v[e1];
          adam_step(*adam, 1.f, g0 + (a0 - gw), p0, m0, v0);
          adam_step(*adam, 1.f, g1 + (a1 + gw), p1, m1, v1);
          adam->p[e0] = p0;
          adam->m[e0] = m0;
          adam->v[e0] = v0;
          adam->p[e1] = p1;
          adam->m[e1] = m1;
          adam->v[e1] = v1;
          if (g0 != 0.f) gmin[c] = 0.f;
          if (g1 != 0.f) gmax[c] = 0.f;
        } else {
          gmin[c] += a0 - gw;
          gmax[c] += a1 + gw;
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0 && loss) {
    float tot = 0.f;
    for (int zz = 0; zz < Z; ++zz) tot += red[zz];
    float smax = 0.f, smin = 0.f;
    for (int kk = 0; kk < S1; ++kk) {
      smax += smx[kk];
      smin += smn[kk];
    }
    *loss = tot + weight * (smax - smin);
  }
}

}  // namespace drpo
