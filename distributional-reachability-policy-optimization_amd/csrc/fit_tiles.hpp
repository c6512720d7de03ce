// The trunk-width layer of the 512-thread, 16-row-tile kernels that keep a forward and its
// backward-data in one workgroup (fit.hip: fit_fb_kernel; rollout_adjoint.hip:
// rollout_adjoint_kernel): the tile geometry, the weight rings and the product of one
// 200 | 256-wide layer. One definition, included by both.
#pragma once
#include "common.hpp"
#include "ens_nll.hpp"

using namespace drpo;

namespace {
constexpr int FF_NW = 8;
constexpr int FF_NT = FF_NW * 64;
constexpr int FF_ROWS = ENS_TILE_ROWS;
constexpr int FF_LDH = 264;   // == 8 (mod 64): conflict-free A-fragment reads
}  // namespace

// Weight rings. Every layer's first FPT-1 (the fit's heads phase: FPH-1) k-steps of packed-mirror
// fragments are issued by the PREVIOUS phase, right after its last MFMA and before its
// epilogue and barrier, so the first touch of a layer's weights overlaps that epilogue instead of
// stalling the layer's first MFMA; the ring then streams the rest of the layer as tile_dense_mma
// does. (In the fit that touch is cold: the mirrors were rewritten by the previous step's Adam.
// In the adjoint the member, and with it the mirrors, changes from step to step.)
// File scope and `using namespace drpo`, as in fit.hip, whose code these lines were: the move
// keeps fit_fb_kernel's code object.
constexpr int FPT = 3;   // ring depth of the trunk-width (2 blocks per wave) layers (6: +1 %,
                         // profiles/r06/ring_ab2/fit)
constexpr int FPH = 4;   // ring depth of the heads phase (3-4 blocks per wave)
constexpr int FP1 = 5;   // the first layer's ring: K <= 64 (4 k-steps) preloaded whole

// Trunk-width layers: wave w owns column blocks w and w + 8 (clamped to a valid block:
// a wave with one valid block computes a discarded copy of it, which costs nothing -- the
// phase is bounded by SIMD 0's 4 blocks at N = 200, 2 per wave at N = 256)
template <int NK, int R = FPT>
__device__ __forceinline__ void ff_pre2(const float* __restrict__ P, int NCB, f32x4 (&bq)[R][2]) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int u = 0; u < R - 1; ++u)
    if (u < NK)
#pragma unroll
      for (int c = 0; c < 2; ++c) bq[u][c] = load_pk(P, min(wave + FF_NW * c, NCB - 1), u, NK);
}

template <int NK, int R = FPT>
__device__ __forceinline__ void ff_mma2(const float* in, const float* __restrict__ P, int NCB, f32x4 (&bq)[R][2],
                                        f32x4 (&acc)[1][2]) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cbs[2] = {min(wave, NCB - 1), min(wave + FF_NW, NCB - 1)};
#pragma unroll
  for (int c = 0; c < 2; ++c) acc[0][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 an = *reinterpret_cast<const f32x4*>(in + l15 * FF_LDH + 4 * g), ac;
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    if (s + R - 1 < NK) {
#pragma unroll
      for (int c = 0; c < 2; ++c) bq[(s + R - 1) % R][c] = load_pk(P, cbs[c], s + R - 1, NK);
    }
    ac = an;
    if (s + 1 < NK) an = *reinterpret_cast<const f32x4*>(in + l15 * FF_LDH + 16 * (s + 1) + 4 * g);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        acc[0][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[m], bq[s % R][c][m], acc[0][c], 0, 0, 0);
  }
}

__device__ __forceinline__ void ff_bias2(const float* __restrict__ bias, int N, float (&bv)[2]) {
  const int wave = threadIdx.x >> 6, l15 = threadIdx.x & 15;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = (wave + FF_NW * c) * 16 + l15;
    bv[c] = col < N ? gload(bias + col) : 0.f;
  }
}
