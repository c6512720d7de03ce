// Keyed pseudo-random permutation of [0, N): the device-side stand-in for
// np.random.choice(N, B, replace=False), shared by the rollout engines (initial
// states) and drpo_sample_without_replacement.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace drpo {

__device__ __forceinline__ uint32_t prp_round(uint32_t r, uint32_t k) {
  uint32_t h = r * 0x9E3779B1u ^ k;
  h ^= h >> 15;
  h *= 0x85EBCA77u;
  h ^= h >> 13;
  h *= 0xC2B2AE3Du;
  h ^= h >> 16;
  return h;
}

// Keyed 4-round Feistel permutation of [0, 2^(2*hb)) with cycle walking into
// [0, N): the first B outputs are B distinct indices (sampling without
// replacement, the production stand-in for np.random.choice(N, B, replace=False)).
__device__ inline int64_t prp_index(uint64_t i, uint64_t N, int hb, const uint32_t key[4]) {
  const uint32_t mask = (hb >= 32) ? 0xFFFFFFFFu : ((1u << hb) - 1u);
  uint64_t x = i;
  for (int it = 0; it < 64; ++it) {
    uint32_t L = (uint32_t)(x >> hb) & mask, R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uint32_t F = prp_round(R, key[r]) & mask;
      uint32_t nl = R;
      R = L ^ F;
      L = nl;
    }
    x = ((uint64_t)L << hb) | R;
    if (x < N) return (int64_t)x;
  }
  return (int64_t)(x % N);   // unreachable in practice (expected walk < 4)
}

// half the bit width of the smallest even-width domain that holds n
inline int hb_for(int64_t n) {
  int b = 1;
  while ((1ull << (2 * b)) < (uint64_t)n) ++b;
  return b;
}

// the four round keys of one draw (seed, ctr)
inline void prp_keys(uint64_t seed, uint64_t ctr, uint32_t key[4]) {
  for (int i = 0; i < 4; ++i) key[i] = (uint32_t)(seed >> (8 * i)) * 0x9E3779B9u + (uint32_t)ctr * (2 * i + 1) + i;
}

}  // namespace drpo
