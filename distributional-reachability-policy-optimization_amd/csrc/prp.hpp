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
//
// The walk has no cap. The Feistel network is a permutation of the domain of
// D = 4^hb elements, and i < N lies on a cycle of it that returns to i; the walk
// from i therefore meets an element of [0, N) (i itself at the latest) after at
// most D - N + 1 steps, so the loop terminates, and two different i < N can never
// stop at the same element. A walk step lands outside [0, N) with probability
// 1 - N / D <= 3/4 (hb_for), so a walk longer than k has probability
// (1 - N / D)^k: below 1e-25 at k = 200. (A capped walk that falls back to x % N
// is not a permutation: at N just above a power of 4 about 1e-8 of the elements
// exceed 64 steps, and the fallback then repeats another row's index.)
__device__ inline int64_t prp_index(uint64_t i, uint64_t N, int hb, const uint32_t key[4]) {
  const uint32_t mask = (hb >= 32) ? 0xFFFFFFFFu : ((1u << hb) - 1u);
  uint64_t x = i;
  for (;;) {
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
