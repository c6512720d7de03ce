// The fused-horizon engine's kernel, rollout_persist_kernel, with everything one of its
// instantiations needs, and the launcher of a family of them. Included by the four objects
// that instantiate it: rollout.hip (the plain family, and every entry point) and
// rollout_given.hip, rollout_shield.hip, rollout_proposed.hip (one family each), so the
// families compile side by side and an edit to one recompiles its object. Templates and
// inline functions only: a non-template kernel or a __device__ variable here would be
// defined once per object and collide at link.
#pragma once

#include <type_traits>

#include <hip/hip_runtime.h>

#define DRPO_UNIFORM_WEIGHT_LOADS 1   // scalar-base weight loads (see load_pk)

#if defined(DRPO_STAMPS) && defined(DRPO_ROLLOUT_STAMPS_HERE)
// profiling builds only (profiles/stamps.py): per-workgroup s_memtime stamps into
// g_stamps_roll, which rollout.hip defines in front of this header (with
// DRPO_ROLLOUT_STAMPS_HERE). The stamps are read after SMBPO.rollout only, so the step
// kernel and the plain family carry them; the three family objects' kernels carry none.
#define RSTAMP(i)                                                                                 \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    unsigned long long _t;                                                                        \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                    \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    if (threadIdx.x == 0 && blockIdx.x < (1u << 14)) g_stamps_roll[blockIdx.x][(i)] = _t;         \
  } while (0)
#define CORE_STAMP(i) RSTAMP(i)   // sub-phase stamps inside the layer cores (profiles/stamps.py)
#define CORE_STAMP_W4(i)                                                                          \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    unsigned long long _t;                                                                        \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                    \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    if (threadIdx.x == 256 && blockIdx.x < (1u << 14)) g_stamps_roll[blockIdx.x][(i)] = _t;       \
  } while (0)
#else
#define RSTAMP(i) \
  do {            \
  } while (0)
#endif

#include "common.hpp"
#include "path_shapes.hpp"
#include "env_constraints.hpp"
#include "prp.hpp"
#include "sac_rows.hpp"
#include "shield_mix.hpp"

using namespace drpo;

// ---------------------------------------------------------------------------
// Pieces both engines share. Args: RolloutStepArgs or PersistArgs (the field names agree).
// ---------------------------------------------------------------------------

// Exclusive scan over the NT threads of a workgroup: each thread passes the total of
// its own run and gets the sum of the runs of the threads before it; `total` is the
// sum over all threads. part: NT ints of LDS, free again after the next barrier.
template <int NT>
__device__ __forceinline__ int block_exclusive_scan(int run, int* part, int& total) {
  const int tid = threadIdx.x;
  part[tid] = run;
  __syncthreads();
  if (tid < 64) {   // inclusive scan of the NT partials in one wave
    constexpr int PPL = NT / 64;
    int v[PPL], sum = 0;
    for (int q = 0; q < PPL; ++q) { v[q] = part[tid * PPL + q]; sum += v[q]; }
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (tid >= o) incl += y;
    }
    int e = incl - sum;
    for (int q = 0; q < PPL; ++q) { e += v[q]; part[tid * PPL + q] = e; }
  }
  __syncthreads();
  total = part[NT - 1];
  return part[tid] - run;
}

// normalizer mean / std + 1e-6 and the log-var bounds into four 64-float LDS vectors
// (issued first: the latency of these tiny loads hides behind what follows)
template <class Args>
__device__ __forceinline__ void preload_vecs(const Args& p, float* v_nm, float* v_ns, float* v_lo, float* v_hi) {
  const int tid = threadIdx.x, S = p.S, S1 = p.S + 1;
  if (tid < 256) {
    const int j = tid & 63, w = tid >> 6;
    if (w == 0 && j < S) v_nm[j] = p.norm_mean[j];
    if (w == 1 && j < S) v_ns[j] = p.norm_std[j] + 1e-6f;
    if (w == 2 && j < S1) v_lo[j] = p.min_lv[j];
    if (w == 3 && j < S1) v_hi[j] = p.max_lv[j];
  }
}

// physical replay row of batch row `row`: its chronological index (given, or the PRP
// sample without replacement) turned by the circular buffer's write pointer
template <class Args>
__device__ __forceinline__ int64_t replay_row(const Args& p, int row) {
  const int64_t c = p.init_idx ? p.init_idx[row]
                               : prp_index((uint64_t)row, (uint64_t)p.replay_len, p.prp_half_bits, p.prp_key);
  return (p.replay_ptr > p.replay_cap) ? (p.replay_ptr % p.replay_cap + c) % p.replay_cap : c;
}

// (The gather loop around replay_row stays written out in each kernel: as a helper it
// changed the persistent kernel's code, +1 % at bench config 4; profiles/rollout_refactor.)

// ---------------------------------------------------------------------------
// Fused-horizon engine (engine 2). A row's trajectory depends only on its own
// earlier steps (SMBPO.rollout, src/smbpo.py:229-249: the batch only loses rows),
// so each workgroup keeps its 16/32-row tile for ALL H steps, with the states in
// LDS, and no workgroup ever waits for another. Rows that finish (done) stay in
// the tile masked off. Each step's surviving rows go to a staging area indexed
// [t][original row] together with per-(t, tile) counts and in-tile maps;
// rollout_emit_kernel then writes them into the circular buffer in the
// reference's order (step-major, surviving rows in batch order), which is the
// order the step engine's compaction produces.
//
// Against one launch per step this removes the per-step launch and drain, the
// device-wide count scan and the binary-searched gather of the previous step's
// states (bench workload: 37.3 -> 30.9 us per step). The step's Gaussian draws
// are generated into LDS by waves 1..7 while wave 0 evaluates the previous
// step's constraints, and the LDS hand-offs use lds_barrier() (no wait on
// outstanding global loads or the staging stores).
//
// Measured and rejected: issuing each layer's first weight k-steps ahead of the
// barrier / elementwise phase in front of it (and holding the actor's
// loop-invariant input/output fragments in registers). Across all placements the
// step time did not change, and the held fragments pushed the kernel to 256 VGPRs
// with scratch reloads in front of the MFMA loops.
// ---------------------------------------------------------------------------
constexpr int PERSIST_MAX_H = DRPO_ROLLOUT_FUSED_MAX_H;

// The actor's weights are the same every step: without this the compiler hoists
// all of a layer's (restrict, loop-invariant) fragment loads out of the horizon
// loop and keeps them live in registers for the whole loop (hundreds of spills).
__device__ __forceinline__ const float* step_opaque(const float* ptr) {
  asm volatile("" : "+s"(ptr));
  return ptr;
}

// Two choices of the persistent kernel, each measured (A/B, one box):
//  - the per-step pointers / sizes are read through an opaque kernarg pointer at their
//    point of use (PARG: scalar loads) instead of holding the whole argument block in
//    SGPRs across the loop (SGPR spills): config 2 248 -> 242 us per launch
//    (profiles/r03/ab_persist);
//  - the elite member's first-layer fragments and biases are issued at the top of the
//    step, so they arrive while the actor runs: +0.7-1.3 % (profiles/r05/rollout_ab).
// (Actor biases staged in LDS once per launch measured no gain: profiles/r05/rollout_ab.)

struct PersistArgs {
  int S, A, C, Ha, Hm, B, H, ntiles;
  EnvParams env;
  const float *aW1, *ab1, *aW2, *ab2, *aW3, *ab3;
  // member 0 of the ensemble mirrors / biases; member m adds m * (mstride | bstride)
  const float *mW1, *mb1, *mW2, *mb2, *dW1, *db1, *dW2, *db2, *lW1, *lb1, *lW2, *lb2;
  int64_t ms_in, ms_hid, ms_out;    // packed strides: (S+A -> Hm), (Hm -> Hm), (Hm -> S+1)
  const float *norm_mean, *norm_std, *min_lv, *max_lv;
  const float* replay_states;
  const int64_t* init_idx;
  int64_t replay_len, replay_ptr, replay_cap;
  uint32_t prp_key[4];
  int prp_half_bits;
  const float* eps_a;   // [H][B][A] original-row layout, or nullptr (Philox)
  const float* eps_m;   // [H][B][S+1]
  uint64_t seed, ctr;
  float *st_s, *st_s2, *st_a, *st_r, *st_h;
  uint8_t* st_dv;       // bit0 done, bit1 violation
  int* cnt;             // [H][ntiles] rows alive at the start of step t
  int* inv;             // [H][ntiles*ROWS] in-tile index of the k-th alive row
  int ldx, ldh, ldm, lds;
  // small rollouts: block 0 copies the buffer pointer into base_slot before any emit
  // (rollout_emit_self_kernel then reads the copy and advances *vptr itself)
  const int64_t* vptr_in;
  int64_t* base_slot;
  int members[PERSIST_MAX_H];
  // env id 4: the constraint program (device memory; read by the PG instantiations only).
  // Last, so that every other field keeps its kernarg offset.
  const void* env_prog;
  // given actions [B][n_given][A], trajectory-major (read by the GA instantiations only):
  // steps t < n_given take given[row][t] in place of the actor's sample. Appended likewise.
  const float* given;
  int n_given;
  // the shield (read by the SH instantiations only; appended likewise). Safe actor (the
  // actor's shape) and constraint critic: packed mirrors + biases. cW: trunk, qW: mean
  // head, zW: log-std head (null when !sh_dist). cW1 != null selects the SH kernels.
  const float *sW1, *sb1, *sW2, *sb2, *sW3, *sb3;
  const float *cW1, *cb1, *cW2, *cb2, *qW1, *qb1, *qW2, *qb2, *zW1, *zb1, *zW2, *zb2;
  int Hc, Cq, sh_dist;
  float sh_ratio, sh_lmin, sh_lmax, sh_thr;
  uint8_t* sh_iv;     // [B][H] or null
  float* sh_cert;     // [B][H] or null
  // the linear shield (src/sampling.py:430-437) on the same kernels: K candidates, 0: the
  // threshold shield. sh_ab: float offset into the LDS of a_perf / a_safe, 2 x [ROWS][8],
  // behind everything else (LDS-resident actor weights included).
  int sh_lin_k, sh_ab;
  uint8_t* sh_blend;  // [B][H] or null
};

typedef const __attribute__((address_space(4))) PersistArgs* PersistArgsK;   // scalar (constant) loads
__device__ __forceinline__ PersistArgsK persist_args() {
  PersistArgsK q = (PersistArgsK)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(q));
  return q;
}
#define PARG(f) (persist_args()->f)

// First layer with K <= 16 (one k-step) whose fragments / biases were loaded ahead
// (top of the step): the wave's MAXC blocks, clamped to the last valid block (its
// duplicate results are discarded by the epilogue).
template <int NW, int MAXC>
struct Layer1Frags {
  f32x4 w[MAXC];
  float b[MAXC];
};

template <int NW, int MAXC>
__device__ __forceinline__ void layer1_prefetch(const float* P, const float* bias, int N, Layer1Frags<NW, MAXC>& f) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NCB = (N + 15) >> 4;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) f.w[c] = load_pk(P, min(wave + NW * c, NCB - 1), 0, 1);
  load_bias<NW, MAXC>(bias, N, f.b);
}

template <int NW, int RB, int MAXC, int ACT>
__device__ __forceinline__ void layer1_run(const float* in, int ldi, const Layer1Frags<NW, MAXC>& f, int N, float* out,
                                           int ldo) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  f32x4 acc[RB][MAXC], a[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    a[rb] = *reinterpret_cast<const f32x4*>(in + (rb * 16 + l15) * ldi + 4 * g);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[rb][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
        acc[rb][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][m], f.w[c][m], acc[rb][c], 0, 0, 0);
  dense_epilogue<NW, RB, MAXC, ACT>(acc, f.b, N, out, ldo, GSave{nullptr, nullptr, 0, 0});
}

// The dynamics model's two hidden heads and their narrow output layers
// (src/dynamics.py:84-91, 112-122) as ONE phase. Each wave runs one head's hidden layer
// (pair_wave_code: waves 0, 1, 2, 7 the diff head, 3-6 the log-var head) and owns its
// blocks base, base + NW/2, ...: 7 / 6 / 6 / 7 blocks on the four SIMDs for 13 blocks
// per head, the 4-block wave the older one on both 7-block SIMDs. Each wave then forms its split-K share of
// its head's output layer from exactly the columns it produced (read back from LDS by the
// same wave: no workgroup barrier between the two layers), the output layer's fragments
// issued before the hidden epilogue. Partials land in red slot [head][w mod NW/2], the
// layout narrow_pair_sum reduces.
template <int NW, int RB, int NC, int NK>
__device__ __forceinline__ void pair_split_core(int base, const float* in, int ldi, const float* __restrict__ P,
                                                const float* __restrict__ bias, int N, float* out, int ldo,
                                                const float* __restrict__ Pn, float* red_slot) {
  constexpr int HW = NW / 2;
  const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  int cbs[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) cbs[c] = base + HW * c;
  f32x4 acc[RB][NC];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[rb][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // a 2-deep ring: deeper rings only queue behind the L1 (4: +0.6-0.9 %, 6: +3 %, 8: +5 %
  // per launch; profiles/r06/ring_ab, profiles/r06/feed_probe)
  constexpr int PF = 2;
  f32x4 bq[PF][NC];
#pragma unroll
  for (int u = 0; u < PF - 1; ++u)
#pragma unroll
    for (int c = 0; c < NC; ++c) bq[u][c] = load_pk(P, cbs[c], u < NK ? u : NK - 1, NK);
  float bvs[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = cbs[c] * 16 + l15;
    bvs[c] = col < N ? gload(bias + col) : 0.f;
  }
  f32x4 an[RB], ac[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) an[rb] = *reinterpret_cast<const f32x4*>(in + (rb * 16 + l15) * ldi + 4 * g);
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    if (s + PF - 1 < NK) {
#pragma unroll
      for (int c = 0; c < NC; ++c) bq[(s + PF - 1) % PF][c] = load_pk(P, cbs[c], s + PF - 1, NK);
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) ac[rb] = an[rb];
    if (s + 1 < NK) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
        an[rb] = *reinterpret_cast<const f32x4*>(in + (rb * 16 + l15) * ldi + 16 * (s + 1) + 4 * g);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          acc[rb][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[rb][m], bq[s % PF][c][m], acc[rb][c], 0, 0, 0);
  }
  CORE_STAMP(13);
  CORE_STAMP_W4(11);
  // the output layer's k-steps == this wave's hidden column blocks (K = N = Hm)
  f32x4 nb[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) nb[c] = load_pk(Pn, 0, cbs[c], NK);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = cbs[c] * 16 + l15;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y = act_fn<ACT_SILU>(acc[rb][c][r] + bvs[c]);
        out[(rb * 16 + 4 * g + r) * ldo + col] = col < N ? y : 0.f;
      }
  }
  CORE_STAMP_W4(12);
  CORE_STAMP(14);
  wave_lds_sync();
  f32x4 pacc[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) pacc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(out + (rb * 16 + l15) * ldo + 16 * cbs[c] + 4 * g);
#pragma unroll
      for (int m = 0; m < 4; ++m) pacc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], nb[c][m], pacc[rb], 0, 0, 0);
    }
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) red_slot[rb * 256 + (4 * g + r) * 16 + l15] = pacc[rb][r];
  CORE_STAMP(15);
}

template <int NW, int RB, int NC, int NK>
__device__ __forceinline__ void pair_split_nc(int nc, int base, const float* in, int ldi, const float* P,
                                              const float* bias, int N, float* out, int ldo, const float* Pn,
                                              float* red_slot) {
  if (nc == NC) pair_split_core<NW, RB, NC, NK>(base, in, ldi, P, bias, N, out, ldo, Pn, red_slot);
  else if constexpr (NC > 1) pair_split_nc<NW, RB, NC - 1, NK>(nc, base, in, ldi, P, bias, N, out, ldo, Pn, red_slot);
}

// in: the trunk output (K = N = Hm, NK k-steps); out1 / out2: the heads' hidden
// activations; Pn1 / Pn2: the output layers (Hm -> S+1 <= 16). Ends with the barrier
// that publishes the partials.
template <int NW, int RB, int MAXC, int NK>
__device__ __forceinline__ void pair_split_heads(const float* in, int ldi, int N, const float* P1, const float* b1,
                                                 float* out1, const float* Pn1, const float* P2, const float* b2,
                                                 float* out2, const float* Pn2, float* red) {
  constexpr int HW = NW / 2;
  static_assert(NW == 8, "pair_wave_code maps 8 waves");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned code = pair_wave_code(wave);
  const bool second = code >> 2;
  const int base = code & 3;
  const int NCB = (N + 15) >> 4;
  const int nc = base < NCB ? min(MAXC, (NCB - base + HW - 1) / HW) : 0;
  // head 0's slot q holds base q, head 1's slot q holds base HW - 1 - q (narrow_pair_sum's order)
  float* slot = red + (size_t)(second ? HW + (HW - 1 - base) : base) * RB * 256;
  if (nc > 0)
    pair_split_nc<NW, RB, MAXC, NK>(nc, base, in, ldi, second ? P2 : P1, second ? b2 : b1, N, second ? out2 : out1,
                                    ldi, second ? Pn2 : Pn1, slot);

  else {   // a wave without blocks contributes zero partials
    const int lane = threadIdx.x & 63;
    for (int e = lane; e < RB * 256; e += 64) slot[e] = 0.f;
  }
  lds_barrier();
}

// This step's Gaussian draws into LDS: recorded (original-row layout) or the step
// engine's Philox keys with the original row. Threads [first, first + count) work.
// GA: at a step t < n_given the action slots take the row's given action instead of a
// draw (the step then copies it, see the kernel); the draws are keyed by (row, step,
// kind), so leaving one out shifts no other.
template <int ROWS, bool GA = false>
__device__ __forceinline__ void persist_noise(const float* eps_a, const float* eps_m, uint64_t seed, uint64_t ctr,
                                              int A, int S1, int B, int t, int row0, int nrows, float* nz_a,
                                              float* nz_m, int first, int count, const float* given = nullptr,
                                              int n_given = 0) {
  const int NA4 = (A + 3) >> 2, NM4 = (S1 + 3) >> 2;
  const int total = ROWS * (NA4 + NM4);
  for (int base = 0; base < total; base += count) {   // uniform trip count, divergent body
    const int i = base + (int)threadIdx.x - first;
    if (i < base || i >= base + count || i >= total) continue;
    const int r = i / (NA4 + NM4), q = i - r * (NA4 + NM4);
    const uint32_t row = (uint32_t)(row0 + r);
    if constexpr (GA) {
      if (t < n_given && q < NA4) {
        for (int d = 4 * q; d < min(A, 4 * q + 4); ++d)
          nz_a[r * 8 + d] = r < nrows ? given[((size_t)row * n_given + t) * A + d] : 0.f;
        continue;
      }
    }
    if (eps_a) {
      if (q < NA4) {
        for (int d = 4 * q; d < min(A, 4 * q + 4); ++d)
          nz_a[r * 8 + d] = r < nrows ? eps_a[((size_t)t * B + row) * A + d] : 0.f;
      } else {
        const int q2 = q - NA4;
        for (int j = 4 * q2; j < min(S1, 4 * q2 + 4); ++j)
          nz_m[r * 64 + j] = r < nrows ? eps_m[((size_t)t * B + row) * S1 + j] : 0.f;
      }
    } else {
      float z[4];
      if (q < NA4) {
        philox_normal4(seed, row, ((uint32_t)t << 8) | 0u, (uint32_t)q, (uint32_t)ctr, z);
        for (int u = 0; u < 4; ++u) nz_a[r * 8 + 4 * q + u] = z[u];
      } else {
        const int q2 = q - NA4;
        philox_normal4(seed, row, ((uint32_t)t << 8) | 1u, (uint32_t)q2, (uint32_t)ctr, z);
        for (int u = 0; u < 4; ++u) nz_m[r * 64 + 4 * q2 + u] = z[u];
      }
    }
  }
}

// log-var soft clamp into [lo, hi] + Gaussian sample on the hardware transcendentals
// (the step engine keeps libm's expf / sqrtf on purpose)
__device__ __forceinline__ float clamp_sample(float mean, float lv, float lo, float hi, float eps) {
  lv = hi - fast_softplus(hi - lv);
  lv = lo + fast_softplus(lv - lo);
  return mean + fast_exp(0.5f * lv) * eps;
}

// LW: the actor's first layer, its output head and the first PERSIST_L2_LDS k-steps of
// its hidden layer stay in LDS for the whole launch (the actor is the same every
// step; with one 16-row tile per CU every weight byte is otherwise re-read from L2
// each step, and the layers run at the CU's L2 read rate). Needs S <= 16,
// Ha == 256, 2A <= 16 and the LDS to spare (host check).
constexpr int PERSIST_L2_LDS = 3;

// PM: the dynamics heads' path fixed at compile time (1: paired heads, S+1 <= 16 and
// Hm = 200; 0: the general path), so each kernel holds registers for one path only
// (spilled VGPRs 53 -> 33 / 1 -> 0 against one kernel with a run-time path choice,
// profiles/r03/pm_ab)
// PG: the constraint phase (on the step's critical path) runs the program interpreter
// (env id 4): instantiations of their own, the built-in environments' kernels keep
// their code, registers and LDS. The program needs no LDS (scalar loads).
// GA: given actions (drpo_rollout_trajectories_given). Steps t < n_given skip the actor
// and take the row's action from memory, staged into nz_a by persist_noise one step
// ahead like a recorded draw; later steps are the actor's. Instantiations of their own
// again: the production kernels keep their code.
// SH: the safety shield of the real-environment controller (src/smbpo.py:124-136) inside
// the step (drpo_rollout_trajectories_shielded). Between the actor's sample and the
// member's normalisation, while xin still holds [s_raw, a]: the constraint critic's
// certificate of (s, a) (cc_bound_row), the decision certificate > threshold, the safe
// actor's mean action for the tiles with an intervening row, and the select into act /
// xin. No draw is made or moved. Instantiations of their own once more.
// The same kernels run the evaluation's linear shield (src/sampling.py:430-437,
// drpo_rollout_trajectories_linear) on a kernarg, sh_lin_k = K candidates: rows whose
// certificate fails try the blends j = 1 .. K-2 between the two actions one certificate
// pass each, closest to the policy's first, and take the first that passes or, at K-1,
// the safe action. The passes end as soon as no alive row of the tile is undecided.
// GA && SH: the shield judges the given actions (drpo_rollout_trajectories_proposed). At a
// step t < n_given the given action is the proposal: it is in act / xin before the shield's
// first barrier as the actor's sample is at any other step, and everything behind that
// barrier is the SH step unchanged (certificate of the proposal, decision, safe actor,
// select or blend). Steps t >= n_given are the SH kernel's steps. With n_given == H the
// host leaves LW off, and the safe actor streams from its packed mirrors as it always does.
template <int RB, int NW, bool LW, int PM, bool PG = false, bool GA = false, bool SH = false>
__global__ __launch_bounds__(NW * 64) void rollout_persist_kernel(PersistArgs p) {
  constexpr int ROWS = RB * 16;
  constexpr int NT = NW * 64;
  constexpr int MAXC = (16 + NW - 1) / NW;      // column blocks per wave for widths <= 256
  constexpr int PMAXC = (32 + NW - 1) / NW;     // paired 200-wide heads: 26 blocks
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int S = p.S, A = p.A, C = p.C, S1 = p.S + 1, B = p.B;
  if (p.base_slot && blockIdx.x == 0 && tid == 0) *p.base_slot = *p.vptr_in;

  // LDS carve-up. Re-derived at the top of every horizon step from an opaque zero
  // and opaque leading dimensions: otherwise LICM hoists every (loop-invariant)
  // per-lane LDS address of the unrolled layers out of the loop and spills them.
#define PERSIST_LDS_LAYOUT(ZO, LDX, LDH, LDM, LDSS)                                         \
  float* xin = smem + (ZO);                  /* ROWS x ldx  actor in / model in / next states */ \
  float* h1 = xin + ROWS * (LDX);                                                             \
  float* h2 = h1 + ROWS * (LDH);                                                              \
  float* h3 = h2 + ROWS * (LDH);                                                              \
  float* sraw = h3 + ROWS * (LDH);           /* ROWS x lds  states at the start of the step */  \
  float* dout = sraw + ROWS * (LDSS);       /* ROWS x ldm  (tracking's output layers) */        \
  float* lout = dout + ROWS * (LDM);                                                          \
  float* act = lout + ROWS * (LDM);          /* ROWS x 8 */                                     \
  float* rew = act + ROWS * 8;                                                                \
  float* nz_a = rew + ROWS;                  /* ROWS x 8    this step's action draws */         \
  float* nz_m = nz_a + ROWS * 8;             /* ROWS x 64   this step's model draws */          \
  int* flags = reinterpret_cast<int*>(nz_m + ROWS * 64);                                      \
  int* alive = flags + ROWS;                                                                  \
  int* s_nalive = alive + ROWS;                                                               \
  float* red = reinterpret_cast<float*>(s_nalive + 4);  /* NW*RB*256 narrow partials */       \
  float* vecs = red + NW * RB * 256;                    /* 4 x 64 */                          \
  float* v_nm = vecs;                                                                         \
  float* v_ns = vecs + 64;                                                                    \
  float* v_lo = vecs + 128;                                                                   \
  float* v_hi = vecs + 192;                                                                   \
  float* wl1 = vecs + 256;                  /* LW: actor L1 mirror [16 cb][256] */               \
  float* wl3 = wl1 + 16 * 256;              /* LW: actor head mirror [16 k-steps][256] */        \
  float* wl2 = wl3 + 16 * 256;              /* LW: actor L2 [16 cb][PERSIST_L2_LDS][256] */      \
  (void)wl1; (void)wl2; (void)wl3;                                                            \
  (void)h3; (void)dout; (void)lout; (void)act; (void)rew; (void)nz_a; (void)nz_m;    \
  (void)flags; (void)alive; (void)s_nalive; (void)red; (void)v_nm; (void)v_ns; (void)v_lo; (void)v_hi;
  const int tile = blockIdx.x;
  const int row0 = tile * ROWS;
  const int nrows = min(ROWS, B - row0);
  const int Ha = p.Ha, Hm = p.Hm;
  constexpr bool paired = PM == 1;
  {
  PERSIST_LDS_LAYOUT(0, p.ldx, p.ldh, p.ldm, p.lds)
  preload_vecs(p, v_nm, v_ns, v_lo, v_hi);
  if constexpr (LW) {
    // packed mirrors: aW1 is [16 cb][1 k-step][256], aW3 [1 cb][16 k-steps][256];
    // aW2 keeps k-steps [0, PERSIST_L2_LDS) of each of its 16 column blocks
    const f32x4* a1 = reinterpret_cast<const f32x4*>(p.aW1);
    const f32x4* a3 = reinterpret_cast<const f32x4*>(p.aW3);
    const f32x4* a2 = reinterpret_cast<const f32x4*>(p.aW2);
    for (int e = tid; e < 16 * 64; e += NT) {
      reinterpret_cast<f32x4*>(wl1)[e] = gload(a1 + e);
      reinterpret_cast<f32x4*>(wl3)[e] = gload(a3 + e);
    }
    for (int e = tid; e < 16 * PERSIST_L2_LDS * 64; e += NT) {
      const int cb = e / (PERSIST_L2_LDS * 64), r = e - cb * PERSIST_L2_LDS * 64;
      reinterpret_cast<f32x4*>(wl2)[e] = gload(a2 + cb * 16 * 64 + r);
    }
  }

  // ---- initial states (t = 0): chronological replay index -> physical row -----
  const int kpad = round_up(S + A, 16);
  for (int e = tid; e < ROWS * kpad; e += NT) {
    const int r = e / kpad, k = e - r * kpad;
    float v = 0.f;
    if (r < nrows && k < S) {
      v = p.replay_states[replay_row(p, row0 + r) * S + k];
    }
    xin[r * p.ldx + k] = v;
    if (k < S) sraw[r * p.lds + k] = v;
  }
  if (tid < ROWS) alive[tid] = tid < nrows;
  // step 0's draws
  if constexpr (GA)
    persist_noise<ROWS, true>(p.eps_a, p.eps_m, p.seed, p.ctr, A, S1, B, 0, row0, nrows, nz_a, nz_m, 0, NT, p.given,
                              p.n_given);
  else
  persist_noise<ROWS>(p.eps_a, p.eps_m, p.seed, p.ctr, A, S1, B, 0, row0, nrows, nz_a, nz_m, 0, NT);
  lds_barrier();
  }
  for (int t = 0; t < p.H; ++t) {
    int zo = 0, ldx = p.ldx, ldh = p.ldh, ldm = p.ldm, ldss = p.lds;
    asm volatile("" : "+s"(zo), "+s"(ldx), "+s"(ldh), "+s"(ldm), "+s"(ldss));
    PERSIST_LDS_LAYOUT(zo, ldx, ldh, ldm, ldss)
    const int m = PARG(members[t]);
    const float* aW2 = step_opaque(PARG(aW2));
    const float* ab2 = step_opaque(PARG(ab2));
    // the elite member's slices, formed where they are used (PARG: re-read per use)
#define MW(f, st) (PARG(f) + (size_t)m * PARG(st))
#define MB(f, n) (PARG(f) + (size_t)m * (n))
    Layer1Frags<NW, MAXC> m1;
    const bool m1_pre = S + A <= 16;
    if (m1_pre) layer1_prefetch<NW, MAXC>(MW(mW1, ms_in), MB(mb1, Hm), Hm, m1);

    if (t == 2) RSTAMP(0);
    if (t == 2) RSTAMP(1);
    // alive flags of this step's rows / of the next step's (double-buffered: the
    // constraint wave writes the next step's while the staging waves read these)
    int* alive_cur = (t & 1) ? flags : alive;
    int* alive_nxt = (t & 1) ? alive : flags;
    // GA: a given step has no actor (workgroup-uniform, on a kernarg)
    bool given_step = false;
    if constexpr (GA) given_step = t < PARG(n_given);
    if (!given_step) {
    // ---- actor MLP (src/policy.py:61-100) ------------------------------------
    if constexpr (LW) {
      tile_dense_impl<NW, RB, MAXC, ACT_RELU, 1, 1>(xin, ldx, S, step_opaque(PARG(aW1)),
                                                   step_opaque(PARG(ab1)), Ha, h1, ldh,
                                                   GSave{nullptr, nullptr, 0, 0}, wl1);
      lds_barrier();
      if (t == 2) RSTAMP(2);
      tile_dense_impl<NW, RB, MAXC, ACT_RELU, 16, PERSIST_L2_LDS>(h1, ldh, Ha, aW2, ab2,
                                                                 Ha, h2, ldh, GSave{nullptr, nullptr, 0, 0}, wl2);
    } else {
      tile_dense<NW, RB, MAXC, ACT_RELU>(xin, ldx, S, step_opaque(PARG(aW1)), step_opaque(PARG(ab1)), Ha, h1, ldh);
      lds_barrier();
      if (t == 2) RSTAMP(2);
      tile_dense<NW, RB, MAXC, ACT_RELU>(h1, ldh, Ha, aW2, ab2, Ha, h2, ldh);
    }
    // the head's split-K share of wave w is k-steps w, w + NW, ...: exactly the hidden
    // column blocks wave w just wrote (Ha <= 256), so no workgroup barrier here. That
    // holds while tile_dense's column-block map (block wave + NW*c) and
    // tile_dense_narrow_partials' k-step map (step wave + NW*q) are the same map and
    // NW divides the 16 blocks of a 256-wide layer.
    static_assert(16 % NW == 0, "wave-local head hand-off needs NW | 16");
    wave_lds_sync();
    if (t == 2) RSTAMP(3);
    }
    // ---- actor head + squashed Gaussian sample + model input [normalize(s), a]:
    //      the head's split-K partials are reduced by the threads that sample
    //      (one thread per (row, action dim) sums the mu and log-std columns) ----
    {
      if (given_step) {
        // the action as given (post-tanh, neither clamped nor squashed); 0 in the rows
        // past a partial tile's last
        if (tid < ROWS * A) {
          const int r = tid / A, d = tid - r * A;
          const float a = nz_a[r * 8 + d];
          act[r * 8 + d] = a;
          xin[r * ldx + S + d] = a;
        }
      } else {
      float bmu = 0.f, braw = 0.f;
      if (tid < ROWS * A) {   // ROWS * A <= NT (A <= 8)
        const int d = tid % A;
        const float* ab3 = step_opaque(PARG(ab3));
        bmu = gload(ab3 + d);
        braw = gload(ab3 + A + d);
      }
      tile_dense_narrow_partials<NW, RB, LW>(h2, ldh, Ha, step_opaque(PARG(aW3)), red, wl3);
      if (tid < ROWS * A) {
        const int r = tid / A, d = tid - r * A;
        const float mu = narrow_sum<NW, RB>(red, r, d) + bmu;
        const float raw = narrow_sum<NW, RB>(red, r, A + d) + braw;
        const float ls = -6.f + 10.f * fast_sigmoid(raw);
        const float a = fast_tanh(nz_a[r * 8 + d] * fast_exp(ls) + mu);
        act[r * 8 + d] = a;
        xin[r * ldx + S + d] = a;
      }
      }
      if constexpr (SH) {
        // ---- the shield (src/smbpo.py:124-136) on [s_raw, a]: xin's states are still raw.
        //      All weights streamed from the packed mirrors; h1 / h2 / h3, dout / lout and
        //      red are free between the actor and the member ----
        // act / xin[.., S + d] of every row (GA: at a given step the proposal, written above by
        // the same tid < ROWS * A threads); the sampling threads are done with red
        lds_barrier();
        const int Hc = PARG(Hc), Cq = PARG(Cq);
        const bool dist = PARG(sh_dist) != 0;
        // LK candidates (0: the threshold shield, one pass). Pass j scores candidate j of the
        // rows still undecided (ivm; all rows at j = 0, where the candidate is the policy's
        // action). Every exit below is on j, a kernarg or ivm: workgroup-uniform.
        const int LK = PARG(sh_lin_k);
        unsigned ivm = ~0u;
        for (int j = 0;; ++j) {
        // the LDS carve-up once more per pass, as at the top of the step and for its reason:
        // the per-lane addresses of the unrolled layers must not be hoisted out of this loop
        int zj = 0, ldxj = ldx, ldhj = ldh, ldmj = ldm;
        asm volatile("" : "+s"(zj), "+s"(ldxj), "+s"(ldhj), "+s"(ldmj));
        {
        const int ldx = ldxj, ldh = ldhj, ldm = ldmj;
        PERSIST_LDS_LAYOUT(zj, ldx, ldh, ldm, ldss)
        // 1. certificate: the constraint critic's trunk [S+A -> Hc -> Hc] (ReLU, ReLU
        //    output), the heads [Hc -> Hc -> Cq] (src/ssac.py:64-92)
        tile_dense<NW, RB, MAXC, ACT_RELU>(xin, ldx, S + A, step_opaque(PARG(cW1)), step_opaque(PARG(cb1)), Hc, h1,
                                           ldh);
        lds_barrier();
        tile_dense<NW, RB, MAXC, ACT_RELU>(h1, ldh, Hc, step_opaque(PARG(cW2)), step_opaque(PARG(cb2)), Hc, h2, ldh);
        lds_barrier();
        // the heads' hidden layers: mean -> h3, log-std -> h1 (the trunk is done with it)
        tile_dense<NW, RB, MAXC, ACT_RELU>(h2, ldh, Hc, step_opaque(PARG(qW1)), step_opaque(PARG(qb1)), Hc, h3, ldh);
        if (dist)
          tile_dense<NW, RB, MAXC, ACT_RELU>(h2, ldh, Hc, step_opaque(PARG(zW1)), step_opaque(PARG(zb1)), Hc, h1,
                                             ldh);
        lds_barrier();
        // the output layers one after the other through the one set of narrow partials
        // (ROWS * Cq <= NT: Cq <= 8): mu -> dout, raw log-std -> lout
        {
          float bq = 0.f;
          if (tid < ROWS * Cq) bq = gload(step_opaque(PARG(qb2)) + tid % Cq);
          tile_dense_narrow_partials<NW, RB>(h3, ldh, Hc, step_opaque(PARG(qW2)), red);
          if (tid < ROWS * Cq) {
            const int r = tid / Cq, c = tid - r * Cq;
            dout[r * ldm + c] = narrow_sum<NW, RB>(red, r, c) + bq;
          }
          lds_barrier();
        }
        if (dist) {
          float bz = 0.f;
          if (tid < ROWS * Cq) bz = gload(step_opaque(PARG(zb2)) + tid % Cq);
          tile_dense_narrow_partials<NW, RB>(h1, ldh, Hc, step_opaque(PARG(zW2)), red);
          if (tid < ROWS * Cq) {
            const int r = tid / Cq, c = tid - r * Cq;
            lout[r * ldm + c] = narrow_sum<NW, RB>(red, r, c) + bz;
          }
          lds_barrier();
        }
        // 2. decision (wave 0, one lane per row): the float comparison of
        //    drpo_shield_select mode 1 (linear: mode 2, a NaN does not qualify); the tile's
        //    intervening (linear: undecided) rows as a bit mask in LDS
        if (tid < 64) {
          bool iv = false;
          if (tid < ROWS && alive_cur[tid] && ((ivm >> tid) & 1u)) {
            const float* mu = dout + tid * ldm;
            const float* ls = lout + tid * ldm;
            const CcBound b = cc_bound_row([&](int c) { return mu[c]; }, [&](int c) { return ls[c]; }, Cq, dist,
                                           PARG(sh_ratio), PARG(sh_lmin), PARG(sh_lmax));
            iv = LK ? !(b.best <= PARG(sh_thr)) : b.best > PARG(sh_thr);
            const size_t o = (size_t)(row0 + tid) * PARG(H) + t;   // alive: row0 + tid < B
            if (j == 0) {
              if (PARG(sh_cert)) PARG(sh_cert)[o] = b.best;
              if (PARG(sh_iv)) PARG(sh_iv)[o] = iv ? 1 : 0;
            } else if (!iv && PARG(sh_blend)) {
              PARG(sh_blend)[o] = (uint8_t)j;   // decided at j (0: the zero fill)
            }
          }
          const uint64_t ivk = __ballot(iv);
          if (tid == 0) s_nalive[1] = (int)(uint32_t)ivk;   // ROWS <= 32
        }
        lds_barrier();
        ivm = (unsigned)__builtin_amdgcn_readfirstlane(s_nalive[1]);
        if (ivm == 0u) break;
        // 3. safe actor (the actor's shape), only in a tile with an intervening row: the
        //    test is workgroup-uniform, so every barrier below is reached by all waves or none
        if (j == 0) {
          tile_dense<NW, RB, MAXC, ACT_RELU>(xin, ldx, S, step_opaque(PARG(sW1)), step_opaque(PARG(sb1)), Ha, h1, ldh);
          lds_barrier();
          tile_dense<NW, RB, MAXC, ACT_RELU>(h1, ldh, Ha, step_opaque(PARG(sW2)), step_opaque(PARG(sb2)), Ha, h2, ldh);
          lds_barrier();
          float bmu = 0.f;
          if (tid < ROWS * A) bmu = gload(step_opaque(PARG(sb3)) + tid % A);
          tile_dense_narrow_partials<NW, RB>(h2, ldh, Ha, step_opaque(PARG(sW3)), red);
          // 4. select: a_safe = tanh(mu_safe) (the squashing of the actor's sample, no draw)
          if (tid < ROWS * A) {
            const int r = tid / A, d = tid - r * A;
            if ((ivm >> r) & 1u) {
              const float a = fast_tanh(narrow_sum<NW, RB>(red, r, d) + bmu);
              if (LK) {
                // linear: both ends of the blend stay in LDS for the passes to come (read
                // back below by the thread that writes them). GA: at a given step the
                // policy's end is the proposal
                float* ab = smem + PARG(sh_ab);
                ab[r * 8 + d] = act[r * 8 + d];
                ab[ROWS * 8 + r * 8 + d] = a;
              } else {
                act[r * 8 + d] = a;
                xin[r * ldx + S + d] = a;
              }
            }
          }
          if (LK == 0) break;
        }
        // 5. the next candidate of the undecided rows into act / xin: blend j + 1 (mix_k of
        //    drpo_shield_mix, k = LK-1 - (j+1)), or, at the last, the safe action itself,
        //    whose certificate decides nothing and is not computed
        const bool last = j + 1 >= LK - 1;
        if (tid < ROWS * A) {
          const int r = tid / A, d = tid - r * A;
          if ((ivm >> r) & 1u) {
            const float* ab = smem + PARG(sh_ab);
            const float as = ab[ROWS * 8 + r * 8 + d];
            const float a = last ? as : shield_mix_k(as, ab[r * 8 + d], LK, LK - 2 - j);
            act[r * 8 + d] = a;
            xin[r * ldx + S + d] = a;
          }
        }
        if (last) {
          if (tid < ROWS && ((ivm >> tid) & 1u) && PARG(sh_blend))   // undecided: alive
            PARG(sh_blend)[(size_t)(row0 + tid) * PARG(H) + t] = (uint8_t)(LK - 1);
          break;
        }
        lds_barrier();   // the candidates, before the next pass reads xin
        }
        }
      }
      for (int e = tid; e < ROWS * S; e += NT) {
        const int r = e / S, k = e - r * S;
        xin[r * ldx + k] = (sraw[r * ldss + k] - v_nm[k]) / v_ns[k];
      }
    }
    lds_barrier();
    if (t == 2) RSTAMP(4);

    // ---- elite member forward (src/dynamics.py:112-122) -----------------------
    if (m1_pre) layer1_run<NW, RB, MAXC, ACT_SILU>(xin, ldx, m1, Hm, h1, ldh);
    else
    tile_dense<NW, RB, MAXC, ACT_SILU>(xin, ldx, S + A, MW(mW1, ms_in), MB(mb1, Hm), Hm, h1, ldh);
    lds_barrier();
    if (t == 2) RSTAMP(5);
    if (RB == 1 && NW == 8 && Hm == 200) {
      // member hidden layer balanced over the SIMDs (13th block split over K;
      // profiles/r04/m2_split)
      const float b12 = tile_dense_13s<ACT_SILU>(h1, ldh, MW(mW2, ms_hid), MB(mb2, Hm), h2, ldh, red);
      lds_barrier();
      tile_dense_13s_finish<ACT_SILU>(red, b12, h2, ldh);
    } else
    tile_dense<NW, RB, MAXC, ACT_SILU>(h1, ldh, Hm, MW(mW2, ms_hid), MB(mb2, Hm), Hm, h2, ldh);
    lds_barrier();
    if (t == 2) RSTAMP(6);
    const float* dW1 = MW(dW1, ms_hid);
    const float* lW1 = MW(lW1, ms_hid);
    const float* db1 = MB(db1, Hm);
    const float* lb1 = MB(lb1, Hm);
    if (paired) {
      // output-layer biases first (their latency hides behind the hidden layers)
      float bd = 0.f, bl = 0.f;
      if (tid < ROWS * S1) {   // ROWS * S1 <= NT (S1 <= 16)
        const int j = tid % S1;
        bd = gload(MB(db2, S1) + j);
        bl = gload(MB(lb2, S1) + j);
      }
      // both hidden heads + their output layers' split-K partials, one barrier
      pair_split_heads<NW, RB, (13 + NW / 2 - 1) / (NW / 2), 13>(h2, ldh, Hm, dW1, db1, h1, MW(dW2, ms_out), lW1,
                                                                 lb1, h3, MW(lW2, ms_out), red);
      if (t == 2) RSTAMP(7);
      // the partials reduced by the threads that form the residual mean, soft-clamp the
      // log-variance and sample the next state
      if (tid < ROWS * S1) {
        const int r = tid / S1, j = tid - r * S1;
        const float mean = (narrow_pair_sum<NW, RB>(red, 0, r, j) + bd) + (j < S ? sraw[r * ldss + j] : 0.f);
        const float lv = narrow_pair_sum<NW, RB>(red, 1, r, j) + bl;
        const float x = clamp_sample(mean, lv, v_lo[j], v_hi[j], nz_m[r * 64 + j]);
        if (j < S) xin[r * ldx + j] = x;
        else rew[r] = x;
      }
    } else {
      if (Hm == 200 && 2 * ((S1 + 15) >> 4) <= NW) {
        // wide state (tracking, S + 1 = 52): the two hidden layers as one 400-wide layer,
        // then both output layers side by side (two inputs, one block per wave): two
        // phases instead of four
        tile_dense_pair<NW, RB, PMAXC, ACT_SILU, 13>(h2, ldh, Hm, dW1, db1, Hm, h1, lW1, lb1, Hm, h3, ldh);
        lds_barrier();
        if (t == 2) RSTAMP(7);
        // one block per wave: a ring as deep as K (every fragment in flight at once), else
        // this latency-bound layer waits one L2 round trip per few k-steps
        tile_dense_pair2<NW, RB, 1, ACT_NONE, 13, 13>(h1, h3, ldh, MW(dW2, ms_out), MB(db2, S1), S1, dout,
                                                       MW(lW2, ms_out), MB(lb2, S1), S1, lout, ldm);
      } else {
        const float* dW2 = MW(dW2, ms_out);
        const float* lW2 = MW(lW2, ms_out);
        const float* db2 = MB(db2, S1);
        const float* lb2 = MB(lb2, S1);
        tile_dense<NW, RB, MAXC, ACT_SILU>(h2, ldh, Hm, dW1, db1, Hm, h1, ldh);
        lds_barrier();
        if (S1 <= 16) tile_dense_narrow<NW, RB, ACT_NONE>(h1, ldh, Hm, dW2, db2, S1, dout, ldm, red);
        else tile_dense<NW, RB, MAXC, ACT_NONE>(h1, ldh, Hm, dW2, db2, S1, dout, ldm);
        lds_barrier();
        tile_dense<NW, RB, MAXC, ACT_SILU>(h2, ldh, Hm, lW1, lb1, Hm, h1, ldh);
        lds_barrier();
        if (t == 2) RSTAMP(7);
        if (S1 <= 16) tile_dense_narrow<NW, RB, ACT_NONE>(h1, ldh, Hm, lW2, lb2, S1, lout, ldm, red);
        else tile_dense<NW, RB, MAXC, ACT_NONE>(h1, ldh, Hm, lW2, lb2, S1, lout, ldm);
      }
      lds_barrier();
      if (t == 2) RSTAMP(10);
      // residual mean, log-var soft clamp, Gaussian sample
      for (int e = tid; e < ROWS * S1; e += NT) {
        const int r = e / S1, j = e - r * S1;
        const float mean = dout[r * ldm + j] + (j < S ? sraw[r * ldss + j] : 0.f);
        const float x = clamp_sample(mean, lout[r * ldm + j], v_lo[j], v_hi[j], nz_m[r * 64 + j]);
        if (j < S) xin[r * ldx + j] = x;
        else rew[r] = x;
      }
    }
    lds_barrier();
    if (t == 2) RSTAMP(8);

    // ---- one phase: constraints + alive map + their staging writes (wave 0, one
    //      lane per row), the states / actions staging writes and the state
    //      hand-off (waves 1 .. NW/2-1), the next step's draws (waves NW/2 ..) ----
    const size_t sb = (size_t)t * B + row0;
    if (tid < 64) {
      bool in_r = false, dn = false, vl = false;
      if (tid < ROWS && alive_cur[tid]) {
        float hh[8];
        const void* prog = nullptr;
        if constexpr (PG) {
          // opaque per step: the program's (loop-invariant) scalar loads stay in the step
          prog = PARG(env_prog);
          asm volatile("" : "+s"(prog));
        }
        constraint_row<PG>(p.env, prog, xin + tid * ldx, dn, vl, hh);
        for (int c = 0; c < C; ++c) PARG(st_h)[(sb + tid) * C + c] = hh[c];
        PARG(st_r)[sb + tid] = rew[tid];
        PARG(st_dv)[sb + tid] = (uint8_t)((dn ? 1 : 0) | (vl ? 2 : 0));
        in_r = true;
      }
      const uint64_t mk = __ballot(in_r);
      if (in_r) PARG(inv)[((size_t)t * PARG(ntiles) + tile) * ROWS + __popcll(mk & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) PARG(cnt)[(size_t)t * PARG(ntiles) + tile] = __popcll(mk);
      const uint64_t still = __ballot(in_r && !dn);
      if (tid < ROWS) alive_nxt[tid] = in_r && !dn;
      if (tid == 0) *s_nalive = __popcll(still);
    } else if (tid < NT / 2) {
      constexpr int NS = NT / 2 - 64;
      const int ts = tid - 64;
      for (int e = ts; e < ROWS * S; e += NS) {
        const int r = e / S, k = e - r * S;
        const float x = xin[r * ldx + k];
        if (alive_cur[r]) {
          PARG(st_s)[(sb + r) * S + k] = sraw[r * ldss + k];
          PARG(st_s2)[(sb + r) * S + k] = x;
        }
        sraw[r * ldss + k] = x;   // same element, same thread
      }
      for (int e = ts; e < nrows * A; e += NS) {
        const int r = e / A, d = e - r * A;
        if (alive_cur[r]) PARG(st_a)[(sb + r) * A + d] = act[r * 8 + d];
      }
    } else if (t + 1 < PARG(H)) {
      if constexpr (GA)
        persist_noise<ROWS, true>(PARG(eps_a), PARG(eps_m), PARG(seed), PARG(ctr), A, S1, B, t + 1, row0, nrows, nz_a,
                                  nz_m, NT / 2, NT / 2, PARG(given), PARG(n_given));
      else
      persist_noise<ROWS>(PARG(eps_a), PARG(eps_m), PARG(seed), PARG(ctr), A, S1, B, t + 1, row0, nrows, nz_a, nz_m, NT / 2, NT / 2);
    }
    lds_barrier();
    if (t == 2) RSTAMP(9);
    const int n_alive = __builtin_amdgcn_readfirstlane(*s_nalive);   // uniform exit
    if (n_alive == 0) {   // the whole tile finished: later steps see no rows from it
      for (int t2 = t + 1 + tid; t2 < PARG(H); t2 += NT) PARG(cnt)[(size_t)t2 * PARG(ntiles) + tile] = 0;
      break;
    }
  }
}

#undef MW
#undef MB
#undef PERSIST_LDS_LAYOUT

// One family of the horizon kernel, the 12 instantiations RB x LW x PM x PG of a (GA, SH):
// the launch is written here, so a family's kernels exist in the one object that
// instantiates this template. rpt: rows per tile (32: RB = 2, else 1); lw: the LDS-resident
// actor weights (16-row tiles only); lds_bytes: everything the launch needs.
// 8-wave workgroups (16 waves measured 3.5 % slower at config 2, profiles/r02/rollout_ab)
template <bool GA, bool SH>
static void launch_persist_family(int rpt, bool lw, bool paired, bool pg, const PersistArgs& a, size_t lds_bytes,
                                  hipStream_t stream) {
  auto launch = [&](auto rb, auto lwc) {
    constexpr int RB = decltype(rb)::value;
    constexpr bool LW = decltype(lwc)::value;
    auto k = paired ? (pg ? rollout_persist_kernel<RB, 8, LW, 1, true, GA, SH>
                          : rollout_persist_kernel<RB, 8, LW, 1, false, GA, SH>)
                    : (pg ? rollout_persist_kernel<RB, 8, LW, 0, true, GA, SH>
                          : rollout_persist_kernel<RB, 8, LW, 0, false, GA, SH>);
    k<<<a.ntiles, 8 * 64, lds_bytes, stream>>>(a);
  };
  if (rpt == 32) launch(std::integral_constant<int, 2>{}, std::false_type{});
  else if (lw) launch(std::integral_constant<int, 1>{}, std::true_type{});
  else launch(std::integral_constant<int, 1>{}, std::false_type{});
}

// The families compiled outside rollout.hip, one object each: launch_persist_family<true, false>
// (rollout_given.hip), <false, true> (rollout_shield.hip) and <true, true>
// (rollout_proposed.hip). Plain host functions, hidden by -fvisibility=hidden like every
// symbol without DRPO_API; persist_run (rollout.hip) selects among them and its own
// launch_persist_family<false, false>.
void launch_persist_given(int rpt, bool lw, bool paired, bool pg, const PersistArgs& a, size_t lds_bytes,
                          hipStream_t stream);
void launch_persist_shield(int rpt, bool lw, bool paired, bool pg, const PersistArgs& a, size_t lds_bytes,
                           hipStream_t stream);
void launch_persist_proposed(int rpt, bool lw, bool paired, bool pg, const PersistArgs& a, size_t lds_bytes,
                             hipStream_t stream);

