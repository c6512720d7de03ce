// Imagined model rollouts (SMBPO.rollout, src/smbpo.py:229-249): two engines behind
// drpo_rollout, and the replay sampler they share.
//
// Both engines give each 512-thread workgroup (8 wave64s, 2 per SIMD) a 16- or 32-row
// tile whose activations stay in LDS while it runs
//   actor MLP S->H->H->2A (ReLU)  +  squashed-Gaussian sample   (src/policy.py:89-97)
//   elite member MLP trunk/diff/log-var heads (SiLU) + log-var clamp + Gaussian
//   sample                                                      (src/dynamics.py:112-122,198-203)
//   env constraint functions or a constraint program            (env_constraints.hpp)
// and both write the 7-component rows into the circular virtual buffer
// (src/sampling.py:128-145) in the reference's order: step-major, surviving rows in
// batch order. Row counts and buffer offsets live on the device, so a whole rollout
// needs no host synchronisation.
//
// Engine 1, rollout_step_kernel: the parity reference. One launch per horizon step over
// the alive rows. The launch performs the order-preserving `next_states[~dones]`
// compaction (src/smbpo.py:243-246) itself: each workgroup scans the previous step's
// tile counts and binary-searches the source row of each of its rows. It consumes
// recorded draws in the reference's compacted layout and keeps libm arithmetic.
//
// Engine 2, rollout_persist_kernel: production. One launch for all H steps, each
// workgroup keeping its tile for the whole horizon; surviving rows go to a staging area
// and one of two emit tails orders them into the buffer:
//   H x tiles <= EMIT_SELF_MAX   rollout_emit_self_kernel (count scan, emit and pointer
//                                advance in one launch)
//   larger                       rollout_scan_kernel + rollout_emit_kernel +
//                                rollout_persist_finalize_kernel
// drpo_rollout_trajectories runs the same kernel with rollout_traj_kernel as its tail: the
// staging read per original row (trajectory-major outputs and per-trajectory summaries,
// src/smbpo.py:229-249 with row identity kept), the virtual buffer untouched.
//
// The horizon kernel and what its instantiations need are in rollout_persist.hpp. Its 48
// instantiations are four families of 12, one object each: the plain family here, the given
// actions (GA), shield (SH) and proposals (GA && SH) families in rollout_given.hip,
// rollout_shield.hip and rollout_proposed.hip, which hold nothing but their family's launch.
// This file keeps the rest: the step engine, the tails, the cut and recount kernels, the
// workspace, every check and every entry point (persist_run selects the family), and the
// PRP sampler.
#include <hip/hip_runtime.h>

#ifdef DRPO_STAMPS
// profiling builds only (profiles/stamps.py): the stamps of this object's kernels (see
// RSTAMP in rollout_persist.hpp) and their reader, defined in this object alone
#define DRPO_ROLLOUT_STAMPS_HERE 1
__device__ unsigned long long g_stamps_roll[1 << 14][16];
extern "C" __attribute__((visibility("default"))) int drpo_debug_stamps_rollout(unsigned long long* dst, int n) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps_roll), sizeof(unsigned long long) * 16 * (size_t)n);
}
#endif

#include "rollout_persist.hpp"

struct RolloutStepArgs {
  int S, A, C, Ha, Hm, t, Bmax;
  EnvParams env;
  // actor (row-major [out][in] weights)
  const float *aW1, *ab1, *aW2, *ab2, *aW3, *ab3;
  // elite member slices of the ensemble
  const float *mW1, *mb1, *mW2, *mb2, *dW1, *db1, *dW2, *db2, *lW1, *lb1, *lW2, *lb2;
  const float *norm_mean, *norm_std, *min_lv, *max_lv;
  // step-0 source: replay buffer states (physical layout) + chronological indices
  const float* replay_states;
  const int64_t* init_idx;        // nullptr -> device PRP sample without replacement
  int64_t replay_len, replay_ptr, replay_cap;
  uint32_t prp_key[4];
  int prp_half_bits;
  // step t>0 source: previous step's next states + compaction map
  const float* prev_nxt;
  const int* prev_cnt;
  const int* prev_inv;
  // device step bookkeeping (n[t], off[t] written by workgroup 0 of step t)
  int* n;
  int64_t* off;
  // noise: parity mode (caller-provided eps rows for this step) or Philox
  const float* eps_a;             // [Bmax][A]
  const float* eps_m;             // [Bmax][S+1]
  uint64_t seed, ctr;
  // virtual buffer
  float *vs, *va, *vs2, *vr, *vh;
  uint8_t *vd, *vv;
  const int64_t* vptr;
  int64_t vcap;
  // this step's outputs for the next step
  float* nxt;
  int* cnt;
  int* inv;
  // LDS strides
  int ldx, ldh, ldm, lds;
  // env id 4: the constraint program (device memory; read by the PG instantiations only)
  const void* env_prog;
};

// PG: the constraint phase runs the program interpreter (env id 4) instead of the
// built-in functions: an instantiation of its own, so the built-in environments'
// kernels keep their code and registers
template <int RB, int NW, bool PG = false>
__global__ __launch_bounds__(NW * 64) void rollout_step_kernel(RolloutStepArgs p) {
  constexpr int ROWS = RB * 16;
  constexpr int NT = NW * 64;                   // 2 waves per SIMD at NW = 8
  constexpr int MAXC = (16 + NW - 1) / NW;      // column blocks per wave for widths <= 256
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int S = p.S, A = p.A, C = p.C, S1 = p.S + 1;

  float* xin = smem;                       // ROWS x ldx  actor in / model in / next states
  float* h1 = xin + ROWS * p.ldx;          // ROWS x ldh
  float* h2 = h1 + ROWS * p.ldh;           // ROWS x ldh
  float* h3 = h2 + ROWS * p.ldh;           // ROWS x ldh  (log-var head hidden)
  float* sraw = h3 + ROWS * p.ldh;         // ROWS x lds  raw states
  float* ao = sraw + ROWS * p.lds;         // ROWS x 20   actor head
  float* dout = ao + ROWS * 20;            // ROWS x ldm  diff head
  float* lout = dout + ROWS * p.ldm;       // ROWS x ldm  log-var head
  float* act = lout + ROWS * p.ldm;        // ROWS x 8    sampled actions
  float* rew = act + ROWS * 8;             // ROWS
  float* hval = rew + ROWS;                // ROWS x 8    constraint values
  int* flags = reinterpret_cast<int*>(hval + ROWS * 8);   // ROWS: bit0 done, bit1 violation
  int* srcrow = flags + ROWS;                              // ROWS
  float* red = reinterpret_cast<float*>(srcrow + ROWS);    // NW*RB*256 narrow-layer partials
  int* s_part = reinterpret_cast<int*>(red + NW * RB * 256);   // NT scan partials
  int* scan = s_part + NT;                                 // prev tiles + 1 (exclusive prefix)
  float* vecs = reinterpret_cast<float*>(scan + ((p.Bmax + ROWS - 1) / ROWS) + 1);   // 4 x 64: small vectors
  float* v_nm = vecs;            // normalizer mean
  float* v_ns = vecs + 64;       // normalizer std + 1e-6
  float* v_lo = vecs + 128;      // min_log_var
  float* v_hi = vecs + 192;      // max_log_var
  preload_vecs(p, v_nm, v_ns, v_lo, v_hi);

  RSTAMP(0);
  // ---- 0. row count / buffer offset of this step + compaction map ----------
  int n;
  int64_t off;
  const int row0 = blockIdx.x * ROWS;
  if (p.t == 0) {
    n = p.Bmax;
    off = 0;
  } else {
    const int n_prev = p.n[p.t - 1];
    const int T = (n_prev + ROWS - 1) / ROWS;
    // exclusive scan of the previous step's tile counts (T <= ntiles), NT threads
    const int per = (T + NT - 1) / NT;
    const int b0 = tid * per;
    int run = 0;
    for (int i = 0; i < per; ++i) {
      const int ti = b0 + i;
      if (ti < T) {
        scan[ti] = run;
        run += p.prev_cnt[ti];
      }
    }
    const int base = block_exclusive_scan<NT>(run, s_part, n);   // total alive == n for this step
    for (int i = 0; i < per; ++i) {
      const int ti = b0 + i;
      if (ti < T) scan[ti] += base;
    }
    __syncthreads();
    off = p.off[p.t - 1] + n_prev;
    if (tid < ROWS && row0 + tid < n) {   // binary search: last tile with scan[tile] <= i
      const int i = row0 + tid;
      int lo = 0, hi = T - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scan[mid] <= i) lo = mid; else hi = mid - 1;
      }
      srcrow[tid] = lo * ROWS + p.prev_inv[lo * ROWS + (i - scan[lo])];
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    p.n[p.t] = n;
    p.off[p.t] = off;
  }
  if (row0 >= n) return;
  const int rows = min(ROWS, n - row0);
  const int64_t vbase = *p.vptr + off + row0;
  __syncthreads();

  // ---- 1. gather the tile's states (zero-padded) ---------------------------
  const int kpad = round_up(S + A, 16);
  for (int e = tid; e < ROWS * kpad; e += NT) {
    const int r = e / kpad, k = e - r * kpad;
    float v = 0.f;
    if (r < rows && k < S)
      v = p.t == 0 ? p.replay_states[replay_row(p, row0 + r) * S + k] : p.prev_nxt[(int64_t)srcrow[r] * S + k];
    xin[r * p.ldx + k] = v;
    if (k < S) sraw[r * p.lds + k] = v;
  }
  __syncthreads();

  RSTAMP(1);
  // ---- 2. actor MLP (src/policy.py:61-100; mlp() ReLU hidden) ---------------
  tile_dense<NW, RB, MAXC, ACT_RELU>(xin, p.ldx, S, p.aW1, p.ab1, p.Ha, h1, p.ldh);
  __syncthreads();
  RSTAMP(2);
  tile_dense<NW, RB, MAXC, ACT_RELU>(h1, p.ldh, p.Ha, p.aW2, p.ab2, p.Ha, h2, p.ldh);
  __syncthreads();
  RSTAMP(3);
  tile_dense_narrow<NW, RB, ACT_NONE>(h2, p.ldh, p.Ha, p.aW3, p.ab3, 2 * A, ao, 20, red);
  __syncthreads();
  RSTAMP(4);

  // ---- 3. squashed Gaussian sample + model input [normalize(s), a] ----------
  for (int e = tid; e < ROWS * A; e += NT) {
    const int r = e / A, d = e - r * A;
    const float mu = ao[r * 20 + d], raw = ao[r * 20 + A + d];
    const float ls = -6.f + 10.f * sigmoidf(raw);
    const float sd = expf(ls) * 1.0f;
    float eps;
    if (p.eps_a) {
      eps = (r < rows) ? p.eps_a[(int64_t)(row0 + r) * A + d] : 0.f;
    } else {
      float z[4];
      philox_normal4(p.seed, (uint32_t)(row0 + r), ((uint32_t)p.t << 8) | 0u, (uint32_t)(d >> 2), (uint32_t)p.ctr, z);
      eps = z[d & 3];
    }
    const float a = tanhf(eps * sd + mu);
    act[r * 8 + d] = a;
    xin[r * p.ldx + S + d] = a;
  }
  for (int e = tid; e < ROWS * S; e += NT) {
    const int r = e / S, k = e - r * S;
    xin[r * p.ldx + k] = (sraw[r * p.lds + k] - v_nm[k]) / v_ns[k];
  }
  __syncthreads();

  RSTAMP(5);
  // ---- 4. elite member forward (src/dynamics.py:112-122, swish) -------------
  tile_dense<NW, RB, MAXC, ACT_SILU>(xin, p.ldx, S + A, p.mW1, p.mb1, p.Hm, h1, p.ldh);
  __syncthreads();
  RSTAMP(6);
  tile_dense<NW, RB, MAXC, ACT_SILU>(h1, p.ldh, p.Hm, p.mW2, p.mb2, p.Hm, h2, p.ldh);
  __syncthreads();
  RSTAMP(7);
  if (S1 <= 16 && p.Hm == 200) {
    // diff and log-var heads side by side: one fused hidden layer (2 x 13 column
    // blocks, 4 per wave) and one fused split-K output layer
    tile_dense_pair<NW, RB, (26 + NW - 1) / NW, ACT_SILU, 13>(h2, p.ldh, p.Hm, p.dW1, p.db1, p.Hm, h1, p.lW1,
                                                               p.lb1, p.Hm, h3, p.ldh);
    __syncthreads();
    RSTAMP(8);
    RSTAMP(9);
    tile_dense_narrow_pair<NW, RB, ACT_NONE>(h1, h3, p.ldh, p.Hm, p.dW2, p.db2, S1, dout, p.lW2, p.lb2, S1, lout,
                                             p.ldm, red);
    __syncthreads();
    RSTAMP(10);
    RSTAMP(11);
  } else {
    tile_dense<NW, RB, MAXC, ACT_SILU>(h2, p.ldh, p.Hm, p.dW1, p.db1, p.Hm, h1, p.ldh);
    __syncthreads();
    RSTAMP(8);
    if (S1 <= 16) tile_dense_narrow<NW, RB, ACT_NONE>(h1, p.ldh, p.Hm, p.dW2, p.db2, S1, dout, p.ldm, red);
    else tile_dense<NW, RB, MAXC, ACT_NONE>(h1, p.ldh, p.Hm, p.dW2, p.db2, S1, dout, p.ldm);
    __syncthreads();
    RSTAMP(9);
    tile_dense<NW, RB, MAXC, ACT_SILU>(h2, p.ldh, p.Hm, p.lW1, p.lb1, p.Hm, h1, p.ldh);
    __syncthreads();
    RSTAMP(10);
    if (S1 <= 16) tile_dense_narrow<NW, RB, ACT_NONE>(h1, p.ldh, p.Hm, p.lW2, p.lb2, S1, lout, p.ldm, red);
    else tile_dense<NW, RB, MAXC, ACT_NONE>(h1, p.ldh, p.Hm, p.lW2, p.lb2, S1, lout, p.ldm);
    __syncthreads();
    RSTAMP(11);
  }

  // ---- 5. residual mean, log-var soft clamp, Gaussian sample ---------------
  for (int e = tid; e < ROWS * S1; e += NT) {
    const int r = e / S1, j = e - r * S1;
    const float mean = dout[r * p.ldm + j] + (j < S ? sraw[r * p.lds + j] : 0.f);
    float lv = lout[r * p.ldm + j];
    lv = v_hi[j] - softplusf(v_hi[j] - lv);
    lv = v_lo[j] + softplusf(lv - v_lo[j]);
    const float sd = sqrtf(expf(lv));
    float eps;
    if (p.eps_m) {
      eps = (r < rows) ? p.eps_m[(int64_t)(row0 + r) * S1 + j] : 0.f;
    } else {
      float z[4];
      philox_normal4(p.seed, (uint32_t)(row0 + r), ((uint32_t)p.t << 8) | 1u, (uint32_t)(j >> 2), (uint32_t)p.ctr, z);
      eps = z[j & 3];
    }
    const float x = mean + sd * eps;
    if (j < S) xin[r * p.ldx + j] = x;
    else rew[r] = x;
  }
  __syncthreads();

  RSTAMP(12);
  // ---- 6. constraints + in-tile compaction ranks ---------------------------
  if (tid < 64) {
    bool alive_r = false;
    if (tid < rows) {
      bool dn, vl;
      float hh[8];
      constraint_row<PG>(p.env, p.env_prog, xin + tid * p.ldx, dn, vl, hh);
      for (int c = 0; c < C; ++c) hval[tid * 8 + c] = hh[c];
      flags[tid] = (dn ? 1 : 0) | (vl ? 2 : 0);
      alive_r = !dn;
    }
    const uint64_t m = __ballot(alive_r);
    if (alive_r) p.inv[row0 + __popcll(m & ((1ull << tid) - 1ull))] = tid;   // k-th alive row of the tile
    if (tid == 0) p.cnt[blockIdx.x] = __popcll(m);
  }
  __syncthreads();

  RSTAMP(13);
  // ---- 7. row writes into the circular virtual buffer + next-state scratch --
  int64_t* qrow = reinterpret_cast<int64_t*>(red);           // ROWS physical buffer rows (red is free now)
  if (tid < rows) qrow[tid] = (vbase + tid) % p.vcap;
  __syncthreads();
  for (int e = tid; e < rows * S; e += NT) {
    const int r = e / S, k = e - r * S;
    const int64_t q = qrow[r];
    p.vs[q * S + k] = sraw[r * p.lds + k];
    const float x = xin[r * p.ldx + k];
    p.vs2[q * S + k] = x;
    p.nxt[(int64_t)(row0 + r) * S + k] = x;
  }
  for (int e = tid; e < rows * A; e += NT) {
    const int r = e / A, d = e - r * A;
    p.va[qrow[r] * A + d] = act[r * 8 + d];
  }
  for (int e = tid; e < rows * C; e += NT) {
    const int r = e / C, c = e - r * C;
    p.vh[qrow[r] * C + c] = hval[r * 8 + c];
  }
  if (tid < rows) {
    const int64_t q = qrow[tid];
    p.vr[q] = rew[tid];
    p.vd[q] = flags[tid] & 1;
    p.vv[q] = (flags[tid] >> 1) & 1;
  }
  RSTAMP(14);
}

// total rows written = off[H-1] + n[H-1]; advance the buffer pointer
__global__ void rollout_finalize_kernel(int64_t* vptr, const int* n, int64_t* off, int H) {
  const int64_t total = off[H - 1] + n[H - 1];
  off[H] = total;
  *vptr += total;
}

// per step t: exclusive prefix of the tile counts -> pos[t][tile], n[t]
__global__ __launch_bounds__(256) void rollout_scan_kernel(const int* __restrict__ cnt, int* __restrict__ pos,
                                                           int* __restrict__ n, int ntiles) {
  __shared__ int part[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int* c = cnt + (size_t)t * ntiles;
  int* ps = pos + (size_t)t * ntiles;
  const int per = (ntiles + 255) / 256, b0 = tid * per;
  int run = 0;
  for (int i = 0; i < per; ++i)
    if (b0 + i < ntiles) run += c[b0 + i];
  int total;
  int e = block_exclusive_scan<256>(run, part, total);
  if (tid == 0) n[t] = total;
  for (int i = 0; i < per; ++i)
    if (b0 + i < ntiles) { ps[b0 + i] = e; e += c[b0 + i]; }
}

// the circular virtual buffer's seven components and its capacity in rows
struct EmitDst {
  float *vs, *va, *vs2, *vr, *vh;
  uint8_t *vd, *vv;
  int64_t vcap;
};

// staged row src -> buffer row q. The destinations are restrict parameters (a struct's
// members cannot say so): the row's loads need not wait for its stores.
__device__ __forceinline__ void emit_row(const PersistArgs& p, size_t src, int64_t q, float* __restrict__ vs,
                                         float* __restrict__ va, float* __restrict__ vs2, float* __restrict__ vr,
                                         float* __restrict__ vh, uint8_t* __restrict__ vd, uint8_t* __restrict__ vv) {
  const int S = p.S, A = p.A, C = p.C;
  for (int j = 0; j < S; ++j) {
    vs[q * S + j] = p.st_s[src * S + j];
    vs2[q * S + j] = p.st_s2[src * S + j];
  }
  for (int d = 0; d < A; ++d) va[q * A + d] = p.st_a[src * A + d];
  for (int c = 0; c < C; ++c) vh[q * C + c] = p.st_h[src * C + c];
  vr[q] = p.st_r[src];
  const uint8_t dv = p.st_dv[src];
  vd[q] = dv & 1;
  vv[q] = (dv >> 1) & 1;
}

// staged row src -> buffer row pos (mod capacity)
__device__ __forceinline__ void emit_row(const PersistArgs& p, const EmitDst& o, size_t src, int64_t pos) {
  emit_row(p, src, pos % o.vcap, o.vs, o.va, o.vs2, o.vr, o.vh, o.vd, o.vv);
}

// staged rows -> circular virtual buffer, in the reference's order
template <int ROWS>
__global__ __launch_bounds__(256) void rollout_emit_kernel(PersistArgs p, const int* __restrict__ pos,
                                                           const int* __restrict__ n, const int64_t* __restrict__ vptr,
                                                           EmitDst dst) {
  __shared__ int64_t s_off;
  const int t = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    int64_t o = 0;
    for (int u = 0; u < t; ++u) o += n[u];
    s_off = o + *vptr;
  }
  __syncthreads();
  const int slot = blockIdx.x * 256 + tid;
  const int tile = slot / ROWS, k = slot - tile * ROWS;
  if (tile >= p.ntiles) return;
  const size_t ti = (size_t)t * p.ntiles + tile;
  if (k >= p.cnt[ti]) return;
  emit_row(p, dst, (size_t)t * p.B + (size_t)tile * ROWS + p.inv[ti * ROWS + k], s_off + pos[ti] + k);
}

// Small rollouts (H x tiles <= EMIT_SELF_MAX counts): count scan, ordered emit and
// pointer advance in ONE launch. Every workgroup reads the whole [H][ntiles] count
// array (<= 32 KB, L2-resident: the persist kernel just wrote it) and reduces it to
// its own flat prefix (all rows of steps < t, and of tiles before its first tile at
// step t) and the total, so no workgroup waits on another. The buffer pointer was
// copied into base_slot by rollout_persist_kernel, so the one workgroup that advances
// *vptr races with no reader.
constexpr int EMIT_SELF_MAX = 8192;
template <int ROWS>
__global__ __launch_bounds__(256) void rollout_emit_self_kernel(PersistArgs p, const int64_t* __restrict__ base_slot,
                                                                int64_t* __restrict__ vptr, int64_t* __restrict__ off,
                                                                EmitDst dst) {
  constexpr int TPB = 256 / ROWS;   // tiles per workgroup
  __shared__ int s_pre[4], s_tot[4], s_loc[TPB];
  const int t = blockIdx.y, tid = threadIdx.x;
  const int tile0 = blockIdx.x * TPB;
  const int nflat = p.H * p.ntiles, P = t * p.ntiles + tile0;
  const int* __restrict__ cnt = p.cnt;
  int pre = 0, tot = 0;
  for (int i = tid; i < nflat; i += 256) {
    const int c = cnt[i];
    tot += c;
    pre += i < P ? c : 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    pre += __shfl_xor(pre, o, 64);
    tot += __shfl_xor(tot, o, 64);
  }
  if ((tid & 63) == 0) { s_pre[tid >> 6] = pre; s_tot[tid >> 6] = tot; }
  if (tid < TPB) s_loc[tid] = tile0 + tid < p.ntiles ? cnt[(size_t)t * p.ntiles + tile0 + tid] : 0;
  __syncthreads();
  pre = s_pre[0] + s_pre[1] + s_pre[2] + s_pre[3];
  tot = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
  const int64_t base = *base_slot;
  if (t == p.H - 1 && blockIdx.x == gridDim.x - 1 && tid == 0) {
    off[p.H] = tot;
    *vptr = base + tot;
  }
  const int j = tid / ROWS, k = tid - j * ROWS, tile = tile0 + j;
  if (tile >= p.ntiles || k >= s_loc[j]) return;
  int loc = 0;
  for (int u = 0; u < j; ++u) loc += s_loc[u];
  const size_t ti = (size_t)t * p.ntiles + tile;
  emit_row(p, dst, (size_t)t * p.B + (size_t)tile * ROWS + p.inv[ti * ROWS + k], base + pre + loc + k);
}

// off[t] = sum n[<t], off[H] = total; advance the buffer pointer
__global__ void rollout_persist_finalize_kernel(int64_t* vptr, const int* n, int64_t* off, int H) {
  int64_t o = 0;
  for (int t = 0; t < H; ++t) {
    off[t] = o;
    o += n[t];
  }
  off[H] = o;
  *vptr += o;
}

// ---------------------------------------------------------------------------
// The trajectory tail (drpo_rollout_trajectories): runs after rollout_persist_kernel in
// place of the ordered emit and reads the same staging trajectory-major. A row was
// staged at step t exactly when it was alive at t, so a row's done bits say how far its
// staging reaches; nothing is read beyond that (a tile that empties leaves the horizon
// loop, so later steps were never written).
//
// One workgroup per TRAJ_ROWS original rows, two phases:
//  A. one lane per row walks the row's done bits (the only dependent chain: one load per
//     step), and handles what is one value per (row, step) on the way: rewards, dones,
//     violations, the return, first violation, terminated, length.
//  B. one lane per (row, k) element of the states, actions and constraint values, each
//     looping over the steps of its element with the lengths known (independent loads).
//     At a fixed step adjacent lanes read adjacent staging addresses (coalesced reads);
//     each lane writes one float per step into its row's own block, so a row's S floats
//     of a step form one segment and the segments of a row fill whole lines over the
//     loop. The constraint lanes keep the running maximum: no atomics.
// Every element of every output given is written (zero at or beyond the length).
// ---------------------------------------------------------------------------
constexpr int TRAJ_ROWS = 16;   // rows x (S + A + C) ~ one 256-lane pass at quadrotor dims; B 4096 -> 256 workgroups
constexpr int TRAJ_NT = 256;

struct TrajArgs {
  int S, A, C, B, H;
  const float *st_s, *st_s2, *st_a, *st_r, *st_h;   // staging [t][original row], real widths A and C
  const uint8_t* st_dv;
  drpo_rollout_traj_t out;
  const int* newlen;   // [B] or nullptr: row i keeps its first newlen[i] <= its natural length steps (rollout_cut_kernel)
};

// the weights are wave-uniform data no kernel writes: read like the constraint programs
typedef const __attribute__((address_space(4))) double* TrajWeightsK;

// n >= 1 steps of one element: dst[t * ds] = src[t * ss] (dst may be null), four loads in
// flight at a time; restrict parameters (a struct's members cannot say so), so the loads
// need not wait for earlier stores. MAX: returns the maximum the way numpy does (a NaN stays).
template <bool MAX>
__device__ __forceinline__ float traj_steps(const float* __restrict__ src, size_t ss, float* __restrict__ dst,
                                            size_t ds, int n) {
  float m = MAX ? src[0] : 0.f;
  int t = 0;
  for (; t + 4 <= n; t += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[(size_t)(t + u) * ss];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (dst) dst[(size_t)(t + u) * ds] = v[u];
      if (MAX) m = (v[u] > m || v[u] != v[u]) ? v[u] : m;
    }
  }
  for (; t < n; ++t) {
    const float v = src[(size_t)t * ss];
    if (dst) dst[(size_t)t * ds] = v;
    if (MAX) m = (v > m || v != v) ? v : m;
  }
  return m;
}

__global__ __launch_bounds__(TRAJ_NT) void rollout_traj_kernel(TrajArgs p) {
  __shared__ int s_len[TRAJ_ROWS];
  const int tid = threadIdx.x;
  const int S = p.S, A = p.A, C = p.C, H = p.H;
  const size_t B = (size_t)p.B;
  const int row0 = blockIdx.x * TRAJ_ROWS;
  const int nr = min(TRAJ_ROWS, p.B - row0);
  const drpo_rollout_traj_t& o = p.out;

  // ---- A. length walk + the per-(row, step) scalars and the summaries ---------
  if (tid < TRAJ_ROWS) {
    int len = 0;
    if (tid < nr) {
      const size_t i = (size_t)row0 + tid;
      TrajWeightsK w = (TrajWeightsK)(uintptr_t)o.weights;
      int fv = -1;
      unsigned last = 0;
      double acc = 0.0;
      // a cut row (newlen < its natural length) ends alive: last keeps a clear done bit
      const int lim = p.newlen ? min(max(p.newlen[i], 0), H) : H;
      for (int t = 0; t < lim; ++t) {
        const size_t src = (size_t)t * B + i;
        const unsigned dv = p.st_dv[src];
        const float r = p.st_r[src];
        if (o.rewards) o.rewards[i * H + t] = r;
        if (o.dones) o.dones[i * H + t] = dv & 1;
        if (o.violations) o.violations[i * H + t] = (dv >> 1) & 1;
        if (o.ret) acc = __dadd_rn(acc, __dmul_rn(w[t], (double)r));
        if ((dv & 2) && fv < 0) fv = t;
        last = dv;
        len = t + 1;
        if (dv & 1) break;
      }
      for (int t = len; t < H; ++t) {
        if (o.rewards) o.rewards[i * H + t] = 0.f;
        if (o.dones) o.dones[i * H + t] = 0;
        if (o.violations) o.violations[i * H + t] = 0;
      }
      o.len[i] = len;
      if (o.ret) o.ret[i] = (float)acc;
      if (o.first_violation) o.first_violation[i] = fv;
      if (o.terminated) o.terminated[i] = last & 1;
    }
    s_len[tid] = len;
  }
  __syncthreads();

  // ---- B. the [row][step][k] arrays, one lane per (row, k) ---------------------
  const int nS = o.states ? nr * S : 0;
  const int nA = o.actions ? nr * A : 0;
  const int nC = (o.constraint_values || o.hmax) ? nr * C : 0;
  for (int e = tid; e < nS + nA + nC; e += TRAJ_NT) {
    if (e < nS) {
      const int r = e / S, k = e - r * S, len = s_len[r];
      const size_t i = (size_t)row0 + r;
      float* dst = o.states + i * (H + 1) * S + k;
      traj_steps<false>(p.st_s + i * S + k, B * S, dst, S, len);
      // length 0 (a row cut at its first step): the start state, which step 0 staged
      dst[(size_t)len * S] = len > 0 ? p.st_s2[((size_t)(len - 1) * B + i) * S + k] : p.st_s[i * S + k];
      for (int t = len + 1; t <= H; ++t) dst[(size_t)t * S] = 0.f;
    } else if (e < nS + nA) {
      const int q = e - nS, r = q / A, d = q - r * A, len = s_len[r];
      const size_t i = (size_t)row0 + r;
      float* dst = o.actions + i * H * A + d;
      traj_steps<false>(p.st_a + i * A + d, B * A, dst, A, len);
      for (int t = len; t < H; ++t) dst[(size_t)t * A] = 0.f;
    } else {
      const int q = e - nS - nA, r = q / C, c = q - r * C, len = s_len[r];
      const size_t i = (size_t)row0 + r;
      float* dst = o.constraint_values ? o.constraint_values + i * H * C + c : nullptr;
      const float m = len > 0 ? traj_steps<true>(p.st_h + i * C + c, B * C, dst, C, len) : -INFINITY;   // max's identity
      if (dst)
        for (int t = len; t < H; ++t) dst[(size_t)t * C] = 0.f;
      if (o.hmax) o.hmax[i * C + c] = m;
    }
  }
}

// ---------------------------------------------------------------------------
// Halting (drpo_rollout_emit_cut, drpo_rollout_trajectories_cut): a post-pass on the
// staged horizon. Row i is cut at the first step t of its life whose score is not
// <= thr (a NaN cuts, a score equal to thr does not); steps t >= the cut do not exist.
// Neither kernel makes a draw or touches the staged rows themselves.
// ---------------------------------------------------------------------------

// One lane per original row: walks the row's done bits as phase A of rollout_traj_kernel
// does (a row was staged at t exactly when it was alive at t) and its scores, which the
// caller lays out by a row and a step stride in elements. Scores at or beyond the row's
// length are never read. newlen[i]: the cut if there is one, else the natural length.
// Both walks load four steps at a time: the loads of a group do not wait for one another
// (one load per step in a chain measured 10.5 us for cut + recount at B 4096, H 10).
__global__ __launch_bounds__(256) void rollout_cut_kernel(const uint8_t* __restrict__ st_dv,
                                                          const float* __restrict__ scores, int64_t row_stride,
                                                          int64_t step_stride, float thr, int B, int H,
                                                          int* __restrict__ newlen, int* __restrict__ halted_at) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  // the natural length: the first done bit. Every [t][i] slot with t < H lies inside the
  // staging; those behind the first done bit were never staged and are not looked at.
  int len = -1;
  for (int t0 = 0; t0 < H && len < 0; t0 += 4) {
    unsigned dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) dv[u] = t0 + u < H ? st_dv[(int64_t)(t0 + u) * B + i] : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (len < 0 && (dv[u] & 1)) len = t0 + u + 1;
  }
  if (len < 0) len = H;   // cut by the horizon
  // the first score of the row's life that is not <= thr (thr itself stands in beyond it)
  int cut = -1;
  for (int t0 = 0; t0 < len && cut < 0; t0 += 4) {
    float sc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) sc[u] = t0 + u < len ? scores[i * row_stride + (int64_t)(t0 + u) * step_stride] : thr;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (cut < 0 && !(sc[u] <= thr)) cut = t0 + u;
  }
  newlen[i] = cut >= 0 ? cut : len;
  if (halted_at) halted_at[i] = cut;
}

// One wave per (step, tile): the tile's list of rows alive at the step, filtered by
// t < newlen[row], order kept (ballot + prefix popcount), in place; the new count. A tile
// that had emptied keeps count 0. Counts and in-tile indices come back from memory and are
// clamped to the tile, so that a workspace that is not the staging of this shape gives
// wrong rows and never an access outside the tile's rows.
template <int ROWS>
__global__ __launch_bounds__(256) void rollout_recount_kernel(int* __restrict__ cnt, int* __restrict__ inv,
                                                              const int* __restrict__ newlen, int B, int H,
                                                              int ntiles) {
  const int lane = threadIdx.x & 63;
  const int64_t ti = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // t * ntiles + tile
  if (ti >= (int64_t)H * ntiles) return;                             // wave-uniform
  const int t = (int)(ti / ntiles), tile = (int)(ti - (int64_t)t * ntiles);
  const int c = min(max(cnt[ti], 0), ROWS);
  int r = 0;
  bool keep = false;
  if (lane < c) {
    r = min(max(inv[ti * ROWS + lane], 0), ROWS - 1);
    const int64_t row = (int64_t)tile * ROWS + r;
    keep = row < B && t < newlen[row];
  }
  const uint64_t mk = __ballot(keep);
  // every lane has read its entry before any lane writes: one wave, in lockstep
  if (keep) inv[ti * ROWS + __popcll(mk & ((1ull << lane) - 1ull))] = r;
  if (lane == 0) cnt[ti] = __popcll(mk);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The workspace, piece by piece (in this order, each 256-byte aligned).
struct RolloutWs {
  // step engine: double-buffered next states, per-tile alive counts, in-tile maps
  float* nxt[2];
  int* cnt[2];
  int* inv[2];
  // both engines: n[t] rows of step t; off[t] their buffer offset, off[H] the rows the
  // last call wrote, off[H + 1] the fused engine's copy of the buffer pointer
  int* n;
  int64_t* off;
  // fused engine: staging indexed [t][original row] (A, C <= 8 slots), per-(t, tile)
  // counts / in-tile maps / positions
  float *st_s, *st_s2, *st_a, *st_r, *st_h;
  uint8_t* st_dv;
  int *st_cnt, *st_inv, *pos;
  // halting: the rows' lengths after the cut (rollout_cut_kernel); last, so no other piece moves
  int* newlen;
};

// Carves the workspace at `base` (0: the pieces' byte offsets); returns its size in bytes.
static size_t rollout_ws(int B, int S, int H, uintptr_t base, RolloutWs& w) {
  const size_t HB = (size_t)H * B, T16 = (size_t)B / 16 + 1;
  size_t o = 0;
  auto take = [&](auto*& piece, size_t bytes) {
    piece = reinterpret_cast<std::remove_reference_t<decltype(piece)>>(base + o);
    o += align256(bytes);
  };
  take(w.nxt[0], sizeof(float) * (size_t)B * S);
  take(w.nxt[1], sizeof(float) * (size_t)B * S);
  take(w.cnt[0], sizeof(int) * T16);
  take(w.cnt[1], sizeof(int) * T16);
  take(w.inv[0], sizeof(int) * (size_t)B);
  take(w.inv[1], sizeof(int) * (size_t)B);
  take(w.n, sizeof(int) * (size_t)(H + 1));
  take(w.off, sizeof(int64_t) * (size_t)(H + 2));
  take(w.st_s, sizeof(float) * HB * S);
  take(w.st_s2, sizeof(float) * HB * S);
  take(w.st_a, sizeof(float) * HB * 8);
  take(w.st_r, sizeof(float) * HB);
  take(w.st_h, sizeof(float) * HB * 8);
  take(w.st_dv, HB);
  take(w.st_cnt, sizeof(int) * (size_t)H * T16);
  take(w.st_inv, sizeof(int) * (size_t)H * (B + 32));
  take(w.pos, sizeof(int) * (size_t)H * T16);
  take(w.newlen, sizeof(int) * (size_t)B);
  return o;
}

DRPO_API size_t drpo_rollout_workspace_size(int B, int S, int H) {
  RolloutWs w;
  return rollout_ws(B, S, H, 0, w);
}

// Byte offset (inside the workspace) of the device int64 that holds the number of
// transitions written by the last drpo_rollout call (off[H]).
DRPO_API size_t drpo_rollout_count_offset(int B, int S, int H) {
  RolloutWs w;
  rollout_ws(B, S, H, 0, w);
  return (size_t)reinterpret_cast<uintptr_t>(w.off + H);
}

// Byte offsets (inside the workspace) of the fused engine's staged states [H][B][S] and
// actions [H][B][A] (step-major, original row; a row's step is staged iff the row was alive).
DRPO_API int drpo_rollout_staging_offsets(int B, int S, int H, size_t* st_s, size_t* st_a) {
  DRPO_REQUIRE(B >= 1 && S >= 1 && H >= 1 && st_s && st_a, "drpo_rollout_staging_offsets: B=%d S=%d H=%d or a null output",
               B, S, H);
  RolloutWs w;
  rollout_ws(B, S, H, 0, w);
  *st_s = (size_t)reinterpret_cast<uintptr_t>(w.st_s);
  *st_a = (size_t)reinterpret_cast<uintptr_t>(w.st_a);
  return DRPO_OK;
}

// The fields RolloutStepArgs and PersistArgs share, from the descriptor.
template <class Args>
static void fill_shared_args(Args& a, const drpo_rollout_desc_t* d, int64_t rlen) {
  const int S = d->S, A = d->A;
  a.S = S; a.A = A; a.C = d->C; a.Ha = d->Ha; a.Hm = d->Hm;
  a.env.id = d->env_id; a.env.surr_start = d->tracking_surr_start; a.env.n_surr = d->tracking_n_surr;
  a.env.thr0 = d->env_thr0; a.env.thr1 = d->env_thr1;
  a.aW1 = d->aW1; a.ab1 = d->ab1; a.aW2 = d->aW2; a.ab2 = d->ab2; a.aW3 = d->aW3; a.ab3 = d->ab3;
  a.norm_mean = d->norm_mean; a.norm_std = d->norm_std; a.min_lv = d->min_lv; a.max_lv = d->max_lv;
  a.replay_states = d->replay_states; a.init_idx = d->init_idx;
  a.replay_len = rlen; a.replay_ptr = d->replay_ptr; a.replay_cap = d->replay_cap;
  a.prp_half_bits = hb_for(rlen);
  prp_keys(d->seed, d->ctr, a.prp_key);
  a.seed = d->seed; a.ctr = d->ctr;
  a.ldx = lds_ld(S + A);
  a.ldh = lds_ld(d->Ha > d->Hm ? d->Ha : d->Hm);
  a.ldm = round_up(S + 1, 16) + 4;
  a.lds = round_up(S, 4);
  a.env_prog = d->env_id == DRPO_ENV_PROGRAM ? d->env_program : nullptr;
}

// LDS bytes of rollout_persist_kernel for `rpt`-row tiles (without the LDS-resident
// actor weights): per row xin, h1-h3, sraw, dout, lout, act, rew, nz_a, nz_m, flags,
// alive; then s_nalive, the split-K partials and the normalizer / log-var vectors.
// (Tracking, S = 51: 162.7 KB at 32-row tiles, inside the 160 KiB, so B >= 8192 runs
// 32-row tiles there too.)
static size_t persist_lds_bytes(int S, int A, int Ha, int Hm, int rpt, int nw) {
  const int S1 = S + 1;
  const int ldx = lds_ld(S + A), ldh = lds_ld(Ha > Hm ? Ha : Hm), ldm = round_up(S1, 16) + 4, ldss = round_up(S, 4);
  return sizeof(float) * ((size_t)rpt * (ldx + 3 * ldh + ldss + 2 * ldm + 8 + 1 + 8 + 64 + 2) + 4 +
                          (size_t)nw * (rpt / 16) * 256 + 256);
}

// The linear shield's share on top: a_perf and a_safe, [rpt][8] floats each.
static size_t persist_linear_lds_bytes(int rpt) { return sizeof(float) * (size_t)rpt * 16; }

// LDS bytes of rollout_step_kernel: per row xin, h1-h3, sraw, ao, dout, lout, act, rew,
// hval, flags, srcrow; then the split-K partials, the scan partials, the previous step's
// tile prefix and the normalizer / log-var vectors.
static size_t step_lds_bytes(int S, int A, int Ha, int Hm, int rpt, int nw, int tiles) {
  const int S1 = S + 1;
  const int ldx = lds_ld(S + A), ldh = lds_ld(Ha > Hm ? Ha : Hm), ldm = round_up(S1, 16) + 4, ldss = round_up(S, 4);
  return sizeof(float) * ((size_t)rpt * (ldx + 3 * ldh + ldss + 20 + 2 * ldm + 8 + 1 + 8 + 2) +
                          (size_t)nw * (rpt / 16) * 256 + nw * 64 + (size_t)tiles + 1 + 256);
}

// engine 2's horizon kernel for either tail (`who`: the entry point, for its messages).
// Fills `a`, which the tails read too. self_emit: the kernel copies the buffer pointer for
// rollout_emit_self_kernel; without it the kernel touches neither the buffer nor its pointer.
// given: actions for the first given->steps steps (nullptr or steps == 0: none).
// shield: the safety shield inside the step (checked by the caller). With given, the shield
// judges the given actions too (the GA && SH instantiations).
// linear: the shield is the linear one (with shield only; checked by the caller).
static int persist_run(const drpo_rollout_desc_t* d, const RolloutWs& w, int rpt, int64_t rlen, bool self_emit,
                       const char* who, hipStream_t stream, PersistArgs& a,
                       const drpo_rollout_given_t* given = nullptr, const drpo_rollout_shield_t* shield = nullptr,
                       const drpo_rollout_linear_t* linear = nullptr) {
  DRPO_REQUIRE(d->H <= PERSIST_MAX_H, "%s: engine 2 supports horizon <= %d", who, PERSIST_MAX_H);
  const int S = d->S, A = d->A, S1 = d->S + 1, B = d->B, H = d->H;
  fill_shared_args(a, d, rlen);
  a.B = B; a.H = H;
  a.ntiles = (B + rpt - 1) / rpt;
  a.mW1 = d->mW1; a.mb1 = d->mb1; a.mW2 = d->mW2; a.mb2 = d->mb2; a.dW1 = d->dW1; a.db1 = d->db1;
  a.dW2 = d->dW2; a.db2 = d->db2; a.lW1 = d->lW1; a.lb1 = d->lb1; a.lW2 = d->lW2; a.lb2 = d->lb2;
  a.ms_in = drpo_packed_size(S + A, d->Hm);
  a.ms_hid = drpo_packed_size(d->Hm, d->Hm);
  a.ms_out = drpo_packed_size(d->Hm, S1);
  a.eps_a = d->eps_a; a.eps_m = d->eps_m;
  a.st_s = w.st_s; a.st_s2 = w.st_s2; a.st_a = w.st_a; a.st_r = w.st_r; a.st_h = w.st_h; a.st_dv = w.st_dv;
  a.cnt = w.st_cnt; a.inv = w.st_inv;
  for (int t = 0; t < H; ++t) a.members[t] = d->members[t];
  if (given && given->steps > 0) {
    a.given = given->actions;
    a.n_given = given->steps;
  }
  // the critic's hidden activations share h1 - h3 with the actor's and the member's
  int Hw = d->Ha;
  if (shield) {
    const drpo_rollout_shield_t& s = *shield;
    a.sW1 = s.sW1; a.sb1 = s.sb1; a.sW2 = s.sW2; a.sb2 = s.sb2; a.sW3 = s.sW3; a.sb3 = s.sb3;
    a.cW1 = s.cW1; a.cb1 = s.cb1; a.cW2 = s.cW2; a.cb2 = s.cb2;
    a.qW1 = s.qW1; a.qb1 = s.qb1; a.qW2 = s.qW2; a.qb2 = s.qb2;
    a.zW1 = s.zW1; a.zb1 = s.zb1; a.zW2 = s.zW2; a.zb2 = s.zb2;
    a.Hc = s.Hc; a.Cq = s.Cq; a.sh_dist = s.distributional ? 1 : 0;
    a.sh_ratio = s.std_ratio; a.sh_lmin = s.log_std_min; a.sh_lmax = s.log_std_max; a.sh_thr = s.threshold;
    a.sh_iv = s.interventions; a.sh_cert = s.certificate;
    if (s.Hc > Hw) Hw = s.Hc;
    a.ldh = lds_ld(Hw > d->Hm ? Hw : d->Hm);
  }

  const size_t lds_bytes = persist_lds_bytes(S, A, Hw, d->Hm, rpt, 8);
  // the linear shield's a_perf / a_safe, behind everything else
  const size_t lin_bytes = linear ? persist_linear_lds_bytes(rpt) : 0;
  DRPO_REQUIRE(lds_bytes + lin_bytes <= 160 * 1024, "%s: LDS %zu too large", who, lds_bytes + lin_bytes);
  // LDS-resident actor weights (see rollout_persist_kernel) when they fit
  const size_t lw_bytes = sizeof(float) * (size_t)(32 + 16 * PERSIST_L2_LDS) * 256;
  // (not when every step's action is given: the actor never runs)
  const bool lw = rpt == 16 && S <= 16 && d->Ha == 256 && 2 * A <= 16 &&
                  lds_bytes + lw_bytes + lin_bytes <= 160 * 1024 && a.n_given < H;
  if (linear) {
    a.sh_lin_k = linear->candidates;
    a.sh_ab = (int)((lds_bytes + (lw ? lw_bytes : 0)) / sizeof(float));
    a.sh_blend = linear->blend;
  }
  const bool paired = S1 <= 16 && d->Hm == 200;   // the kernel's PM specialisation
  const bool pg = d->env_id == DRPO_ENV_PROGRAM;
  if (self_emit) {
    a.vptr_in = d->vptr;
    a.base_slot = w.off + H + 1;
  }
  if (shield) {
    // after every refusal: the kernel's rows write their own steps, zero at and beyond a
    // row's length comes from here
    const size_t BH = (size_t)B * H;
    if (shield->interventions) DRPO_CHECK_HIP(hipMemsetAsync(shield->interventions, 0, BH, stream));
    if (shield->certificate) DRPO_CHECK_HIP(hipMemsetAsync(shield->certificate, 0, BH * sizeof(float), stream));
    if (linear && linear->blend) DRPO_CHECK_HIP(hipMemsetAsync(linear->blend, 0, BH, stream));
  }
  if (d->step_events) hipEventRecord((hipEvent_t)d->step_events[0], stream);
  // a.cW1: the shield family; a.n_given > 0: the given-actions family; both: the proposals
  // family (each in its own object); neither: the plain family, instantiated here
  auto launch = a.cW1 ? (a.n_given > 0 ? launch_persist_proposed : launch_persist_shield)
                      : (a.n_given > 0 ? launch_persist_given : launch_persist_family<false, false>);
  launch(rpt, lw, paired, pg, a, lds_bytes + (lw ? lw_bytes : 0) + lin_bytes, stream);   // lw: 16-row tiles only
  DRPO_LAUNCH_CHECK("rollout_persist");
  if (d->step_events) hipEventRecord((hipEvent_t)d->step_events[1], stream);
  return DRPO_OK;
}

// which of the two emit tails a (horizon, tile count) takes
static bool emit_is_self(int H, int B, int rpt) { return (int64_t)H * ((B + rpt - 1) / rpt) <= EMIT_SELF_MAX; }

// The emit tail over the staging and counts `a` names: one launch for small rollouts (the
// horizon kernel has copied the buffer pointer into off[H + 1]), else scan + emit + finalize.
static int emit_tail(const drpo_rollout_desc_t* d, const RolloutWs& w, int rpt, const PersistArgs& a, bool self_emit,
                     hipStream_t stream) {
  const int H = d->H;
  const dim3 eg((unsigned)((a.ntiles * rpt + 255) / 256), (unsigned)H);
  const EmitDst dst{d->vs, d->va, d->vs2, d->vr, d->vh, d->vd, d->vv, d->vcap};
  if (self_emit) {
    auto k = rpt == 32 ? rollout_emit_self_kernel<32> : rollout_emit_self_kernel<16>;
    k<<<eg, 256, 0, stream>>>(a, w.off + H + 1, d->vptr, w.off, dst);
    DRPO_LAUNCH_CHECK("rollout_emit_self");
    return DRPO_OK;
  }
  rollout_scan_kernel<<<H, 256, 0, stream>>>(a.cnt, w.pos, w.n, a.ntiles);
  DRPO_LAUNCH_CHECK("rollout_scan");
  auto k = rpt == 32 ? rollout_emit_kernel<32> : rollout_emit_kernel<16>;
  k<<<eg, 256, 0, stream>>>(a, w.pos, w.n, d->vptr, dst);
  DRPO_LAUNCH_CHECK("rollout_emit");
  rollout_persist_finalize_kernel<<<1, 1, 0, stream>>>(d->vptr, w.n, w.off, H);
  DRPO_LAUNCH_CHECK("rollout_finalize");
  return DRPO_OK;
}

// engine 2: fused-horizon kernel + one of the two emit tails
static int rollout_fused(const drpo_rollout_desc_t* d, const RolloutWs& w, int rpt, int64_t rlen, hipStream_t stream) {
  const bool self_emit = emit_is_self(d->H, d->B, rpt);
  PersistArgs a{};
  if (const int rc = persist_run(d, w, rpt, rlen, self_emit, "drpo_rollout", stream, a)) return rc;
  return emit_tail(d, w, rpt, a, self_emit, stream);
}

// engine 1: one launch per horizon step + pointer advance
static int rollout_stepwise(const drpo_rollout_desc_t* d, const RolloutWs& w, int rpt, int64_t rlen,
                            hipStream_t stream) {
  const int S = d->S, A = d->A, S1 = d->S + 1;
  RolloutStepArgs a{};
  fill_shared_args(a, d, rlen);
  a.Bmax = d->B;
  a.vs = d->vs; a.va = d->va; a.vs2 = d->vs2; a.vr = d->vr; a.vh = d->vh; a.vd = d->vd; a.vv = d->vv;
  a.vptr = d->vptr; a.vcap = d->vcap;
  a.n = w.n; a.off = w.off;

  const int tiles = (d->B + rpt - 1) / rpt;
  constexpr int NW = 8;
  const size_t lds_bytes = step_lds_bytes(S, A, d->Ha, d->Hm, rpt, NW, tiles);
  DRPO_REQUIRE(lds_bytes <= 160 * 1024, "drpo_rollout: LDS %zu too large", lds_bytes);
  const bool pg = d->env_id == DRPO_ENV_PROGRAM;
  auto k = rpt == 32 ? (pg ? rollout_step_kernel<2, NW, true> : rollout_step_kernel<2, NW, false>)
                     : (pg ? rollout_step_kernel<1, NW, true> : rollout_step_kernel<1, NW, false>);

  const int E_out_in[6][2] = {{d->Hm, S + A}, {d->Hm, d->Hm}, {d->Hm, d->Hm}, {S1, d->Hm}, {d->Hm, d->Hm}, {S1, d->Hm}};
  const float* Wb[6] = {d->mW1, d->mW2, d->dW1, d->dW2, d->lW1, d->lW2};
  const float* Bb[6] = {d->mb1, d->mb2, d->db1, d->db2, d->lb1, d->lb2};

  for (int t = 0; t < d->H; ++t) {
    const int m = d->members[t];
    const float* Wm[6];
    const float* Bm[6];
    for (int i = 0; i < 6; ++i) {
      // packed mirrors: member stride = drpo_packed_size(in, out)
      Wm[i] = Wb[i] + (size_t)m * drpo_packed_size(E_out_in[i][1], E_out_in[i][0]);
      Bm[i] = Bb[i] + (size_t)m * E_out_in[i][0];
    }
    a.mW1 = Wm[0]; a.mW2 = Wm[1]; a.dW1 = Wm[2]; a.dW2 = Wm[3]; a.lW1 = Wm[4]; a.lW2 = Wm[5];
    a.mb1 = Bm[0]; a.mb2 = Bm[1]; a.db1 = Bm[2]; a.db2 = Bm[3]; a.lb1 = Bm[4]; a.lb2 = Bm[5];
    a.t = t;
    const int cur = t & 1, prv = cur ^ 1;
    a.prev_nxt = w.nxt[prv]; a.prev_cnt = w.cnt[prv]; a.prev_inv = w.inv[prv];
    a.nxt = w.nxt[cur]; a.cnt = w.cnt[cur]; a.inv = w.inv[cur];
    a.eps_a = d->eps_a ? d->eps_a + (size_t)t * d->B * A : nullptr;
    a.eps_m = d->eps_m ? d->eps_m + (size_t)t * d->B * S1 : nullptr;
    if (d->step_events) hipEventRecord((hipEvent_t)d->step_events[2 * t], stream);
    k<<<tiles, NW * 64, lds_bytes, stream>>>(a);
    DRPO_LAUNCH_CHECK("rollout_step");
    if (d->step_events) hipEventRecord((hipEvent_t)d->step_events[2 * t + 1], stream);
  }
  rollout_finalize_kernel<<<1, 1, 0, stream>>>(d->vptr, w.n, w.off, d->H);
  DRPO_LAUNCH_CHECK("rollout_finalize");
  return DRPO_OK;
}

// What drpo_rollout and drpo_rollout_trajectories check alike, and the tile choice (`who`:
// the entry point, for its messages). buffer: the checks on the virtual-buffer fields
// (vptr, vcap), which only drpo_rollout writes.
static int rollout_checks(const drpo_rollout_desc_t* d, const char* who, bool buffer, int& rpt_out, int64_t& rlen_out) {
  DRPO_REQUIRE(d, "%s: null descriptor", who);
  DRPO_REQUIRE(d->S >= 1 && d->S <= 64 && d->A >= 1 && d->A <= 8, "%s: S=%d A=%d out of range", who, d->S, d->A);
  DRPO_REQUIRE(d->Ha >= 1 && d->Ha <= 256 && d->Hm >= 1 && d->Hm <= 256, "%s: hidden dims must be <= 256", who);
  DRPO_REQUIRE(d->S + 1 <= 64, "%s: state_dim+1 must be <= 64", who);
  DRPO_REQUIRE(d->env_id >= 0 && d->env_id <= DRPO_ENV_PROGRAM, "%s: unknown env id %d", who, d->env_id);
  if (d->env_id == DRPO_ENV_PROGRAM)
    // the program's row count lives in device memory: the caller states it (C) and has
    // checked the program with drpo_env_program_check before the upload
    DRPO_REQUIRE(d->C >= 1 && d->C <= DRPO_PROG_MAX_ROWS && d->env_program,
                 "%s: env id %d needs 1 <= con_dim (%d) <= %d and a device program (env_program)", who, d->env_id,
                 d->C, (int)DRPO_PROG_MAX_ROWS);
  else
    DRPO_REQUIRE(d->C >= 1 && d->C <= 8 && d->C == env_con_dim(d->env_id, d->tracking_n_surr),
                 "%s: con_dim %d does not match env %d", who, d->C, d->env_id);
  if (buffer) {
    DRPO_REQUIRE(d->B >= 1 && d->H >= 1 && (int64_t)d->B * d->H <= d->vcap,
                 "%s: B*H=%lld exceeds buffer capacity %lld", who, (long long)d->B * d->H, (long long)d->vcap);
    DRPO_REQUIRE(d->workspace && d->vptr && d->replay_states, "%s: null pointer", who);
  } else {
    DRPO_REQUIRE(d->B >= 1 && d->H >= 1, "%s: B=%d H=%d must be positive", who, d->B, d->H);
    DRPO_REQUIRE(d->workspace && d->replay_states, "%s: null pointer", who);
  }
  DRPO_REQUIRE(d->B <= 16 * 8192, "%s: batch %d too large (max 131072)", who, d->B);
  const int64_t rlen = d->replay_ptr < d->replay_cap ? d->replay_ptr : d->replay_cap;
  DRPO_REQUIRE(rlen >= d->B, "%s: replay has %lld rows < batch %d (sampling without replacement)", who,
               (long long)rlen, d->B);
  if (d->env_id == ENV_TRACKING)
    DRPO_REQUIRE(d->tracking_surr_start + 4 * d->tracking_n_surr <= d->S, "%s: tracking layout", who);

  // 32-row tiles halve the weight bytes per MFMA once the batch fills the chip with
  // them (B >= 8192), when the wider tile still fits the LDS (not for tracking's S=51)
  const int rpt = d->rows_per_tile ? d->rows_per_tile
                                   : (d->B >= 256 * 32 &&
                                              persist_lds_bytes(d->S, d->A, d->Ha, d->Hm, 32, 8) <= 160 * 1024
                                          ? 32 : 16);
  DRPO_REQUIRE(rpt == 16 || rpt == 32, "%s: rows_per_tile must be 16 or 32", who);
  DRPO_REQUIRE(d->engine >= 0 && d->engine <= 2 && (d->eps_layout == 0 || d->eps_layout == 1),
               "%s: engine %d / eps_layout %d", who, d->engine, d->eps_layout);
  DRPO_REQUIRE((d->eps_a == nullptr) == (d->eps_m == nullptr), "%s: eps_a and eps_m go together", who);
  rpt_out = rpt;
  rlen_out = rlen;
  return DRPO_OK;
}

// validation, tile choice, engine choice
DRPO_API int drpo_rollout(const drpo_rollout_desc_t* d, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rpt;
  int64_t rlen;
  if (const int rc = rollout_checks(d, "drpo_rollout", true, rpt, rlen)) return rc;
  const int engine = rollout_engine(d);
  if (d->eps_a)
    DRPO_REQUIRE(d->eps_layout == engine - 1, "drpo_rollout: eps_layout %d cannot drive engine %d (compacted draws "
                 "need engine 1, original-row draws engine 2)", d->eps_layout, engine);
  RolloutWs w;
  rollout_ws(d->B, d->S, d->H, reinterpret_cast<uintptr_t>(d->workspace), w);
  return engine == 2 ? rollout_fused(d, w, rpt, rlen, stream) : rollout_stepwise(d, w, rpt, rlen, stream);
}

// The fused engine's horizon kernel + the trajectory tail: the rollout per original row
// (row identity) instead of into the virtual buffer, which it never touches.
static int rollout_trajectories(const drpo_rollout_desc_t* d, const drpo_rollout_given_t* given,
                                const drpo_rollout_shield_t* shield, const drpo_rollout_linear_t* linear,
                                const drpo_rollout_traj_t* out, const char* who, hipStream_t stream) {
  if (linear) {
    DRPO_REQUIRE(shield, "%s: the linear shield needs the shield's networks (linear without shield)", who);
    DRPO_REQUIRE(linear->candidates >= 2 && linear->candidates <= 32, "%s: linear shield candidates %d outside 2..32",
                 who, linear->candidates);
  }
  if (shield) {
    // the shapes the SH instantiations run; anything else is refused, never run another way
    const drpo_rollout_shield_t& s = *shield;
    DRPO_REQUIRE(s.Hc >= 1 && s.Hc <= 256, "%s: shield critic hidden width %d outside 1..256", who, s.Hc);
    DRPO_REQUIRE(s.Cq >= 1 && s.Cq <= 8, "%s: shield critic outputs %d outside 1..8", who, s.Cq);
    DRPO_REQUIRE(s.sW1 && s.sb1 && s.sW2 && s.sb2 && s.sW3 && s.sb3, "%s: shield with a null safe-actor pointer", who);
    DRPO_REQUIRE(s.cW1 && s.cb1 && s.cW2 && s.cb2 && s.qW1 && s.qb1 && s.qW2 && s.qb2,
                 "%s: shield with a null critic trunk / mean head pointer", who);
    DRPO_REQUIRE(!s.distributional || (s.zW1 && s.zb1 && s.zW2 && s.zb2),
                 "%s: distributional shield needs the log-std head", who);
  }
  int rpt;
  int64_t rlen;
  if (const int rc = rollout_checks(d, who, false, rpt, rlen)) return rc;
  // the wider of the actor's and the critic's hidden layers sizes the tile: an automatic
  // 32-row tile that no longer fits falls back to 16 rows (a requested one is refused below)
  if (shield && !d->rows_per_tile && rpt == 32 &&
      persist_lds_bytes(d->S, d->A, d->Ha > shield->Hc ? d->Ha : shield->Hc, d->Hm, 32, 8) +
              (linear ? persist_linear_lds_bytes(32) : 0) > 160 * 1024)
    rpt = 16;
  DRPO_REQUIRE(d->engine != 1, "%s: runs the fused engine only (engine 0 or 2, not 1)", who);
  DRPO_REQUIRE(!(d->eps_a && d->eps_layout == 0),
               "%s: recorded draws must be indexed by original row (eps_layout 1), not compacted per step", who);
  DRPO_REQUIRE(out && out->len, "%s: null len (the one required output)", who);
  DRPO_REQUIRE(!out->ret || out->weights, "%s: ret needs weights", who);
  if (given) {
    DRPO_REQUIRE(given->steps >= 0 && given->steps <= d->H, "%s: given steps %d outside [0, horizon %d]", who,
                 given->steps, d->H);
    DRPO_REQUIRE(given->steps == 0 || given->actions, "%s: given steps %d need actions", who, given->steps);
  }
  RolloutWs w;
  rollout_ws(d->B, d->S, d->H, reinterpret_cast<uintptr_t>(d->workspace), w);
  PersistArgs a{};
  if (const int rc = persist_run(d, w, rpt, rlen, false, who, stream, a, given, shield, linear)) return rc;
  const TrajArgs ta{d->S, d->A, d->C, d->B, d->H, w.st_s, w.st_s2, w.st_a, w.st_r, w.st_h, w.st_dv, *out};
  rollout_traj_kernel<<<(d->B + TRAJ_ROWS - 1) / TRAJ_ROWS, TRAJ_NT, 0, stream>>>(ta);
  DRPO_LAUNCH_CHECK("rollout_traj");
  return DRPO_OK;
}

DRPO_API int drpo_rollout_trajectories(const drpo_rollout_desc_t* d, const drpo_rollout_traj_t* out,
                                       drpo_stream_t stream) {
  return rollout_trajectories(d, nullptr, nullptr, nullptr, out, "drpo_rollout_trajectories", (hipStream_t)stream);
}

// The same under given actions: the first given->steps steps take their action from
// memory instead of from the actor (the GA instantiations of rollout_persist_kernel).
DRPO_API int drpo_rollout_trajectories_given(const drpo_rollout_desc_t* d, const drpo_rollout_given_t* given,
                                             const drpo_rollout_traj_t* out, drpo_stream_t stream) {
  return rollout_trajectories(d, given, nullptr, nullptr, out, "drpo_rollout_trajectories_given", (hipStream_t)stream);
}

// The same under the shielded controller (src/smbpo.py:124-136): the SH instantiations of
// rollout_persist_kernel. shield == nullptr is drpo_rollout_trajectories.
DRPO_API int drpo_rollout_trajectories_shielded(const drpo_rollout_desc_t* d, const drpo_rollout_shield_t* shield,
                                                const drpo_rollout_traj_t* out, drpo_stream_t stream) {
  return rollout_trajectories(d, nullptr, shield, nullptr, out, "drpo_rollout_trajectories_shielded",
                              (hipStream_t)stream);
}

// The same under the evaluation's controller, the linear shield (src/sampling.py:430-437):
// the SH instantiations with sh_lin_k candidates. linear == nullptr is the call above.
DRPO_API int drpo_rollout_trajectories_linear(const drpo_rollout_desc_t* d, const drpo_rollout_shield_t* shield,
                                              const drpo_rollout_linear_t* linear, const drpo_rollout_traj_t* out,
                                              drpo_stream_t stream) {
  return rollout_trajectories(d, nullptr, shield, linear, out, "drpo_rollout_trajectories_linear", (hipStream_t)stream);
}

// Given actions as proposals: the shield (either one) judges the first given->steps steps'
// given actions as it judges the actor's samples (the GA && SH instantiations). Without
// given actions or without a shield the call is one of the four above, and refused here.
DRPO_API int drpo_rollout_trajectories_proposed(const drpo_rollout_desc_t* d, const drpo_rollout_given_t* given,
                                                const drpo_rollout_shield_t* shield,
                                                const drpo_rollout_linear_t* linear, const drpo_rollout_traj_t* out,
                                                drpo_stream_t stream) {
  const char* who = "drpo_rollout_trajectories_proposed";
  DRPO_REQUIRE(given && given->steps != 0, "%s: no given actions (NULL or steps == 0): without proposals the call "
               "is drpo_rollout_trajectories_shielded / _linear", who);
  DRPO_REQUIRE(shield, "%s: null shield: without one the call is drpo_rollout_trajectories_given", who);
  return rollout_trajectories(d, given, shield, linear, out, who, (hipStream_t)stream);
}

// ---- halting: stage, then cut + emit; or cut + the trajectory tail ------------------

// What the three halting entry points check alike after rollout_checks: the fused engine.
static int halt_engine_checks(const drpo_rollout_desc_t* d, const char* who) {
  DRPO_REQUIRE(d->engine != 1, "%s: runs the fused engine only (engine 0 or 2, not 1)", who);
  DRPO_REQUIRE(d->H <= PERSIST_MAX_H, "%s: engine 2 supports horizon <= %d", who, PERSIST_MAX_H);
  DRPO_REQUIRE(!(d->eps_a && d->eps_layout == 0),
               "%s: recorded draws must be indexed by original row (eps_layout 1), not compacted per step", who);
  return DRPO_OK;
}

static int cut_checks(const drpo_rollout_cut_t* cut, const char* who) {
  DRPO_REQUIRE(cut && cut->scores, "%s: null cut descriptor or scores", who);
  DRPO_REQUIRE(cut->row_stride != 0 && cut->step_stride != 0, "%s: score strides %lld / %lld must not be zero", who,
               (long long)cut->row_stride, (long long)cut->step_stride);
  DRPO_REQUIRE(cut->threshold == cut->threshold, "%s: the threshold is NaN", who);
  return DRPO_OK;
}

static void launch_cut(const drpo_rollout_desc_t* d, const RolloutWs& w, const drpo_rollout_cut_t* cut,
                       hipStream_t stream) {
  rollout_cut_kernel<<<(d->B + 255) / 256, 256, 0, stream>>>(w.st_dv, cut->scores, cut->row_stride, cut->step_stride,
                                                             cut->threshold, d->B, d->H, w.newlen, cut->halted_at);
}

// The horizon kernel alone: the staging, counts and the buffer pointer's copy stay in the
// workspace for drpo_rollout_emit_cut. Neither the buffer nor its pointer is written.
DRPO_API int drpo_rollout_stage(const drpo_rollout_desc_t* d, drpo_stream_t stream_) {
  const char* who = "drpo_rollout_stage";
  int rpt;
  int64_t rlen;
  if (const int rc = rollout_checks(d, who, true, rpt, rlen)) return rc;
  if (const int rc = halt_engine_checks(d, who)) return rc;
  RolloutWs w;
  rollout_ws(d->B, d->S, d->H, reinterpret_cast<uintptr_t>(d->workspace), w);
  PersistArgs a{};
  return persist_run(d, w, rpt, rlen, true, who, (hipStream_t)stream_, a);
}

// Cut + recount over the staging drpo_rollout_stage left, then drpo_rollout's emit tail on
// the new counts.
DRPO_API int drpo_rollout_emit_cut(const drpo_rollout_desc_t* d, const drpo_rollout_cut_t* cut, drpo_stream_t stream_) {
  const char* who = "drpo_rollout_emit_cut";
  hipStream_t stream = (hipStream_t)stream_;
  int rpt;
  int64_t rlen;
  if (const int rc = rollout_checks(d, who, true, rpt, rlen)) return rc;
  if (const int rc = halt_engine_checks(d, who)) return rc;
  if (const int rc = cut_checks(cut, who)) return rc;
  RolloutWs w;
  rollout_ws(d->B, d->S, d->H, reinterpret_cast<uintptr_t>(d->workspace), w);
  // what the emit kernels read of the horizon kernel's arguments
  PersistArgs a{};
  a.S = d->S; a.A = d->A; a.C = d->C; a.B = d->B; a.H = d->H;
  a.ntiles = (d->B + rpt - 1) / rpt;
  a.st_s = w.st_s; a.st_s2 = w.st_s2; a.st_a = w.st_a; a.st_r = w.st_r; a.st_h = w.st_h; a.st_dv = w.st_dv;
  a.cnt = w.st_cnt; a.inv = w.st_inv;
  launch_cut(d, w, cut, stream);
  DRPO_LAUNCH_CHECK("rollout_cut");
  const unsigned rg = (unsigned)(((int64_t)d->H * a.ntiles + 3) / 4);
  auto k = rpt == 32 ? rollout_recount_kernel<32> : rollout_recount_kernel<16>;
  k<<<rg, 256, 0, stream>>>(a.cnt, a.inv, w.newlen, d->B, d->H, a.ntiles);
  DRPO_LAUNCH_CHECK("rollout_recount");
  return emit_tail(d, w, rpt, a, emit_is_self(d->H, d->B, rpt), stream);
}

// Cut + the trajectory tail over the staging the last drpo_rollout_trajectories* call left.
DRPO_API int drpo_rollout_trajectories_cut(const drpo_rollout_desc_t* d, const drpo_rollout_cut_t* cut,
                                           const drpo_rollout_traj_t* out, drpo_stream_t stream_) {
  const char* who = "drpo_rollout_trajectories_cut";
  hipStream_t stream = (hipStream_t)stream_;
  int rpt;
  int64_t rlen;
  if (const int rc = rollout_checks(d, who, false, rpt, rlen)) return rc;
  if (const int rc = halt_engine_checks(d, who)) return rc;
  if (const int rc = cut_checks(cut, who)) return rc;
  DRPO_REQUIRE(out && out->len, "%s: null len (the one required output)", who);
  DRPO_REQUIRE(!out->ret || out->weights, "%s: ret needs weights", who);
  RolloutWs w;
  rollout_ws(d->B, d->S, d->H, reinterpret_cast<uintptr_t>(d->workspace), w);
  launch_cut(d, w, cut, stream);
  DRPO_LAUNCH_CHECK("rollout_cut");
  const TrajArgs ta{d->S, d->A, d->C, d->B, d->H, w.st_s, w.st_s2, w.st_a, w.st_r, w.st_h, w.st_dv, *out, w.newlen};
  rollout_traj_kernel<<<(d->B + TRAJ_ROWS - 1) / TRAJ_ROWS, TRAJ_NT, 0, stream>>>(ta);
  DRPO_LAUNCH_CHECK("rollout_traj");
  return DRPO_OK;
}

__global__ void prp_kernel(int64_t* out, int64_t B, int64_t N, int hb, uint32_t k0, uint32_t k1, uint32_t k2,
                           uint32_t k3) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint32_t key[4] = {k0, k1, k2, k3};
  out[i] = prp_index((uint64_t)i, (uint64_t)N, hb, key);
}

DRPO_API int drpo_sample_without_replacement(int64_t* out, int64_t B, int64_t N, uint64_t seed, uint64_t ctr,
                                             drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(B >= 0 && B <= N && N < (1ll << 62), "drpo_sample_without_replacement: need 0 <= B <= N");
  if (B == 0) return DRPO_OK;
  uint32_t k[4];
  prp_keys(seed, ctr, k);
  prp_kernel<<<(unsigned)((B + 255) / 256), 256, 0, stream>>>(out, B, N, hb_for(N), k[0], k[1], k[2], k[3]);
  DRPO_LAUNCH_CHECK("prp");
  return DRPO_OK;
}
