// Model-based lookahead of the two critics along imagined trajectories
// (drpo_rollout_lookahead; include/drpo_hip.h has the definition): the k-step value
// expansion and the constraint critic's own backup (src/ssac.py:284-294, 304-413) unrolled
// k steps, for every k = 0..H of every row, on the trajectory-major tensors of
// drpo_rollout_trajectories*. A post-pass: it reads what the rollout and the stand-alone
// critic forwards wrote and writes two tensors of its own.
#include <math.h>

#include "common.hpp"

// The definition is ordered double arithmetic, one rounding per operation: the per-step pieces
// (dadd / dmul, the preprocessing, the two backup steps, look_max, look_store) are in
// lookahead_rows.hpp, shared with csrc/plan.hip; that header turns contraction off for the
// rest of this file.
#include "lookahead_rows.hpp"

namespace drpo {

// ---------------------------------------------------------------------------
// rollout_lookahead_kernel. One workgroup per LOOK_ROWS rows.
//   A. The rows' steps are staged in LDS once, preprocessed in double as the critics'
//      training batches are (src/smbpo.py:260-270): r'[row][t], the done / violation bits,
//      the weights, and per pass of LOOK_CC constraint columns h'[row][t][cc]. Lengths come
//      from memory and are clamped to 0..H before they index anything.
//   B. One lane per (row, k) sums the value expansion forwards, one lane per (row, k, c)
//      runs the certificate's recursion backwards. Its bootstrap is the lane's one global
//      load, issued before the chain; inside the chain a lane reads LDS only, so the longest
//      dependent chain is k <= H steps of two double operations (value) or three and a
//      select (certificate), not H^2 / 2 loads.
// All arithmetic is double, dadd / dmul of lookahead_rows.hpp (no contraction), rounded to float32 once
// at the store; a NaN is stored as the canonical quiet NaN, so that the result does not
// depend on which NaN an operation produced. Every element of every given output is
// written, by plain vector stores: lanes of a pass store consecutive addresses.
// ---------------------------------------------------------------------------
constexpr int LOOK_ROWS = 8;   // most rows per workgroup: H 128, C 4 would be 43 KB of LDS
constexpr int LOOK_CC = 4;     // constraint columns staged per pass
constexpr int LOOK_NT = 256;

struct LookArgs {
  drpo_rollout_lookahead_t d;
  int rows;   // rows per workgroup, 1..LOOK_ROWS (look_rows)
};

// Rows per workgroup: as many as give every lane of one certificate pass a (row, k, c), at
// most LOOK_ROWS. A chain is as long as its k whatever the row count, so fewer rows per
// workgroup at a long horizon mean more workgroups, not more work: H 10, C 2 -> 8 rows
// (B 4096: 512 workgroups); H 128 -> 1 row (B 256: 256 workgroups of two passes, where 8 rows
// gave 32 workgroups of twelve and measured 159 us against 102 us of the trajectory tail).
__host__ __device__ inline int look_rows(int H, int C) {
  const int per_row = (H + 1) * (C < LOOK_CC ? C : LOOK_CC);
  const int r = LOOK_NT / per_row;
  return r < 1 ? 1 : (r > LOOK_ROWS ? LOOK_ROWS : r);
}

__host__ __device__ inline size_t look_lds_bytes(int H, int R) {
  // w[H+1], r'[R][H], h'[R][H][CC] doubles; len / term [LOOK_ROWS] ints; the bits [R][H]
  return sizeof(double) * ((size_t)(H + 1) + (size_t)R * H * (1 + LOOK_CC)) + sizeof(int) * 2 * LOOK_ROWS +
         (size_t)R * H;
}

__global__ __launch_bounds__(LOOK_NT) void rollout_lookahead_kernel(LookArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char look_smem[];
  const drpo_rollout_lookahead_t& d = p.d;
  const int H = d.H, C = d.C, tid = threadIdx.x;
  const int H1 = H + 1;
  const int R = min(max(p.rows, 1), LOOK_ROWS);
  double* s_w = reinterpret_cast<double*>(look_smem);   // [H + 1]
  double* s_r = s_w + H1;                               // [R][H]
  double* s_h = s_r + R * H;                            // [R][H][CC]
  int* s_len = reinterpret_cast<int*>(s_h + (size_t)R * H * LOOK_CC);
  int* s_term = s_len + LOOK_ROWS;
  unsigned char* s_bits = reinterpret_cast<unsigned char*>(s_term + LOOK_ROWS);   // [R][H]: 1 done, 2 violation

  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int nr = (int)min((int64_t)R, (int64_t)d.B - row0);
  const double g = d.gamma, one_minus_g = 1.0 - d.gamma;
  const double rs = d.reward_scale, ab = d.alive_bonus, cs = d.constraint_scale, co = d.constraint_offset;
  const bool cost = d.mode == 1;

  // ---- A. the rows' steps ------------------------------------------------------
  for (int e = tid; e < H1; e += LOOK_NT) s_w[e] = d.weights[e];
  if (tid < LOOK_ROWS) {
    const bool in = tid < nr;
    s_len[tid] = in ? min(max(d.lengths[row0 + tid], 0), H) : 0;
    s_term[tid] = in ? (d.terminated[row0 + tid] != 0) : 0;
  }
  for (int e = tid; e < nr * H; e += LOOK_NT) {
    const size_t src = (size_t)row0 * H + e;
    s_r[e] = look_reward(d.rewards[src], rs, ab);
    s_bits[e] = (d.dones[src] ? 1 : 0) | ((cost && d.violations[src]) ? 2 : 0);
  }
  __syncthreads();

  // ---- B1. the value expansion, one lane per (row, k) ---------------------------
  if (d.value) {
    for (int e = tid; e < nr * H1; e += LOOK_NT) {
      const int r = e / H1, k = e - r * H1;
      const int len = s_len[r], kk = min(k, len);
      const size_t i = (size_t)row0 + r;
      const bool boot = kk < len || !s_term[r];
      const float q = kk < len ? d.step_q[i * H + kk] : d.terminal_q[i];
      const double* rp = s_r + r * H;
      double acc = 0.0;
      int t = 0;
      for (; t + 4 <= kk; t += 4) {   // four steps' LDS reads in flight; the order of the sum is unchanged
        double pr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pr[u] = dmul(s_w[t + u], rp[t + u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = dadd(acc, pr[u]);
      }
      for (; t < kk; ++t) acc = dadd(acc, dmul(s_w[t], rp[t]));
      if (boot) acc = dadd(acc, dmul(s_w[kk], (double)q));
      d.value[i * H1 + k] = look_store(acc);
    }
  }
  if (!d.certificate) return;

  // ---- B2. the certificate, LOOK_CC columns per pass, one lane per (row, k, c) ---
  for (int c0 = 0; c0 < C; c0 += LOOK_CC) {
    const int cw = min(LOOK_CC, C - c0);
    if (!cost) {
      if (c0) __syncthreads();   // the pass before has read its h'
      for (int e = tid; e < nr * H * cw; e += LOOK_NT) {
        const int rt = e / cw, cc = e - rt * cw;   // rt = row * H + t
        s_h[rt * LOOK_CC + cc] = look_hprime(d.constraint_values[((size_t)row0 * H + rt) * C + c0 + cc], cs, co);
      }
      __syncthreads();
    }
    for (int e = tid; e < nr * H1 * cw; e += LOOK_NT) {
      const int rk = e / cw, cc = e - rk * cw;
      const int r = rk / H1, k = rk - r * H1;
      const int len = s_len[r], kk = min(k, len);
      const size_t i = (size_t)row0 + r;
      const int c = c0 + cc;
      const bool boot = kk < len || !s_term[r];
      const float xb = kk < len ? d.step_qc[(i * H + kk) * C + c] : d.terminal_qc[i * C + c];
      // a terminated row has no bootstrap: the scan starts from 0.0, which the done select
      // of its last step replaces
      double x = boot ? (double)xb : 0.0;
      const unsigned char* bp = s_bits + r * H;
      if (cost) {
        for (int t = kk - 1; t >= 0; --t) x = look_cost_step(bp[t], g, x);
      } else {
        const double* hp = s_h + (size_t)r * H * LOOK_CC + cc;
        int t = kk - 1;
        for (; t >= 3; t -= 4) {   // four steps' LDS reads and (1 - g) h' products off the chain
          double h[4], a[4];
          unsigned b[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            h[u] = hp[(t - u) * LOOK_CC];
            b[u] = bp[t - u];
            a[u] = dmul(one_minus_g, h[u]);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) x = look_reach_step(b[u] & 1, h[u], a[u], g, x);
        }
        for (; t >= 0; --t) {
          const double h = hp[t * LOOK_CC];
          x = look_reach_step(bp[t] & 1, h, dmul(one_minus_g, h), g, x);
        }
      }
      d.certificate[(i * H1 + k) * C + c] = look_store(x);
    }
  }
}

}  // namespace drpo

using namespace drpo;

DRPO_API int drpo_rollout_lookahead(const drpo_rollout_lookahead_t* d, drpo_stream_t stream_) {
  const char* who = "drpo_rollout_lookahead";
  DRPO_REQUIRE(d, "%s: null descriptor", who);
  DRPO_REQUIRE(d->B >= 0, "%s: B=%d is negative", who, d->B);
  DRPO_REQUIRE(d->H >= 1 && d->H <= DRPO_ROLLOUT_FUSED_MAX_H, "%s: H=%d outside 1..%d", who, d->H,
               DRPO_ROLLOUT_FUSED_MAX_H);
  DRPO_REQUIRE(d->C >= 1, "%s: C=%d, need C >= 1", who, d->C);
  DRPO_REQUIRE(d->mode == 0 || d->mode == 1, "%s: mode %d (0 reachability, 1 cost)", who, d->mode);
  DRPO_REQUIRE(isfinite(d->gamma) && d->gamma >= 0.0 && d->gamma <= 1.0, "%s: gamma %g outside [0, 1]", who, d->gamma);
  DRPO_REQUIRE(d->rewards && d->constraint_values && d->dones && d->lengths && d->terminated && d->weights &&
                   d->step_q && d->step_qc && d->terminal_q && d->terminal_qc,
               "%s: null input pointer", who);
  DRPO_REQUIRE(d->mode == 0 || d->violations, "%s: null violations in cost mode", who);
  if (d->B == 0) return DRPO_OK;
  const int rows = look_rows(d->H, d->C);
  LookArgs a{*d, rows};
  const int64_t nwg = ((int64_t)d->B + rows - 1) / rows;
  DRPO_REQUIRE(nwg * LOOK_NT < (int64_t(1) << 32), "%s: B=%d at %d rows per workgroup exceeds one grid", who, d->B, rows);
  rollout_lookahead_kernel<<<(unsigned)nwg, LOOK_NT, look_lds_bytes(d->H, rows), (hipStream_t)stream_>>>(a);
  DRPO_LAUNCH_CHECK("rollout_lookahead");
  return DRPO_OK;
}
