// Sampling-based planning on the learned model (drpo_plan_sample, drpo_plan_refit;
// include/drpo_hip.h has the definitions): the two launches of an MPPI / CEM iteration around
// one given-actions rollout of P * N rows and the terminal critic forwards, and the two of
// receding-horizon control (drpo_plan_sample_ar, drpo_plan_shift), and the refit over G runs of
// the candidates, one per ensemble member (drpo_plan_refit_particles). The score of a
// candidate is entry k = H of the model-based lookahead (src/ssac.py:284-294 unrolled along the
// trajectory, in the units of src/smbpo.py:260-270), from the per-step pieces of
// lookahead_rows.hpp that csrc/lookahead.hip runs for every k.
#include <math.h>

#include "common.hpp"

// ordered double arithmetic, nothing contracted, from here to the end of the file
#include "lookahead_rows.hpp"

namespace drpo {

constexpr int PLAN_NT = 256;

// ---------------------------------------------------------------------------
// plan_sample_kernel. One lane per element of cand[P * N][K][A]; a lane's element index is
// its draw index, so consecutive lanes store consecutive addresses.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PLAN_NT) void plan_sample_kernel(drpo_plan_sample_t d) {
  const int64_t KA = (int64_t)d.K * d.A;
  const int64_t total = (int64_t)d.P * d.N * KA;
  const int64_t e = (int64_t)blockIdx.x * PLAN_NT + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / KA, j = e - r * KA;
  const int64_t p = r / d.N;
  const int n = (int)(r - p * d.N);
  const int64_t src = p * KA + j;
  if (n == 0) {
    d.cand[e] = d.incumbent[src];
    return;
  }
  const float z = normal_at(nullptr, e, d.seed, d.ctr, (uint32_t)DRPO_PLAN_SITE);
  float x = fmaf(d.std[src], z, d.mean[src]);
  x = x < d.lo ? d.lo : x;
  x = x > d.hi ? d.hi : x;
  d.cand[e] = x;
}

// ---------------------------------------------------------------------------
// plan_sample_ar_kernel. One lane per series (r, a) of cand[P * N][K][A], walking t = 0..K-1: the
// recursion is sequential in t, and a lane per element would redraw its whole prefix. Lane
// r * A + a stores element (r * K + t) * A + a at step t: the A lanes of a row store A
// consecutive floats, rows K * A apart, and over its K steps a workgroup fills one contiguous
// range of cand. mean / std / incumbent are read the same way. Untuned (profiles/plan_mpc).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PLAN_NT) void plan_sample_ar_kernel(drpo_plan_sample_ar_t d) {
  const int64_t series = (int64_t)d.P * d.N * d.A;
  const int64_t s = (int64_t)blockIdx.x * PLAN_NT + threadIdx.x;
  if (s >= series) return;
  const int64_t r = s / d.A;
  const int a = (int)(s - r * d.A);
  const int64_t p = r / d.N;
  const int n = (int)(r - p * d.N);
  const int64_t KA = (int64_t)d.K * d.A;
  const int64_t e0 = r * KA + a, src0 = p * KA + a;
  if (n == 0) {
    for (int t = 0; t < d.K; ++t) d.cand[e0 + (int64_t)t * d.A] = d.incumbent[src0 + (int64_t)t * d.A];
    return;
  }
  double u = 0.0;
  for (int t = 0; t < d.K; ++t) {
    const int64_t e = e0 + (int64_t)t * d.A, src = src0 + (int64_t)t * d.A;
    const double z = (double)normal_at(nullptr, e, d.seed, d.ctr, (uint32_t)DRPO_PLAN_SITE);
    u = t == 0 ? z : dadd(dmul(d.corr, u), dmul(d.innov, z));
    float x = fmaf(d.std[src], (float)u, d.mean[src]);
    x = x < d.lo ? d.lo : x;
    x = x > d.hi ? d.hi : x;
    d.cand[e] = x;
  }
}

// ---------------------------------------------------------------------------
// plan_shift_kernel. One lane per element (p, t, a) of the three outputs [P][K][A]; consecutive
// lanes read and store consecutive addresses (the kept steps are the inputs shift * A further on).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PLAN_NT) void plan_shift_kernel(drpo_plan_shift_t d) {
  const int64_t KA = (int64_t)d.K * d.A;
  const int64_t total = (int64_t)d.P * KA;
  const int64_t e = (int64_t)blockIdx.x * PLAN_NT + threadIdx.x;
  if (e >= total) return;
  const int64_t p = e / KA, j = e - p * KA;
  const int t = (int)(j / d.A), a = (int)(j - (int64_t)t * d.A);
  float m, inc, s;
  if (d.reset && d.reset[p]) {
    m = inc = d.tail ? d.tail[p * d.A + a] : 0.0f;
    s = d.fresh_std;
  } else if (t + d.shift < d.K) {      // (t < K and shift <= K: no overflow)
    const int64_t src = e + (int64_t)d.shift * d.A;
    m = d.mean[src];
    inc = d.incumbent[src];
    s = d.std[src];
    s = s < d.std_floor ? d.std_floor : s;
  } else {
    const int64_t last = p * KA + (int64_t)(d.K - 1) * d.A + a;
    m = d.tail ? d.tail[p * d.A + a] : d.mean[last];
    inc = d.tail ? d.tail[p * d.A + a] : d.incumbent[last];
    s = d.fresh_std;
  }
  d.mean_out[e] = m;
  d.incumbent_out[e] = inc;
  d.std_out[e] = s;
}

// ---------------------------------------------------------------------------
// plan_refit_kernel. One workgroup of 256 lanes per start state.
//   A. One lane per candidate (N <= 1024: at most four passes) runs the row's two chains at
//      k = H: the value expansion forwards and, per critic output, the certificate's recursion
//      backwards, reading its own row's steps directly. The float32 results go to LDS.
//   B. Ranks by counting over the keys in LDS: lane n counts the rows that precede row n
//      (N reads that every lane of a wave makes at the same address).
//   C. The elites' weights, doubles in LDS.
//   D. One lane per (t, a) of the given steps sums over the elites in candidate order; lanes
//      read cand[n][t][a] at consecutive addresses. Rows of weight 0 are skipped (the branch
//      is uniform), so only the elites' actions are fetched.
// Plain stores, no atomics, no waits between workgroups.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr size_t plan_lds_bytes(int N, int H) {
  // w[H + 1], weight[N] doubles; score, cert, key [N] floats; class [N] bytes; 4 ints
  return sizeof(double) * ((size_t)(H + 1) + N) + sizeof(float) * 3 * (size_t)N + sizeof(int) * 4 + (size_t)N;
}

// the position of row m before row n in a state's order: class (0 feasible, 1 valid and not
// feasible, 2 invalid), then the key descending (score; -cert; 0), then the lower n
__device__ __forceinline__ bool plan_precedes(int cm, float km, int m, int cn, float kn, int n) {
  return cm < cn || (cm == cn && (km > kn || (km == kn && m < n)));
}

// score and cert of the row whose tensors start at flat row r (step a of drpo_plan_refit), each
// rounded to float32 once. D: either refit descriptor; s_w: weights[H + 1] in LDS.
template <typename D>
__device__ __forceinline__ void plan_row_values(const D& d, const double* s_w, size_t r, float& sc, float& ce) {
  const int H = d.H, C = d.C;
  const double g = d.gamma, one_minus_g = 1.0 - d.gamma;
  const double rs = d.reward_scale, ab = d.alive_bonus, cs = d.constraint_scale, co = d.constraint_offset;
  const bool cost = d.mode == 1;
  const int len = min(max(d.lengths[r], 0), H);
  const bool boot = d.terminated[r] == 0;
  const float* rw = d.rewards + r * H;
  const uint8_t* dn = d.dones + r * H;
  double acc = 0.0;
  for (int t = 0; t < len; ++t) acc = dadd(acc, dmul(s_w[t], look_reward(rw[t], rs, ab)));
  if (boot) acc = dadd(acc, dmul(s_w[len], (double)d.terminal_q[r]));
  double top = 0.0;
  for (int c = 0; c < C; ++c) {
    // a terminated row has no bootstrap: the scan starts from 0.0, which the done select of
    // its last step replaces
    double x = boot ? (double)d.terminal_qc[r * C + c] : 0.0;
    if (cost) {
      const uint8_t* vi = d.violations + r * H;
      for (int t = len - 1; t >= 0; --t) x = look_cost_step((dn[t] ? 1u : 0u) | (vi[t] ? 2u : 0u), g, x);
    } else {
      const float* hv = d.constraint_values + r * H * C + c;
      for (int t = len - 1; t >= 0; --t) {
        const double h = look_hprime(hv[(size_t)t * C], cs, co);
        x = look_reach_step(dn[t] != 0, h, dmul(one_minus_g, h), g, x);
      }
    }
    top = c == 0 ? x : look_max(top, x);
  }
  sc = look_store(acc);
  ce = look_store(top);
}

// the float32 score and cert of candidate n of the workgroup's state as the order reads them
// (LDS: score, cert, class, key) and as the caller gets them (score[r], cert[r])
template <typename D>
__device__ __forceinline__ void plan_row_keep(const D& d, size_t r, int n, float sc, float ce, float* s_score,
                                              float* s_cert, float* s_key, unsigned char* s_cls) {
  const bool valid = sc == sc && ce == ce;
  const int cls = valid ? (ce <= d.threshold ? 0 : 1) : 2;
  s_score[n] = sc;
  s_cert[n] = ce;
  s_cls[n] = (unsigned char)cls;
  s_key[n] = cls == 0 ? sc : (cls == 1 ? -ce : 0.f);
  if (d.score) d.score[r] = sc;
  if (d.cert) d.cert[r] = ce;
}

// phases B-E of a refit kernel, from the candidates' score, cert, class and key in LDS (written
// by every lane: the caller has synchronised). D: either refit descriptor.
template <typename D>
__device__ __forceinline__ void plan_order_refit(const D& d, double* s_wt, const float* s_score, const float* s_cert,
                                                 const float* s_key, int* s_int, const unsigned char* s_cls) {
  const int N = d.N, tid = threadIdx.x;
  const int KA = d.K * d.A;
  const size_t p = blockIdx.x;
  const size_t row0 = p * (size_t)N;

  // ---- B. the order ---------------------------------------------------------------
  // every lane counts the classes itself (the same N reads as its ranks): no reduction
  int nf = 0, nv = 0;
  for (int m = 0; m < N; ++m) {
    const int c = s_cls[m];
    nf += c == 0;
    nv += c <= 1;
  }
  const int Ke = min(d.elites, nf > 0 ? nf : nv);
  int my_rank[DRPO_PLAN_MAX_CANDIDATES / PLAN_NT];
#pragma unroll
  for (int j = 0; j < DRPO_PLAN_MAX_CANDIDATES / PLAN_NT; ++j) {
    const int n = tid + j * PLAN_NT;
    int rank = 0;
    if (n < N) {
      const int cn = s_cls[n];
      const float kn = s_key[n];
      for (int m = 0; m < N; ++m) rank += plan_precedes(s_cls[m], s_key[m], m, cn, kn, n) ? 1 : 0;
      if (rank == 0) s_int[0] = n;
      if (d.rank) d.rank[row0 + n] = rank;
    }
    my_rank[j] = rank;
  }
  __syncthreads();
  const int best = s_int[0];

  // ---- C. the elites' weights -------------------------------------------------------
  const double key_best = (double)s_key[best];
  const bool flat = isinf(d.temperature);
#pragma unroll
  for (int j = 0; j < DRPO_PLAN_MAX_CANDIDATES / PLAN_NT; ++j) {
    const int n = tid + j * PLAN_NT;
    if (n < N) {
      double w = 0.0;
      if (my_rank[j] < Ke) {
        const double key = (double)s_key[n];
        const double diff = key == key_best ? 0.0 : key - key_best;
        w = flat ? 1.0 : exp(diff / d.temperature);
      }
      s_wt[n] = w;
      if (d.weight) d.weight[row0 + n] = (float)w;
    }
  }
  __syncthreads();

  // ---- D. the refit, E. the best candidate ------------------------------------------
  const double mom = d.momentum, keep = 1.0 - d.momentum;
  const float* cand0 = d.cand + row0 * KA;
  for (int e = tid; e < KA; e += PLAN_NT) {
    const size_t o = p * KA + e;
    const float mean_in = d.mean_in[o], std_in = d.std_in[o];
    float mean_out = mean_in, std_out = std_in;
    double sw = 0.0, swx = 0.0;
    for (int n = 0; n < N; ++n) {
      const double w = s_wt[n];
      if (w > 0.0) {
        sw = dadd(sw, w);
        swx = dadd(swx, dmul(w, (double)cand0[(size_t)n * KA + e]));
      }
    }
    if (sw > 0.0) {
      const double m = swx / sw;
      double sv = 0.0;
      for (int n = 0; n < N; ++n) {
        const double w = s_wt[n];
        if (w > 0.0) {
          const double dx = dadd((double)cand0[(size_t)n * KA + e], -m);
          sv = dadd(sv, dmul(w, dmul(dx, dx)));
        }
      }
      const double v = sv / sw;
      const double s = dadd(dmul(keep, sqrt(v)), dmul(mom, (double)std_in));
      mean_out = (float)dadd(dmul(keep, m), dmul(mom, (double)mean_in));
      std_out = (float)(s < d.min_std ? d.min_std : s);
    }
    d.mean_out[o] = mean_out;
    d.std_out[o] = std_out;
    d.best_actions[o] = cand0[(size_t)best * KA + e];
  }
  if (tid == 0) {
    d.best[p] = best;
    d.n_feasible[p] = nf;
    d.best_score[p] = s_score[best];
    d.best_cert[p] = s_cert[best];
    d.best_feasible[p] = s_cls[best] == 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(PLAN_NT) void plan_refit_kernel(drpo_plan_refit_t d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char plan_smem[];
  const int N = d.N, H = d.H, tid = threadIdx.x;
  double* s_w = reinterpret_cast<double*>(plan_smem);   // [H + 1]
  double* s_wt = s_w + (H + 1);                         // [N]
  float* s_score = reinterpret_cast<float*>(s_wt + N);  // [N]
  float* s_cert = s_score + N;                          // [N]
  float* s_key = s_cert + N;                            // [N]
  int* s_int = reinterpret_cast<int*>(s_key + N);       // best, n_feasible, n_valid
  unsigned char* s_cls = reinterpret_cast<unsigned char*>(s_int + 4);   // [N]
  const size_t row0 = blockIdx.x * (size_t)N;

  for (int e = tid; e <= H; e += PLAN_NT) s_w[e] = d.weights[e];
  __syncthreads();

  // ---- A. score and cert of every candidate -------------------------------------
  for (int n = tid; n < N; n += PLAN_NT) {
    float sc, ce;
    plan_row_values(d, s_w, row0 + n, sc, ce);
    plan_row_keep(d, row0 + n, n, sc, ce, s_score, s_cert, s_key, s_cls);
  }
  __syncthreads();
  plan_order_refit(d, s_wt, s_score, s_cert, s_key, s_int, s_cls);
}

// ---------------------------------------------------------------------------
// plan_refit_particles_kernel. plan_refit_kernel over G runs of the same candidates, one per
// ensemble member, member-major [G][P * N]. One workgroup of 256 lanes per start state.
//   A. One lane per candidate walks the members j = 0..G-1: the row's two chains at k = H on
//      member j's tensors (plan_row_values), the float32 member score into the lane's own column
//      of s_ms[G][256], the cert aggregated as it goes. Then the lane alone, on its column (no
//      barrier: it reads what it wrote): the spread, and the score as the mean of the T lowest
//      member scores, picked one after the other in (score, j) order so that the double sum runs
//      in that order (T passes over the G values: no sorted copy, no private array).
//   B-E. plan_order_refit on the aggregated float32 score and cert.
// Plain stores, no atomics, no waits between workgroups.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr size_t plan_particles_lds_bytes(int N, int H, int G) {
  return plan_lds_bytes(N, H) + sizeof(float) * (size_t)G * PLAN_NT;
}

__global__ __launch_bounds__(PLAN_NT) void plan_refit_particles_kernel(drpo_plan_refit_particles_t d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char plan_smem[];
  const int N = d.N, H = d.H, G = d.G, T = d.score_tail, tid = threadIdx.x;
  double* s_w = reinterpret_cast<double*>(plan_smem);   // [H + 1]
  double* s_wt = s_w + (H + 1);                         // [N]
  float* s_ms = reinterpret_cast<float*>(s_wt + N);     // [G][256]: a pass's member scores
  float* s_score = s_ms + (size_t)G * PLAN_NT;          // [N]
  float* s_cert = s_score + N;                          // [N]
  float* s_key = s_cert + N;                            // [N]
  int* s_int = reinterpret_cast<int*>(s_key + N);
  unsigned char* s_cls = reinterpret_cast<unsigned char*>(s_int + 4);   // [N]
  const size_t row0 = blockIdx.x * (size_t)N;
  const size_t B = (size_t)d.P * N;
  float* col = s_ms + tid;

  for (int e = tid; e <= H; e += PLAN_NT) s_w[e] = d.weights[e];
  __syncthreads();

  // ---- A. member values and their aggregate, of every candidate --------------------
  for (int n = tid; n < N; n += PLAN_NT) {
    const size_t r = row0 + n;
    double ctop = 0.0, csum = 0.0, ssum = 0.0;
    bool nan = false;
    for (int j = 0; j < G; ++j) {
      float sc, ce;
      plan_row_values(d, s_w, (size_t)j * B + r, sc, ce);
      if (d.member_score) d.member_score[(size_t)j * B + r] = sc;
      if (d.member_cert) d.member_cert[(size_t)j * B + r] = ce;
      col[j * PLAN_NT] = sc;
      nan |= sc != sc;
      ssum = dadd(ssum, (double)sc);
      csum = dadd(csum, (double)ce);
      ctop = j == 0 ? (double)ce : look_max(ctop, (double)ce);
    }
    if (d.score_spread) {
      const double m = ssum / (double)G;
      double sq = 0.0;
      for (int j = 0; j < G; ++j) {
        const double dx = dadd((double)col[j * PLAN_NT], -m);
        sq = dadd(sq, dmul(dx, dx));
      }
      d.score_spread[r] = look_store(sqrt(sq / (double)G));
    }
    // the T lowest member scores in (score, j) order: each pick is the least (score, j) above the last
    double tail = 0.0;
    float last_s = 0.f;
    int last_j = -1;
    for (int t = 0; t < T && !nan; ++t) {
      float pick_s = 0.f;
      int pick_j = -1;
      for (int j = 0; j < G; ++j) {
        const float s = col[j * PLAN_NT];
        const bool after = last_j < 0 || s > last_s || (s == last_s && j > last_j);
        if (after && (pick_j < 0 || s < pick_s)) {
          pick_s = s;
          pick_j = j;
        }
      }
      tail = dadd(tail, (double)pick_s);
      last_s = pick_s;
      last_j = pick_j;
    }
    const float sc = nan ? __int_as_float(0x7FC00000) : look_store(tail / (double)T);
    const float ce = look_store(d.cert_mode == 0 ? ctop : csum / (double)G);
    plan_row_keep(d, r, n, sc, ce, s_score, s_cert, s_key, s_cls);
  }
  __syncthreads();
  plan_order_refit(d, s_wt, s_score, s_cert, s_key, s_int, s_cls);
}

}  // namespace drpo

using namespace drpo;

// what drpo_plan_sample and drpo_plan_sample_ar refuse alike (D: either descriptor)
template <typename D>
static int plan_sample_check(const char* who, const D* d) {
  DRPO_REQUIRE(d, "%s: null descriptor", who);
  DRPO_REQUIRE(d->P >= 0, "%s: P=%d is negative", who, d->P);
  DRPO_REQUIRE(d->N >= 2 && d->N <= DRPO_PLAN_MAX_CANDIDATES, "%s: N=%d outside 2..%d", who, d->N,
               DRPO_PLAN_MAX_CANDIDATES);
  DRPO_REQUIRE(d->K >= 1, "%s: K=%d, need K >= 1", who, d->K);
  DRPO_REQUIRE(d->A >= 1, "%s: A=%d, need A >= 1", who, d->A);
  DRPO_REQUIRE(d->lo <= d->hi, "%s: clamp [%g, %g] is empty or NaN", who, (double)d->lo, (double)d->hi);
  DRPO_REQUIRE(d->mean && d->std && d->incumbent && d->cand, "%s: null pointer", who);
  // (K * A may not overflow the 64-bit product: each factor is below 2^31, P * N below 2^41)
  const double total = (double)d->P * d->N * d->K * d->A;
  DRPO_REQUIRE(d->P == 0 || total < 1099511627776.0, "%s: P*N*K*A = %.0f elements exceed one grid (2^40)", who,
               total);
  return DRPO_OK;
}

DRPO_API int drpo_plan_sample(const drpo_plan_sample_t* d, drpo_stream_t stream_) {
  if (const int rc = plan_sample_check("drpo_plan_sample", d)) return rc;
  if (d->P == 0) return DRPO_OK;
  const int64_t n = (int64_t)d->P * d->N * d->K * d->A;
  plan_sample_kernel<<<(unsigned)((n + PLAN_NT - 1) / PLAN_NT), PLAN_NT, 0, (hipStream_t)stream_>>>(*d);
  DRPO_LAUNCH_CHECK("plan_sample");
  return DRPO_OK;
}

DRPO_API int drpo_plan_sample_ar(const drpo_plan_sample_ar_t* d, drpo_stream_t stream_) {
  const char* who = "drpo_plan_sample_ar";
  if (const int rc = plan_sample_check(who, d)) return rc;
  DRPO_REQUIRE(d->corr >= 0.0 && d->corr < 1.0, "%s: corr %g outside [0, 1)", who, d->corr);
  DRPO_REQUIRE(d->innov > 0.0 && d->innov <= 1.0, "%s: innov %g outside (0, 1]", who, d->innov);
  if (d->P == 0) return DRPO_OK;
  const int64_t n = (int64_t)d->P * d->N * d->A;      // one lane per series
  plan_sample_ar_kernel<<<(unsigned)((n + PLAN_NT - 1) / PLAN_NT), PLAN_NT, 0, (hipStream_t)stream_>>>(*d);
  DRPO_LAUNCH_CHECK("plan_sample_ar");
  return DRPO_OK;
}

DRPO_API int drpo_plan_shift(const drpo_plan_shift_t* d, drpo_stream_t stream_) {
  const char* who = "drpo_plan_shift";
  DRPO_REQUIRE(d, "%s: null descriptor", who);
  DRPO_REQUIRE(d->P >= 0, "%s: P=%d is negative", who, d->P);
  DRPO_REQUIRE(d->K >= 1, "%s: K=%d, need K >= 1", who, d->K);
  DRPO_REQUIRE(d->A >= 1, "%s: A=%d, need A >= 1", who, d->A);
  DRPO_REQUIRE(d->shift >= 0 && d->shift <= d->K, "%s: shift=%d outside 0..K=%d", who, d->shift, d->K);
  DRPO_REQUIRE(isfinite(d->fresh_std) && d->fresh_std > 0.f, "%s: fresh_std %g, need finite and > 0", who,
               (double)d->fresh_std);
  DRPO_REQUIRE(d->std_floor >= 0.f, "%s: std_floor %g is negative or NaN", who, (double)d->std_floor);
  DRPO_REQUIRE(d->mean && d->std && d->incumbent && d->mean_out && d->std_out && d->incumbent_out,
               "%s: null pointer", who);
  const void* const in[] = {d->mean, d->std, d->incumbent, d->reset, d->tail};
  const void* const out[] = {d->mean_out, d->std_out, d->incumbent_out};
  for (const void* o : out)
    for (const void* i : in)
      DRPO_REQUIRE(o != i, "%s: an output aliases an input (a shifted read races an in-place write)", who);
  const double total = (double)d->P * d->K * d->A;
  DRPO_REQUIRE(d->P == 0 || total < 1099511627776.0, "%s: P*K*A = %.0f elements exceed one grid (2^40)", who, total);
  if (d->P == 0) return DRPO_OK;
  const int64_t n = (int64_t)d->P * d->K * d->A;
  plan_shift_kernel<<<(unsigned)((n + PLAN_NT - 1) / PLAN_NT), PLAN_NT, 0, (hipStream_t)stream_>>>(*d);
  DRPO_LAUNCH_CHECK("plan_shift");
  return DRPO_OK;
}

// what drpo_plan_refit and drpo_plan_refit_particles refuse alike (D: either descriptor)
template <typename D>
static int plan_refit_check(const char* who, const D* d) {
  DRPO_REQUIRE(d, "%s: null descriptor", who);
  DRPO_REQUIRE(d->P >= 0, "%s: P=%d is negative", who, d->P);
  DRPO_REQUIRE(d->N >= 2 && d->N <= DRPO_PLAN_MAX_CANDIDATES, "%s: N=%d outside 2..%d", who, d->N,
               DRPO_PLAN_MAX_CANDIDATES);
  DRPO_REQUIRE((int64_t)d->P * d->N <= INT32_MAX, "%s: P*N = %lld rows exceed int32", who,
               (long long)((int64_t)d->P * d->N));
  DRPO_REQUIRE(d->H >= 1 && d->H <= DRPO_ROLLOUT_FUSED_MAX_H, "%s: H=%d outside 1..%d", who, d->H,
               DRPO_ROLLOUT_FUSED_MAX_H);
  DRPO_REQUIRE(d->K >= 1 && d->K <= d->H, "%s: K=%d outside 1..H=%d", who, d->K, d->H);
  DRPO_REQUIRE(d->A >= 1, "%s: A=%d, need A >= 1", who, d->A);
  DRPO_REQUIRE((int64_t)d->K * d->A <= INT32_MAX, "%s: K*A exceeds int32", who);
  DRPO_REQUIRE(d->C >= 1, "%s: C=%d, need C >= 1", who, d->C);
  DRPO_REQUIRE(d->mode == 0 || d->mode == 1, "%s: mode %d (0 reachability, 1 cost)", who, d->mode);
  DRPO_REQUIRE(isfinite(d->gamma) && d->gamma >= 0.0 && d->gamma <= 1.0, "%s: gamma %g outside [0, 1]", who, d->gamma);
  DRPO_REQUIRE(d->elites >= 1 && d->elites <= d->N, "%s: elites=%d outside 1..N=%d", who, d->elites, d->N);
  DRPO_REQUIRE(d->temperature > 0.0, "%s: temperature %g, need > 0 (+inf allowed)", who, d->temperature);
  DRPO_REQUIRE(d->momentum >= 0.0 && d->momentum < 1.0, "%s: momentum %g outside [0, 1)", who, d->momentum);
  DRPO_REQUIRE(isfinite(d->min_std) && d->min_std >= 0.0, "%s: min_std %g, need finite and >= 0", who, d->min_std);
  DRPO_REQUIRE(d->threshold == d->threshold, "%s: threshold is NaN", who);
  DRPO_REQUIRE(d->rewards && d->constraint_values && d->dones && d->lengths && d->terminated && d->weights &&
                   d->terminal_q && d->terminal_qc && d->cand && d->mean_in && d->std_in,
               "%s: null input pointer", who);
  DRPO_REQUIRE(d->mode == 0 || d->violations, "%s: null violations in cost mode", who);
  DRPO_REQUIRE(d->mean_out && d->std_out && d->best_actions && d->best && d->n_feasible && d->best_score &&
                   d->best_cert && d->best_feasible,
               "%s: null per-state output pointer", who);
  return DRPO_OK;
}

DRPO_API int drpo_plan_refit(const drpo_plan_refit_t* d, drpo_stream_t stream_) {
  if (const int rc = plan_refit_check("drpo_plan_refit", d)) return rc;
  if (d->P == 0) return DRPO_OK;
  plan_refit_kernel<<<(unsigned)d->P, PLAN_NT, plan_lds_bytes(d->N, d->H), (hipStream_t)stream_>>>(*d);
  DRPO_LAUNCH_CHECK("plan_refit");
  return DRPO_OK;
}

DRPO_API int drpo_plan_refit_particles(const drpo_plan_refit_particles_t* d, drpo_stream_t stream_) {
  const char* who = "drpo_plan_refit_particles";
  if (const int rc = plan_refit_check(who, d)) return rc;
  DRPO_REQUIRE(d->G >= 1 && d->G <= DRPO_PLAN_MAX_PARTICLES, "%s: G=%d outside 1..%d", who, d->G,
               DRPO_PLAN_MAX_PARTICLES);
  DRPO_REQUIRE(d->score_tail >= 1 && d->score_tail <= d->G, "%s: score_tail=%d outside 1..G=%d", who, d->score_tail,
               d->G);
  DRPO_REQUIRE(d->cert_mode == 0 || d->cert_mode == 1, "%s: cert_mode %d (0 max, 1 mean)", who, d->cert_mode);
  DRPO_REQUIRE((int64_t)d->G * d->P * d->N <= INT32_MAX, "%s: G*P*N = %lld rows exceed int32", who,
               (long long)((int64_t)d->G * d->P * d->N));
  // (N <= 1024, H <= 128, G <= 32: at most 55,320 bytes, under the 64 KB a workgroup may take)
  static_assert(plan_particles_lds_bytes(DRPO_PLAN_MAX_CANDIDATES, DRPO_ROLLOUT_FUSED_MAX_H, DRPO_PLAN_MAX_PARTICLES) <=
                    65536, "plan_refit_particles: dynamic LDS beyond 64 KB");
  if (d->P == 0) return DRPO_OK;
  plan_refit_particles_kernel<<<(unsigned)d->P, PLAN_NT, plan_particles_lds_bytes(d->N, d->H, d->G),
                                (hipStream_t)stream_>>>(*d);
  DRPO_LAUNCH_CHECK("plan_refit_particles");
  return DRPO_OK;
}
