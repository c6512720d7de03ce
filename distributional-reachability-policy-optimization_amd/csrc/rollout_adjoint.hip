// The adjoint of the imagined rollout (drpo_rollout_adjoint, include/drpo_hip.h): upstream
// gradients of a stored run's states and rewards backed through the deterministic model step
// to the actions and the start state, in ONE launch. One 512-thread workgroup keeps a 16-row
// tile (fit.hip's decomposition) for the whole reverse sweep, t from the tile's largest length
// down to 0. A step is the forward of the member's trunk and of its diff head's hidden layer
// at the stored (s_t, a_t) and the four backward-data products on the transposed mirrors:
//   x_t -> y1 -> y2 -> (head hidden)       each epilogue leaves swish'(z) in LDS beside y
//   [lam | g_r] -> dZ_h -> dZ_2 -> dZ_1 -> dx   swish'(z) applied in the products' epilogues
// The output layer's forward is not run: it is linear, and s_{t+1} is stored. lam stays in
// LDS from step to step; nothing but grad_actions[:, t] and, at the end, grad_start leaves
// the CU. The member changes per step: its mirrors are member * stride behind member 0's
// (rollout_persist.hpp). Weight rings as in fit.hip: a layer's first fragments are issued by
// the phase before it, ahead of that phase's epilogue and barrier.
//
// LDS: six [16][264] tiles (x / the upstream, y1, y2 and the three swish' tiles; the
// backward's dZ tiles reuse y1 / y2 as they die), lam [16][16] and the tile's lengths:
// 100 KiB, one workgroup per CU.
#include "common.hpp"
#include "fit_tiles.hpp"
#include "path_shapes.hpp"

using namespace drpo;

struct AdjointArgs {
  drpo_rollout_adjoint_t d;
  int64_t ms_in, ms_hid, ms_out;   // packed strides: (S+A -> Hm), (Hm -> Hm), (Hm -> S+1)
  int members[DRPO_ROLLOUT_FUSED_MAX_H];
};
typedef const __attribute__((address_space(4))) AdjointArgs AdjK;   // read in place (scalar loads)

namespace {
constexpr int ADJ_LAM = 16;   // lam's row stride: S <= 15
}

// forward epilogue (swish): y -> out (LDS; nullptr: not needed), swish'(z) -> db (LDS: the
// backward's factor, ff_epi_bwd's expression); padding columns zero
__device__ __forceinline__ void adj_epi_fwd(const f32x4 (&acc)[1][2], const float (&bvs)[2], int N, float* out,
                                            float* db) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int NB = (N + 15) >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int cb = wave + FF_NW * c;
    if (cb >= NB) continue;
    const int col = cb * 16 + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;
      const float z = acc[0][c][r] + bvs[c];
      const float s = fast_sigmoid(z);
      if (out) out[row * FF_LDH + col] = col < N ? z * s : 0.f;
      db[row * FF_LDH + col] = col < N ? s * (1.f + z * (1.f - s)) : 0.f;
    }
  }
}

// backward epilogue: dZ = (dZ_next W) * swish'(z) -> out (LDS, the next product's input;
// db is zero in the padding columns, so they stay zero)
__device__ __forceinline__ void adj_epi_bwd(const f32x4 (&acc)[1][2], int N, float* out, const float* db) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int NB = (N + 15) >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int cb = wave + FF_NW * c;
    if (cb >= NB) continue;
    const int col = cb * 16 + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;
      out[row * FF_LDH + col] = acc[0][c][r] * db[row * FF_LDH + col];
    }
  }
}

// The input layer's backward, dx = dZ_1 W_1: N = S + A <= 64 columns, so wave w < ncb owns
// the one column block w and the other waves wait at the next barrier. ncb = ceil((S + A) / 16)
// is 1 at S + A <= 16 (quadrotor, point-robot): one wave then runs the NK k-steps alone, 4 NK
// MFMAs against the 16 NK per SIMD of a trunk-width phase. Two accumulators take the even and the
// odd k-steps (the 16x16x4 MFMA's dependent latency exceeds its issue interval). Splitting K over
// the idle waves is not built.
template <int NK>
__device__ __forceinline__ void adj_pre1(const float* __restrict__ P, int cb, f32x4 (&bq)[FPT]) {
#pragma unroll
  for (int u = 0; u < FPT - 1; ++u) bq[u] = load_pk(P, cb, u, NK);
}

template <int NK>
__device__ __forceinline__ f32x4 adj_mma1(const float* in, const float* __restrict__ P, int cb, f32x4 (&bq)[FPT]) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  f32x4 an = *reinterpret_cast<const f32x4*>(in + l15 * FF_LDH + 4 * g), ac;
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    if (s + FPT - 1 < NK) bq[(s + FPT - 1) % FPT] = load_pk(P, cb, s + FPT - 1, NK);
    ac = an;
    if (s + 1 < NK) an = *reinterpret_cast<const f32x4*>(in + l15 * FF_LDH + 16 * (s + 1) + 4 * g);
#pragma unroll
    for (int m = 0; m < 4; ++m)
      acc[s & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[m], bq[s % FPT][m], acc[s & 1], 0, 0, 0);
  }
  return acc[0] + acc[1];
}

template <int NK>
__device__ __forceinline__ void adjoint_body(AdjK& k, float* smem) {
  auto& D = k.d;
  float* X = smem;                      // x_t; from the heads phase on the upstream [lam | g_r]
  float* T1 = X + FF_ROWS * FF_LDH;     // trunk L1 y; later trunk-L2 dZ
  float* T2 = T1 + FF_ROWS * FF_LDH;    // trunk L2 y; later head hidden dZ, then trunk-L1 dZ
  float* D1 = T2 + FF_ROWS * FF_LDH;    // swish'(z): trunk L1, trunk L2, head hidden
  float* D2 = D1 + FF_ROWS * FF_LDH;
  float* DH = D2 + FF_ROWS * FF_LDH;
  float* LAM = DH + FF_ROWS * FF_LDH;   // [16][ADJ_LAM]
  int* s_len = reinterpret_cast<int*>(LAM + FF_ROWS * ADJ_LAM);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const int64_t B = D.B;
  const int64_t row0 = (int64_t)blockIdx.x * FF_ROWS;
  if (row0 >= B) return;
  const int nrows = (int)min((int64_t)FF_ROWS, B - row0);
  const int S = D.S, A = D.A, H = D.H, Hm = D.Hm;
  const int din0 = S + A;
  const int nk1 = round_up(din0, 16) >> 4;
  const int kpad = nk1 * 16;
  const int NCB = (Hm + 15) >> 4;
  const float* __restrict__ gs = D.g_states;
  const float* __restrict__ gr = D.g_rewards;
  float* __restrict__ ga = D.grad_actions;

  if (tid < FF_ROWS) s_len[tid] = tid < nrows ? min(max(gload(D.lengths + row0 + tid), 0), H) : 0;
  if (tid < FF_ROWS * ADJ_LAM) LAM[tid] = 0.f;
  lds_barrier();
  int tmax = 0;
#pragma unroll
  for (int r = 0; r < FF_ROWS; ++r) tmax = max(tmax, s_len[r]);
  tmax = __builtin_amdgcn_readfirstlane(tmax);
  // grad_actions at and beyond a row's length: zero (the sweep stores the steps a row lived)
  for (int e = tid; e < nrows * H * A; e += FF_NT) {
    const int r = e / (H * A), ta = e - r * (H * A);
    if (ta / A >= s_len[r]) gstore(ga + (size_t)(row0 + r) * H * A + ta, 0.f);
  }

  // the upstream element and the lam element of threads < 256
  const int ur = tid >> 4, uk = tid & 15;
  const bool urow = tid < FF_ROWS * 16 && ur < nrows;
  const int ulen = urow ? s_len[ur] : 0;
  // the dx element columns of waves < nk1 (block `wave`): lam's columns (< S) or an action's
  const int xcol = wave * 16 + l15;
  const float xsd = wave < nk1 && xcol < S ? gload(D.norm_std + xcol) : 1.f;
  int xlen[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xlen[r] = 4 * g + r < nrows ? s_len[4 * g + r] : 0;

  for (int t = tmax - 1; t >= 0; --t) {
    const int m = k.members[t];
    const float* W1 = D.mW1 + (size_t)m * k.ms_in;
    const float* W2 = D.mW2 + (size_t)m * k.ms_hid;
    const float* Wh = D.dW1 + (size_t)m * k.ms_hid;
    const float* Tho = D.dT2 + (size_t)m * k.ms_out;
    const float* Thh = D.dT1 + (size_t)m * k.ms_hid;
    const float* Tt2 = D.mT2 + (size_t)m * k.ms_hid;
    const float* Tt1 = D.mT1 + (size_t)m * k.ms_in;
    // ---- x_t = [normalize(s_t), a_t], the first layer's weights ahead of it ---------------
    f32x4 bq1[FP1][2];
    float bv[2];
    switch (nk1) {
      case 1: ff_pre2<1, FP1>(W1, NCB, bq1); break;
      case 2: ff_pre2<2, FP1>(W1, NCB, bq1); break;
      case 3: ff_pre2<3, FP1>(W1, NCB, bq1); break;
      default: ff_pre2<4, FP1>(W1, NCB, bq1); break;
    }
    ff_bias2(D.mb1 + (size_t)m * Hm, Hm, bv);
    // this step's upstream loads, off the chain: lam's start g_states[i][len] and g_r
    float uv = 0.f;
    const bool uact = urow && t < ulen;
    if (uact) {
      if (uk < S) {
        if (t == ulen - 1 && gs) uv = gload(gs + ((size_t)(row0 + ur) * (H + 1) + ulen) * S + uk);
      } else if (uk == S && gr) {
        uv = gload(gr + (size_t)(row0 + ur) * H + t);
      }
    }
    float xg[4] = {0.f, 0.f, 0.f, 0.f};   // g_states[i][t] of the lam elements
    if (wave == 0 && xcol < S && gs) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t < xlen[r]) xg[r] = gload(gs + ((size_t)(row0 + 4 * g + r) * (H + 1) + t) * S + xcol);
    }
    stage_input_tile<FF_NT>(X, FF_LDH, FF_ROWS, nrows, row0, kpad, D.states + (size_t)t * S,
                            D.actions + (size_t)t * A, nullptr, S, A, 0, (H + 1) * S, H * A, 0, D.norm_mean,
                            D.norm_std, false, nullptr, 0);
    lds_barrier();
    // ---- forward: trunk L1, trunk L2, the diff head's hidden layer -------------------------
    f32x4 bqt[FPT][2];
    {
      f32x4 acc[1][2];
      switch (nk1) {
        case 1: ff_mma2<1, FP1>(X, W1, NCB, bq1, acc); break;
        case 2: ff_mma2<2, FP1>(X, W1, NCB, bq1, acc); break;
        case 3: ff_mma2<3, FP1>(X, W1, NCB, bq1, acc); break;
        default: ff_mma2<4, FP1>(X, W1, NCB, bq1, acc); break;
      }
      const float b1[2] = {bv[0], bv[1]};
      ff_pre2<NK>(W2, NCB, bqt);
      ff_bias2(D.mb2 + (size_t)m * Hm, Hm, bv);
      adj_epi_fwd(acc, b1, Hm, T1, D1);
    }
    lds_barrier();
    {
      f32x4 acc[1][2];
      ff_mma2<NK>(T1, W2, NCB, bqt, acc);
      const float b2[2] = {bv[0], bv[1]};
      ff_pre2<NK>(Wh, NCB, bqt);
      ff_bias2(D.db1 + (size_t)m * Hm, Hm, bv);
      adj_epi_fwd(acc, b2, Hm, T2, D2);
    }
    lds_barrier();
    {
      f32x4 acc[1][2];
      ff_mma2<NK>(T2, Wh, NCB, bqt, acc);
      ff_pre2<1>(Tho, NCB, bqt);   // the backward's first product (K = S + 1: one k-step)
      adj_epi_fwd(acc, bv, Hm, nullptr, DH);
      // the upstream [lam | g_r | 0] over x_t, which died with the first layer; zero rows at
      // and beyond a row's length. A row's lam starts at its last step.
      if (tid < FF_ROWS * 16) {
        float v = 0.f;
        if (uact) {
          if (uk < S) {
            if (t == ulen - 1) LAM[ur * ADJ_LAM + uk] = uv;
            else uv = LAM[ur * ADJ_LAM + uk];
          }
          v = uv;
        }
        X[ur * FF_LDH + uk] = v;
      }
    }
    lds_barrier();
    // ---- backward: head out -> head hidden -> trunk L2 -> trunk L1 -> dx -------------------
    {
      f32x4 acc[1][2];
      ff_mma2<1>(X, Tho, NCB, bqt, acc);
      ff_pre2<NK>(Thh, NCB, bqt);
      adj_epi_bwd(acc, Hm, T2, DH);
    }
    lds_barrier();
    {
      f32x4 acc[1][2];
      ff_mma2<NK>(T2, Thh, NCB, bqt, acc);
      ff_pre2<NK>(Tt2, NCB, bqt);
      adj_epi_bwd(acc, Hm, T1, D2);
    }
    lds_barrier();
    f32x4 bqx[FPT];
    {
      f32x4 acc[1][2];
      ff_mma2<NK>(T1, Tt2, NCB, bqt, acc);
      if (wave < nk1) adj_pre1<NK>(Tt1, wave, bqx);
      adj_epi_bwd(acc, Hm, T2, D1);
    }
    lds_barrier();
    if (wave < nk1) {
      const f32x4 dx = adj_mma1<NK>(T2, Tt1, wave, bqx);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        if (t >= xlen[r]) continue;
        if (xcol < S) {
          float* l = LAM + row * ADJ_LAM + xcol;
          *l = (xg[r] + *l) + dx[r] / (xsd + 1e-6f);
        } else if (xcol < din0) {
          gstore(ga + ((size_t)(row0 + row) * H + t) * A + (xcol - S), dx[r]);
        }
      }
    }
    // (no barrier: the next step's first LDS write that this phase's reads could meet is two
    // barriers away, and so is the next read of lam)
  }
  lds_barrier();
  if (urow && uk < S) {
    const size_t i = (size_t)(row0 + ur);
    const float v = ulen == 0 ? (gs ? gload(gs + i * (H + 1) * S + uk) : 0.f) : LAM[ur * ADJ_LAM + uk];
    gstore(D.grad_start + i * S + uk, v);
  }
}

__global__ __launch_bounds__(FF_NT) void rollout_adjoint_kernel(AdjointArgs args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  AdjK& k = *(AdjK*)__builtin_amdgcn_kernarg_segment_ptr();
  (void)args;
  if (k.d.Hm == 200) adjoint_body<13>(k, smem);
  else adjoint_body<16>(k, smem);
}

static_assert(sizeof(AdjointArgs) <= 4096, "rollout adjoint kernarg");

DRPO_API int drpo_rollout_adjoint(const drpo_rollout_adjoint_t* d, drpo_stream_t stream) {
  const char* who = "drpo_rollout_adjoint";
  DRPO_REQUIRE(d, "%s: null descriptor", who);
  DRPO_REQUIRE(d->B >= 0, "%s: B=%lld is negative", who, (long long)d->B);
  DRPO_REQUIRE(d->H >= 1 && d->H <= DRPO_ROLLOUT_FUSED_MAX_H, "%s: H=%d outside 1..%d", who, d->H,
               DRPO_ROLLOUT_FUSED_MAX_H);
  DRPO_REQUIRE(rollout_adjoint_shapes(d->S, d->A, d->Hm),
               "%s: S=%d A=%d Hm=%d: needs 1 <= S, S + 1 <= 16, 1 <= A, S + A <= 64 and a hidden width of 200 | 256 "
               "(drpo_rollout_adjoint_ok)", who, d->S, d->A, d->Hm);
  DRPO_REQUIRE(d->mW1 && d->mb1 && d->mW2 && d->mb2 && d->dW1 && d->db1 && d->mT1 && d->mT2 && d->dT1 && d->dT2 &&
                   d->norm_mean && d->norm_std,
               "%s: null weight, bias or normalizer pointer", who);
  DRPO_REQUIRE(d->members && d->states && d->actions && d->lengths && d->grad_actions && d->grad_start,
               "%s: null members, input or output pointer", who);
  DRPO_REQUIRE(d->E >= 1, "%s: E=%d, need an ensemble of at least one member", who, d->E);
  for (int t = 0; t < d->H; ++t)
    DRPO_REQUIRE(d->members[t] >= 0 && d->members[t] < d->E, "%s: members[%d]=%d outside an ensemble of %d", who, t,
                 d->members[t], d->E);
  const int64_t ntiles = (d->B + FF_ROWS - 1) / FF_ROWS;
  // (a launch takes fewer than 2^32 threads in x)
  DRPO_REQUIRE(ntiles * FF_NT < (int64_t(1) << 32), "%s: B=%lld exceeds one grid of 16-row tiles", who,
               (long long)d->B);
  if (d->B == 0) return DRPO_OK;
  AdjointArgs a{};
  a.d = *d;
  a.d.members = nullptr;   // host memory: the kernel reads the copy below
  a.ms_in = drpo_packed_size(d->S + d->A, d->Hm);
  a.ms_hid = drpo_packed_size(d->Hm, d->Hm);
  a.ms_out = drpo_packed_size(d->Hm, d->S + 1);
  for (int t = 0; t < d->H; ++t) a.members[t] = d->members[t];
  const size_t lds = sizeof(float) * ((size_t)6 * FF_ROWS * FF_LDH + FF_ROWS * ADJ_LAM + FF_ROWS);
  rollout_adjoint_kernel<<<dim3((unsigned)ntiles), FF_NT, lds, (hipStream_t)stream>>>(a);
  DRPO_LAUNCH_CHECK("rollout_adjoint");
  return DRPO_OK;
}
