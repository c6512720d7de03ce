// Stand-alone batched constraint evaluation (tests, evaluation, the robust certificate
// target): the built-in environments' functions or a constraint program (env id 4),
// one thread per state row; and the host-side check of a program before its upload.
// The row functions themselves are in env_constraints.hpp, shared with the rollout.
#include "common.hpp"
#include "env_constraints.hpp"

using namespace drpo;

template <bool PG>
__global__ void env_constraints_kernel(EnvParams ep, const void* prog, const float* s, int64_t n, int S, int C,
                                       uint8_t* done, uint8_t* viol, float* h) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool dn, vl;
  float hh[8];
  constraint_row<PG>(ep, prog, s + i * S, dn, vl, hh);
  if (done) done[i] = dn;
  if (viol) viol[i] = vl;
  if (h)
    for (int c = 0; c < C; ++c) h[i * C + c] = hh[c];
}

DRPO_API int drpo_env_constraints(int env_id, int tracking_surr_start, int tracking_n_surr, double env_thr0,
                                  double env_thr1, const float* states, int64_t n, int S, uint8_t* done,
                                  uint8_t* violation, float* h, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(env_id != DRPO_ENV_PROGRAM,
               "drpo_env_constraints: env id %d is a constraint program: call drpo_env_constraints_program", env_id);
  DRPO_REQUIRE(env_id >= 0 && env_id <= 3, "drpo_env_constraints: unknown env id %d", env_id);
  if (n == 0) return DRPO_OK;
  EnvParams ep{env_id, tracking_surr_start, tracking_n_surr, env_thr0, env_thr1};
  const int C = env_con_dim(env_id, tracking_n_surr);
  env_constraints_kernel<false><<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(ep, nullptr, states, n, S, C, done,
                                                                                violation, h);
  DRPO_LAUNCH_CHECK("env_constraints");
  return DRPO_OK;
}

DRPO_API int drpo_env_constraints_program(const drpo_env_program_t* dev_prog, int C, const float* states, int64_t n,
                                          int S, uint8_t* done, uint8_t* violation, float* h, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DRPO_REQUIRE(dev_prog && C >= 1 && C <= DRPO_PROG_MAX_ROWS,
               "drpo_env_constraints_program: needs a device program and 1 <= C (%d) <= %d", C, (int)DRPO_PROG_MAX_ROWS);
  DRPO_REQUIRE(S >= 1 && S <= 256 && n >= 0, "drpo_env_constraints_program: S=%d n=%lld", S, (long long)n);
  if (n == 0) return DRPO_OK;
  DRPO_REQUIRE(states, "drpo_env_constraints_program: null states");
  env_constraints_kernel<true><<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(EnvParams{}, dev_prog, states, n, S, C,
                                                                               done, violation, h);
  DRPO_LAUNCH_CHECK("env_program");
  return DRPO_OK;
}

// Host-only validation of a program in host memory (no device needed).
DRPO_API int drpo_env_program_check(const drpo_env_program_t* q, int S) {
  DRPO_REQUIRE(q, "drpo_env_program_check: null program");
  DRPO_REQUIRE(S >= 1 && S <= 256, "drpo_env_program_check: state dim %d out of range (indices are bytes)", S);
  DRPO_REQUIRE(q->C >= 1 && q->C <= DRPO_PROG_MAX_ROWS, "drpo_env_program_check: %d constraint rows (1..%d)", (int)q->C,
               (int)DRPO_PROG_MAX_ROWS);
  for (int c = 0; c < q->C; ++c) {
    const drpo_env_program_row_t& r = q->rows[c];
    DRPO_REQUIRE(r.kind == DRPO_PROG_AFFINE || r.kind == DRPO_PROG_BALLS, "drpo_env_program_check: row %d has unknown kind %d",
                 c, (int)r.kind);
    int nidx;
    if (r.kind == DRPO_PROG_AFFINE) {
      DRPO_REQUIRE(r.n >= 1 && r.n <= DRPO_PROG_MAX_TERMS, "drpo_env_program_check: affine row %d has %d terms (1..%d)", c,
                   (int)r.n, (int)DRPO_PROG_MAX_TERMS);
      nidx = r.n;
    } else {
      DRPO_REQUIRE(r.n >= 1 && r.n <= DRPO_PROG_MAX_CENTRES, "drpo_env_program_check: balls row %d has %d centres (1..%d)",
                   c, (int)r.n, (int)DRPO_PROG_MAX_CENTRES);
      DRPO_REQUIRE(r.nd == 2 || r.nd == 3, "drpo_env_program_check: balls row %d has %d dims (2 or 3)", c, (int)r.nd);
      nidx = r.nd;
    }
    for (int k = 0; k < nidx; ++k)
      DRPO_REQUIRE(r.dims[k] < S, "drpo_env_program_check: row %d reads state index %d >= state dim %d", c, (int)r.dims[k], S);
  }
  DRPO_REQUIRE(q->box_n <= DRPO_PROG_MAX_BOX, "drpo_env_program_check: done box has %d dims (max %d)", (int)q->box_n,
               (int)DRPO_PROG_MAX_BOX);
  for (int k = 0; k < q->box_n; ++k)
    DRPO_REQUIRE(q->box_dims[k] < S, "drpo_env_program_check: done box reads state index %d >= state dim %d",
                 (int)q->box_dims[k], S);
  DRPO_REQUIRE(q->ball_nd == 0 || q->ball_nd == 2 || q->ball_nd == 3, "drpo_env_program_check: done ball has %d dims (2 or 3)",
               (int)q->ball_nd);
  for (int k = 0; k < q->ball_nd; ++k)
    DRPO_REQUIRE(q->ball_dims[k] < S, "drpo_env_program_check: done ball reads state index %d >= state dim %d",
                 (int)q->ball_dims[k], S);
  DRPO_REQUIRE(q->done_on_violation <= 1, "drpo_env_program_check: done_on_violation %d", (int)q->done_on_violation);
  DRPO_REQUIRE(q->done_on_violation || q->box_n || q->ball_nd, "drpo_env_program_check: empty done rule");
  return DRPO_OK;
}
