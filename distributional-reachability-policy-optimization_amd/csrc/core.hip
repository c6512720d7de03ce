// Library-wide C ABI: version, error reporting.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>

#include "common.hpp"
#include "path_shapes.hpp"

static thread_local char g_err[1024] = "";

void drpo_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

DRPO_API const char* drpo_last_error(void) { return g_err; }

DRPO_API int drpo_version(void) { return 17; }

// HIP event helpers so hosts without a HIP binding (ctypes/cgo/JNI) can time
// individual kernels on the stream they run on. The events are timing-only: created
// without the system-scope release a default event record carries (measured: a
// default timing event left the GPU idle ~5.7 us per record between two kernels,
// profiles/r04a), since nothing reads memory through them.
DRPO_API int drpo_event_create(void** ev) {
  hipEvent_t e;
  hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  if (r != hipSuccess) {
    drpo_set_error("hipEventCreate: %s", hipGetErrorString(r));
    return DRPO_EHIP;
  }
  *ev = (void*)e;
  return DRPO_OK;
}

DRPO_API int drpo_event_destroy(void* ev) { return hipEventDestroy((hipEvent_t)ev) == hipSuccess ? DRPO_OK : DRPO_EHIP; }

DRPO_API int drpo_event_record(void* ev, drpo_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  return hipEventRecord((hipEvent_t)ev, stream) == hipSuccess ? DRPO_OK : DRPO_EHIP;
}

// stream waits for an event recorded on another stream of the same device (the model
// fit's side stream, ensemble_engine.fit): with the events above, the hand-off costs no
// system-scope fence
DRPO_API int drpo_stream_wait_event(drpo_stream_t stream_, void* ev) {
  const hipError_t r = hipStreamWaitEvent((hipStream_t)stream_, (hipEvent_t)ev, 0);
  if (r != hipSuccess) {
    drpo_set_error("hipStreamWaitEvent: %s", hipGetErrorString(r));
    return DRPO_EHIP;
  }
  return DRPO_OK;
}

DRPO_API int drpo_event_elapsed_ms(float* ms, void* start, void* stop) {
  hipError_t r = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
  if (r != hipSuccess) {
    drpo_set_error("hipEventElapsedTime: %s", hipGetErrorString(r));
    return DRPO_EHIP;
  }
  return DRPO_OK;
}

// sizeof of every ABI struct by name (binding self-check: tests/test_abi.py compares
// these with the ctypes mirrors); -1 for an unknown name
DRPO_API int64_t drpo_abi_sizeof(const char* name) {
  struct E { const char* n; size_t s; };
  static const E table[] = {
      {"drpo_rollout_desc_t", sizeof(drpo_rollout_desc_t)}, {"drpo_mlp_layer_t", sizeof(drpo_mlp_layer_t)},
      {"drpo_mlp_net_t", sizeof(drpo_mlp_net_t)},           {"drpo_policy_head_t", sizeof(drpo_policy_head_t)},
      {"drpo_mlp_fwd_t", sizeof(drpo_mlp_fwd_t)},           {"drpo_mlp_bwd_layer_t", sizeof(drpo_mlp_bwd_layer_t)},
      {"drpo_mlp_bwd_net_t", sizeof(drpo_mlp_bwd_net_t)},   {"drpo_mlp_bwd_t", sizeof(drpo_mlp_bwd_t)},
      {"drpo_mlp_fb_job_t", sizeof(drpo_mlp_fb_job_t)},   {"drpo_actor_head_t", sizeof(drpo_actor_head_t)},
      {"drpo_wgrad_item_t", sizeof(drpo_wgrad_item_t)},     {"drpo_buffer_view_t", sizeof(drpo_buffer_view_t)},
      {"drpo_critic_head_t", sizeof(drpo_critic_head_t)},   {"drpo_pack_item_t", sizeof(drpo_pack_item_t)},
      {"drpo_pack_map_t", sizeof(drpo_pack_map_t)},         {"drpo_optim_seg_t", sizeof(drpo_optim_seg_t)},
      {"drpo_ens_reduce_t", sizeof(drpo_ens_reduce_t)},     {"drpo_env_program_t", sizeof(drpo_env_program_t)},
      {"drpo_env_program_row_t", sizeof(drpo_env_program_row_t)}, {"drpo_rollout_traj_t", sizeof(drpo_rollout_traj_t)},
      {"drpo_rollout_given_t", sizeof(drpo_rollout_given_t)}, {"drpo_rollout_shield_t", sizeof(drpo_rollout_shield_t)},
      {"drpo_rollout_linear_t", sizeof(drpo_rollout_linear_t)}, {"drpo_ens_spread_t", sizeof(drpo_ens_spread_t)},
      {"drpo_rollout_cut_t", sizeof(drpo_rollout_cut_t)},     {"drpo_rollout_lookahead_t", sizeof(drpo_rollout_lookahead_t)},
      {"drpo_plan_sample_t", sizeof(drpo_plan_sample_t)},     {"drpo_plan_refit_t", sizeof(drpo_plan_refit_t)},
      {"drpo_plan_sample_ar_t", sizeof(drpo_plan_sample_ar_t)}, {"drpo_plan_shift_t", sizeof(drpo_plan_shift_t)},
      {"drpo_plan_refit_particles_t", sizeof(drpo_plan_refit_particles_t)},
      {"drpo_rollout_adjoint_t", sizeof(drpo_rollout_adjoint_t)},
  };
  for (const E& e : table)
    if (strcmp(e.n, name) == 0) return (int64_t)e.s;
  return -1;
}

// every constant of the header a binding mirrors, by name; -1 for an unknown name
DRPO_API int64_t drpo_abi_const(const char* name) {
  struct E { const char* n; int64_t v; };
#define K(x) {#x, x}
  static const E table[] = {
      K(DRPO_ACT_NONE), K(DRPO_ACT_RELU), K(DRPO_ACT_SILU), K(DRPO_ACT_TANH),
      K(DRPO_ENV_POINT_ROBOT), K(DRPO_ENV_QUADROTOR), K(DRPO_ENV_CARTPOLE), K(DRPO_ENV_TRACKING), K(DRPO_ENV_PROGRAM),
      K(DRPO_PROG_AFFINE), K(DRPO_PROG_BALLS),
      K(DRPO_PROG_MAX_ROWS), K(DRPO_PROG_MAX_TERMS), K(DRPO_PROG_MAX_CENTRES), K(DRPO_PROG_MAX_BOX),
      K(DRPO_HEAD_NONE), K(DRPO_HEAD_SAMPLE), K(DRPO_HEAD_RSAMPLE), K(DRPO_HEAD_MEAN),
      K(DRPO_UPSTREAM_GOUT), K(DRPO_UPSTREAM_CRITIC), K(DRPO_UPSTREAM_CERT), K(DRPO_UPSTREAM_ENS),
      K(DRPO_UPSTREAM_ACTOR_CC), K(DRPO_UPSTREAM_SAFE_CC), K(DRPO_UPSTREAM_NEG_MEAN), K(DRPO_UPSTREAM_SQUASH),
      K(DRPO_UPSTREAM_SQUASH_SAFE),
      K(DRPO_ROLLOUT_FUSED_MAX_H), K(DRPO_OPTIM_MAX_SEGS), K(DRPO_MLP_MULTI_MAX_JOBS), K(DRPO_MLP_MULTI_MAX_SLOTS),
      K(DRPO_MLP_FB_MAX_JOBS), K(DRPO_PLAN_MAX_CANDIDATES), K(DRPO_PLAN_SITE), K(DRPO_PLAN_MAX_PARTICLES),
  };
#undef K
  for (const E& e : table)
    if (strcmp(e.n, name) == 0) return e.v;
  return -1;
}

// ---------------------------------------------------------------------------
// path queries: the shape conditions of csrc/path_shapes.hpp, as the entry points call them
// ---------------------------------------------------------------------------
using namespace drpo;

// the trunk job of three nets, and the backward that describes a forward's layers
static drpo_mlp_fwd_t trunk_job(const drpo_mlp_net_t* t, const drpo_mlp_net_t* h1, const drpo_mlp_net_t* h2) {
  drpo_mlp_fwd_t f{};
  f.trunk = 1;
  f.nnets = 3;
  f.net[0] = *t, f.net[1] = *h1, f.net[2] = *h2;
  return f;
}

static drpo_mlp_bwd_t bwd_of(const drpo_mlp_fwd_t& f) {
  drpo_mlp_bwd_t b{};
  b.trunk = f.trunk;
  b.nnets = f.nnets;
  for (int j = 0; j < f.nnets; ++j) {
    b.net[j].nl = f.net[j].nl;
    for (int l = 0; l < MLP_MAXL; ++l) {
      b.net[j].L[l].din = f.net[j].L[l].din;
      b.net[j].L[l].dout = f.net[j].L[l].dout;
      b.net[j].L[l].act = f.net[j].L[l].act;
    }
  }
  return b;
}

DRPO_API int drpo_mlp_pair_ok(const drpo_mlp_net_t* a, const drpo_mlp_net_t* b) { return a && b && pair_shapes(*a, *b); }

DRPO_API int drpo_mlp_heads_paired(const drpo_mlp_net_t* trunk, const drpo_mlp_net_t* h1, const drpo_mlp_net_t* h2) {
  if (!trunk || !h1 || !h2) return 0;
  const drpo_mlp_fwd_t f = trunk_job(trunk, h1, h2);
  return heads_pairable(&f);
}

DRPO_API int drpo_mlp_post_ok(int cols0, const drpo_mlp_net_t* post) { return post && post_shapes(cols0, *post); }

DRPO_API int drpo_mlp_fb_ok(int cols0, const drpo_mlp_net_t* trunk, const drpo_mlp_net_t* h1, const drpo_mlp_net_t* h2,
                            const drpo_mlp_net_t* post, const drpo_mlp_net_t* q0, const drpo_mlp_net_t* q1, int C) {
  if (!trunk || !h1 || !h2 || !post || !q0 || !q1 || C < 1 || C > 16) return 0;
  for (const drpo_mlp_net_t* n : {trunk, h1, h2, q0, q1})
    if (!net_shape_ok(*n, n->L[0].din)) return 0;
  const drpo_mlp_fwd_t f = trunk_job(trunk, h1, h2);
  // the chained first forward (bound + multiplier), then each job's nets and upstream
  if (!heads_pairable(&f) || !post_shapes(cols0, *post) || !fb_post_shapes(*post)) return 0;
  if (!fb_trunk_shapes(&f, bwd_of(f), C) || !fb_net_shapes(*trunk, true)) return 0;
  for (const drpo_mlp_net_t* n : {h1, h2, q0, q1})
    if (!fb_net_shapes(*n, false)) return 0;
  return fb_single_shapes(*q0) && fb_single_shapes(*q1);
}

DRPO_API int drpo_ens_fit_paths(const drpo_mlp_fwd_t* fwd, const drpo_mlp_bwd_t* bwd, const drpo_ens_upstream_t* up) {
  if (!fwd || !bwd || !up) return 0;
  bool ens = bwd->nnets >= 1 && bwd->nnets <= MLP_MAXN;
  for (int h = 0; ens && h < bwd->nnets; ++h) {
    const drpo_mlp_bwd_net_t& n = bwd->net[h];
    ens = n.nl >= 1 && n.nl <= MLP_MAXL;
    for (int l = 0; ens && l < n.nl; ++l) ens = bwd_layer_dims(n.L[l]);
  }
  ens = ens && ens_bwd_shapes(*bwd, up->S + 1);
  return (ens ? 1 : 0) | (ens_fit_fb_shapes(*fwd, *bwd, up->S) ? 2 : 0);
}

DRPO_API int drpo_rollout_engine(const drpo_rollout_desc_t* d) { return d ? rollout_engine(d) : 0; }

DRPO_API int drpo_rollout_adjoint_ok(int S, int A, int Hm) { return rollout_adjoint_shapes(S, A, Hm); }
