/*
 * drpo_hip.h -- C ABI of libdrpo_hip.so, the MI355X (gfx950) hot path of
 * Distributional Reachability Policy Optimization.
 *
 * The reference (ManUtdMoon/Distributional-Reachability-Policy-Optimization) is
 * pure Python/PyTorch with no FFI; these entry points are what a binding for its
 * hot path binds (the Python package drpo_amd binds them with ctypes, see
 * INTEGRATION.md). Conventions:
 *   - all pointers are DEVICE pointers (fp32 row-major, uint8 flags, int64
 *     indices) unless marked "host"; memory is owned by the caller (PyTorch's
 *     caching allocator), the library never allocates on the hot path;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, DRPO_EINVAL / DRPO_EHIP / DRPO_EUNSUPPORTED
 *     otherwise, with a message in drpo_last_error() (thread-local);
 *   - noise: a non-NULL eps pointer is "parity mode" (the caller supplies the
 *     reference's standard-normal draws); NULL means Philox4x32-10 on the device
 *     keyed by (seed, ctr, call-site).
 * Reference citations are path:line in the reference repository.
 */
#ifndef DRPO_HIP_H
#define DRPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* drpo_stream_t; /* hipStream_t */

enum { DRPO_OK = 0, DRPO_EINVAL = 1, DRPO_EHIP = 2, DRPO_EUNSUPPORTED = 3 };

/* activation ids used by the MLP descriptors (src/torch_util.py:169-178) */
enum { DRPO_ACT_NONE = 0, DRPO_ACT_RELU = 1, DRPO_ACT_SILU = 2, DRPO_ACT_TANH = 3 };

/* device environment ids for the batched constraint functions (src/smbpo.py:63-65) */
enum { DRPO_ENV_POINT_ROBOT = 0, DRPO_ENV_QUADROTOR = 1, DRPO_ENV_CARTPOLE = 2, DRPO_ENV_TRACKING = 3,
       DRPO_ENV_PROGRAM = 4 /* constraint functions described by a drpo_env_program_t */ };

/* ---------------------------------------------------------------- constraint programs
 * A declarative description of an environment's check_done / check_violation /
 * get_constraint_values (src/smbpo.py:63-65) for environments the library has no
 * built-in id for: C constraint rows, each affine (the reference's LinearConstraint
 * h = A x - b, src/env/poles/constraints.py:159-247) or the distance to the nearest of
 * a few balls (hazard discs), and a done rule. It is evaluated by an interpreter in
 * the rollout kernels' constraint phase. States are float32 promoted to double; every
 * constant is a double, all arithmetic and comparisons are in double (no fused
 * multiply-add), h is rounded to float32 on output AFTER the violation test h > 0.
 * Plain data, no pointers; every byte array is 4-byte aligned (the kernels read them
 * as whole words).                                                              */
enum { DRPO_PROG_AFFINE = 0, DRPO_PROG_BALLS = 1 };
enum { DRPO_PROG_MAX_ROWS = 8, DRPO_PROG_MAX_TERMS = 8, DRPO_PROG_MAX_CENTRES = 8, DRPO_PROG_MAX_BOX = 8 };

typedef struct {
  uint8_t kind;        /* DRPO_PROG_AFFINE: h = sum_k v[k] * s[dims[k]] + k0 (terms added left to right);
                          DRPO_PROG_BALLS:  h = k0 - min_j || s[dims] - v[j*nd .. j*nd+nd) ||_2 */
  uint8_t n;           /* affine: terms, 1..8; balls: centres, 1..8 */
  uint8_t nd;          /* balls: dims, 2 or 3 (affine: 0) */
  uint8_t pad_;
  uint8_t dims[8];     /* affine: the state index of each term; balls: the nd state indices */
  uint32_t pad2_;
  double k0;           /* affine: bias; balls: radius */
  double v[24];        /* affine: coefficients [n]; balls: centres [n][nd] */
} drpo_env_program_row_t;

typedef struct {
  int32_t C;                   /* constraint rows, 1..8 */
  uint8_t done_on_violation;   /* done |= any(h > 0) */
  uint8_t box_n;               /* done |= s[box_dims[k]] < box_lo[k] || s[box_dims[k]] > box_hi[k], k < box_n <= 8 */
  uint8_t ball_nd;             /* 0: none; 2 | 3: done |= || s[ball_dims] - ball_centre ||_2 <= ball_radius */
  uint8_t pad_;
  uint8_t box_dims[8];
  uint8_t ball_dims[4];
  uint32_t pad2_;
  double box_lo[8], box_hi[8];
  double ball_centre[3], ball_radius;
  drpo_env_program_row_t rows[8];
} drpo_env_program_t;

/* Host-only check of a program (in HOST memory) against a state dimension S: kinds,
 * counts, and every state index < S. The ONLY place a program can be validated: once
 * uploaded it is device memory to the library, and a bad index would be an
 * out-of-bounds read in the kernel. DRPO_EINVAL with a message otherwise. */
int drpo_env_program_check(const drpo_env_program_t* host_prog, int S);

/* limits of the launches; a binding that mirrors one checks it against drpo_abi_const */
enum {
  DRPO_ROLLOUT_FUSED_MAX_H = 128, /* horizon of the fused rollout engine (engine 2, drpo_rollout_trajectories*) */
  DRPO_OPTIM_MAX_SEGS = 8,        /* segments of one drpo_optim_step */
  DRPO_MLP_MULTI_MAX_JOBS = 8,    /* jobs of one drpo_mlp_forward_multi / drpo_mlp_backward_multi* */
  DRPO_MLP_MULTI_MAX_SLOTS = 16,  /* (job, net) workgroup slots of such a launch */
  DRPO_MLP_FB_MAX_JOBS = 4,       /* jobs of one drpo_mlp_fb_multi */
  DRPO_PLAN_MAX_CANDIDATES = 1024, /* candidates per start state of drpo_plan_sample / drpo_plan_refit */
  DRPO_PLAN_SITE = 0x91a7,        /* the Philox site (third counter word) of drpo_plan_sample's draws */
  DRPO_PLAN_MAX_PARTICLES = 32    /* runs (ensemble members) of one drpo_plan_refit_particles */
};

/* ---------------------------------------------------------------- library */
int drpo_version(void);
int64_t drpo_abi_sizeof(const char* struct_name);   /* binding self-check */
/* the value of an enum constant or DRPO_UPSTREAM_* macro of this header by its name
 * ("DRPO_ACT_RELU"), -1 for an unknown name: a binding's mirrors are checked against it */
int64_t drpo_abi_const(const char* name);
const char* drpo_last_error(void);
/* SHA-256 (hex) of the csrc/include sources this binary was built from; the Python
 * binding refuses a library whose digest differs from the sources beside it */
const char* drpo_build_digest(void);
int drpo_event_create(void** ev);
int drpo_event_destroy(void* ev);
int drpo_event_record(void* ev, drpo_stream_t stream);
int drpo_event_elapsed_ms(float* ms /* host */, void* start, void* stop);
int drpo_stream_wait_event(drpo_stream_t stream, void* ev);   /* hipStreamWaitEvent (cross-stream hand-off) */

/* ---------------------------------------------------------------- rollout
 * Replaces SMBPO.rollout (src/smbpo.py:229-249) together with
 * BatchedGaussianEnsemble.sample (src/dynamics.py:198-203, _forward1 :112-122),
 * SquashedGaussianPolicy.act(eval=False) (src/policy.py:77-97), the env
 * check_done / check_violation / get_constraint_values round trips
 * (src/smbpo.py:63-65) and ConstraintSafetySampleBuffer.extend into the virtual
 * buffer (src/sampling.py:128-145). Rows that are done leave the batch; the
 * buffer receives each step's surviving rows in order, as the reference's
 * next_states[~dones] compaction does. Engine 1 runs one kernel per horizon
 * step; engine 2 (default) keeps each row tile on one workgroup for the whole
 * horizon and orders the rows into the buffer afterwards.                   */
typedef struct {
  int S, A, C, Ha, Hm, B, H;
  int env_id, tracking_surr_start, tracking_n_surr;
  double env_thr0, env_thr1;     /* quadrotor: x/z_threshold (safe-control-gym); cartpole: x_threshold,
                                    th_threshold (SafeInvertedPendulumEnv); unused otherwise */
  const float *aW1, *ab1, *aW2, *ab2, *aW3, *ab3;          /* actor: packed weight mirrors + biases */
  const float *mW1, *mb1, *mW2, *mb2, *dW1, *db1, *dW2, *db2, *lW1, *lb1, *lW2, *lb2; /* ensemble: packed mirrors [E] (member stride drpo_packed_size) + biases [E][out] */
  const float *norm_mean, *norm_std, *min_lv, *max_lv;
  const int* members;            /* host [H]: elite member per step (random.choice, src/dynamics.py:199) */
  const float* replay_states;    /* real buffer states, physical layout */
  int64_t replay_ptr, replay_cap;
  const int64_t* init_idx;       /* [B] chronological indices (np.random.choice) or NULL: device sampling w/o replacement */
  const float* eps_a;            /* [H][B][A] or NULL */
  const float* eps_m;            /* [H][B][S+1] or NULL */
  uint64_t seed, ctr;
  float *vs, *va, *vs2, *vr, *vh;  /* virtual buffer components */
  uint8_t *vd, *vv;
  int64_t* vptr;                 /* device int64 write pointer, advanced by the rollout */
  int64_t vcap;
  void* workspace;               /* drpo_rollout_workspace_size bytes; one rollout at a time per workspace */
  int rows_per_tile;             /* 16 or 32, 0 = auto */
  void** step_events;            /* optional [2*H] events: engine 1 records pair t around step t's kernel,
                                    engine 2 records pair 0 around the fused horizon kernel */
  int engine;                    /* 0 auto, 1 one launch per horizon step, 2 fused horizon (persistent per tile) */
  int eps_layout;                /* eps_a/eps_m rows: 0 compacted per step (reference draw order; engine 1),
                                    1 original batch row (row i of step t = trajectory i; engine 2) */
  const void* env_program;       /* env_id == DRPO_ENV_PROGRAM: a drpo_env_program_t in DEVICE memory (caller-
                                    owned, checked with drpo_env_program_check before its upload, not written
                                    while a rollout runs), C = its row count; unused otherwise */
} drpo_rollout_desc_t;

size_t drpo_rollout_workspace_size(int B, int S, int H);
size_t drpo_rollout_count_offset(int B, int S, int H); /* byte offset of the int64 row count in the workspace */
int drpo_rollout(const drpo_rollout_desc_t* d /* host */, drpo_stream_t stream);

/* The same imagined rollout (src/smbpo.py:229-249), kept per trajectory instead of
 * written into the virtual buffer. drpo_rollout's ordered emit compacts each step's
 * surviving rows, after which no buffer row can be traced to its start state; this
 * entry point adds exactly that, row identity: trajectory i of every output is the
 * rollout from initial state i. It runs the fused engine's horizon kernel and, in
 * place of the emit, a tail that reads the staging trajectory-major.
 *   - `d` is drpo_rollout's descriptor, unchanged. vs .. vv, vptr and vcap are ignored
 *     (NULL / 0 allowed): neither the virtual buffer nor its pointer is written. Every
 *     other check of drpo_rollout applies. Fused engine only: H <= 128, engine 0 or 2,
 *     recorded draws (eps_a / eps_m) in original-row layout (eps_layout 1).
 *   - workspace: drpo_rollout_workspace_size(B, S, H) bytes.
 *   - A row is alive at step 0, and at step t + 1 iff it was alive at t and not done
 *     there; len[i] in 1..H counts its steps. Every output is optional (NULL skips it)
 *     except len; every element of a given output is written, those at or beyond a
 *     row's length as zero.
 *   - ret[i] = sum_{t < len} weights[t] * rewards[i][t], accumulated in step order in
 *     double without contraction and rounded to float32 once; hmax propagates NaN. */
typedef struct {            /* all device pointers */
  int32_t* len;             /* [B], required */
  float* states;            /* [B][H+1][S]: [i][t] the state at the start of step t, [i][len] the last next state */
  float* actions;           /* [B][H][A] */
  float* rewards;           /* [B][H] */
  float* constraint_values; /* [B][H][C] */
  uint8_t* dones;           /* [B][H] */
  uint8_t* violations;      /* [B][H] */
  const double* weights;    /* [H] per-step weights of ret (discount^t); required iff ret != NULL; not written
                               while the call runs */
  float* ret;               /* [B] */
  float* hmax;              /* [B][C]: max_{t < len} constraint_values[i][t][c] */
  int32_t* first_violation; /* [B]: smallest t whose violation bit is set, -1 if none */
  uint8_t* terminated;      /* [B]: the done bit of step len - 1; 0 = cut by the horizon */
} drpo_rollout_traj_t;

int drpo_rollout_trajectories(const drpo_rollout_desc_t* d /* host */, const drpo_rollout_traj_t* out /* host */,
                              drpo_stream_t stream);

/* The imagined rollout (src/smbpo.py:229-249) from given (state, action) pairs: the
 * first `steps` steps of trajectory i take actions[i][t] in place of the policy's
 * action (src/smbpo.py:238, the actor.act call), later steps are the policy's again.
 * The reference has no counterpart: its rollout always asks the actor.
 *   - Everything of drpo_rollout_trajectories holds: its descriptor, outputs and checks.
 *     given == NULL or steps == 0 is that call. steps < 0, steps > H, or steps > 0 with
 *     NULL actions: DRPO_EINVAL before any launch.
 *   - An action is used as given, neither clamped nor squashed: pass post-tanh actions,
 *     as drpo_rollout_traj_t.actions holds them (whose layout `actions` shares).
 *   - The draws are keyed by (row, step, kind): a given step makes no action draw and
 *     shifts no other, so every model draw and every later action draw is the one the
 *     call without `given` makes. With steps == H the actor is never evaluated. */
typedef struct {
  const float* actions;   /* device [B][steps][A], trajectory-major; not written while the call runs */
  int steps;              /* K: steps 0 .. K-1 take actions[i][t] in place of the policy's action; 1 <= K <= H */
} drpo_rollout_given_t;

int drpo_rollout_trajectories_given(const drpo_rollout_desc_t* d /* host */,
                                    const drpo_rollout_given_t* given /* host; NULL or steps == 0: none */,
                                    const drpo_rollout_traj_t* out /* host */, drpo_stream_t stream);

/* The imagined rollout (src/smbpo.py:229-249) under the controller that drives the real
 * environment: the actor behind the safety shield (SMBPO._shielded_action,
 * src/smbpo.py:124-136). Each step, after a ~ actor(s): the certificate Qc(s, a) of the
 * constraint critic (src/ssac.py:64-92), max over its Cq outputs of mu_c + std_ratio *
 * std_c (distributional) or of mu_c, the first maximum winning a tie; where it exceeds
 * `threshold` (the float comparison of drpo_shield_select mode 1) the step takes the safe
 * actor's mean action tanh(mu_safe(s)) instead. All inside the fused horizon kernel.
 *   - Everything of drpo_rollout_trajectories holds: its descriptor, outputs and checks.
 *     shield == NULL is that call.
 *   - The shield makes and moves no draw: every action and model draw is the one the
 *     unshielded call makes, so the two runs of the same start states are paired.
 *   - Shapes: the safe actor has the actor's shape (S -> Ha -> Ha -> 2A); the critic's
 *     trunk is S+A -> Hc -> Hc (ReLU, ReLU output), each head Hc -> Hc -> Cq (the
 *     reference's ConstraintCritic: trunk_layers 2, head_layers 1). 1 <= Hc <= 256,
 *     1 <= Cq <= 8, no NULL safe-actor / trunk / mean-head pointer, the log-std head
 *     present iff distributional: anything else DRPO_EINVAL before any launch.
 *   - interventions / certificate: [B][H], either may be NULL; written for the steps a
 *     row is alive at, zero at and beyond its length (zero-filled on the stream first). */
typedef struct {
  const float *sW1, *sb1, *sW2, *sb2, *sW3, *sb3;   /* safe actor: packed weight mirrors + biases */
  const float *cW1, *cb1, *cW2, *cb2;               /* critic trunk */
  const float *qW1, *qb1, *qW2, *qb2;               /* mean head */
  const float *zW1, *zb1, *zW2, *zb2;               /* log-std head; NULL when !distributional */
  int Hc, Cq, distributional;
  float std_ratio, log_std_min, log_std_max;        /* std_c = exp(soft clamp of the raw log-std into [min, max]) */
  float threshold;
  uint8_t* interventions;   /* device [B][H]: 1 where the step took the safe actor's action */
  float* certificate;       /* device [B][H]: the certificate of the actor's action */
} drpo_rollout_shield_t;

int drpo_rollout_trajectories_shielded(const drpo_rollout_desc_t* d /* host */,
                                       const drpo_rollout_shield_t* shield /* host; NULL: none */,
                                       const drpo_rollout_traj_t* out /* host */, drpo_stream_t stream);

/* The imagined rollout under the controller every evaluation runs: the actor behind the
 * linear shield (sample_episodes_batched with shield_type 'linear', src/sampling.py:430-437).
 * K candidates; blend j = 0 .. K-1 is candidate k = K-1-j of drpo_shield_mix, with its
 * arithmetic: j = 0 the policy's action, j = K-1 the safe actor's tanh(mu_safe(s)). A row
 * takes the smallest j < K-1 whose certificate (that of drpo_rollout_trajectories_shielded)
 * is <= shield->threshold (the float comparison of drpo_shield_select mode 2: a NaN does
 * not qualify), and j = K-1 if none is: the reference's "start from a_safe, later
 * candidates override". The safe action's own certificate decides nothing and is not
 * computed. One certificate pass per candidate tried, inside the fused horizon kernel; a
 * tile's passes end when none of its alive rows is undecided, so a tile whose rows all
 * pass at j = 0 costs what the threshold shield costs and never runs the safe actor.
 *   - Everything of drpo_rollout_trajectories_shielded holds: its descriptors, outputs and
 *     checks, no draw made or moved. shield->certificate stays the certificate of the
 *     policy's action, shield->interventions is (j != 0). linear == NULL is that call.
 *   - linear != NULL with shield == NULL, or candidates outside 2..32: DRPO_EINVAL before
 *     any launch or memset. With candidates == 2 the controller is the threshold shield
 *     (but for a NaN certificate, which intervenes here and not there).
 *   - An automatic 32-row tile that no longer fits the LDS with the [rows][16] floats this
 *     adds falls back to 16 rows. */
typedef struct {
  int candidates;      /* K, 2..32 (the reference: 11) */
  uint8_t* blend;      /* device [B][H] or NULL: j of the action taken; 0 at and beyond a row's length */
} drpo_rollout_linear_t;

int drpo_rollout_trajectories_linear(const drpo_rollout_desc_t* d /* host */,
                                     const drpo_rollout_shield_t* shield /* host */,
                                     const drpo_rollout_linear_t* linear /* host; NULL: the threshold shield */,
                                     const drpo_rollout_traj_t* out /* host */, drpo_stream_t stream);

/* The imagined rollout under the shielded controller from proposed actions: "what would the
 * controller execute if this is what is proposed". SMBPO._shielded_action (src/smbpo.py:124-136)
 * passes a proposed action through the certificate before the environment sees it; here the
 * proposal of steps t < given->steps of trajectory i is given->actions[i][t] in place of the
 * actor's sample, and the shield of the step is the one of the two calls above: the
 * threshold shield (linear == NULL), or the linear shield (src/sampling.py:430-437), whose
 * blend j = 0 is then the proposal. Steps t >= given->steps are those calls' steps.
 *   - Everything of drpo_rollout_trajectories_given and of drpo_rollout_trajectories_shielded
 *     (linear != NULL: of drpo_rollout_trajectories_linear) holds: their descriptors, outputs
 *     and checks. given == NULL, given->steps == 0 or shield == NULL are those calls and are
 *     refused here: DRPO_EINVAL before any launch or memset.
 *   - drpo_rollout_traj_t.actions holds the executed actions: the proposal where the shield
 *     let it pass, else the safe actor's (or the blend's). A proposal is judged as given,
 *     neither clamped nor squashed.
 *   - At a step t < given->steps shield->certificate is the certificate of the proposal,
 *     shield->interventions and linear->blend mean what they mean in the calls above.
 *   - No draw is made or moved: a given step makes no action draw and shifts no other, the
 *     shield draws nothing. At threshold +inf the call computes what
 *     drpo_rollout_trajectories_given computes; with given->steps == H the actor is never
 *     evaluated, the safe actor only in tiles with an intervening row. */
int drpo_rollout_trajectories_proposed(const drpo_rollout_desc_t* d /* host */,
                                       const drpo_rollout_given_t* given /* host; steps >= 1 */,
                                       const drpo_rollout_shield_t* shield /* host */,
                                       const drpo_rollout_linear_t* linear /* host; NULL: the threshold shield */,
                                       const drpo_rollout_traj_t* out /* host */, drpo_stream_t stream);

/* Halting the imagined rollout (src/smbpo.py:229-249) where a per-step score says the
 * model should not be trusted. The reference has a fixed horizon and no counterpart. With
 * score[i][t] = scores[i * row_stride + t * step_stride] and len_i the row's natural length:
 * c_i is the first t < len_i with !(score[i][t] <= threshold), so a NaN score halts and a
 * score equal to the threshold does not; halted_at[i] = c_i, or -1 if there is none; a
 * halted row's length becomes c_i (0 is allowed: the row contributes nothing). Steps
 * t >= c_i do not exist; step c_i - 1 stays as staged: its done bit is 0 and its next
 * state is the state the row halted at. Scores at or beyond len_i are never read.
 * A post-pass on the staged horizon: no draw is made, no counter moves, and every step a
 * halted and an unhalted run share is bit-identical.
 * Contract: the two _cut entry points read the staging that the last drpo_rollout_stage /
 * drpo_rollout_trajectories* call left in d->workspace; `d` must have that call's shapes
 * (B, S, A, C, H) and rows_per_tile. Tile counts and in-tile indices read back from the
 * workspace are clamped to the tile, so a caller that breaks this gets wrong rows, never
 * an access outside the workspace or the buffer.
 * DRPO_EINVAL before any launch: a null cut or scores, a zero stride, a NaN threshold,
 * engine 1, H above DRPO_ROLLOUT_FUSED_MAX_H, and whatever drpo_rollout refuses. */
typedef struct {
  const float* scores;   /* device; [H][B] staging order (row_stride 1, step_stride B), [B][H] trajectory order
                            (row_stride H, step_stride 1) or any other strided layout; not written while a call runs */
  int64_t row_stride;    /* in elements, != 0 */
  int64_t step_stride;   /* in elements, != 0 */
  float threshold;       /* not NaN; +inf halts NaN scores only, -inf every row at step 0 */
  int32_t* halted_at;    /* device [B] or NULL */
} drpo_rollout_cut_t;

/* The first half of drpo_rollout (src/smbpo.py:229-249): its checks and the fused
 * engine's horizon kernel (engine 1 is refused), which stages every row's steps in the
 * workspace and copies the buffer pointer there. Nothing is emitted: neither the virtual
 * buffer nor *vptr is written. Records the event pair of drpo_rollout's engine 2. */
int drpo_rollout_stage(const drpo_rollout_desc_t* d /* host */, drpo_stream_t stream);

/* The second half of drpo_rollout (src/smbpo.py:229-249) under a cut: shortens the staged
 * rows (one launch for the cut, one that filters each (step, tile) list of alive rows,
 * order kept) and runs the emit tail drpo_rollout would have run, chosen by the same
 * rule. off[H] (drpo_rollout_count_offset) and *vptr advance by the rows actually
 * emitted, which keep the reference's order. */
int drpo_rollout_emit_cut(const drpo_rollout_desc_t* d /* host */, const drpo_rollout_cut_t* cut /* host */,
                          drpo_stream_t stream);

/* The trajectory tail (src/smbpo.py:229-249 per trajectory) again under a cut, on the
 * staging of the preceding drpo_rollout_trajectories* call in any of its five forms:
 * rewrites every output given as drpo_rollout_trajectories defines it with len[i] the new
 * length, 0..H. A halted row's terminated is 0 and its first_violation -1 unless it lies
 * before the cut; ret sums the kept steps in the same double order. A row of length 0:
 * states[i][0] the start state, every other element zero, ret 0, hmax -inf (the
 * identity of max). The shield's outputs are not this call's: the caller masks them. */
int drpo_rollout_trajectories_cut(const drpo_rollout_desc_t* d /* host */, const drpo_rollout_cut_t* cut /* host */,
                                  const drpo_rollout_traj_t* out /* host */, drpo_stream_t stream);

/* Host only: the byte offsets in the workspace of the fused engine's staged states
 * ([H][B][S] float32) and actions ([H][B][A] float32) of the rollout (src/smbpo.py:229-249),
 * step-major and indexed by original row; the step of a row is staged iff the row was
 * alive at it, every other slot holds whatever was there. For viewing the staged
 * (state, action) rows without a copy. DRPO_EINVAL for a non-positive shape or a null output. */
int drpo_rollout_staging_offsets(int B, int S, int H, size_t* st_s /* host */, size_t* st_a /* host */);

/* Model-based lookahead of the two critics along imagined trajectories: for every row and
 * every k = 0..H, the k-step value expansion sum_{t<k} gamma^t r_t + gamma^k min Q(s_k, a_k)
 * and the constraint critic's own backup (compute_cons_target, src/ssac.py:284-294, inside
 * the critic loss src/ssac.py:304-413) unrolled k steps along the trajectory and closed with
 * Qc(s_k, a_k). The reference has one-step targets only and no counterpart. A post-pass on the
 * trajectory-major tensors of drpo_rollout_trajectories* (after a cut as well): it needs no
 * workspace and no staging, makes no draw and writes nothing but its two outputs. The critics'
 * values are inputs: the caller evaluates them with the stand-alone forwards.
 * With len_i = lengths[i] clamped to 0..H, term_i = terminated[i], w = weights, g = gamma, and
 * the critics' training units (src/smbpo.py:260-270), formed in double from the float32 inputs:
 *   r'_t = rewards[i][t] (* reward_scale if reward_scale != 0) (+ alive_bonus if alive_bonus != 0)
 *   h'_t = constraint_values[i][t][c] * constraint_scale;  h'_t += (h'_t > 0 ? 1 : 0) * constraint_offset
 * entry k of row i, with kk = min(k, len_i) (entries beyond a row's length repeat the one at it):
 *   bootstrap  kk < len_i: q = step_q[i][kk], x = step_qc[i][kk][c];
 *              kk == len_i and !term_i: q = terminal_q[i], x = terminal_qc[i][c];
 *              kk == len_i and term_i: none (the scan below starts from x = 0.0, which the done
 *              select of the row's last step replaces; terminal_q / terminal_qc are not used)
 *   value[i][k]  acc = 0.0; acc += w[t] * r'_t for t = 0 .. kk-1 in that order; + w[kk] * q if
 *              there is a bootstrap
 *   certificate[i][k][c]  from x, for t = kk-1 down to 0:
 *              mode 0 (reachability): x = dones[i][t] ? h'_t : (1 - g) * h'_t + g * max(h'_t, x),
 *                a NaN in either operand of the max stays (torch.maximum);
 *              mode 1 (cost): x = dones[i][t] ? v_t : v_t + g * x, v_t = violations[i][t] as 0 / 1
 *              (the same for every c); the done branch is a select, never a product with zero
 * Every operation is one double add or multiply, round to nearest, nothing contracted, in the
 * order written; the result is rounded to float32 once and a NaN stored as 0x7FC00000. A row of
 * length 0 has every entry equal to its bootstrap (w[0] * terminal_q; terminal_qc).
 * Every element of every given output is written. DRPO_EINVAL before any launch: a null
 * descriptor or input pointer (violations may be NULL in mode 0), H outside
 * 1..DRPO_ROLLOUT_FUSED_MAX_H, C < 1, a mode other than 0 / 1, gamma not finite or outside
 * [0, 1], B < 0, or a B beyond one grid (2^24 rows at the longest horizons, where a workgroup
 * takes one row). B == 0: DRPO_OK without a launch. */
typedef struct {
  int B, H, C, mode;            /* rows, horizon, critic outputs; mode 0 reachability, 1 cost */
  double gamma;
  double reward_scale, alive_bonus, constraint_scale, constraint_offset;
  /* inputs, device, not written while the call runs */
  const float* rewards;            /* [B][H] */
  const float* constraint_values;  /* [B][H][C]; required, though mode 1 does not read it */
  const uint8_t* dones;            /* [B][H] */
  const uint8_t* violations;       /* [B][H]; read in mode 1 only, may be NULL in mode 0 */
  const int32_t* lengths;          /* [B]; clamped to 0..H as read */
  const uint8_t* terminated;       /* [B] */
  const double* weights;           /* [H + 1]: gamma^k */
  const float* step_q;             /* [B][H]: min Q at (states[i][t], actions[i][t]) */
  const float* step_qc;            /* [B][H][C]: Qc at the same rows */
  const float* terminal_q;         /* [B]: min Q at (states[i][len_i], the policy's mean action there) */
  const float* terminal_qc;        /* [B][C]: Qc at (states[i][len_i], the safe actor's mean action there) */
  /* outputs, device; either may be NULL */
  float* value;                    /* [B][H + 1] */
  float* certificate;              /* [B][H + 1][C] */
} drpo_rollout_lookahead_t;

int drpo_rollout_lookahead(const drpo_rollout_lookahead_t* d /* host */, drpo_stream_t stream);

/* The adjoint of the imagined rollout: the reverse sweep along stored trajectories of the
 * deterministic model step, which the reference (src/smbpo.py:229-249, rolled forward only) has
 * no counterpart of. That step is s_{t+1} = s_t + diff_m(x_t)[:S], r_t = diff_m(x_t)[S] with
 * x_t = [(s_t - mean) / (std + 1e-6), a_t] and diff_m member m's trunk -> diff-head output
 * (S+1 columns): what a drpo_rollout_trajectories_given run without model noise executes
 * (_forward1's means, src/dynamics.py:112-122). The call backs upstream gradients of the states
 * and rewards of such a run through it, to the actions and the start state.
 * For row i, with len = lengths[i] clamped to 0..H, m_t = members[t] and J_t the Jacobian of
 * member m_t's diff-head output with respect to x, taken at the stored (states[i][t], actions[i][t]):
 *   lam = g_states[i][len]                              [S]; entries beyond len are never read
 *   for t = len-1 .. 0:
 *       dx = J_t^T [lam, g_rewards[i][t]]               [S+A]
 *       grad_actions[i][t] = dx[S:]
 *       lam = g_states[i][t] + lam + dx[:S] / (std + 1e-6)
 *   grad_start[i] = lam;   grad_actions[i][t] = 0 for t >= len
 * g_states and g_rewards are the upstream gradients; either may be NULL, meaning zeros (and
 * computing what explicit zeros compute). Dones, lengths and constraint checks are constants of
 * the sweep; the log-var head is not read. The sum is formed left to right as written, in float32;
 * the products are exact-float32 MFMA chains. One launch: a workgroup keeps a 16-row tile for the
 * whole sweep, each step's forward (trunk, the diff head's hidden layer) and four backward-data
 * products on chip; only grad_actions and, at the end, grad_start leave it. Every element of both
 * outputs is written; the call makes no draw and has no workspace the caller must zero.
 * DRPO_EINVAL before any launch: a null descriptor or required pointer, H outside
 * 1..DRPO_ROLLOUT_FUSED_MAX_H, S < 1, A < 1, S + A > 64, S + 1 > 16, a hidden width other than
 * 200 | 256 (drpo_rollout_adjoint_ok: the per-step launches drpo_mlp_forward +
 * drpo_mlp_backward compose the same definition for the others), E < 1, a member index outside
 * 0..E-1, B < 0, or B beyond one grid (a launch takes fewer than 2^32 threads: 2^23 - 1 tiles of
 * 16 rows, 512 threads each). B == 0: DRPO_OK without a launch. */
typedef struct {
  int64_t B;                /* rows */
  int H, S, A, Hm, E;       /* horizon, state and action dims, hidden width, ensemble members */
  /* the ensemble's trunk and diff head as drpo_rollout_desc_t names them: packed forward mirrors
     and biases of member 0 (member stride drpo_packed_size / the layer's outputs), swish hidden
     layers; the output layer's forward is not run (it is linear and s_{t+1} is stored) */
  const float *mW1, *mb1, *mW2, *mb2, *dW1, *db1;
  /* the packed TRANSPOSED mirrors of the four layers (drpo_mlp_bwd_layer_t.W), member 0 */
  const float *mT1, *mT2, *dT1, *dT2;
  const float *norm_mean, *norm_std;   /* [S] */
  const int* members;       /* host [H] */
  /* the stored run, device, not written while the call runs */
  const float* states;      /* [B][H+1][S] */
  const float* actions;     /* [B][H][A] */
  const int32_t* lengths;   /* [B]; clamped to 0..H as read */
  const float* g_states;    /* [B][H+1][S] or NULL */
  const float* g_rewards;   /* [B][H] or NULL */
  /* outputs, device */
  float* grad_actions;      /* [B][H][A] */
  float* grad_start;        /* [B][S] */
} drpo_rollout_adjoint_t;

int drpo_rollout_adjoint(const drpo_rollout_adjoint_t* d /* host */, drpo_stream_t stream);

/* Sampling-based planning on the learned model (MPPI / CEM over action sequences, for P start
 * states at once): the two launches around one drpo_rollout_trajectories_given run of
 * B = P * N rows and the terminal critic forwards. The reference has no counterpart on the
 * device (its MPC baseline, src/viz_tracking/opt_controller.py, solves one state at a time on
 * the host).
 *
 * drpo_plan_sample: the candidates cand[P * N][K][A] of one iteration from mean, std and
 * incumbent (each [P][K][A]). Row r = p * N + n, element (r, t, a):
 *   n == 0: incumbent[p][t][a], copied bit for bit;
 *   n >= 1: x = fmaf(std[p][t][a], z, mean[p][t][a]); x = x < lo ? lo : x; x = x > hi ? hi : x
 *           (selects: a NaN stays), z = normal_at(idx = (r * K + t) * A + a, seed, ctr,
 *           DRPO_PLAN_SITE), the generator of every normal_at site (counter words
 *           (idx >> 2, idx >> 34, site, ctr), lane idx & 3).
 * Every element of cand is written. DRPO_EINVAL before any launch: a null descriptor or
 * pointer, P < 0, N outside 2..DRPO_PLAN_MAX_CANDIDATES, K < 1, A < 1, lo > hi or either NaN, or
 * more elements than one grid (2^40). P == 0: DRPO_OK without a launch. */
typedef struct {
  int P, N, K, A;          /* start states, candidates per state, given steps, action dim */
  float lo, hi;            /* the clamp of the drawn candidates */
  uint64_t seed, ctr;
  const float* mean;       /* [P][K][A], device */
  const float* std;        /* [P][K][A] */
  const float* incumbent;  /* [P][K][A] */
  float* cand;             /* [P * N][K][A], out */
} drpo_plan_sample_t;

int drpo_plan_sample(const drpo_plan_sample_t* d /* host */, drpo_stream_t stream);

/* drpo_plan_sample_ar: drpo_plan_sample with AR(1) noise along the steps (time-correlated
 * candidates for receding-horizon control). Row r = p * N + n, action dimension a:
 *   n == 0: incumbent[p][t][a], copied bit for bit, for every t;
 *   n >= 1: z_t = normal_at(idx = (r * K + t) * A + a, seed, ctr, DRPO_PLAN_SITE), the index and
 *           site of drpo_plan_sample (the same draws), and in ordered double arithmetic, nothing
 *           contracted:
 *             u_0 = (double)z_0;  u_t = corr * u_{t-1} + innov * (double)z_t   (t = 1..K-1)
 *             x_t = fmaf(std[p][t][a], (float)u_t, mean[p][t][a]);
 *             x_t = x_t < lo ? lo : x_t; x_t = x_t > hi ? hi : x_t   (selects: a NaN stays).
 * innov = sqrt(1 - corr^2) keeps u_t at unit variance; the relation is the caller's and is not
 * checked. corr = 0, innov = 1 gives drpo_plan_sample's cand bit for bit. Every element of cand
 * is written. DRPO_EINVAL before any launch: whatever drpo_plan_sample refuses, corr outside
 * [0, 1) or NaN, innov outside (0, 1] or NaN. P == 0: DRPO_OK without a launch. */
typedef struct {
  int P, N, K, A;          /* start states, candidates per state, given steps, action dim */
  float lo, hi;            /* the clamp of the drawn candidates */
  uint64_t seed, ctr;
  const float* mean;       /* [P][K][A], device */
  const float* std;        /* [P][K][A] */
  const float* incumbent;  /* [P][K][A] */
  float* cand;             /* [P * N][K][A], out */
  double corr, innov;      /* the lag-1 correlation and the innovation's scale */
} drpo_plan_sample_ar_t;

int drpo_plan_sample_ar(const drpo_plan_sample_ar_t* d /* host */, drpo_stream_t stream);

/* drpo_plan_shift: the warm start of the next control step from mean, std and incumbent (each
 * [P][K][A]) of the previous one, in one launch. Element (p, t, a):
 *   reset && reset[p]:  mean_out = incumbent_out = tail ? tail[p][a] : 0.0f; std_out = fresh_std;
 *   else t + shift < K: mean_out = mean[p][t + shift][a], incumbent_out = incumbent[p][t + shift][a],
 *                       copied bit for bit; s = std[p][t + shift][a];
 *                       std_out = s < std_floor ? std_floor : s   (a select: a NaN stays);
 *   else:               mean_out = tail ? tail[p][a] : mean[p][K - 1][a],
 *                       incumbent_out = tail ? tail[p][a] : incumbent[p][K - 1][a]; std_out = fresh_std.
 * Copies and selects only. Every element of the three outputs is written; nothing else is.
 * DRPO_EINVAL before any launch: a null descriptor or pointer (reset and tail may be NULL), P < 0,
 * K < 1, A < 1, more than 2^40 elements, shift outside 0..K, fresh_std not finite or <= 0,
 * std_floor NaN or negative, an output equal to an input (a shifted read races an in-place
 * write). P == 0: DRPO_OK without a launch. */
typedef struct {
  int P, K, A, shift;            /* start states, given steps, action dim, steps to drop */
  float fresh_std, std_floor;    /* the std of the fresh steps; the floor of the kept steps' */
  const float* mean;             /* [P][K][A], device */
  const float* std;              /* [P][K][A] */
  const float* incumbent;        /* [P][K][A] */
  const uint8_t* reset;          /* [P] or NULL: non-zero starts the state cold */
  const float* tail;             /* [P][A] or NULL: the action of the fresh steps */
  float* mean_out;               /* [P][K][A] */
  float* std_out;                /* [P][K][A] */
  float* incumbent_out;          /* [P][K][A] */
} drpo_plan_shift_t;

int drpo_plan_shift(const drpo_plan_shift_t* d /* host */, drpo_stream_t stream);

/* drpo_plan_refit: scores and ranks the candidates of every start state and refits mean and
 * std, on the trajectory-major tensors that the run of B = P * N rows (row r = p * N + n) and
 * horizon H under cand left. One workgroup serves one start state.
 * a. Score. score[r] is exactly value[r][H] of drpo_rollout_lookahead above (the critics'
 *    training units of src/smbpo.py:260-270, the backup of src/ssac.py:284-294), and cert[r]
 *    the maximum over c (a NaN stays) of its certificate[r][H][c]: at k = H a row's bootstrap
 *    is its terminal one (kk = min(H, len_r) = len_r), so step_q / step_qc are not inputs.
 *    The same ordered double operations, nothing contracted, lengths clamped to 0..H as read;
 *    each rounded to float32 once, a NaN stored as 0x7FC00000.
 * b. Order, on the float32 values as stored. A row is valid if neither its score nor its cert
 *    is NaN, feasible if valid and cert <= threshold. A state's order: the feasible rows by
 *    score descending, then the valid infeasible rows by cert ascending, then the invalid rows;
 *    ties to the lower n. rank[r]: the row's position; n_feasible[p]; best[p]: n of rank 0.
 * c. Elites. Ke = min(elites, n_feasible) if n_feasible > 0, else min(elites, n_valid); the
 *    elites are the rows of rank < Ke. With key = score if the state has a feasible row, else
 *    -cert, an elite's weight is w = exp(((double)key - (double)key_best) / temperature),
 *    where the difference of equal keys is 0 (two infinities included) and temperature +inf
 *    gives w = 1 exactly. Every other row has w = 0.
 * d. Refit, per (t, a) of the K given steps, over the rows with w > 0 in the order n = 0..N-1,
 *    in ordered double arithmetic (nothing contracted):
 *      m = sum(w * x) / sum(w);  v = sum(w * ((x - m) * (x - m))) / sum(w),  x = cand[r][t][a]
 *      mean_out = (1 - momentum) * m + momentum * mean_in
 *      std_out = (1 - momentum) * sqrt(v) + momentum * std_in, raised to min_std if below it
 *    stored as float32. With no valid row, or when sum(w) is not positive, mean_in and std_in
 *    pass through; with no valid row best = 0. mean_out / std_out may alias their inputs.
 * e. best_actions[p] = cand[p * N + best[p]], copied; best_score, best_cert, best_feasible.
 * Every element of every given output is written; nothing else is. DRPO_EINVAL before any
 * launch: a null descriptor, input or per-state output (violations may be NULL in mode 0), P < 0
 * or P * N beyond int32, N outside 2..DRPO_PLAN_MAX_CANDIDATES, H outside
 * 1..DRPO_ROLLOUT_FUSED_MAX_H, K outside 1..H, A < 1, C < 1, a mode other than 0 / 1, gamma not
 * finite or outside [0, 1], elites outside 1..N, temperature not > 0 (+inf is allowed), momentum
 * outside [0, 1), min_std negative or not finite, a NaN threshold. P == 0: DRPO_OK without a
 * launch. */
typedef struct {
  int P, N, H, K, A, C, mode, elites;
  double gamma;
  double reward_scale, alive_bonus, constraint_scale, constraint_offset;
  double temperature, momentum, min_std;
  float threshold;
  int pad_;
  /* inputs, device, not written while the call runs (mean_in / std_in excepted, see d.) */
  const float* rewards;            /* [B][H] */
  const float* constraint_values;  /* [B][H][C]; required, though mode 1 does not read it */
  const uint8_t* dones;            /* [B][H] */
  const uint8_t* violations;       /* [B][H]; read in mode 1 only, may be NULL in mode 0 */
  const int32_t* lengths;          /* [B]; clamped to 0..H as read */
  const uint8_t* terminated;       /* [B] */
  const double* weights;           /* [H + 1]: gamma^k */
  const float* terminal_q;         /* [B] */
  const float* terminal_qc;        /* [B][C] */
  const float* cand;               /* [B][K][A] */
  const float* mean_in;            /* [P][K][A] */
  const float* std_in;             /* [P][K][A] */
  /* outputs, device */
  float* mean_out;                 /* [P][K][A] */
  float* std_out;                  /* [P][K][A] */
  float* best_actions;             /* [P][K][A] */
  int32_t* best;                   /* [P] */
  int32_t* n_feasible;             /* [P] */
  float* best_score;               /* [P] */
  float* best_cert;                /* [P] */
  uint8_t* best_feasible;          /* [P] */
  /* per row; each may be NULL */
  float* score;                    /* [B] */
  float* cert;                     /* [B] */
  int32_t* rank;                   /* [B] */
  float* weight;                   /* [B]: w rounded to float32 */
} drpo_plan_refit_t;

int drpo_plan_refit(const drpo_plan_refit_t* d /* host */, drpo_stream_t stream);

/* drpo_plan_refit_particles: drpo_plan_refit over G runs of the same candidates, one per
 * ensemble member (particle): planning over the ensemble, risk-aware. Every per-row input is
 * member-major [G][B][...], B = P * N (run j's row r at flat row j * B + r), the layout that G
 * runs stacked leave; cand stays [B][K][A]. One workgroup serves one start state.
 * Member values. member_score[j][r] and member_cert[j][r] are exactly score[r] and cert[r] of
 *    drpo_plan_refit's step a on run j's tensors (the same operations), each rounded to float32
 *    once, a NaN stored as 0x7FC00000. From them, as stored:
 * Score. With T = score_tail (1..G), order the members by (member score ascending, j ascending);
 *    score[r] is the double sum of the first T in that order, added in that order, nothing
 *    contracted, divided by (double)T and rounded to float32 once. T = 1: the worst member;
 *    T = G: the mean over all members; between them the mean of the lower tail (CVaR). A NaN
 *    member score makes the score NaN (0x7FC00000).
 * Cert. cert_mode 0: the maximum over j = 0..G-1 (a NaN stays): every member must certify.
 *    cert_mode 1: the double sum in j order divided by (double)G, rounded to float32 once.
 * Spread. With m = (sum_j s_j) / G in j order, score_spread[r] = sqrt(sum_j (s_j - m)^2 / G) in
 *    ordered double arithmetic, stored as float32 (a NaN as 0x7FC00000).
 * Steps b-e are drpo_plan_refit's on the aggregated float32 score and cert (the same code).
 * With G = 1 every output is bit-equal to drpo_plan_refit's (score_spread is 0 or NaN).
 * Every element of every given output is written; nothing else is. DRPO_EINVAL before any
 * launch: whatever drpo_plan_refit refuses, G outside 1..DRPO_PLAN_MAX_PARTICLES, score_tail
 * outside 1..G, a cert_mode other than 0 / 1, G * P * N beyond int32. P == 0: DRPO_OK without a
 * launch. */
typedef struct {
  int P, N, H, K, A, C, mode, elites;
  double gamma;
  double reward_scale, alive_bonus, constraint_scale, constraint_offset;
  double temperature, momentum, min_std;
  float threshold;
  int pad_;
  /* inputs, device, as drpo_plan_refit_t's with G * B rows where it has B */
  const float* rewards;            /* [G][B][H] */
  const float* constraint_values;  /* [G][B][H][C] */
  const uint8_t* dones;            /* [G][B][H] */
  const uint8_t* violations;       /* [G][B][H]; read in mode 1 only, may be NULL in mode 0 */
  const int32_t* lengths;          /* [G][B]; clamped to 0..H as read */
  const uint8_t* terminated;       /* [G][B] */
  const double* weights;           /* [H + 1]: gamma^k */
  const float* terminal_q;         /* [G][B] */
  const float* terminal_qc;        /* [G][B][C] */
  const float* cand;               /* [B][K][A] */
  const float* mean_in;            /* [P][K][A] */
  const float* std_in;             /* [P][K][A] */
  /* outputs, device, as drpo_plan_refit_t's: per state, and per row of the aggregate */
  float* mean_out;                 /* [P][K][A] */
  float* std_out;                  /* [P][K][A] */
  float* best_actions;             /* [P][K][A] */
  int32_t* best;                   /* [P] */
  int32_t* n_feasible;             /* [P] */
  float* best_score;               /* [P] */
  float* best_cert;                /* [P] */
  uint8_t* best_feasible;          /* [P] */
  float* score;                    /* [B], may be NULL */
  float* cert;                     /* [B], may be NULL */
  int32_t* rank;                   /* [B], may be NULL */
  float* weight;                   /* [B], may be NULL */
  /* the particles */
  int G;                           /* runs, 1..DRPO_PLAN_MAX_PARTICLES */
  int score_tail;                  /* T: the score is the mean of the T lowest member scores */
  int cert_mode;                   /* 0: max over the members; 1: their mean */
  int pad2_;
  float* member_score;             /* [G][B], may be NULL */
  float* member_cert;              /* [G][B], may be NULL */
  float* score_spread;             /* [B], may be NULL */
} drpo_plan_refit_particles_t;

int drpo_plan_refit_particles(const drpo_plan_refit_particles_t* d /* host */, drpo_stream_t stream);

/* batched env constraint functions, e.g. PointRobot.get_constraint_values /
 * check_violation / check_done (src/env/point_robot.py:96-131); h is [n][C] */
int drpo_env_constraints(int env_id, int tracking_surr_start, int tracking_n_surr, double env_thr0,
                         double env_thr1, const float* states, int64_t n, int S, uint8_t* done,
                         uint8_t* violation, float* h, drpo_stream_t stream);
/* the same for a constraint program (device memory, C = its row count); drpo_env_constraints
 * refuses DRPO_ENV_PROGRAM */
int drpo_env_constraints_program(const drpo_env_program_t* dev_prog, int C, const float* states, int64_t n, int S,
                                 uint8_t* done, uint8_t* violation, float* h, drpo_stream_t stream);

/* ---------------------------------------------------------------- safety shields
 * Real-env step shield (SMBPO.step_generator, src/smbpo.py:127-136) and the
 * evaluation shields of sample_episodes_batched (src/sampling.py:423-439).
 * drpo_shield_mix writes the linear shield's K candidate actions
 * mix_i = a_safe*(K-1-i)/(K-1) + a_perf*(1-(K-1-i)/(K-1)) as [K][n][A] (scored by one
 * constraint-critic forward over K*n rows); drpo_shield_select picks per row:
 * mode 0 a_perf; mode 1 a_safe where max_C q > threshold (q [n][C]); mode 2 linear
 * shield: a_safe, overridden by mix_i wherever max_C q_i <= threshold (q [K][n][C]). */
int drpo_shield_mix(const float* a_perf, const float* a_safe, int64_t n, int A, int K, float* mixes,
                    drpo_stream_t stream);
int drpo_shield_select(const float* q, int K, int64_t n, int C, int A, int mode, float threshold, const float* a_perf,
                       const float* a_safe, const float* mixes, float* out, drpo_stream_t stream);

/* B distinct indices in [0, N): production stand-in for random_choice(replace=False)
 * (src/torch_util.py:41-48) */
int drpo_sample_without_replacement(int64_t* out, int64_t B, int64_t N, uint64_t seed, uint64_t ctr,
                                    drpo_stream_t stream);

/* ---------------------------------------------------------------- MLPs
 * Fused forward / backward-data / weight-gradient passes for mlp() nets
 * (src/torch_util.py:190-211) and BatchedLinear ensembles (src/dynamics.py:26-52,
 * nbatch = ensemble members). Used by the SAC update (src/ssac.py:437-578),
 * the ensemble fit (src/dynamics.py:143-187) and every network forward.      */
typedef struct {
  const float* W; /* packed forward mirror of the [dout][din] weight (drpo_pack_weights) */
  const float* b; /* [dout] */
  int din, dout, act;
  float* sy;      /* optional: post-activation save [rows][dout] */
  float* sz;      /* optional: pre-activation save */
  int64_t wstride, bstride; /* per batch item (ensemble member): packed-mirror / bias strides */
} drpo_mlp_layer_t;

typedef struct {
  int nl;
  drpo_mlp_layer_t L[3];
} drpo_mlp_net_t;

/* squashed-Gaussian policy head fused into a forward pass: applied to net[0]'s
 * final output (2A columns = [mu | log-std pre-activation]), src/policy.py:88-97 */
enum { DRPO_HEAD_NONE = 0, DRPO_HEAD_SAMPLE = 1, DRPO_HEAD_RSAMPLE = 2, DRPO_HEAD_MEAN = 3 };
typedef struct {
  int mode;            /* DRPO_HEAD_*: 0 none, 1 sample (Normal.sample), 2 rsample, 3 mean only (tanh(mu)) */
  int A;
  const float* eps;    /* [rows][A] recorded draws, or NULL: Philox (launch seed/ctr, this site) */
  uint32_t site;
  float *a, *logp, *u, *e, *amean;   /* optional outputs */
} drpo_policy_head_t;

typedef struct {
  const float* src[3]; /* column-concatenated input sources (e.g. torch.cat([s, a], -1)) */
  int cols[3];
  int ld[3];
  int64_t sstride[3];
  const float* nmean;  /* optional (src[0] - mean) / (std + 1e-6) (src/normalization.py:22-23) */
  const float* nstd;
  float* save_x;       /* optional save of the assembled input */
  drpo_mlp_net_t net[3];
  int nnets;
  int trunk;           /* 1: net[0] trunk, net[1..] heads on its output */
  int64_t rows;
  int nbatch;
  drpo_policy_head_t head;   /* multi-job launches only (mode 0 elsewhere) */
  int split_heads;     /* trunk mode, single launches: one workgroup per (row tile, head); each
                          recomputes the trunk (only head 1's workgroup saves it) -- twice the
                          workgroups for small ensembles (fit: 16 tiles x 7 members) */
  float* ccb_out;      /* multi-job launches, trunk job with paired heads (the constraint critic,
                          src/ssac.py:46-92): per-row max over the C constraints of the quantile
                          bound mu + ccb_ratio * std(log-std raw) (ccb_dist) or of mu, formed from
                          the heads' outputs in the launch (the bound drpo_cc_head computes,
                          src/ssac.py:474-494,536-560); NULL: none */
  int ccb_dist;
  float ccb_ratio, ccb_lmin, ccb_lmax;
  /* multi-job launches: */
  int pair;            /* non-trunk job, 2 nets of ONE shape on the same input (the twin critics; the
                          actor and the safe actor): ONE workgroup runs both as paired layers (one
                          staging, one k-loop per layer pair) instead of one workgroup per net */
  drpo_policy_head_t head2;   /* pair jobs: the fused head of net[1] (head: net[0]'s) */
  drpo_mlp_net_t pre;  /* chain (pre.nl > 0): a policy net run first, in the same workgroup, on the
                          src[0] columns; its head (pre_head, mode 1 or 2) samples the action that
                          is this job's src[1] column block (cols[1] == A) straight from LDS: the
                          next-state policy feeding the target critics / certificate
                          (src/ssac.py:284-294,387-400) without a launch or an HBM round trip */
  drpo_policy_head_t pre_head;
  drpo_mlp_net_t post; /* post chain (post.nl > 0; a trunk job with ccb_out): a net run after the bound in
                          the same workgroup on [src[0] columns (cols[0] wide), the bound] -- the
                          MLPMultiplier lam(s, max_C Qc_ub(s, a)) of src/ssac.py:473-478,548-552
                          without its own launch; its layer saves as any net's */
  float* post_x;       /* optional save of the post net's assembled input [rows][cols[0] + 1] */
} drpo_mlp_fwd_t;

typedef struct {
  const float* W;      /* packed TRANSPOSED mirror of the [dout][din] weight */
  int din, dout, act;
  const float* sy;
  const float* sz;
  float* dz;           /* optional save of dL/dZ for weight gradients */
  int64_t wstride;
  float* dz2;          /* split_heads trunk layers: the second head's partial dL/dZ (trunk
                          dZ = dz + dz2) */
} drpo_mlp_bwd_layer_t;

typedef struct {
  int nl;
  drpo_mlp_bwd_layer_t L[3];
  const float* gout;   /* dL/d(output) [rows][dout_last]: read (and required) only with
                          DRPO_UPSTREAM_GOUT, and never for the trunk of a trunk job */
  float* dx;           /* optional dL/d(input) for input columns [dx_col0, dx_col0 + dx_cols) */
  int dx_col0, dx_cols, dx_accumulate;
} drpo_mlp_bwd_net_t;

typedef struct {
  drpo_mlp_bwd_net_t net[3];
  int nnets;
  int trunk;
  int64_t rows;
  int nbatch;
  int split_heads;     /* trunk mode, single launches, trunk dx unused: one workgroup per (row
                          tile, head) backs its head's gradient through the trunk (linear in
                          the head gradients), writing dz (head 1) / dz2 (head 2) */
  int upstream;        /* where the output gradients come from: DRPO_UPSTREAM_* */
} drpo_mlp_bwd_t;

/* The model fit's NLL loss (src/dynamics.py:136-153,236-253): the inputs of drpo_ens_loss,
 * and of the same arithmetic as the upstream of the ensemble backward launch
 * (drpo_mlp_backward_ens, drpo_ens_fit_fb), where the head outputs' gradients are formed
 * in-kernel and the loss partials are left for the deferred reduction
 * (drpo_mlp_wgrad_reduce). */
typedef struct {
  const float *D, *LVR;        /* diff / raw log-var head outputs [Z][b][S+1] */
  const float* s;              /* raw states [Z][b][S] (member stride s_zstride) */
  int64_t s_zstride;
  const float* t;              /* targets [Z][b][S+1] */
  int64_t t_zstride;
  int64_t b;                   /* rows per member */
  int S, Z;
  const float *minlv, *maxlv;
  const float* gscale;         /* optional device scale of the gradients (NULL = 1) */
  float* part;                 /* loss workspace (drpo_ens_loss_workspace_size) */
} drpo_ens_upstream_t;

/* The actor update's output gradients (src/ssac.py:458-527), formed in-kernel by its
 * backward launches (drpo_mlp_backward_multi_actor): dL/d(Q_k, constraint-critic heads) of
 * the actor / safe-actor losses and the chain rule through rsample + tanh + log_prob. */
typedef struct {
  int64_t B;
  int C, A, distributional;
  float std_ratio, log_std_min, log_std_max;
  const float* lams;            /* MLPMultiplier pre-transform outputs [B], or NULL: fixed_lam */
  float lam_upper_bound, fixed_lam, clamp_lb, clamp_ub;
  const float* u[2];            /* pre-tanh samples of the actor [0] / safe actor [1] [B][A] */
  const float* e[2];            /* their standard-normal draws [B][A] */
  const float* dA[2];           /* dL/d action [B][A] */
  const float* dA2[2];          /* optional second term of dL/d action (NULL) */
  const float* logp;            /* actor log-probs [B] */
  const float* log_alpha;       /* the actor's log-prob terms scaled by exp(*log_alpha) * lp_scale; NULL: none */
  float lp_scale, target_entropy;
  float* alpha_sum;             /* per row tile: sum(logp + target_entropy) of the actor's rows, or NULL
                                   (one float per 16-row tile, overwritten; drpo_optim_seg_t.grad_sum_n) */
} drpo_actor_head_t;

/* drpo_mlp_bwd_t.upstream */
#define DRPO_UPSTREAM_GOUT 0     /* the nets' gout arrays */
#define DRPO_UPSTREAM_CRITIC 1   /* twin-critic job: net k's output gradient is (q_k - y) / B with the soft
                                    Bellman target y of the launch's critic head; adds the critic loss */
#define DRPO_UPSTREAM_CERT 2     /* constraint-critic job (trunk + mean [+ log-std] heads): the
                                    certificate loss gradients of the launch's critic head; adds its loss */
#define DRPO_UPSTREAM_ENS 3      /* ensemble job (trunk + diff / log-var heads): the NLL gradients of the
                                    launch's drpo_ens_upstream_t; writes its loss partials */
#define DRPO_UPSTREAM_ACTOR_CC 4 /* constraint critic at (s, a): lam / B on the max-C certificate bound of
                                    the launch's drpo_actor_head_t (src/ssac.py:474-488) */
#define DRPO_UPSTREAM_SAFE_CC 5  /* constraint critic at (s, a_safe): 1 / B on its max-C bound (:490-494) */
#define DRPO_UPSTREAM_NEG_MEAN 6 /* single net with one output: -1 / B (the actor loss's -mean(Q_k)) */
#define DRPO_UPSTREAM_SQUASH 7   /* actor (net 0 of the launch's head: [0]) / safe actor ([1]): the
                                    squashed-Gaussian backward of the head's action gradients */
#define DRPO_UPSTREAM_SQUASH_SAFE 8

typedef struct {
  const float* dz; /* [rows][dout] */
  const float* y;  /* layer input [rows][din] */
  float* gW;       /* gW += dZ^T Y (no two items of one launch may share gW) */
  float* gb;       /* gb += colsum(dZ) */
  int dout, din;
  int64_t rows;
  int64_t zstride, ystride, gwstride, gbstride;
  int nbatch;
  float* sq;       /* optional clip partials: sq[sq_off + t] = sum of squares of the
                      FINISHED gradient (weights + bias) of output tile t of this item,
                      t < drpo_mlp_wgrad_tiles(item) (summed by drpo_optim_step) */
  int sq_off;
  const float* dz2;  /* optional second dL/dZ term, same layout as dz: the product is
                        (dz + dz2)^T y (a split-heads backward leaves the trunk's dZ as
                        the sum of the two heads' shares) */
} drpo_wgrad_item_t;

/* the reduction step of drpo_ens_loss, as data: run by drpo_mlp_wgrad_reduce */
typedef struct {
  const float* part;   /* the loss workspace */
  int nbx, Z, S1;
  const float *minlv, *maxlv;
  float weight;
  const float* gscale;
  float *mse, *loss, *gmin, *gmax;
} drpo_ens_reduce_t;

/* the safe-SAC critic losses of one update_critic (src/ssac.py:284-435), formed by
 * drpo_mlp_backward_multi_head */
typedef struct {
  int64_t B;
  int C;
  int distributional, deterministic_backup;
  float discount, qc_td_bound, lmin, lmax;
  const float* log_alpha;
  const float *r, *h;
  const uint8_t* d;
  const uint8_t* dc;    /* certificate-target done flags (robust branch: model-predicted); NULL = d */
  const float *q0t, *q1t, *logp2;
  const float *mu_t, *ls_t;
  const float* eps3;
  uint64_t seed, ctr;
  const float *q0, *q1;
  const float *mu, *ls;
  float* loss; /* [2]: critic loss, constraint-critic loss (the sums of loss_part) */
  float* loss_part;   /* per-workgroup loss partials, no atomics: [3][row tiles] = twin 0, twin 1,
                         certificate (summed into loss by a drpo_mlp_wgrad_sums reduction) */
  /* constrained_fcn='cost' (src/ssac.py:306-310): certificate target = violation + discount *
     (1 - done) * mu_t, MSE loss (distributional must be 0); v = the batch's violation flags */
  int cost;
  const uint8_t* v;
} drpo_critic_head_t;

/* one job; head, head2, pair, pre, post, post_x and ccb_out are refused (the multi launch
 * runs them) */
int drpo_mlp_forward(const drpo_mlp_fwd_t* desc /* host */, drpo_stream_t stream);
/* Up to 8 independent forward jobs (different inputs / nets, e.g. every forward of
 * one SAC loss that does not depend on another) in ONE launch, each with an
 * optional fused policy head. jobs_dev: the same descriptors in device memory
 * (read by the kernel; static across calls), jobs_host: for the grid. */
int drpo_mlp_forward_multi(const drpo_mlp_fwd_t* jobs_host, const drpo_mlp_fwd_t* jobs_dev, int njobs, uint64_t seed,
                           uint64_t ctr, drpo_stream_t stream);
/* one job, upstream DRPO_UPSTREAM_GOUT */
int drpo_mlp_backward(const drpo_mlp_bwd_t* desc /* host */, drpo_stream_t stream);
/* independent backward-data jobs in one launch (descriptors in device memory) */
int drpo_mlp_backward_multi(const drpo_mlp_bwd_t* jobs_host, const drpo_mlp_bwd_t* jobs_dev, int njobs,
                            drpo_stream_t stream);
/* the same with the critic losses fused in (update_critic, src/ssac.py:284-456): jobs with
 * upstream = DRPO_UPSTREAM_CRITIC / _CERT form their output gradients from `head` (the
 * forward outputs, targets and batch of drpo_critic_head_t), leaving the loss partials in
 * head->loss_part -- no separate head launch */
int drpo_mlp_backward_multi_head(const drpo_mlp_bwd_t* jobs_host, const drpo_mlp_bwd_t* jobs_dev, int njobs,
                                 const drpo_critic_head_t* head /* host */, drpo_stream_t stream);
/* the actor update's backward launches: jobs with upstream >= DRPO_UPSTREAM_ACTOR_CC form
 * their output gradients from `head` */
int drpo_mlp_backward_multi_actor(const drpo_mlp_bwd_t* jobs_host, const drpo_mlp_bwd_t* jobs_dev, int njobs,
                                  const drpo_actor_head_t* head /* host */, drpo_stream_t stream);
/* One job of drpo_mlp_fb_multi: forward descriptors fwd[0 .. nfwd) (indices into the launch's
 * forward array, run in this order) and then backward descriptor bwd (an index into its
 * backward array), all for the same 16-row tile in one workgroup. */
typedef struct {
  int nfwd;            /* 1 or 2 */
  int fwd[2];
  int bwd;
} drpo_mlp_fb_job_t;
/* Forward + backward-data of up to 4 jobs in ONE launch (the actor update's pass through the
 * frozen critics, src/ssac.py:470-494): one workgroup per (job, 16-row tile) runs the job's
 * forwards as drpo_mlp_forward_multi would, forms the output gradients as
 * drpo_mlp_backward_multi_actor would -- from the forward's outputs in LDS -- and runs the
 * backward products. The ReLU masks of the last forward's hidden layers stay in LDS and
 * are applied in the backward products' epilogues, so the hidden layers need no sy save
 * (the backward descriptors' sy / sz are not read). Computes what the two launches compute.
 *   - every forward: one batch item, no pair / head / head2 / pre; the first of two forwards
 *     carries a post chain whose single output per row is the job's multiplier value lam
 *     (instead of actor->lams)
 *   - the last forward and the backward describe the same nets: ONE net [K -> 256.. -> 1]
 *     with DRPO_UPSTREAM_NEG_MEAN, or a trunk with paired 256-wide heads [256 -> 256 -> C <= 16]
 *     with DRPO_UPSTREAM_ACTOR_CC / _SAFE_CC; ReLU hidden layers, identity outputs
 *   - no dz / dz2 saves (the nets are frozen); the input gradient dx as in the backward launch */
int drpo_mlp_fb_multi(const drpo_mlp_fwd_t* fwd_host, const drpo_mlp_fwd_t* fwd_dev, int nfwd,
                      const drpo_mlp_bwd_t* bwd_host, const drpo_mlp_bwd_t* bwd_dev, int nbwd,
                      const drpo_mlp_fb_job_t* jobs /* host */, int njobs, const drpo_actor_head_t* head /* host */,
                      uint64_t seed, uint64_t ctr, drpo_stream_t stream);
/* the model fit's backward with the NLL loss fused in: desc->upstream = DRPO_UPSTREAM_ENS,
 * trunk + paired diff / log-var heads. reduce_out receives the deferred reduction
 * (mse / loss / gmin / gmax / weight: from `red_in`, partial layout from this launch). */
int drpo_mlp_backward_ens(const drpo_mlp_bwd_t* desc /* host */, const drpo_ens_upstream_t* up /* host */,
                          const drpo_ens_reduce_t* red_in /* host */, drpo_ens_reduce_t* reduce_out,
                          drpo_stream_t stream);
/* The model fit step's forward + NLL + backward-data in ONE launch (csrc/fit.hip;
 * BatchedGaussianEnsemble.fit's compute_loss + loss.backward(), src/dynamics.py:112-122,
 * 136-153,236-253): replaces drpo_mlp_forward(fwd) + drpo_mlp_backward_ens(bwd, up) for
 * the ensemble trunk [S+A <= 64 -> H -> H] with diff / log-var heads [H -> H -> S+1 <= 16]
 * (swish hidden layers, H = 200 | 256). fwd: the split-heads forward descriptor with its
 * y saves (head output saves and z saves are not written); bwd: the split-heads backward
 * descriptor (trunk dz + dz2); up: as for drpo_mlp_backward_ens (D / LVR unused). Writes
 * the same saves, dZ and loss partials as the two launches. */
int drpo_ens_fit_fb(const drpo_mlp_fwd_t* fwd /* host */, const drpo_mlp_bwd_t* bwd /* host */,
                    const drpo_ens_upstream_t* up /* host */, const drpo_ens_reduce_t* red_in /* host */,
                    drpo_ens_reduce_t* reduce_out, drpo_stream_t stream);
/* Weight gradients of up to 16 layers (items) in ONE launch: gW += dZ^T Y, gb +=
 * colsum(dZ) (the autograd of nn.Linear / BatchedLinear, src/dynamics.py:26-52,
 * src/torch_util.py:190-211), split into (output tile x row chunk) workgroups whose
 * partial tiles are combined in a fixed order by the tile's last workgroup (no float
 * atomics: deterministic). workspace: drpo_mlp_wgrad_workspace_size(items, n) bytes,
 * ZEROED by the caller once before its first use (the launch leaves it zeroed). */
size_t drpo_mlp_wgrad_workspace_size(const drpo_wgrad_item_t* items /* host */, int n);
/* output tiles of one item (the number of sq partials it writes) */
int drpo_mlp_wgrad_tiles(const drpo_wgrad_item_t* item /* host */);
int drpo_mlp_wgrad(const drpo_wgrad_item_t* items /* host */, int n, void* workspace, size_t workspace_bytes,
                   drpo_stream_t stream);
/* drpo_mlp_wgrad plus one extra workgroup running a deferred ensemble-loss
 * reduction (drpo_ens_loss with reduce_out); red may be NULL */
int drpo_mlp_wgrad_reduce(const drpo_wgrad_item_t* items /* host */, int n, const drpo_ens_reduce_t* red /* host */,
                          void* workspace, size_t workspace_bytes, drpo_stream_t stream);
/* drpo_mlp_wgrad plus one extra workgroup adding up partial sums in a fixed order:
 * *out = part[0] + part[1] + ... + part[n-1] for each of nsums (<= 4) entries (the
 * per-workgroup loss partials of drpo_mlp_backward_multi_head; no float atomics) */
typedef struct {
  const float* part;
  int n;
  float* out;
} drpo_sum_t;
int drpo_mlp_wgrad_sums(const drpo_wgrad_item_t* items /* host */, int n, const drpo_sum_t* sums /* host */,
                        int nsums, void* workspace, size_t workspace_bytes, drpo_stream_t stream);

/* The Adam step fused into the weight-gradient launch (no clip, no data-parallel
 * exchange between the gradient and the step: the single-process model fit,
 * src/dynamics.py:155-183 with torch.optim.Adam): the workgroup that finishes an output
 * tile applies Adam to it (the drpo_optim_step arithmetic, so results are bitwise
 * those of drpo_mlp_wgrad + drpo_optim_step) and refreshes the tile's packed mirrors;
 * the optional reduction block does the same for the log-var bounds. The gradient
 * buffer is consumed without being written (it must hold zeros or terms to add; any
 * nonzero term is cleared, like drpo_optim_step's zero_grad). */
struct drpo_pack_map_s;
typedef struct {
  const float* g;             /* base of the flat gradient the items' gW / gb (and gmin / gmax) point into */
  float *p, *m, *v;           /* the group's data and Adam moments, indexed like g */
  float lr_over_bc1, bc2_sqrt, beta1, beta2, eps, weight_decay;
  const struct drpo_pack_map_s* map;      /* device pack map of the group (mirrors refreshed) or NULL */
  const struct drpo_pack_map_s* map_host; /* its host copy (which matrix each item is) */
} drpo_wgrad_adam_t;
int drpo_mlp_wgrad_adam(const drpo_wgrad_item_t* items /* host */, int n, const drpo_ens_reduce_t* red /* host or NULL */,
                        const drpo_wgrad_adam_t* adam /* host */, void* workspace, size_t workspace_bytes,
                        drpo_stream_t stream);

/* ---------------------------------------------------------------- packed weight mirrors
 * Every MLP kernel streams weights from fragment-linear mirrors of the PyTorch
 * [nbatch][dout][din] tensors (layout: csrc/pack_layout.hpp). The mirrors are refreshed
 * by one drpo_pack_weights launch per parameter group after it changes.        */
typedef struct {
  const float* W;     /* [nbatch][dout][din], member stride wstride */
  float* P;           /* forward mirror (or NULL), member stride pstride */
  float* PT;          /* transposed (backward-data) mirror (or NULL), stride ptstride */
  int din, dout, nbatch;
  int64_t wstride, pstride, ptstride;
} drpo_pack_item_t;

int64_t drpo_packed_size(int din, int dout); /* floats per mirror of one [dout][din] matrix */
int drpo_pack_weights(const drpo_pack_item_t* items /* host, <= 16 */, int n, drpo_stream_t stream);

/* ---------------------------------------------------------------- SAC heads
 * (src/ssac.py:284-578, src/smbpo.py:251-279, src/policy.py:89-97)            */
typedef struct {
  const float *s, *a, *s2, *r, *h;
  const uint8_t *d, *v;
  int64_t len;          /* rows available, or -1: min(*ptr_dev, cap) read on the device */
  const int64_t* ptr_dev;
  int64_t cap;
} drpo_buffer_view_t;

/* mixed real/virtual minibatch (src/smbpo.py:253-270; SampleBuffer.sample src/sampling.py:147-151) */
int drpo_sample_batch(const drpo_buffer_view_t* real, const drpo_buffer_view_t* virt, int n_real, int B, int S, int A,
                      int C, const int64_t* idx_real, const int64_t* idx_virt, uint64_t seed, uint64_t ctr,
                      float reward_scale, float alive_bonus, float constraint_scale, float constraint_offset, float* s,
                      float* a, float* s2, float* r, uint8_t* d, uint8_t* v, float* h, drpo_stream_t stream);

/* squashed Gaussian (src/policy.py:89-97, src/squashed_gaussian.py): mode 0 sample,
 * 1 rsample, 2 mean (tanh(mu)), 3 distribution parameters (loc -> u, scale -> e); raw = [mu | log-std pre-activation] [B][2A] */
int drpo_policy_head(const float* raw, int64_t B, int A, int mode, const float* eps, uint64_t seed, uint64_t ctr,
                     uint32_t site, float* a, float* logp, float* u, float* e, float* amean, drpo_stream_t stream);

/* ConstraintCritic.forward per-constraint outputs (src/ssac.py:75-92): mode 0 uncertainty
 * q = mu + std_ratio*std, mode 1 sample (std, mu + clamp(eps, +-2)*std); eps NULL -> Philox */
int drpo_cc_dist(const float* mu, const float* lsraw, int64_t n, int mode, float std_ratio, float log_std_min,
                 float log_std_max, const float* eps, uint64_t seed, uint64_t ctr, float* std_out, float* q,
                 drpo_stream_t stream);

/* ConstraintCritic log-std clamp + quantile bound mu + std_ratio*std, max over C
 * (src/ssac.py:64-92, _get_qc :588-600) */
int drpo_cc_head(const float* mu, const float* lsraw, int64_t B, int C, int distributional, float std_ratio,
                 float log_std_min, float log_std_max, float* ubmax, int* argmax, drpo_stream_t stream);

/* The critic / certificate losses, the actor losses' output gradients and the
 * squashed-Gaussian backward have no launch of their own: drpo_mlp_backward_multi_head and
 * drpo_mlp_backward_multi_actor form them in the backward launch; the alpha gradient is a
 * drpo_optim_step segment (grad_from_sum). */

/* multiplier loss gradient w.r.t. the MLPMultiplier output (src/ssac.py:529-568). x == NULL
 * (scalar multiplier, src/ssac.py:564-566): *loss accumulates sum_i clamp(actor_qc_i -
 * threshold, lb, ub), the penalty sum of -mean(softplus(m) * penalty); gx unused. */
int drpo_multiplier_head(int64_t B, const float* x, const float* safe_qc, const float* actor_qc, float threshold,
                         float penalty_lb, float penalty_ub, float upper_bound, float lam_epsilon, float* gx,
                         float* loss, drpo_stream_t stream);
/* MLPMultiplier.forward output transform (src/ssac.py:107-111) */
int drpo_multiplier_out(int64_t B, const float* x, float upper_bound, float* lam, drpo_stream_t stream);

/* ---------------------------------------------------------------- dynamics ensemble
 * BatchedGaussianEnsemble (src/dynamics.py:112-253); the MLP passes use
 * drpo_mlp_forward/backward/wgrad with nbatch = ensemble members.              */
/* fit / holdout minibatch gather by chronological replay index (src/dynamics.py:156-166,
 * 175-177); idx NULL -> Philox randint(n) with (seed, ctr); ptr_dev overrides ptr.
 * The minibatches of `steps` consecutive fit steps in one launch: step k fills rows
 * [k*rows, (k+1)*rows) of xs / xa / xt from idx[k*rows ..] (or Philox counter ctr + k) */
int drpo_ens_gather_steps(const float* states, const float* actions, const float* next_states, const float* rewards,
                          int64_t ptr, const int64_t* ptr_dev, int64_t cap, int64_t rows, int64_t steps,
                          const int64_t* idx, uint64_t seed, uint64_t ctr, int S, int A, float* xs, float* xa,
                          float* xt, drpo_stream_t stream);
/* mu = diff + [s, 0], soft log-var clamp, optional sample -> (s', r)
 * (_forward1 / _forward_all / sample / elite_samples, src/dynamics.py:112-134,198-234) */
int drpo_ens_head(const float* D, const float* LVR, const float* s, int64_t s_zstride, int64_t n, int S, int nz_out,
                  const float* minlv, const float* maxlv, const int* zsel, const float* eps, uint64_t seed,
                  uint64_t ctr, float* mu, float* lv, float* s2, float* r, drpo_stream_t stream);
/* How far the members' predictions for one (s, a) are apart: the reduction ACROSS members of
 * an all-member forward's raw head outputs (the inputs of drpo_ens_head, shared rows), in
 * one row-wise launch. It extends means / mean / elite_samples (src/dynamics.py:206-234),
 * which hand the E member predictions back for the caller to reduce, with the statistics
 * themselves, so that no [E][n][S+1] output is written. Over the member list z_0..z_{M-1}
 * (zsel; members may repeat, the order is free), with d_m = D[z_m][r][k] and l_m the soft-
 * clamped log-variance of LVR[z_m][r][k] (drpo_ens_head's clamp), per column k = 0..S:
 *   mean           (k < S ? s[r][k] : 0) + (1/M) sum_m d_m
 *   epistemic_std  sqrt((1/M) sum_m (d_m - mean_m d)^2), two passes over D: the residual s
 *                  is the same for every member and never enters
 *   aleatoric_std  sqrt((1/M) sum_m exp(l_m))
 * and per row, with the column weights w = scale:
 *   disagreement   max over member pairs of sqrt(sum_k (w_k (d_m,k - d_m',k))^2); 0 at M = 1
 *   epistemic      sqrt(sum_k w_k^2 epistemic_std_k^2)
 *   aleatoric      sqrt(sum_k w_k^2 aleatoric_std_k^2)
 * Every output pointer is optional (NULL: not computed); at least one is needed. */
typedef struct drpo_ens_spread_s {
  const float* D;              /* [Z][n][S+1] diff-head outputs, member-major */
  const float* LVR;            /* [Z][n][S+1] raw log-variances; NULL without an aleatoric output */
  const float* s;              /* [n][S] states, shared by all members; NULL without mean */
  int64_t n;
  int S, Z;
  const float* minlv;          /* [S+1] log-variance bounds; NULL without an aleatoric output */
  const float* maxlv;
  const int* zsel;             /* device int[M]; NULL: members 0..Z-1 (M == Z <= 32) */
  int M;                       /* 1..32 */
  const float* scale;          /* [S+1] column weights of the per-row outputs; NULL: all ones */
  float* mean;                 /* [n][S+1] */
  float* epistemic_std;        /* [n][S+1] */
  float* aleatoric_std;        /* [n][S+1] */
  float* disagreement;         /* [n] */
  float* epistemic;            /* [n] */
  float* aleatoric;            /* [n] */
} drpo_ens_spread_t;
int drpo_ens_spread(const drpo_ens_spread_t* desc /* host */, drpo_stream_t stream);
/* per-member NLL (_mse_loss, src/dynamics.py:236-253), total compute_loss (:143-153)
 * and, when gD != NULL, its gradients (scaled by *up->gscale if given; gmin / gmax are
 * accumulated into). up: the head outputs, rows, bounds and the workspace
 * (drpo_ens_loss_workspace_size(b, S, Z) bytes; one call at a time per workspace), in
 * which row blocks leave partial sums; red_in: mse, loss (or NULL), weight and, with
 * gD / gLVR, gmin / gmax (its other fields are ignored). reduce_out NULL: a one-block
 * launch reduces the partials in a fixed order now. Otherwise the reduction is described
 * in *reduce_out and runs as the extra last workgroup of the next drpo_mlp_wgrad_reduce
 * (the fit step's weight-gradient launch, which the reduction does not depend on: one
 * launch fewer per fit step) or by drpo_ens_loss_reduce. */
size_t drpo_ens_loss_workspace_size(int64_t b, int S, int Z);
int drpo_ens_loss(const drpo_ens_upstream_t* up /* host */, const drpo_ens_reduce_t* red_in /* host */, float* gD,
                  float* gLVR, drpo_ens_reduce_t* reduce_out, drpo_stream_t stream);
/* The deferred reduction of drpo_ens_loss / drpo_mlp_backward_ens / drpo_ens_fit_fb as its own
 * one-block launch (replaces the reduction step of BatchedGaussianEnsemble.fit,
 * src/dynamics.py:143-153,163-171): per-member NLL, the step loss and the log-var
 * bound gradients ACCUMULATED into gmin / gmax (no optimizer step). The member-
 * sharded fit runs it on a side stream so the bounds' all-reduce overlaps the
 * members' fused weight-gradient + Adam launch. */
int drpo_ens_loss_reduce(const drpo_ens_reduce_t* red /* host */, drpo_stream_t stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.Adam (coupled L2), clip_grad_norm_, update_ema (src/ssac.py:446-455,
 * src/torch_util.py:223-226), over flat parameter groups: every step is a
 * drpo_optim_step (or the weight-gradient launch's fused step, drpo_mlp_wgrad_adam).
 * clip_grad_norm_'s first pass: drpo_grad_sumsq_blocks(n) partial sums of squares of
 * g[0, n), one per 2048 elements (drpo_grad_sumsq: one slice; _multi below: up to 8) */
int drpo_grad_sumsq_blocks(int64_t n);
int drpo_grad_sumsq(const float* g, int64_t n, float* partial, drpo_stream_t stream);

/* Fused optimizer step over segments of flat groups: clip coefficient from the
 * partial sums (clip_grad_norm_, src/ssac.py:450-451), Adam (src/defaults.py:4),
 * gradient zeroing, EMA of a target group (src/torch_util.py:223-226) and the
 * packed-mirror refresh, in ONE launch.                                        */
typedef struct drpo_pack_map_s { /* device memory: where each weight matrix of a group lives */
  int nlayers;
  int64_t off[16];            /* flat offset of the [nbatch][dout][din] weight */
  int din[16], dout[16], nbatch[16];
  int64_t poff[16];           /* offset of its packed mirrors (forward / transposed / target) */
  float *P, *PT, *Pt;         /* mirrors (PT, Pt may be NULL) */
} drpo_pack_map_t;

typedef struct {
  float *p, *g, *m, *v;       /* flat group (element indices are absolute) */
  int64_t start, end;
  int adam;                   /* 0: no Adam update (EMA / pack only) */
  const float* partial;       /* clip partial sums (drpo_grad_sumsq[_multi]) or NULL */
  int n_partial;
  float max_norm;
  float lr_over_bc1, bc2_sqrt, beta1, beta2, eps, weight_decay;
  int zero_grad;              /* write g = 0 after use */
  float* ema_target;          /* optional: target = rate*p + keep*target */
  float ema_rate, ema_keep;
  const drpo_pack_map_t* map; /* optional (device): packed mirrors to refresh */
  const float* grad_from_sum; /* optional (device scalar): the gradient of element i is
                                 -exp(p_i) * (*grad_from_sum / grad_sum_rows) instead of g[i]:
                                 d alpha_loss / d log_alpha from the alpha-loss sum of the
                                 DRPO_UPSTREAM_SQUASH backward (src/ssac.py:498-501), so the SAC
                                 temperature needs no separate gradient launch */
  int64_t grad_sum_rows;
  int grad_from_sum_kind;     /* 0: -exp(p_i) * sum / rows (the SAC temperature, alpha loss);
                                 1: -sigmoid(p_i) * sum / rows (the scalar Lagrange multiplier,
                                    -mean(softplus(m) * penalty), src/ssac.py:564-566);
                                 2: -sum / rows (use_log_alpha_loss, src/ssac.py:499) */
  float grad_scale;           /* gradient multiplier applied before clip and Adam (the clip
                                 norm is that of the scaled gradient): 1/G folds the data-
                                 parallel mean into the step after a SUM all-reduce. 0 is
                                 read as 1, so zero-initialised descriptors keep plain grads */
  int grad_sum_n;             /* grad_from_sum holds this many partial sums, added in order (0 = 1) */
  const drpo_pack_map_t* map_host; /* optional host copy of *map: the launch then covers each
                                 weight matrix in 4x4 blocks (16-byte loads / stores per row,
                                 16-byte mirror stores per row and per column) instead of
                                 runs of 4 flat elements with scattered transposed-mirror
                                 stores */
} drpo_optim_seg_t;

int drpo_optim_step(const drpo_optim_seg_t* segs /* host, <= 8 */, int n, drpo_stream_t stream);
int drpo_grad_sumsq_multi(const float* const* g /* host arrays */, const int64_t* n, float* const* partial_out, int cnt,
                          drpo_stream_t stream);

/* Normalizer.fit / forward (src/normalization.py:14-23) */
size_t drpo_normalizer_workspace_size(int64_t N, int S);
int drpo_normalizer_fit(const float* X, int64_t N, int S, float* mean, float* std, void* workspace,
                        drpo_stream_t stream);
int drpo_normalize(const float* x, const float* mean, const float* std, float eps, float* y, int64_t n, int S,
                   drpo_stream_t stream);

/* ---------------------------------------------------------------- path queries
 * Every fused launch has a general launch behind it, and an entry point refuses the
 * shapes its kernel cannot run. These host-only queries are those shape conditions
 * (csrc/path_shapes.hpp: the functions the entry points themselves call), for a caller
 * that picks the path before it builds the launch. They need no device, read nothing
 * but the descriptors they are given (never a weight or save pointer; a NULL descriptor
 * is a no), and return 1 (yes) or 0.                                             */
/* drpo_mlp_forward_multi admits a `pair` job over these two nets */
int drpo_mlp_pair_ok(const drpo_mlp_net_t* a, const drpo_mlp_net_t* b);
/* a trunk job over these nets runs its heads paired and may carry ccb_out */
int drpo_mlp_heads_paired(const drpo_mlp_net_t* trunk, const drpo_mlp_net_t* h1, const drpo_mlp_net_t* h2);
/* a job with ccb_out and cols[0] == cols0 may carry this post chain */
int drpo_mlp_post_ok(int cols0, const drpo_mlp_net_t* post);
/* drpo_mlp_fb_multi admits the actor update's three jobs over these nets: the certificate
 * (trunk, h1, h2; C outputs) with `post` chained behind its bound on cols0 columns, the
 * certificate again, and each of q0 / q1 */
int drpo_mlp_fb_ok(int cols0, const drpo_mlp_net_t* trunk, const drpo_mlp_net_t* h1, const drpo_mlp_net_t* h2,
                   const drpo_mlp_net_t* post, const drpo_mlp_net_t* q0, const drpo_mlp_net_t* q1, int C);
/* the model fit step's launches for these descriptors: bit 0 drpo_mlp_backward_ens admits
 * bwd's shapes (its upstream taken as DRPO_UPSTREAM_ENS), bit 1 drpo_ens_fit_fb admits
 * fwd's and bwd's */
int drpo_ens_fit_paths(const drpo_mlp_fwd_t* fwd, const drpo_mlp_bwd_t* bwd, const drpo_ens_upstream_t* up);
/* the engine (1 or 2) drpo_rollout runs for this descriptor (d->engine when it is not 0) */
int drpo_rollout_engine(const drpo_rollout_desc_t* d);
/* drpo_rollout_adjoint admits these dimensions: 1 <= S, S + 1 <= 16, 1 <= A, S + A <= 64 and a
 * hidden width of 200 | 256 */
int drpo_rollout_adjoint_ok(int S, int A, int Hm);

#ifdef __cplusplus
}
#endif
#endif /* DRPO_HIP_H */
