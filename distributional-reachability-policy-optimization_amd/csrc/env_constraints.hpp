// Batched per-row constraint functions of the DRPO environments, evaluated on the
// device (replaces the three host numpy round trips per rollout step,
// src/smbpo.py:63-65). Numerics follow the reference: where numpy promotes to
// float64 (float64 constants / BoundedConstraint matrices) we compute in double,
// where it stays float32 (tracking geometry) we compute in float.
#pragma once
#include "common.hpp"

namespace drpo {

enum EnvId : int { ENV_POINT_ROBOT = 0, ENV_QUADROTOR = 1, ENV_CARTPOLE = 2, ENV_TRACKING = 3 };

struct EnvParams {
  int id;
  int surr_start;     // tracking: first surrounding-vehicle dim (47 for ref_num 1 / pre_horizon 10)
  int n_surr;         // tracking: number of surrounding vehicles
  double thr0, thr1;  // quadrotor: x/z_threshold (safe_control_gym, unpinned); cartpole: x/th_threshold
};

__host__ __device__ inline int env_con_dim(int id, int n_surr) {
  switch (id) {
    case ENV_QUADROTOR: return 2;
    case ENV_CARTPOLE: return 4;
    default: return 1;
  }
}

// s: one state row (float32). Writes done, violation, h[C].
__device__ inline void env_constraints_row(const EnvParams& ep, const float* s, bool& done, bool& viol, float* h) {
  if (ep.id == ENV_POINT_ROBOT) {
    // src/env/point_robot.py:96-131
    const double x = s[0], y = s[1];
    const double hx[2] = {0.4, -0.4}, hy[2] = {-1.2, 1.2};
    double md = __longlong_as_double(0x7ff0000000000000LL);   // +inf
    for (int k = 0; k < 2; ++k) {
      const double dx = hx[k] - x, dy = hy[k] - y;
      const double d = sqrt(dx * dx + dy * dy);
      md = fmin(d, md);
    }
    const double hv = 0.8 - md;
    h[0] = (float)hv;
    viol = hv > 0.0;
    const bool oob = (s[0] < -3.0f) || (s[0] > 3.0f) || (s[1] < -3.0f) || (s[1] > 3.0f);
    const double gx = x - 2.2, gy = y - 2.2;
    done = oob || (sqrt(gx * gx + gy * gy) <= 0.3);
  } else if (ep.id == ENV_QUADROTOR) {
    // src/env/quadrotor/quadrotor.py:83-158 with BoundedConstraint z in [0.5, 1.5]
    const double z = s[2];
    const double h0 = -z - (-0.5), h1 = z - 1.5;
    h[0] = (float)h0;
    h[1] = (float)h1;
    viol = (h0 > 0.0) || (h1 > 0.0);
    const float th = 1.48352986419518f;   // float32(85*pi/180)
    const float xt = (float)ep.thr0, zt = (float)ep.thr1;
    const bool oob = (s[0] < -xt) || (s[0] > xt) || (s[2] < -zt) || (s[2] > zt) || (s[4] < -th) || (s[4] > th);
    done = oob || viol;
  } else if (ep.id == ENV_CARTPOLE) {
    // src/env/poles/inverted_pendulum.py:11-26,79-121, constraints.py:216-247: BoundedConstraint
    // h = x @ F^T @ A^T - b in float64 with b = [x_thr, th_thr, x_thr, th_thr]
    const double x = s[0], t = s[1];
    const double hv[4] = {-x - ep.thr0, -t - ep.thr1, x - ep.thr0, t - ep.thr1};
    bool v = false;
    for (int k = 0; k < 4; ++k) {
      h[k] = (float)hv[k];
      v = v || (hv[k] > 0.0);
    }
    viol = v;
    done = v;
  } else {
    // ENV_TRACKING: src/env/tracking/pyth_veh3dofconti_surrcstr_data.py:253-338
    done = (fabsf(s[0]) > 5.f) || (fabsf(s[1]) > 2.f) || (fabsf(s[2]) > 3.14159274f);
    const float d = 1.4f;
    const float c = cosf(s[6]), sn = sinf(s[6]);
    float md = __int_as_float(0x7f800000);
    for (int v = 0; v < ep.n_surr; ++v) {
      const float* sv = s + ep.surr_start + 4 * v;
      const float xe = sv[0] * c + sv[1] * sn;
      const float ye = -sv[0] * sn + sv[1] * c;
      const float cp = cosf(sv[2]), sp = sinf(sv[2]);
      const float cx[2] = {xe + d * cp, xe - d * cp}, cy[2] = {ye + d * sp, ye - d * sp};
      const float ex[2] = {d, -d};
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
          const float dx = ex[i] - cx[j], dy = 0.f - cy[j];
          md = fminf(md, sqrtf(dx * dx + dy * dy));
        }
    }
    const double hv = 2.8284271247461903 - (double)md;
    h[0] = (float)hv;
    viol = hv > 0.0;
  }
}

// ---------------------------------------------------------------------------
// Constraint programs (drpo_env_program_t): the interpreter of env id 4.
// The program is wave-uniform data in device memory that no kernel writes, so it is
// read through a constant-address-space pointer: every read below has a uniform
// address and compiles to a scalar load (byte arrays are read as whole words).
// Double arithmetic without contraction (__dmul_rn / __dadd_rn), so the result is
// the one ConstraintProgram.evaluate_numpy computes.
// ---------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) drpo_env_program_t* EnvProgK;
typedef const __attribute__((address_space(4))) drpo_env_program_row_t* EnvProgRowK;
typedef const __attribute__((address_space(4))) uint8_t* EnvProgBytesK;
typedef const __attribute__((address_space(4))) uint32_t* EnvProgWordsK;
typedef const __attribute__((address_space(4))) double* EnvProgRealsK;

__device__ __forceinline__ EnvProgK env_program_ptr(const void* dev_prog) {
  return (EnvProgK)(uintptr_t)dev_prog;
}

// byte k of a 4-byte aligned byte array
__device__ __forceinline__ int env_prog_u8(EnvProgBytesK a, int k) {
  return (int)((((EnvProgWordsK)a)[k >> 2] >> (8 * (k & 3))) & 0xffu);
}

// || s[dims[0..nd)] - c[0..nd) ||_2, nd = 2 | 3
__device__ __forceinline__ double env_prog_dist(const float* s, EnvProgBytesK dims, EnvProgRealsK c, int nd) {
  const double d0 = __dsub_rn((double)s[env_prog_u8(dims, 0)], c[0]);
  const double d1 = __dsub_rn((double)s[env_prog_u8(dims, 1)], c[1]);
  double q = __dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1));
  if (nd == 3) {
    const double d2 = __dsub_rn((double)s[env_prog_u8(dims, 2)], c[2]);
    q = __dadd_rn(q, __dmul_rn(d2, d2));
  }
  return sqrt(q);
}

// Same contract as env_constraints_row: s is one state row, writes done, violation,
// h[prog->C]. The program was checked on the host (drpo_env_program_check) before
// its upload: every index is < S and every count within its array.
__device__ inline void env_program_row(EnvProgK prog, const float* s, bool& done, bool& viol, float* h) {
  const int C = prog->C;
  bool v = false;
#pragma unroll
  for (int c = 0; c < DRPO_PROG_MAX_ROWS; ++c) {
    if (c >= C) break;
    EnvProgRowK row = &prog->rows[c];
    const uint32_t head = *(EnvProgWordsK)row;   // kind | n << 8 | nd << 16
    const int kind = head & 0xff, n = (head >> 8) & 0xff, nd = (head >> 16) & 0xff;
    double hv;
    if (kind == DRPO_PROG_AFFINE) {
      hv = __dmul_rn(row->v[0], (double)s[env_prog_u8(row->dims, 0)]);
      for (int k = 1; k < n; ++k) hv = __dadd_rn(hv, __dmul_rn(row->v[k], (double)s[env_prog_u8(row->dims, k)]));
      hv = __dadd_rn(hv, row->k0);
    } else {
      double md = __longlong_as_double(0x7ff0000000000000LL);   // +inf
      for (int j = 0; j < n; ++j) md = fmin(env_prog_dist(s, row->dims, row->v + j * nd, nd), md);
      hv = __dsub_rn(row->k0, md);
    }
    v = v || (hv > 0.0);
    h[c] = (float)hv;
  }
  viol = v;
  const uint32_t rule = ((EnvProgWordsK)prog)[1];   // done_on_violation | box_n << 8 | ball_nd << 16
  const int box_n = (rule >> 8) & 0xff, ball_nd = (rule >> 16) & 0xff;
  bool dn = (rule & 0xff) != 0 && v;
  for (int k = 0; k < box_n; ++k) {
    const double x = (double)s[env_prog_u8(prog->box_dims, k)];
    dn = dn || (x < prog->box_lo[k]) || (x > prog->box_hi[k]);
  }
  if (ball_nd) dn = dn || (env_prog_dist(s, prog->ball_dims, prog->ball_centre, ball_nd) <= prog->ball_radius);
  done = dn;
}

// One state row through the built-in functions of env.id, or (PG) through the program:
// the one place the rollout engines and the stand-alone kernel make that choice.
template <bool PG>
__device__ __forceinline__ void constraint_row(const EnvParams& env, const void* prog, const float* s, bool& done,
                                               bool& viol, float* h) {
  if constexpr (PG) env_program_row(env_program_ptr(prog), s, done, viol, h);
  else env_constraints_row(env, s, done, viol, h);
}

}  // namespace drpo
