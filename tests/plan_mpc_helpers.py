"""What the tests of receding-horizon control on the planner share (drpo_plan_sample_ar,
drpo_plan_shift, SMBPO.plan(warm_start=, noise_beta=), SMBPO.mpc): the two definitions of
include/drpo_hip.h restated in numpy, a recording controller and a scripted environment.

plan_sample_ar_reference takes the normals z themselves (the GPU tests read them off the white
launch: mean 0, std 1 and an infinite clamp return z), runs the recursion in float64 one numpy
operation per step of the definition (numpy's elementwise operations round once and fuse nothing),
rounds u to float32 once and evaluates the fused multiply-add exactly in rationals, rounded to
float32 once (round_f32). plan_shift_reference copies and selects, so it is exact as it stands."""
from fractions import Fraction

import numpy as np
import torch

import fake_envs

INF = float('inf')


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def bits(x):
    x = _np(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def assert_bits(got, want, msg):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (msg, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f'{msg}: {len(bad)} of {g.size} differ, first at {tuple(bad[0])}: ' \
                          f'{_np(got)[tuple(bad[0])]!r} != {_np(want)[tuple(bad[0])]!r}'


def round_f32(q):
    """The float32 nearest to the rational q, ties to even: one rounding."""
    f = np.float32(float(q))                # (two roundings: at most one float32 off)
    if not np.isfinite(f):
        return f
    near = [f, np.nextafter(f, np.float32(-INF)), np.nextafter(f, np.float32(INF))]
    near = [c for c in near if np.isfinite(c)]
    best = min(abs(Fraction(float(c)) - q) for c in near)
    ties = [c for c in near if abs(Fraction(float(c)) - q) == best]
    even = [c for c in ties if not (int(np.float32(c).view(np.int32)) & 1)]
    return (even or ties)[0]


def fma_f32(a, b, c):
    """fmaf(a, b, c) of float32 scalars: exact in rationals, rounded once; IEEE for the rest."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid='ignore'):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))     # inf / NaN: no rounding matters
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:      # the sign of an exact zero: that of the float64 sum (the product is exact in float64)
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    return round_f32(q)


def plan_sample_ar_reference(z, mean, std, incumbent, *, corr, innov, lo=-1.0, hi=1.0):
    """drpo_plan_sample_ar on the normals z [P, N, K, A] (float32): cand [P * N, K, A] float32."""
    z, mean, std, incumbent = (_np(t).astype(np.float32) for t in (z, mean, std, incumbent))
    P, N, K, A = z.shape
    assert mean.shape == std.shape == incumbent.shape == (P, K, A)
    corr, innov = np.float64(corr), np.float64(innov)
    u = np.empty((P, N, K, A), np.float64)
    u[:, :, 0] = z[:, :, 0].astype(np.float64)
    for t in range(1, K):
        u[:, :, t] = corr * u[:, :, t - 1] + innov * z[:, :, t].astype(np.float64)
    u32 = u.astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    x = np.empty((P, N, K, A), np.float32)
    for i in np.ndindex(P, N, K, A):
        p, n, t, a = i
        v = fma_f32(std[p, t, a], u32[i], mean[p, t, a])
        v = lo if v < lo else v
        v = hi if v > hi else v
        x[i] = v
    xb = x.view(np.int32)
    xb[:, 0] = incumbent.view(np.int32)         # candidate 0: the incumbent's bits
    return x.reshape(P * N, K, A), u32.reshape(P * N, K, A)


def plan_shift_reference(mean, std, incumbent, *, shift, fresh_std, std_floor, reset=None, tail=None):
    """drpo_plan_shift: (mean_out, std_out, incumbent_out), float32 [P, K, A], element by element
    as the header states it. Bits are carried as int32 so that a NaN's payload and -0.0 survive."""
    mean, std, incumbent = (_np(t).astype(np.float32) for t in (mean, std, incumbent))
    P, K, A = mean.shape
    reset = None if reset is None else _np(reset).astype(bool)
    tail = None if tail is None else _np(tail).astype(np.float32)
    fresh, floor = np.float32(fresh_std), np.float32(std_floor)
    mo, so, io = (np.empty((P, K, A), np.float32) for _ in range(3))
    mb, sb, ib = mo.view(np.int32), so.view(np.int32), io.view(np.int32)

    def b(x):
        return np.float32(x).view(np.int32)
    for p in range(P):
        for t in range(K):
            for a in range(A):
                e = (p, t, a)
                if reset is not None and reset[p]:
                    mb[e] = ib[e] = b(tail[p, a]) if tail is not None else b(0.0)
                    sb[e] = b(fresh)
                elif t + shift < K:
                    mb[e], ib[e] = b(mean[p, t + shift, a]), b(incumbent[p, t + shift, a])
                    s = std[p, t + shift, a]
                    sb[e] = b(floor) if s < floor else b(s)
                else:
                    mb[e] = b(tail[p, a]) if tail is not None else b(mean[p, K - 1, a])
                    ib[e] = b(tail[p, a]) if tail is not None else b(incumbent[p, K - 1, a])
                    sb[e] = b(fresh)
    return mo, so, io


# ------------------------------------------------------------------ the evaluation loop
class RecordingController:
    """Stands for an ops.PlanController in sample_episodes_batched: records every reset mask and
    returns zero actions."""

    def __init__(self, action_dim):
        self.action_dim, self.masks, self.states = action_dim, [], []

    def act(self, states, reset=None):
        self.masks.append(None if reset is None else [bool(x) for x in reset.cpu().tolist()])
        self.states.append(states.clone())
        return torch.zeros(len(states), self.action_dim, device=states.device)


class ScriptedEnv(fake_envs.PointRobot):
    """fake_envs.PointRobot that can be stepped: the state counts the steps of the episode, and an
    episode ends (done) after ``lengths.pop(0)`` steps (never, once the list is empty)."""

    def __init__(self, lengths):
        super().__init__()
        self.lengths, self.t, self.end = list(lengths), 0, None

    def reset(self):
        self.t, self.end = 0, self.lengths.pop(0) if self.lengths else None
        return torch.zeros(self.S)

    def step(self, action):
        self.t += 1
        return torch.full((self.S,), float(self.t)), 1.0, self.t == self.end, {'violation': False}
