"""A/B/C of the rollout's constraint route at config 2 (quadrotor E7 H10 B4096,
bench.make_alg, device noise, steady mode), alternating launches in one process:

  a  the built-in quadrotor id (env id 1)
  b  the same environment declared by a ConstraintProgram (env id 4)
  c  the same environment with neither: ops.rollout_host_env, the env's numpy
     check_done / check_violation / get_constraint_values on the host each step

Per variant: `kernel_us`, the fused horizon kernel between the library's own events
(step_events pair 0; a and b only), and `rollout_us`, the whole rollout call between
two events on the stream (persist kernel + emit for a / b; every launch, copy and host
round trip for c). Medians and the min .. max over --reps rounds; one round runs each
variant once, in the order a b c.

    python profiles/env_program_ab.py [--reps 40] [--variants abc] [--out FILE.json]

`--variants a` needs nothing of the program feature, so the same file also times a
build of an earlier commit (run it from that tree) for the before/after of the
built-in path. Compare a build's (a) with another build's only between runs of the
same --variants: the absolute figures depend on what else runs in a round (with
variant c the GPU is nearly idle for milliseconds per round, and a and b then read
~10 % slower than in an `ab` run); ratios inside one run share their conditions."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TH = np.float32(85 * np.pi / 180)


def quadrotor_program():
    from drpo_amd.envs import ConstraintProgram
    return (ConstraintProgram().from_linear_constraint([[-1.0], [1.0]], [-0.5, 1.5], [2])
            .done_box((0, 2, 4), [-2.0, -3.0, -TH], [2.0, 3.0, TH], dtype=np.float32).done_on_violation())


def make_env_class(kind):
    """ShapeEnv('quadrotor') dims without the built-in id: 'b' carries the program,
    'c' only the numpy functions a user's env would have."""
    from drpo_amd.envs import ShapeEnv

    class UserQuadrotor(ShapeEnv):
        def __init__(self, name, id=None):
            super().__init__(name)
            del self.drpo_env_id

        def get_constraint_values(self, s):
            z = s[:, 2].astype(np.float64)
            return np.stack([-z + 0.5, z - 1.5], 1)

        def check_violation(self, s):
            return (self.get_constraint_values(s) > 0).any(1)

        def check_done(self, s):
            x, z, th = s[:, 0], s[:, 2], s[:, 4]
            oob = (x < -2) | (x > 2) | (z < -3) | (z > 3) | (th < -TH) | (th > TH)
            return oob | self.check_violation(s)

    if kind == 'b':
        UserQuadrotor.drpo_constraint_program = staticmethod(quadrotor_program)
    return UserQuadrotor


def build(kind, seed):
    import bench
    from drpo_amd import envs
    dev = torch.device('cuda')
    cfg = bench.CONFIGS[2]
    orig = envs.ShapeEnv
    random.seed(seed)
    try:
        if kind != 'a':
            envs.ShapeEnv = make_env_class(kind)
        alg = bench.make_alg(dev, cfg['B'], cfg['H'], cfg['E'], seed, bench.ENV_JSON['quadrotor'], env='quadrotor')
    finally:
        envs.ShapeEnv = orig
    want = {'a': 1, 'b': 4, 'c': None}[kind]
    got = None if alg.env_params is None else alg.env_params['env_id']
    assert got == want, (kind, got)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(seed))
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(dev) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    return alg


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--variants', default='abc')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import drpo_amd
    from drpo_amd import _lib
    from drpo_amd.ops import EventTimer
    algs = {k: build(k, args.seed) for k in args.variants}
    timers = {k: EventTimer(4) for k in algs}
    kern = {k: [] for k in algs}
    whole = {k: [] for k in algs}
    rows = {}
    for r in range(args.warmup + args.reps):
        for k, alg in algs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = alg.rollout(alg.actor, timer=timers[k]) if k != 'c' else alg.rollout(alg.actor)
            e1.record()
            torch.cuda.synchronize()
            rows[k] = len(out)
            if r < args.warmup:
                continue
            whole[k].append(e0.elapsed_time(e1) * 1e3)
            if k != 'c':
                kern[k].append(timers[k].elapsed_pairs(1)[0] * 1e3)
    res = dict(label=args.label, config='quadrotor E7 H10 B4096 (bench config 2, steady mode, device noise)',
               device=torch.cuda.get_device_name(0), library_digest=_lib.build_digest()[:16], reps=args.reps,
               rows_per_rollout=rows,
               kernel_us={k: stats(v) for k, v in kern.items() if v},
               rollout_us={k: stats(v) for k, v in whole.items()})
    med = lambda d, k: d[k]['median']
    if 'a' in algs and 'b' in algs:
        res['b_over_a_kernel'] = med(res['kernel_us'], 'b') / med(res['kernel_us'], 'a')
        res['b_over_a_rollout'] = med(res['rollout_us'], 'b') / med(res['rollout_us'], 'a')
    if 'b' in algs and 'c' in algs:
        res['c_over_b_rollout'] = med(res['rollout_us'], 'c') / med(res['rollout_us'], 'b')
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
