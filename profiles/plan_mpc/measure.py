"""Times and one quality figure of receding-horizon control on the planner
(profiles/plan_mpc/README.md).

    python profiles/plan_mpc/measure.py [--reps 30] [--warmup 5]     the times
    python profiles/plan_mpc/measure.py --quality                    the closed loop on the model

Times. Shape: bench config 2's nets (quadrotor, E 7), P 64 start states x N 64 candidates
(B 4096), H 10, K = H, the bench's scene (synthetic replay, steady model), ensemble member 0,
model_noise=False. Each repetition runs every line in turn, each between two torch events (so the
host's share is in them): plan(iterations=1) and plan(iterations=4) with every new argument off,
the white sample launch, the AR sample launch, the shift launch, and a warm controller.act at
iterations 1 and 4 (noise_beta 0.5, fallback='safe'). Median and p10-p90 over the repetitions. On
a tree without SMBPO.mpc (the parent commit) the two plan() lines alone are timed: run this file
from that tree and from this one in turn, several processes each, for the off-path comparison.

Quality. tests/imagine_helpers._action_scene (its model answers to its actions), member 3 fixed,
model_noise=False, 64 start states over the replay's z range, 20 closed-loop steps on the model:
at each step the planner's action (fallback=None) goes through one model step
(imagine(actions=, horizon=1)). Discounted return of the model's rewards over the steps a row
lives, and the share of (state, step) pairs whose best row was feasible, for a cold plan per step
at iterations 1 and 4 and a warm-started one (SMBPO.mpc) at iterations 1, at noise_beta 0 and 0.5.
One seed; reported, not gated."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import drpo_amd  # noqa: E402
from drpo_amd import ops  # noqa: E402

P, N, H = 64, 64, 10


def scene(dev, B, horizon):
    alg = bench.make_alg(dev, B, horizon, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0), dev, alg.env_params)
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(dev) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    return alg


def stats(x):
    x = np.asarray(x) * 1e3
    return {'median_us': round(float(np.median(x)), 1), 'p10_us': round(float(np.percentile(x, 10)), 1),
            'p90_us': round(float(np.percentile(x, 90)), 1)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def times(args):
    dev = torch.device('cuda', 0)
    alg = scene(dev, P * N, H)
    A = alg.action_dim
    noise = drpo_amd.DeviceNoise(1)
    states = alg.replay_buffer.get('states')[:P].clone()
    has_mpc = hasattr(alg, 'mpc')
    mean, std = torch.zeros(P, H, A, device=dev), torch.full((P, H, A), 0.5, device=dev)
    names = ['plan_1_iteration', 'plan_4_iterations'] + \
        (['sample_white', 'sample_ar', 'shift', 'act_1_iteration', 'act_4_iterations'] if has_mpc else [])
    out = {k: [] for k in names}
    if has_mpc:
        ctl = {i: alg.mpc(horizon=H, candidates=N, iterations=i, members=0, noise_beta=0.5, warm_std=0.1,
                          noise=drpo_amd.DeviceNoise(2 + i)) for i in (1, 4)}
        for c in ctl.values():
            c.act(states)            # the cold call: every timed act() is a warm one
    for rep in range(args.warmup + args.reps):
        t = {}
        t['plan_1_iteration'], _ = timed(lambda: alg.plan(states, H, candidates=N, iterations=1, members=0, noise=noise))
        t['plan_4_iterations'], _ = timed(lambda: alg.plan(states, H, candidates=N, iterations=4, members=0,
                                                           noise=noise))
        if has_mpc:
            t['sample_white'], _ = timed(lambda: ops.plan_sample(mean, std, mean, N, noise.seed, noise.next()))
            t['sample_ar'], _ = timed(lambda: ops.plan_sample(mean, std, mean, N, noise.seed, noise.next(), corr=0.5))
            t['shift'], _ = timed(lambda: ops.plan_shift(mean, std, mean, shift=1, fresh_std=0.5, std_floor=0.1))
            t['act_1_iteration'], _ = timed(lambda: ctl[1].act(states))
            t['act_4_iterations'], _ = timed(lambda: ctl[4].act(states))
        if rep >= args.warmup:
            for k, v in t.items():
                out[k].append(v)
    res = {k: stats(v) for k, v in out.items()}
    res['shape'] = dict(P=P, N=N, B=P * N, H=H, K=H, reps=args.reps, version=int(drpo_amd._lib.lib().drpo_version()))
    print(json.dumps(res))


def quality(args):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from imagine_helpers import MEMBER, _action_scene
    HQ = 3                                # the scene's horizon, as tests/test_gpu_plan.py plans on it
    dev = torch.device('cuda', 0)
    alg = _action_scene(dev)[0]
    gamma = float(alg.solver.discount)
    s0 = alg.replay_buffer.get('states')[3:400:6][:P].clone()
    run = dict(members=MEMBER, model_noise=False)
    kw = dict(candidates=N, **run)
    steps = 20
    rows = []
    for beta in (0.0, 0.5):
        for name, iters, warm in (('cold, iterations=1', 1, False), ('cold, iterations=4', 4, False),
                                  ('warm, iterations=1', 1, True)):
            noise = drpo_amd.DeviceNoise(17)
            ctl = alg.mpc(horizon=HQ, iterations=iters, noise_beta=beta, fallback=None, warm_std=0.1, noise=noise, **kw)
            s, alive = s0.clone(), torch.ones(P, dtype=torch.bool, device=dev)
            ret, feas, lived = torch.zeros(P, device=dev), 0.0, 0.0
            for t in range(steps):
                if not warm:
                    ctl.reset()
                a = ctl.act(s)
                im = alg.imagine(s, horizon=1, actions=a.unsqueeze(1).contiguous(), deterministic=True,
                                 noise=drpo_amd.DeviceNoise(5), **run)
                ret = ret + torch.where(alive, (gamma ** t) * im.rewards[:, 0], torch.zeros_like(ret))
                feas += float((ctl.last.feasible & alive).sum())
                lived += float(alive.sum())
                alive = alive & ~im.dones[:, 0].to(torch.bool)
                s = im.states[:, 1].contiguous()
            rows.append(dict(noise_beta=beta, planner=name, discounted_return_mean=round(float(ret.mean()), 4),
                             feasible_share=round(feas / max(lived, 1.0), 4), steps_lived_mean=round(lived / P, 2),
                             alive_at_the_end=int(alive.sum())))
    print(json.dumps(dict(quality=rows, shape=dict(P=P, N=N, H=HQ, steps=steps, member=MEMBER))))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--quality', action='store_true')
    a = ap.parse_args()
    quality(a) if a.quality else times(a)
