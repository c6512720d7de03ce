"""Times of one SMBPO.plan iteration and of its parts (profiles/plan/README.md).

    python profiles/plan/measure.py [--reps 30] [--warmup 5] [--yardstick-only]

Shape: bench config 2's nets (quadrotor, E 7), P 64 start states x N 64 candidates (B 4096), H 10,
K = H, the bench's scene (synthetic replay, steady model), ensemble member 0, model_noise=False.
Each repetition runs in turn, each between two torch events: the sample launch, imagine(actions=),
the terminal critic forwards, the refit, one whole plan(iterations=1), plan(iterations=4), and the
yardstick imagine(actions=, lookahead=True) at the same B. Median and p10-p90 over the repetitions.
On a tree without SMBPO.plan, or with --yardstick-only, the yardstick alone is timed: the parent
commit's figure and the one of this build that compares with it (run between the other calls of a
repetition the same call has measured about 100 us more than in a loop of its own)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--yardstick-only', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    alg = scene(dev, P * N, H)
    A = alg.action_dim
    noise = drpo_amd.DeviceNoise(1)
    run = dict(members=0, deterministic=True, model_noise=False, noise=noise)
    states = alg.replay_buffer.get('states')[:P].clone()
    tiled = states.repeat_interleave(N, dim=0)
    gamma = float(alg.solver.discount)
    has_plan = hasattr(alg, 'plan') and not args.yardstick_only
    g = torch.Generator(device=dev).manual_seed(0)
    cand = torch.rand(P * N, H, A, device=dev, generator=g) * 2 - 1
    mean, std = torch.zeros(P, H, A, device=dev), torch.full((P, H, A), 0.5, device=dev)
    names = ['imagine_actions_lookahead'] + (['sample', 'imagine_actions', 'terminal_critics', 'refit',
                                              'plan_1_iteration', 'plan_4_iterations'] if has_plan else [])
    times = {k: [] for k in names}
    for rep in range(args.warmup + args.reps):
        t = {}
        if has_plan:
            t['sample'], cand = timed(lambda: ops.plan_sample(mean, std, mean, N, noise.seed, noise.next()))
            t['imagine_actions'], im = timed(lambda: alg.imagine(tiled, horizon=H, actions=cand, **run))
            t['terminal_critics'], (tq, tqc) = timed(lambda: ops._terminal_critics(alg, alg.actor, im, 'mean'))
            t['refit'], fit = timed(lambda: ops.plan_refit(
                alg, im, tq, tqc, cand, mean, std, gamma, candidates=N, threshold=float(alg.safe_shield_threshold),
                elites=N // 8, temperature=float('inf'), momentum=0.0, min_std=0.05))
            t['plan_1_iteration'], _ = timed(lambda: alg.plan(states, H, candidates=N, iterations=1, members=0,
                                                              noise=noise))
            t['plan_4_iterations'], res = timed(lambda: alg.plan(states, H, candidates=N, iterations=4, members=0,
                                                                 noise=noise))
        t['imagine_actions_lookahead'], look = timed(lambda: alg.imagine(tiled, horizon=H, actions=cand,
                                                                         lookahead=True, **run))
        if rep >= args.warmup:
            for k, v in t.items():
                times[k].append(v)
    out = {k: stats(v) for k, v in times.items()}
    out['shape'] = dict(P=P, N=N, B=P * N, H=H, K=H, reps=args.reps,
                        mean_length=round(float(look.lengths.float().mean()), 2))
    if has_plan:
        out['last_plan'] = dict(n_feasible_mean=round(float(res.n_feasible.float().mean()), 1),
                                feasible_states=int(res.feasible.sum()))
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
