"""Times of SMBPO.plan(particles=) and of its parts (profiles/plan_particles/README.md).

    python profiles/plan_particles/measure.py [--reps 30] [--warmup 5]

Shape: bench config 2's nets (quadrotor, E 7, every member an elite: G 7), H 10, K = H, the bench's
scene (synthetic replay, steady model), model_noise=False, at P 8 and P 64 start states x N 64
candidates (P * N 512 and 4096). Each repetition runs in turn, each between two torch events:
imagine(actions=) under one member and under the seven particles (one launch per particle), the
terminal critic forwards on the P * N and on the 7 * P * N rows, the two refit launches, and
plan(iterations=4) under one member and under the particles. Median and p10-p90 over the
repetitions."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'profiles', 'plan'))
import drpo_amd  # noqa: E402
from drpo_amd import ops  # noqa: E402
from measure import scene, stats, timed  # noqa: E402  (profiles/plan/measure.py)

N, H, G = 64, 10, 7


def measure(alg, P, reps, warmup):
    dev, A = alg.device, alg.action_dim
    noise = drpo_amd.DeviceNoise(1)
    one = dict(members=0, deterministic=True, model_noise=False, noise=noise)
    each = dict(particles='elites', deterministic=True, model_noise=False, noise=noise)
    states = alg.replay_buffer.get('states')[:P].clone()
    tiled = states.repeat_interleave(N, dim=0)
    gamma = float(alg.solver.discount)
    g = torch.Generator(device=dev).manual_seed(0)
    cand = torch.rand(P * N, H, A, device=dev, generator=g) * 2 - 1
    mean, std = torch.zeros(P, H, A, device=dev), torch.full((P, H, A), 0.5, device=dev)
    fit = dict(candidates=N, threshold=float(alg.safe_shield_threshold), elites=N // 8, temperature=float('inf'),
               momentum=0.0, min_std=0.05)
    times = {}
    for rep in range(warmup + reps):
        t = {}
        t['imagine_actions_one_member'], im1 = timed(lambda: alg.imagine(tiled, horizon=H, actions=cand, **one))
        t['imagine_actions_particles'], imG = timed(lambda: alg.imagine(tiled, horizon=H, actions=cand, **each))
        flat = imG.flat_runs()
        t['terminal_critics_one_member'], (q1, qc1) = timed(lambda: ops._terminal_critics(alg, alg.actor, im1, 'mean'))
        t['terminal_critics_particles'], (qG, qcG) = timed(lambda: ops._terminal_critics(alg, alg.actor, flat, 'mean'))
        t['refit'], _ = timed(lambda: ops.plan_refit(alg, im1, q1, qc1, cand, mean, std, gamma, **fit))
        t['refit_particles'], _ = timed(lambda: ops.plan_refit(alg, flat, qG, qcG, cand, mean, std, gamma, particles=G,
                                                               **fit))
        t['refit_particles_cvar'], _ = timed(lambda: ops.plan_refit(alg, flat, qG, qcG, cand, mean, std, gamma,
                                                                    particles=G, score_tail=4, **fit))
        t['plan_4_iterations_one_member'], _ = timed(lambda: alg.plan(states, H, candidates=N, iterations=4, members=0,
                                                                      noise=noise))
        t['plan_4_iterations_particles'], res = timed(lambda: alg.plan(states, H, candidates=N, iterations=4,
                                                                       particles='elites', noise=noise))
        if rep >= warmup:
            for k, v in t.items():
                times.setdefault(k, []).append(v)
    out = {k: stats(v) for k, v in times.items()}
    out['shape'] = dict(P=P, N=N, rows=P * N, G=G, H=H, K=H, reps=reps, particle_launches=imG.particle_launches,
                        n_feasible_mean=round(float(res.n_feasible.float().mean()), 1),
                        spread_mean=round(float(res.score_spread.mean()), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    alg = scene(dev, 64 * N, H)
    alg.model_ensemble._elite_inds = list(range(G))
    print(json.dumps({f'rows_{P * N}': measure(alg, P, args.reps, args.warmup) for P in (8, 64)}, indent=1))


if __name__ == '__main__':
    main()
