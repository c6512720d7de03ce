"""Times of imagine(proposals=, shield=) beside its two parents, and of plan(safety_filter=) beside
plan (profiles/rollout_proposals/README.md), measured as profiles/plan/measure.py measures.

    python profiles/rollout_proposals/measure.py [--reps 30] [--warmup 5]

Shape: bench config 2's nets (quadrotor, E 7), B 4096 (P 64 start states x N 64 candidates), H 10,
K = H, the bench's scene (synthetic replay, steady model: every row lives to the horizon),
ensemble member 0, deterministic, model_noise=False. Each repetition runs every line in turn, each
between two torch events, so the times include the host's share. Median and p10-p90."""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import drpo_amd  # noqa: E402

# the shape, the scene and the timing of profiles/plan/measure.py, loaded by path (it shares this file's name)
_spec = importlib.util.spec_from_file_location('plan_measure', os.path.join(ROOT, 'profiles', 'plan', 'measure.py'))
_pm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_pm)
H, N, P, scene, stats, timed = _pm.H, _pm.N, _pm.P, _pm.scene, _pm.stats, _pm.timed

INF = float('inf')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    alg = scene(dev, P * N, H)
    A = alg.action_dim
    noise = drpo_amd.DeviceNoise(1)
    run = dict(members=0, deterministic=True, model_noise=False, noise=noise)
    states = alg.replay_buffer.get('states')[:P].clone()
    tiled = states.repeat_interleave(N, dim=0)
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.rand(P * N, H, A, device=dev, generator=g) * 2 - 1
    calls = {
        'imagine_actions': lambda: alg.imagine(tiled, horizon=H, actions=p, **run),
        'imagine_shield_True': lambda: alg.imagine(tiled, horizon=H, shield=True, **run),
        'imagine_proposals_shield_True': lambda: alg.imagine(tiled, horizon=H, proposals=p, shield=True, **run),
        'imagine_shield_inf': lambda: alg.imagine(tiled, horizon=H, shield=INF, **run),
        'imagine_proposals_shield_inf': lambda: alg.imagine(tiled, horizon=H, proposals=p, shield=INF, **run),
        'imagine_proposals_linear': lambda: alg.imagine(tiled, horizon=H, proposals=p, shield='linear', **run),
        'plan_4_iterations': lambda: alg.plan(states, H, candidates=N, iterations=4, members=0, noise=noise),
        'plan_4_iterations_safety_filter_True': lambda: alg.plan(states, H, candidates=N, iterations=4, members=0,
                                                                 noise=noise, safety_filter=True),
    }
    times = {k: [] for k in calls}
    last = {}
    for rep in range(args.warmup + args.reps):
        for k, fn in calls.items():
            t, last[k] = timed(fn)
            if rep >= args.warmup:
                times[k].append(t)
    out = {k: stats(v) for k, v in times.items()}
    frac = lambda im: round(float(im.interventions[im.mask].float().mean()), 4)   # noqa: E731
    out['shape'] = dict(P=P, N=N, B=P * N, H=H, K=H, reps=args.reps, safe_shield_threshold=float(alg.safe_shield_threshold),
                        mean_length=round(float(last['imagine_actions'].lengths.float().mean()), 2))
    out['intervening_fraction'] = {k: frac(last[k]) for k in ('imagine_shield_True', 'imagine_proposals_shield_True',
                                                              'imagine_proposals_shield_inf', 'imagine_proposals_linear')}
    res = last['plan_4_iterations_safety_filter_True']
    out['last_filtered_plan'] = dict(intervening_fraction=frac(res.imagined),
                                     best_rows_intervening=round(float(res.interventions.float().mean()), 4),
                                     feasible_states=int(res.feasible.sum()))
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
