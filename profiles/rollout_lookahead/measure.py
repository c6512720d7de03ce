"""Times of SMBPO.imagine with and without lookahead= (profiles/rollout_lookahead/README.md).

    python profiles/rollout_lookahead/measure.py [--reps 30] [--warmup 5] [--trace]

Shapes: bench config 2 (quadrotor, B 4096, H 10, E 7) and the longest chain (B 256, H 128), the
bench's scene (synthetic replay, steady model). Each repetition runs the plain call, the call with
lookahead=True and the one with lookahead='bound' in turn; torch events around the Python call,
median and p10-p90 over the repetitions. --trace: no timing, a few calls of each kind for a kernel
trace run of its own (rocprofv3 --kernel-trace --stats -- python ... --trace)."""
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


def scene(dev, B, H):
    alg = bench.make_alg(dev, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0), dev, alg.env_params)
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(dev) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    return alg


def stats(x):
    x = np.asarray(x) * 1e3
    return {'median_us': round(float(np.median(x)), 1), 'p10_us': round(float(np.percentile(x, 10)), 1),
            'p90_us': round(float(np.percentile(x, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--shape', default='both', choices=['config2', 'h128', 'both'])
    ap.add_argument('--kind', default='all', choices=['plain', 'mean', 'bound', 'all'],
                    help='with --trace: the one kind of call this process makes (10 of them)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    kinds = {'plain': None, 'mean': True, 'bound': 'bound'}
    if args.kind != 'all':
        kinds = {args.kind: kinds[args.kind]}
    shapes = {'config2': (4096, 10), 'h128': (256, 128)}
    out = {}
    for B, H in (shapes.values() if args.shape == 'both' else [shapes[args.shape]]):
        alg = scene(dev, B, H)
        noise = drpo_amd.DeviceNoise(1)
        times = {k: [] for k in kinds}
        reps = 10 if args.trace else args.warmup + args.reps
        for rep in range(reps):
            for name, look in kinds.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                im = alg.imagine(noise=noise, lookahead=look)
                b.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[name].append(a.elapsed_time(b))
        lengths = im.lengths.float()
        out[f'B{B}_H{H}'] = dict({k: stats(v) for k, v in times.items() if v},
                                 mean_length=round(float(lengths.mean()), 2), reps=max(map(len, times.values())))
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
