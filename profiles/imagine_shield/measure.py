"""The horizon kernel under the shield, bracketed with the library's HIP event pair
(step_events, around rollout_persist_kernel) in one process:

  P     drpo_rollout_trajectories: the parent's kernel, no shield
  SHhi  drpo_rollout_trajectories_shielded, threshold +inf: the SH kernel, the certificate
        at every step, the safe actor skipped in every tile
  SHlo  threshold -inf: the SH kernel, every tile runs the safe actor at every step

The scene is bench.py's (quadrotor, E 7, steady mode: every row lives the whole horizon).
The variants are interleaved, REPS times each, after a warm-up; medians and the spread are
reported. The large shape runs once each after one warm-up round.

  python profiles/imagine_shield/measure.py --large --out profiles/imagine_shield/measure.json
"""
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

DEV = torch.device('cuda')
# per transition: DESIGN §4's formula; + the critic's certificate; + the safe actor
FLOP = {'P': 395264, 'SHhi': 395264 + 402432, 'SHlo': 395264 + 402432 + 139264}
SHIELD = {'P': None, 'SHhi': float('inf'), 'SHlo': float('-inf')}
PEAK_FP32_MFMA = bench.FP32_PEAK_TFLOPS * 1e12


def measure(B, H, reps, warm):
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0), DEV, alg.env_params)
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    tmr = ops.EventTimer(2)
    noise = drpo_amd.DeviceNoise(0)
    im = ops.rollout_trajectories(alg, alg.actor, None, noise)
    torch.cuda.synchronize()
    assert int(im.lengths.min()) == H, 'steady mode: every row lives the horizon'
    out = {k: getattr(im, k) for k in ops.ImaginedRollout.TENSORS}
    share = {}

    def run(name):
        r = ops.rollout_trajectories(alg, alg.actor, None, noise, out=out, timer=tmr, shield=SHIELD[name])
        torch.cuda.synchronize()
        if r.interventions is not None:
            share[name] = float(r.interventions.float().mean())
        return tmr.elapsed_pairs(1)[0] * 1e3       # us

    for _ in range(warm):
        for name in FLOP:
            run(name)
    us = {name: [] for name in FLOP}
    for _ in range(reps):
        for name in FLOP:
            us[name].append(run(name))
    assert share == {'SHhi': 0.0, 'SHlo': 1.0}, share
    res = {'B': B, 'H': H, 'reps': reps, 'transitions': B * H}
    for name in FLOP:
        a = np.asarray(us[name])
        flop = B * H * FLOP[name]
        med = float(np.median(a))
        res[name] = {'median_us': med, 'min_us': float(a.min()), 'max_us': float(a.max()),
                     'p10_us': float(np.quantile(a, 0.1)), 'p90_us': float(np.quantile(a, 0.9)),
                     'algorithmic_tflops': flop / med / 1e6,
                     'fraction_of_fp32_mfma_peak': flop / (med * 1e-6) / PEAK_FP32_MFMA}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--large', action='store_true', help='also B 65536, H 80, one run each')
    args = ap.parse_args()
    out = [measure(4096, 10, args.reps, 3)]
    print(json.dumps(out[-1]), flush=True)
    if args.large:
        torch.cuda.empty_cache()
        out.append(measure(65536, 80, 1, 1))
        print(json.dumps(out[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
