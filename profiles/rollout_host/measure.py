"""Call-to-synchronize time of SMBPO.imagine() and SMBPO.imagine(shield='linear') at bench.py's
shape (quadrotor, E 7, B 4096, H 10, steady mode): host clock from the call to the end of
torch.cuda.synchronize() after it, the stream idle before the call. The two forms interleaved,
3 warm-up rounds, then REPS (30) repetitions each; median, p10 and p90 in microseconds.

  python profiles/rollout_host/measure.py [--tree DIR] [--label NAME] [--out FILE]

DIR (default: the tree this file lies in) is the checkout whose bench.py and package are
imported, so that the same script times two trees in alternating processes."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='this tree')
ap.add_argument('--reps', type=int, default=30)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import bench  # noqa: E402

DEV = torch.device('cuda')
B, H = 4096, 10
FORMS = {'imagine()': {}, "imagine(shield='linear')": {'shield': 'linear'}}


def main():
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0), DEV, alg.env_params)
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)

    def run(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alg.imagine(**kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for _ in range(3):
        for kw in FORMS.values():
            run(kw)
    us = {k: [] for k in FORMS}
    for _ in range(ARGS.reps):
        for k, kw in FORMS.items():
            us[k].append(run(kw))
    res = {'tree': ARGS.label, 'B': B, 'H': H, 'reps': ARGS.reps}
    for k, v in us.items():
        a = np.asarray(v)
        res[k] = {'median_us': float(np.median(a)), 'p10_us': float(np.quantile(a, 0.1)),
                  'p90_us': float(np.quantile(a, 0.9)), 'min_us': float(a.min()), 'max_us': float(a.max())}
    print(json.dumps(res), flush=True)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
