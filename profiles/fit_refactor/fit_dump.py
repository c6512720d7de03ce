"""Dump what a model fit leaves behind, for a byte comparison of two builds.

    python profiles/fit_refactor/fit_dump.py --out DIR [--root TREE]

For configs 1-4 (model batch 256) under the production dispatch and with each of
fit_fb_enabled / fused_adam / split_bwd turned off, and for the head_hidden_layers = 2
model at config 2: m.fit(steps=5, noise=DeviceNoise(1234)) from a seeded start, then the
step losses, group.data, Adam m / v, both packed mirrors, holdout_losses and _elite_inds
go to DIR/<case>.<name>.bin, and one "sha256  file" line per file to DIR/digests.txt.
It uses m.fit and the engine switches only, so it runs unchanged on older commits
(--root: the checkout to import from; default: the one this file is in)."""
import argparse
import hashlib
import os
import sys

import numpy as np

SWITCHES = [('prod', {}), ('nofb', {'fit_fb_enabled': False}), ('noadam', {'fused_adam': False}),
            ('paired', {'split_bwd': False})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import bench
    from drpo_amd.rng import DeviceNoise
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device('cuda:0')
    lines = []

    def dump(case, name, arr):
        raw = np.ascontiguousarray(arr).tobytes()
        fn = f'{case}.{name}.bin'
        with open(os.path.join(args.out, fn), 'wb') as f:
            f.write(raw)
        lines.append(f'{hashlib.sha256(raw).hexdigest()}  {fn}')

    cases = [(c, 1, tag, sw) for c in (1, 2, 3, 4) for tag, sw in SWITCHES] + [(2, 2, 'prod', {})]
    for c, hhl, tag, sw in cases:
        cd = bench.CONFIGS[c]
        torch.manual_seed(7)
        alg = bench.make_alg(dev, 256, cd['H'], cd['E'], 7, bench.ENV_JSON[cd['env']], env=cd['env'],
                             extra={'model_cfg': {'head_hidden_layers': hhl}})
        rep = bench.synth_replay(cd['env'], 30000, np.random.RandomState(3))
        alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(dev) for k, v in rep.items()})
        m = alg.model_ensemble
        for k, v in sw.items():
            setattr(m.engine, k, v)
        losses = m.fit(alg.replay_buffer, steps=5, noise=DeviceNoise(1234))
        torch.cuda.synchronize()
        g = m.group
        g.ensure_packed()
        case = f'c{c}.h{hhl}.{tag}'
        dump(case, 'losses', np.asarray(losses, np.float64))
        dump(case, 'data', g.data.cpu().numpy())
        dump(case, 'adam_m', m.optimizer.m.cpu().numpy())
        dump(case, 'adam_v', m.optimizer.v.cpu().numpy())
        dump(case, 'packed', g.packed.cpu().numpy())
        dump(case, 'packedT', g.packedT.cpu().numpy())
        dump(case, 'holdout_losses', np.asarray(m.holdout_losses, np.float64))
        dump(case, 'elite_inds', np.asarray(m._elite_inds, np.int64))
        print(case, 'fit_fb', m.engine.fit_fb, 'fit_path', m.engine.fit_path, 'loss', losses[-1], flush=True)
    with open(os.path.join(args.out, 'digests.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
