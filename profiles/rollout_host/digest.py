"""sha256 of every tensor that rollout, the forms of imagine and model_rollout_error return on
one fixed scene, to compare two trees of this repository bit for bit:

  python profiles/rollout_host/digest.py [--tree DIR] > digest_X.txt

DIR (default: the tree this file lies in) is the checkout whose bench.py and package are
imported; it must hold a built library. The scene is the test suite's drifting quadrotor
(bench.make_alg quadrotor, E 7, B 72, H 3, 16-row tiles, steady mode with a +0.1 drift on z, the
replay's z spread over [0.6, 1.6]: rows end at steps 0, 1 and 2), the diff head's last layer
given small per-member weights so that the members differ. Every call gets a DeviceNoise of its
own fixed seed. One line per tensor: call, name, dtype, shape, sha256 of its bytes."""
import argparse
import hashlib
import os
import random
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import bench  # noqa: E402
import drpo_amd  # noqa: E402
from drpo_amd import ops  # noqa: E402

DEV = torch.device('cuda')
B, H, SEED = 72, 3, 1234
GROUPS = ('interventions', 'certificate', 'blend', 'disagreement', 'epistemic', 'aleatoric', 'max_disagreement')


def scene():
    random.seed(11)
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 400, np.random.RandomState(0))
    rep['states'][:, 2] = np.linspace(0.6, 1.6, 400, dtype=np.float32)
    rep['states'][:, [0, 4]] *= 0.1
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    m = alg.model_ensemble
    m.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    _, diff, _ = m.views()
    diff[-1][1][..., 2] = 0.1
    W = diff[-1][0]
    W.add_(0.003 * torch.randn(W.shape, generator=torch.Generator().manual_seed(23)).to(DEV))
    m._elite_inds = [3, 0, 6, 2, 5]
    alg.rollout_engine, alg.rows_per_tile = 2, 16
    return alg


def line(call, name, t):
    t = t.detach().contiguous().cpu()
    raw = t.view(torch.uint8) if t.dtype == torch.bool else t
    digest = hashlib.sha256(raw.numpy().tobytes()).hexdigest()
    print(call, name, str(t.dtype).replace('torch.', ''), list(t.shape), digest)


def imagined(call, im):
    print(call, 'members', im.members, 'given_steps', im.given_steps, 'shield', im.shield_threshold,
          im.shield_candidates)
    for k in ops.ImaginedRollout.TENSORS + GROUPS:
        if getattr(im, k) is not None:
            line(call, k, getattr(im, k))


def main():
    alg = scene()
    out = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED))
    torch.cuda.synchronize()
    print('rollout rows', len(out))
    for k, v in out.get(as_dict=True).items():
        line('rollout', k, v)

    alg = scene()                                   # the virtual buffer untouched again
    acts = torch.rand(B, 2, alg.action_dim, generator=torch.Generator().manual_seed(3)).to(DEV) * 2 - 1
    probe = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), shield=float('inf'))
    thr = float(probe.certificate[:, 0].median())
    thr_mean = float(alg.imagine(noise=drpo_amd.DeviceNoise(SEED), shield=('linear', float('inf'), 11))
                     .certificate[:, 0].median())
    print('thresholds', thr, thr_mean)
    forms = [('imagine()', {}), ('imagine(members=3)', dict(members=3)),
             ("imagine(members='each')", dict(members='each')),
             ('imagine(deterministic=True)', dict(deterministic=True)),
             ('imagine(model_noise=False)', dict(model_noise=False)), ('imagine(actions=[B,2,A])', dict(actions=acts)),
             ('imagine(shield=thr)', dict(shield=thr)),
             ("imagine(shield=('linear',thr,11))", dict(shield=('linear', thr_mean, 11))),
             ('imagine(uncertainty=True)', dict(uncertainty=True))]
    for call, kw in forms:
        im = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), **kw)
        torch.cuda.synchronize()
        imagined(call, im)
    imagined('imagine(), the private stream', alg.imagine())

    # real 3-step segments for model_rollout_error: an 8-step episode member 3 imagines from z = 0.6
    s0 = alg.replay_buffer.get('states')[:1].clone()
    seq = torch.rand(1, 8, alg.action_dim, generator=torch.Generator().manual_seed(19)).to(DEV) - 0.5
    ep = alg.imagine(states=s0, actions=seq, members=3, model_noise=False, horizon=8)
    n = int(ep.lengths[0])
    print('episode length', n)
    alg.replay_buffer.extend(states=ep.states[0, :n], actions=ep.actions[0, :n], next_states=ep.states[0, 1:n + 1],
                             rewards=ep.rewards[0, :n], dones=ep.dones[0, :n], violations=ep.violations[0, :n],
                             constraint_values=ep.constraint_values[0, :n])
    err = alg.model_rollout_error(3, members=0, uncertainty=True)
    torch.cuda.synchronize()
    for k in ('starts', 'state_error', 'reward_error', 'alive', 'disagreement', 'epistemic'):
        line('model_rollout_error(3)', k, getattr(err, k))
    imagined('model_rollout_error(3).imagined', err.imagined)


if __name__ == '__main__':
    main()
