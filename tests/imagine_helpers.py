"""What the tests of SMBPO.imagine share (tests/test_gpu_imagine*.py): the scenes, the oracle's
certificate and the comparisons.

The scene of most tests is gpu_helpers._drifting_quadrotor_alg: B 72 (four full 16-row tiles
and one of 8, or two 32-row tiles and one of 8), H 3, S 12, A 2, C 2, rows leaving at steps 0,
1 and 2 while others survive. Between calls of the kernel everything is compared bit for bit
(float32 as int32); against the oracle |d| <= 2e-4 + 2e-4 |ref| (_tol), the tolerance of the
rollout tests; an actor's mean action against the stand-alone op at the project's forward
tolerance 1e-4 + 1e-4 |ref| (tanhf there, fast_tanh in the kernel).

The action scene (_action_scene). bench.make_alg quadrotor at the default widths, E 7, seed 0,
with the raw initial weights. Those alone make a model that all but ignores its input (two
action sets move its prediction by 4e-5 at most, below the tolerance), so the four weight
matrices on the mean path (trunk.0, trunk.2, diff_head.0, diff_head.2) are scaled by 6: the same
two action sets then move the prediction by 0.012 on average and 0.064 at most, 30 and 160 times
the tolerance. The diff head's z bias adds a drift of +0.05 per step and the replay's z is spread
over [0.6, 1.6], so rows leave z <= 1.5 by their height (the scaled model adds to the drift
where z is high)."""
import random

import numpy as np
import torch

import bench
import drpo_amd
from drpo_amd import ops
from gpu_helpers import COMP, _drifting_quadrotor_alg
from oracle import drpo_oracle as O

B, H = 72, 3
PRE = 'model_ensemble.'
MEMBER = 3
INF = float('inf')
SEED = 1234
TENSORS = ops.ImaginedRollout.TENSORS


# ------------------------------------------------------------------ comparisons
def flatten(im):
    """The trajectories in the reference's order (src/smbpo.py:243-246): for t in 0..H-1,
    the rows with length > t, in batch order. states[:, t] stands for the states and
    states[:, t + 1] for the next states."""
    length = im.lengths.cpu()
    t_ = {k: getattr(im, k).cpu() for k in TENSORS}
    rows = {k: [] for k in COMP}
    for t in range(t_['rewards'].shape[1]):
        keep = length > t
        rows['states'].append(t_['states'][keep, t])
        rows['next_states'].append(t_['states'][keep, t + 1])
        for k in ('actions', 'rewards', 'constraint_values', 'dones', 'violations'):
            rows[k].append(t_[k][keep, t])
    return {k: torch.cat(v) for k, v in rows.items()}


def bits(x):
    x = x.detach().cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def assert_same(a, b, names=TENSORS):
    for k in names:
        x, y = (getattr(a, k), getattr(b, k)) if not isinstance(a, dict) else (a[k], b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(bits(x), bits(y)), k


def _assert_every_length(im):
    """Otherwise the scene shows nothing: rows of every length, ended and cut ones."""
    length, term = im.lengths.cpu().numpy(), im.terminated.cpu().numpy().astype(bool)
    assert set(length.tolist()) == {1, 2, 3}
    assert term.any() and (~term).any()
    assert (length[~term] == H).all()


def _tol(ref):
    return 2e-4 + 2e-4 * ref.abs()


# ------------------------------------------------------------------ scenes and inputs
_ALG = {}


def _scene(rpt):
    """_drifting_quadrotor_alg(rpt), one per tile height for every module: leave it as it is."""
    if rpt not in _ALG:
        _ALG[rpt] = _drifting_quadrotor_alg(rpt)
    return _ALG[rpt]


def _imagine(alg, seed=SEED, **kw):
    im = alg.imagine(noise=drpo_amd.DeviceNoise(seed), **kw)
    torch.cuda.synchronize()
    return im


def _teacher_inputs(alg):
    """72 start states over the whole z range, recorded action and model draws."""
    g = torch.Generator().manual_seed(7)
    s = alg.replay_buffer.get('states')[2:400:5][:B].cpu().clone()
    eps_a = torch.randn(H, B, alg.action_dim, generator=g)
    eps_m = torch.randn(H, B, alg.state_dim + 1, generator=g)
    return s, eps_a, eps_m


SCALE, DRIFT = 6.0, 0.05
EP_LEN, EP2_LEN = 12, 6


def _action_scene(dev, scale=SCALE):
    random.seed(11)
    alg = bench.make_alg(dev, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 400, np.random.RandomState(0))
    rep['states'][:, 2] = np.linspace(0.6, 1.6, 400, dtype=np.float32)
    rep['states'][:, [0, 4]] *= 0.1            # well inside the x and pitch bounds
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(dev) for k, v in rep.items()})
    m = alg.model_ensemble
    mean, std = O.normalizer_fit(torch.from_numpy(rep['states']))
    m.state_normalizer.mean.copy_(mean)
    m.state_normalizer.std.copy_(std)
    trunk, diff, _ = m.views()
    for W in (trunk[0][0], trunk[1][0], diff[0][0], diff[1][0]):
        W.mul_(scale)
    diff[-1][1][..., 2] = DRIFT
    m._elite_inds = [3, 0, 6, 2, 5]
    alg.rollout_engine, alg.rows_per_tile = 2, 16
    P = {k: v.detach().cpu().clone() for k, v in alg.state_dict().items() if k.startswith(PRE)}
    return alg, rep, P


def _episode_inputs(rep):
    """Start states and action sequences of the two model-made episodes."""
    g = torch.Generator().manual_seed(19)
    s0 = torch.from_numpy(rep['states'][[20, 60]].copy())        # z = 0.65 and 0.75
    seq = 0.5 * (torch.rand(2, EP_LEN, 2, generator=g) * 2 - 1)
    return s0, seq


# ------------------------------------------------------------------ the oracle's certificate
def _params(alg):
    """The oracle's flat parameter dict: solver.* without the prefix, model_ensemble.* with it."""
    sd = {k: v.detach().cpu().clone() for k, v in alg.state_dict().items()}
    P = {k[len('solver.'):]: v for k, v in sd.items() if k.startswith('solver.')}
    P.update({k: v for k, v in sd.items() if k.startswith(PRE)})
    return P


def oracle_qc(P, alg, s, a, unc=False):
    """get_qc of the constraint critic at (s, a): its distributional bound (unc; what
    _shielded_action asks for is unc = alg.solver.distributional_qc) or its mean."""
    cc = alg.constraint_critic
    q = O.cons_critic(P, 'constraint_critic.', s, a, 'uncertainty' if unc else 'mean', std_ratio=cc.std_ratio,
                      rng=O.LiveRNG(), lmin=cc.log_std_min, lmax=cc.log_std_max)
    return O.get_qc(q, cc.output_dim)


def check_certificate_at_step_0(alg, im, unc=False):
    """Of a run without interventions (its actions are the actor's): the oracle's
    certificate at the kernel's own (states[:, 0], actions[:, 0])."""
    q = oracle_qc(_params(alg), alg, im.states[:, 0].cpu(), im.actions[:, 0].cpu(), unc)
    err = (im.certificate[:, 0].cpu() - q).abs()
    print(f'certificate at step 0: {float(q.min()):.4f} .. {float(q.max()):.4f}, max |d| {float(err.max()):.3g}')
    assert bool((err <= _tol(q)).all()), float(err.max())


def check_replay_and_safe_action(alg, im, **kw):
    """Of a run in which every alive step took the safe actor's action: the member path saw the
    selected action and nothing else (the replay under the run's own actions, K = H, is the
    run), and the action is the safe actor's."""
    re = _imagine(alg, actions=im.actions, **dict({'members': im.members}, **kw))
    assert re.given_steps == im.rewards.shape[1] and re.interventions is None and re.blend is None
    assert_same(im, re)
    for t in range(im.rewards.shape[1]):
        live = im.mask[:, t]
        ref = alg.actor_safe.act(im.states[:, t], eval=True)
        err = (im.actions[:, t] - ref).abs()[live]
        assert bool((err <= 1e-4 + 1e-4 * ref.abs()[live]).all()), (t, float(err.max()))
