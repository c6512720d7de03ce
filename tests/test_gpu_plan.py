"""SMBPO.plan: sampling-based planning on the model, on the small trainers of the imagine tests
(imagine_helpers._action_scene, the same scene with a cost solver, and
gpu_helpers._drifting_quadrotor_alg where a fresh trainer is needed). P 5 start states over the
replay's z range, N 32 candidates, H 3, the fixed ensemble member 3 and model_noise=False, so that
a trajectory is a function of its start state and actions alone.

Everything is bit for bit (float32 as int32): a plan's last iteration re-run through the public
imagine(actions=, lookahead=) gives its scores and certificates, the pick is the reference
order's (plan_helpers.plan_order), the same seed gives the same bits. The monotonicity checks
compare float32 keys the kernel itself stored."""
import random

import numpy as np
import pytest
import torch

import bench
import drpo_amd
from drpo_amd import _lib, ops
from gpu_helpers import DEV, _drifting_quadrotor_alg
from imagine_helpers import B, DRIFT, MEMBER, SCALE, _action_scene
from plan_helpers import INF, assert_bits, bits, plan_order

pytestmark = pytest.mark.gpu

P, N, H = 5, 32, 3          # (H: imagine_helpers' horizon too)
RUN = dict(members=MEMBER, model_noise=False)


_SCENES = {}


def _alg(scene):
    """The action scene of imagine_helpers, whose model answers to its actions (the drifting scene's
    all but ignores them: every candidate of a state would tie), and the same with a cost solver.
    One each: leave them as they are."""
    if scene not in _SCENES:
        if scene == 'reach':
            alg = _action_scene(DEV)[0]
        else:
            alg = _cost_action_scene()
        _SCENES[scene] = alg
    return _SCENES[scene]


def _cost_action_scene():
    """imagine_helpers._action_scene with a constrained_fcn='cost' solver (one critic output for the
    two constraints), as test_gpu_imagine_lookahead._cost_scene configures it. (That scene's model is
    the bench's steady one, whose last diff layer is zero: its predictions ignore the actions.)"""
    random.seed(11)
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON,
                         extra={'sac_cfg': {'constrained_fcn': 'cost', 'distributional_qc': False,
                                            'qc_under_uncertainty': False, 'mlp_multiplier': False}})
    rep = bench.synth_replay('quadrotor', 400, np.random.RandomState(0))
    rep['states'][:, 2] = np.linspace(0.6, 1.6, 400, dtype=np.float32)
    rep['states'][:, [0, 4]] *= 0.1
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    m = alg.model_ensemble
    m.state_normalizer.fit(alg.replay_buffer.get('states'))
    trunk, diff, _ = m.views()
    for W in (trunk[0][0], trunk[1][0], diff[0][0], diff[1][0]):
        W.mul_(SCALE)
    diff[-1][1][..., 2] = DRIFT
    m._elite_inds = [3, 0, 6, 2, 5]
    alg.rollout_engine, alg.rows_per_tile = 2, 16
    assert alg.solver.constrained_fcn == 'cost' and alg.solver.constraint_critic.output_dim == 1
    return alg


def _states(alg):
    return alg.replay_buffer.get('states')[40:400:72][:P].clone()


def _plan(alg, seed=11, **kw):
    res = alg.plan(_states(alg), H, **dict(dict(candidates=N, noise=drpo_amd.DeviceNoise(seed)), **RUN, **kw))
    torch.cuda.synchronize()
    return res


def _key(feasible, score, cert):
    """the order's key of a best row: feasible rows above the others, then score / -cert"""
    return (1, float(score)) if bool(feasible) else (0, -float(cert))


def _middle_threshold(alg, **kw):
    """a threshold between the candidates' certificates, so that states have feasible rows and others"""
    c = _plan(alg, iterations=1, threshold=INF, **kw).certificates
    return float(c.flatten().sort().values[c.numel() // 2])


# ------------------------------------------------------------------ 1. one iteration, re-run in public
@pytest.mark.parametrize('K', [H, 1], ids=['K=H', 'K=1'])
@pytest.mark.parametrize('scene, kind', [('reach', True), ('reach', 'bound'), ('cost', True)],
                         ids=['reachability', 'bound', 'cost'])
def test_one_iteration_is_imagine_scored_and_ordered(scene, kind, K):
    alg = _alg(scene)
    thr = _middle_threshold(alg, steps=K, lookahead=kind)
    res = _plan(alg, iterations=1, steps=K, lookahead=kind, threshold=thr)
    A = alg.action_dim
    assert res.candidates.shape == (P, N, K, A) and res.scores.shape == res.certificates.shape == res.ranks.shape == (P, N)
    assert res.actions.shape == (P, K, A) and res.action.shape == (P, A) and res.mean.shape == res.std.shape == (P, K, A)
    assert res.history_score.shape == res.history_certificate.shape == res.history_feasible.shape == (1, P)
    assert res.lookahead_kind == ('mean' if kind is True else 'bound') and res.threshold == float(np.float32(thr))
    assert res.feasible.dtype == torch.bool and res.n_feasible.dtype == res.ranks.dtype == torch.int32
    im = alg.imagine(_states(alg).repeat_interleave(N, 0), horizon=H, actions=res.candidates.reshape(P * N, K, A),
                     lookahead=kind, deterministic=True, noise=drpo_amd.DeviceNoise(99), **RUN)
    torch.cuda.synchronize()
    assert_bits(res.scores.reshape(-1), im.value_lookahead[:, H].contiguous(), 'scores')
    assert_bits(res.certificates.reshape(-1), im.certificate_lookahead[:, H].max(dim=-1).values, 'certificates')
    assert_bits(res.imagined.actions, im.actions, 'imagined.actions')
    assert res.imagined.given_steps == K
    # the pick is the reference order's
    s, c = res.scores.cpu().numpy(), res.certificates.cpu().numpy()
    nf = res.n_feasible.cpu().numpy()
    for p in range(P):
        order, cls, _ = plan_order(s[p], c[p], thr)
        best = order[0]
        assert res.ranks[p].cpu().tolist() == [order.index(n) for n in range(N)], p
        assert nf[p] == cls.count(0)
        assert_bits(res.actions[p], res.candidates[p, best], f'actions[{p}]')
        assert bits(res.score)[p] == bits(s)[p, best] and bits(res.certificate)[p] == bits(c)[p, best]
        assert bool(res.feasible[p]) == (cls[best] == 0)
    assert_bits(res.action, res.actions[:, 0].contiguous(), 'action')
    assert_bits(res.history_score[0], res.score, 'history_score')
    assert 0 < int(nf.sum()) < P * N                       # the threshold divides the candidates
    assert len(np.unique(s)) > P * N // 2                  # the candidates differ


# ------------------------------------------------------------------ 2. what the iterations promise
@pytest.mark.parametrize('scene', ['reach', 'cost'])
def test_the_incumbents_key_never_decreases(scene):
    alg = _alg(scene)
    thr = _middle_threshold(alg)
    res = _plan(alg, iterations=4, threshold=thr, temperature=1.0)
    f, s, c = res.history_feasible.cpu(), res.history_score.cpu(), res.history_certificate.cpu()
    assert f.shape == (4, P)
    keys = [[_key(f[i, p], s[i, p], c[i, p]) for p in range(P)] for i in range(4)]
    for i in range(3):
        for p in range(P):
            assert keys[i + 1][p] >= keys[i][p], (i, p, keys[i][p], keys[i + 1][p])
    print('keys of the first and the last iteration:', keys[0], keys[3])
    assert_bits(res.history_score[3], res.score, 'score')
    assert float(res.std.min()) >= np.float32(0.05)


@pytest.mark.parametrize('K', [H, 2])
def test_from_the_policy_it_is_no_worse_than_the_policy(K):
    alg = _alg('reach')
    own = alg.imagine(_states(alg), horizon=H, deterministic=True, lookahead=True, noise=drpo_amd.DeviceNoise(3), **RUN)
    s0, c0 = own.value_lookahead[:, H].cpu(), own.certificate_lookahead[:, H].max(dim=-1).values.cpu()
    thr = float(c0.sort().values[P // 2])
    noise = drpo_amd.DeviceNoise(21)
    res = alg.plan(_states(alg), H, candidates=N, iterations=2, steps=K, init='policy', threshold=thr, noise=noise,
                   **RUN)
    torch.cuda.synchronize()
    assert noise.ctr == 1 + 2 * 2          # the policy's run, then a sample launch and an imagine per iteration
    for p in range(P):
        policy_key = _key(c0[p] <= np.float32(thr), s0[p], c0[p])
        assert _key(res.feasible[p], res.score[p], res.certificate[p]) >= policy_key, p
    first = alg.plan(_states(alg), H, candidates=N, iterations=1, steps=K, init='policy', threshold=thr,
                     noise=drpo_amd.DeviceNoise(21), **RUN)
    assert_bits(first.candidates[:, 0].contiguous(), own.actions[:, :K].contiguous(), 'candidate 0: the policy')
    assert_bits(first.scores[:, 0].contiguous(), own.value_lookahead[:, H].contiguous(), 'its score')


def test_the_infinite_thresholds():
    alg = _alg('reach')
    low, high = _plan(alg, iterations=1, threshold=-INF), _plan(alg, iterations=1, threshold=INF)
    assert_bits(low.scores, high.scores, 'scores')
    assert low.n_feasible.tolist() == [0] * P and not bool(low.feasible.any()) and low.threshold == -INF
    assert high.n_feasible.tolist() == [N] * P and bool(high.feasible.all())
    assert_bits(low.certificate, low.certificates.min(dim=1).values, 'the least certificate')
    assert_bits(high.score, high.scores.max(dim=1).values, 'the largest score')
    assert high.ranks.cpu().gather(1, high.scores.cpu().argmax(dim=1, keepdim=True)).flatten().tolist() == [0] * P


def test_the_same_seed_gives_the_same_bits():
    alg = _alg('reach')
    kw = dict(iterations=3, temperature=0.5, momentum=0.25, steps=2)
    a, b, c = _plan(alg, seed=5, **kw), _plan(alg, seed=5, **kw), _plan(alg, seed=6, **kw)
    for k in ('actions', 'score', 'certificate', 'mean', 'std', 'candidates', 'scores', 'certificates', 'ranks',
              'history_score', 'history_certificate'):
        assert_bits(getattr(a, k), getattr(b, k), k)
    assert not torch.equal(a.candidates, c.candidates)
    # the default stream is private to plan and derived from the trainer's seed
    fresh = [_drifting_quadrotor_alg(16) for _ in range(2)]
    d, e = (x.plan(_states(x), H, candidates=N, iterations=2, **RUN) for x in fresh)
    assert_bits(d.candidates, e.candidates, 'candidates')
    assert fresh[0]._plan_noise.ctr == 4 and fresh[0]._plan_noise is not fresh[0].noise
    assert fresh[0]._plan_noise.seed != fresh[0].noise.seed


# ------------------------------------------------------------------ 3. nothing else moves
def test_plan_leaves_the_training_state_alone(monkeypatch):
    from test_gpu_imagine_lookahead import _virtual
    alg = _drifting_quadrotor_alg(16)
    alg.imagine()                                            # (so that imagine's private stream exists)
    torch.cuda.synchronize()
    before = _virtual(alg)
    ctrs = (alg.noise.ctr, alg._imagine_noise.ctr)
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_refit', 'drpo_rollout_trajectories_given', 'drpo_rollout_lookahead',
                 'drpo_rollout', 'drpo_rollout_trajectories'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    res = alg.plan(_states(alg), H, candidates=N, iterations=2, init='policy', **RUN)
    torch.cuda.synchronize()
    # per iteration one sample launch, one given-actions rollout, one refit; no buffer rollout, no full lookahead
    assert calls == ['drpo_rollout_trajectories'] + ['drpo_plan_sample', 'drpo_rollout_trajectories_given',
                                                     'drpo_plan_refit'] * 2
    assert (alg.noise.ctr, alg._imagine_noise.ctr) == ctrs
    after = _virtual(alg)
    assert before[1:] == after[1:]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    assert res.imagined.step_q is None and res.imagined.value_lookahead is None       # the B * H critic rows are skipped
    # imagine and rollout without plan make the calls they made before
    calls.clear()
    terminal = []
    real_terminal = ops._terminal_critics
    monkeypatch.setattr(ops, '_terminal_critics', lambda *a: (terminal.append(a[3]), real_terminal(*a))[1])
    alg.imagine(lookahead='bound')
    alg.imagine(_states(alg), actions=res.candidates[:, 0].contiguous())
    alg.rollout(alg.actor)
    torch.cuda.synchronize()
    assert calls == ['drpo_rollout_trajectories', 'drpo_rollout_lookahead', 'drpo_rollout_trajectories_given',
                     'drpo_rollout']
    assert terminal == ['bound']
