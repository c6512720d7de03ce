"""SMBPO.plan(safety_filter=): the shield of the real controller inside the planner. The trainers,
start states and shapes are test_gpu_plan.py's (imagine_helpers._action_scene and the same with a
cost solver; P 5, N 32, H 3, the fixed member 3 and model_noise=False, so that a trajectory is a
function of its start state and its proposals alone).

Everything is bit for bit (float32 as int32): at +inf the filtered planner is the planner; a
plan's last iteration re-run through the public imagine(proposals=, shield=, lookahead=) gives
its scores and certificates; the new fields are gathers from that run."""
import numpy as np
import pytest
import torch

import drpo_amd
from drpo_amd import _lib
from gpu_helpers import _drifting_quadrotor_alg
from plan_helpers import INF, assert_bits, bits, plan_order
from test_gpu_plan import H, N, P, RUN, _alg, _key, _middle_threshold, _plan, _states

pytestmark = pytest.mark.gpu

PLAN_TENSORS = ('actions', 'action', 'score', 'certificate', 'feasible', 'n_feasible', 'mean', 'std', 'history_score',
                'history_certificate', 'history_feasible', 'candidates', 'scores', 'certificates', 'ranks')


def _filter_threshold(alg, **kw):
    """a shield threshold between the step-0 certificates of one iteration's candidates"""
    c = _plan(alg, iterations=1, safety_filter=INF, **kw).imagined.certificate[:, 0]
    return float(c.sort().values[c.numel() // 2])


def _best_alive(res, K):
    """[P, K] bool: the planned steps the best row of each state was alive at (beyond its length a
    trajectory holds zeros, whatever was proposed)."""
    rows = torch.arange(P, device=res.ranks.device) * N + res.ranks.argmin(dim=1)
    return res.imagined.mask[rows][:, :K]


def _linear_filter_threshold(alg, **kw):
    c = _plan(alg, iterations=1, safety_filter=('linear', INF), **kw).imagined.certificate[:, 0]
    return float(c.sort().values[c.numel() // 2])


# ------------------------------------------------------------------ 1. +inf is the planner
@pytest.mark.parametrize('spelling', [INF, ('linear', INF)], ids=['threshold', 'linear'])
@pytest.mark.parametrize('scene', ['reach', 'cost'])
def test_a_filter_that_never_steps_in_is_the_planner(scene, spelling):
    alg = _alg(scene)
    thr = _middle_threshold(alg)
    kw = dict(iterations=3, threshold=thr, temperature=1.0, steps=2)
    plain, filt = _plan(alg, **kw), _plan(alg, safety_filter=spelling, **kw)
    for k in PLAN_TENSORS:
        assert_bits(getattr(filt, k), getattr(plain, k), k)
    for k in type(plain.imagined).TENSORS:
        assert_bits(getattr(filt.imagined, k), getattr(plain.imagined, k), 'imagined.' + k)
    assert plain.threshold == filt.threshold and plain.lookahead_kind == filt.lookahead_kind
    assert all(getattr(plain, f) is None for f in type(plain).FILTER_FIELDS)
    assert filt.filter_threshold == INF and not bool(filt.interventions.any())
    assert filt.interventions.dtype == torch.bool and filt.interventions.shape == (P, H)
    assert filt.executed_actions.shape == (P, H, alg.action_dim) and filt.safe_action.shape == (P, alg.action_dim)
    live = _best_alive(filt, 2)
    assert bool(live[:, 0].all())
    assert_bits(filt.executed_actions[:, :2][live], filt.actions[live], 'executed: the proposals')
    assert_bits(filt.safe_action, filt.action, 'safe_action')


# ------------------------------------------------------------------ 2. one iteration, re-run in public
@pytest.mark.parametrize('K', [H, 1], ids=['K=H', 'K=1'])
@pytest.mark.parametrize('scene, kind, linear', [('reach', True, False), ('reach', 'bound', True), ('cost', True, False)],
                         ids=['reachability', 'bound-linear', 'cost'])
def test_one_iteration_is_imagine_proposals_scored_and_ordered(scene, kind, linear, K):
    alg = _alg(scene)
    A = alg.action_dim
    fthr = (_linear_filter_threshold if linear else _filter_threshold)(alg, steps=K, lookahead=kind)
    spelling = ('linear', fthr, 5) if linear else fthr
    thr = _middle_threshold(alg, steps=K, lookahead=kind, safety_filter=spelling)
    res = _plan(alg, iterations=1, steps=K, lookahead=kind, threshold=thr, safety_filter=spelling)
    assert res.filter_threshold == fthr and res.threshold == float(np.float32(thr))
    im = alg.imagine(_states(alg).repeat_interleave(N, 0), horizon=H, proposals=res.candidates.reshape(P * N, K, A),
                     shield=spelling, lookahead=kind, deterministic=True, noise=drpo_amd.DeviceNoise(99), **RUN)
    torch.cuda.synchronize()
    assert_bits(res.scores.reshape(-1), im.value_lookahead[:, H].contiguous(), 'scores')
    assert_bits(res.certificates.reshape(-1), im.certificate_lookahead[:, H].max(dim=-1).values, 'certificates')
    assert_bits(res.imagined.actions, im.actions, 'imagined.actions')
    assert torch.equal(res.imagined.interventions, im.interventions)
    assert res.imagined.given_steps == K
    n_iv, n_live = int(im.interventions[im.mask].sum()), int(im.mask.sum())
    assert 0 < n_iv < n_live, (n_iv, n_live)                  # the filter divides the proposals
    # the pick is the reference order's, on the filtered trajectories
    s, c = res.scores.cpu().numpy(), res.certificates.cpu().numpy()
    nf = res.n_feasible.cpu().numpy()
    for p in range(P):
        order, cls, _ = plan_order(s[p], c[p], thr)
        best = order[0]
        assert res.ranks[p].cpu().tolist() == [order.index(n) for n in range(N)], p
        assert nf[p] == cls.count(0)
        assert_bits(res.actions[p], res.candidates[p, best], f'actions[{p}]: a proposal')
        assert bits(res.score)[p] == bits(s)[p, best] and bits(res.certificate)[p] == bits(c)[p, best]
        # the new fields: the best row of the run
        assert_bits(res.executed_actions[p], im.actions[p * N + best], f'executed_actions[{p}]')
        assert torch.equal(res.interventions[p], im.interventions[p * N + best]), p
    assert_bits(res.action, res.actions[:, 0].contiguous(), 'action')
    assert_bits(res.safe_action, res.executed_actions[:, 0].contiguous(), 'safe_action')
    # executed differs from proposed exactly where the shield stepped in, over the planned steps
    # (the steps the best row was alive at)
    live = _best_alive(res, K).cpu()
    differs = torch.from_numpy((bits(res.executed_actions[:, :K]) != bits(res.actions)).any(axis=-1))
    assert torch.equal(differs[live], res.interventions[:, :K].cpu()[live]), (differs, res.interventions)
    assert not bool(res.interventions[:, :K].cpu()[~live].any())
    assert 0 < int(nf.sum()) < P * N                       # the planner's threshold divides the candidates
    # filtered and unfiltered rank differently: the filter is inside the score
    plain = _plan(alg, iterations=1, steps=K, lookahead=kind, threshold=thr)
    assert_bits(plain.candidates, res.candidates, 'the same proposals')
    assert not np.array_equal(bits(plain.scores), bits(res.scores))


# ------------------------------------------------------------------ 3. what the iterations promise
@pytest.mark.parametrize('scene, linear', [('reach', False), ('reach', True), ('cost', False)],
                         ids=['reachability', 'linear', 'cost'])
def test_the_incumbents_key_never_decreases(scene, linear):
    alg = _alg(scene)
    fthr = (_linear_filter_threshold if linear else _filter_threshold)(alg)
    spelling = ('linear', fthr) if linear else fthr
    thr = _middle_threshold(alg, safety_filter=spelling)
    res = _plan(alg, iterations=4, threshold=thr, temperature=1.0, safety_filter=spelling)
    f, s, c = res.history_feasible.cpu(), res.history_score.cpu(), res.history_certificate.cpu()
    assert f.shape == (4, P)
    keys = [[_key(f[i, p], s[i, p], c[i, p]) for p in range(P)] for i in range(4)]
    for i in range(3):
        for p in range(P):
            assert keys[i + 1][p] >= keys[i][p], (i, p, keys[i][p], keys[i + 1][p])
    print('keys of the first and the last iteration:', keys[0], keys[3])
    assert_bits(res.history_score[3], res.score, 'score')
    # the incumbent is a proposal of the last iteration, copied
    best = res.ranks.cpu().argmin(dim=1)
    assert_bits(res.actions, res.candidates[torch.arange(P), best.to(res.candidates.device)], 'actions')
    assert bool(res.imagined.interventions.any())


# ------------------------------------------------------------------ 4. nothing else moves
def test_plan_leaves_the_training_state_alone(monkeypatch):
    from test_gpu_imagine_lookahead import _virtual
    alg = _drifting_quadrotor_alg(16)
    alg.imagine()                                            # (so that imagine's private stream exists)
    torch.cuda.synchronize()
    before = _virtual(alg)
    ctrs = (alg.noise.ctr, alg._imagine_noise.ctr)
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_refit', 'drpo_rollout_trajectories_given', 'drpo_rollout_lookahead',
                 'drpo_rollout', 'drpo_rollout_trajectories', 'drpo_rollout_trajectories_proposed',
                 'drpo_rollout_trajectories_shielded', 'drpo_rollout_trajectories_linear'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    res = alg.plan(_states(alg), H, candidates=N, iterations=2, init='policy', safety_filter=True, **RUN)
    torch.cuda.synchronize()
    # per iteration one sample launch, one proposals rollout, one refit; the policy's own run is unshielded
    assert calls == ['drpo_rollout_trajectories'] + ['drpo_plan_sample', 'drpo_rollout_trajectories_proposed',
                                                     'drpo_plan_refit'] * 2
    assert res.filter_threshold == alg.safe_shield_threshold
    assert (alg.noise.ctr, alg._imagine_noise.ctr) == ctrs
    after = _virtual(alg)
    assert before[1:] == after[1:]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    assert res.imagined.step_q is None and res.imagined.value_lookahead is None
    # off means off: without a filter and without proposals the new entry point is not reached
    calls.clear()
    alg.plan(_states(alg), H, candidates=N, iterations=1, safety_filter=None, **RUN)
    alg.imagine(shield=True)
    alg.imagine(shield='linear')
    alg.imagine(_states(alg), actions=res.candidates[:, 0].contiguous())
    alg.imagine()
    torch.cuda.synchronize()
    assert calls == ['drpo_plan_sample', 'drpo_rollout_trajectories_given', 'drpo_plan_refit',
                     'drpo_rollout_trajectories_shielded', 'drpo_rollout_trajectories_linear',
                     'drpo_rollout_trajectories_given', 'drpo_rollout_trajectories']
