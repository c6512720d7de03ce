"""plan(refine=): gradient refinement of the planner's incumbent, on the scene of the plan tests
(imagine_helpers._action_scene). P 3 start states, N 16 candidates, H 3, the fixed member 0 and
model_noise=False, so that a trajectory is a function of its start state and actions alone.

Bit for bit (float32 as int32) wherever two computations are the same: refine=0 is the planner as
it is; an accepted trial is the sequence the formula gives from the round's gradient; a round that
accepts nothing leaves the sequence alone. The monotonicity checks compare float32 scores the
ranking kernel itself stored.

One quality figure, recorded and not asserted (a run with -s prints it): the mean
refine_score[-1] - refine_score[0] over the feasible states at R = 2, threshold inf: 0.175 on an
MI355X (scores 5.01, 6.48, 0.75 before)."""
import pytest
import torch

import drpo_amd
from drpo_amd import ops
from gpu_helpers import DEV
from imagine_helpers import _action_scene
from plan_helpers import INF

pytestmark = pytest.mark.gpu

P, N, H = 3, 16, 3
RUN = dict(members=0, model_noise=False)
ETA, TRIALS = 0.5, 8
_SCENE = []


def _alg():
    if not _SCENE:
        _SCENE.append(_action_scene(DEV)[0])
    return _SCENE[0]


def _states(alg):
    return alg.replay_buffer.get('states')[40:400:120][:P].clone()


def _plan(alg, seed=11, **kw):
    res = alg.plan(_states(alg), H, **dict(dict(candidates=N, iterations=2, noise=drpo_amd.DeviceNoise(seed)), **RUN, **kw))
    torch.cuda.synchronize()
    return res


def _bits(x):
    x = x.detach().cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _middle_threshold(alg):
    """between the incumbents' certificates where it can be, so that states are feasible and others not"""
    c = _plan(alg, threshold=INF).certificate.cpu().sort().values
    return float((c[0] + c[1]) / 2) if float(c[0]) < float(c[1]) else float(c[-1])


def test_refine_off_is_the_planner_as_it_is():
    alg = _alg()
    a, b = _plan(alg), _plan(alg, refine=0, refine_trials=3, refine_step=0.25)
    for k in ops.PlanResult.FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        if torch.is_tensor(x):
            assert _same(x, y), k
        elif k == 'imagined':
            for t in x.TENSORS:
                assert _same(getattr(x, t), getattr(y, t)), t
        else:
            assert x == y, k
    assert b.refine_score is None and b.refine_accepted is None and b.refine_gradient is None


@pytest.mark.parametrize('threshold', ['inf', 'middle'])
def test_the_incumbents_score_never_decreases(threshold):
    alg = _alg()
    thr = INF if threshold == 'inf' else _middle_threshold(alg)
    R = 3
    base, res = _plan(alg, threshold=thr), _plan(alg, threshold=thr, refine=R, refine_trials=TRIALS, refine_step=ETA)
    assert tuple(res.refine_score.shape) == (R + 1, P) and tuple(res.refine_accepted.shape) == (R, P)
    assert tuple(res.refine_gradient.shape) == (P, H, alg.action_dim) and res.refine_accepted.dtype == torch.int32
    score, acc = res.refine_score.cpu(), res.refine_accepted.cpu()
    feas0 = base.feasible.cpu()
    print(f'threshold {threshold}: feasible {feas0.tolist()}, refine_score {score.tolist()}, accepted {acc.tolist()}')
    assert _same(score[0], base.score) and _same(res.score, score[-1])
    assert bool((res.feasible.cpu().int() >= feas0.int()).all())                        # never turns false
    assert bool((score[1:, feas0] >= score[:-1, feas0]).all())
    assert bool(((acc >= -1) & (acc < TRIALS)).all())
    assert bool((acc[:, ~feas0] == -1).all()) and _same(res.actions[~feas0.to(DEV)], base.actions[~feas0.to(DEV)])
    moved = (acc >= 0).any(dim=0)
    assert bool((score[-1, moved] >= score[0, moved]).all())
    # everything the sampling iterations left stays theirs
    for k in ('mean', 'std', 'candidates', 'scores', 'certificates', 'ranks', 'n_feasible', 'history_score'):
        assert _same(getattr(res, k), getattr(base, k)), k
    if threshold == 'inf':
        assert feas0.all()
        gain = (score[2] - score[0])[feas0].mean()       # (the figure at R = 2: the rounds do not depend on R)
        print(f'QUALITY: mean refine_score[-1] - refine_score[0] over feasible states at R = 2: {float(gain):.6g}')
        assert bool(moved.any()), 'no state took a gradient step: the scene shows nothing'


def test_an_accepted_trial_is_the_formulas_sequence():
    alg = _alg()
    base, res = _plan(alg, threshold=INF), _plan(alg, threshold=INF, refine=1, refine_trials=TRIALS, refine_step=ETA)
    acc, g, a0 = res.refine_accepted[0].cpu(), res.refine_gradient, base.actions
    assert bool((acc >= 0).any())
    gmax = g.abs().amax(dim=(1, 2))
    for p in range(P):
        j = int(acc[p])
        if j < 0:
            assert _same(res.actions[p], a0[p]), p
            continue
        want = (a0[p] + (ETA * 2.0 ** -j) * (g[p] / gmax[p])).clamp(-1.0, 1.0)
        assert _same(res.actions[p], want), (p, j)
        assert float(res.score[p]) >= float(base.score[p])
    # the refined sequence scores what the planner says it does (the public imagine, re-run)
    im = alg.imagine(_states(alg), horizon=H, actions=res.actions, lookahead=True, deterministic=True,
                     noise=drpo_amd.DeviceNoise(3), **RUN)
    assert _same(im.value_lookahead[:, H], res.score)


def test_infeasible_and_flat_states_are_carried_through(monkeypatch):
    alg = _alg()
    base = _plan(alg, threshold=-INF)
    res = _plan(alg, threshold=-INF, refine=2, refine_trials=TRIALS, refine_step=ETA)
    assert not base.feasible.any() and not res.feasible.any()
    assert bool((res.refine_accepted == -1).all()) and _same(res.actions, base.actions)
    assert _same(res.score, base.score) and _same(res.certificate, base.certificate)
    # a zero gradient (state 0) and a NaN one (state 1): the incumbent stays
    real = ops.value_gradient

    def flat(*a, **k):
        vg = real(*a, **k)
        vg.grad_actions[0] = 0.0
        vg.grad_actions[1, 0, 0] = float('nan')
        return vg
    monkeypatch.setattr(ops, 'value_gradient', flat)
    base, res = _plan(alg, threshold=INF), _plan(alg, threshold=INF, refine=1, refine_trials=TRIALS, refine_step=ETA)
    assert res.refine_accepted[0].cpu().tolist()[:2] == [-1, -1]
    assert _same(res.actions[:2], base.actions[:2]) and _same(res.score[:2], base.score[:2])
    assert torch.isfinite(res.actions).all()


def test_mpc_with_refinement():
    alg = _alg()
    ctl = alg.mpc(horizon=H, candidates=N, iterations=2, threshold=INF, refine=1, refine_trials=4,
                  noise=drpo_amd.DeviceNoise(9), **RUN)
    s = _states(alg)
    for step in range(3):
        a = ctl.act(s)
        torch.cuda.synchronize()
        assert tuple(a.shape) == (P, alg.action_dim) and torch.isfinite(a).all() and bool((a.abs() <= 1).all())
        assert ctl.last.warm_started == (step > 0)
        assert tuple(ctl.last.refine_score.shape) == (2, P)
        assert bool((ctl.last.refine_score[1] >= ctl.last.refine_score[0]).all())
        s = s + 0.01
