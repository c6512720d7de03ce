"""Receding-horizon control on SMBPO.plan: warm_start= / shift= / reset= / tail= / warm_std=,
noise_beta=, SMBPO.mpc's controller and evaluate(controller=), on test_gpu_plan's scene and
sizes (imagine_helpers._action_scene; P 5, N 32, H 3, the fixed member 3, model_noise=False, so
that a row is a function of its start state and actions alone). Everything is bit for bit: a warm
start's candidates are ops.plan_sample of ops.plan_shift of the previous result at the same seed
and counter, their scores are the public imagine(actions=, lookahead=)'s, a reset state's rows
are the cold call's. The one inequality compares float32 keys the kernel itself stored."""
import numpy as np
import pytest
import torch

import drpo_amd
from drpo_amd import _lib, ops
from drpo_amd.envs import ProductEnv
from gpu_helpers import DEV, _drifting_quadrotor_alg, _width_alg
from plan_mpc_helpers import INF, RecordingController, assert_bits
from test_gpu_plan import H, N, P, RUN, _alg, _key, _middle_threshold, _plan, _states

pytestmark = pytest.mark.gpu

OFF = dict(warm_start=None, shift=1, reset=None, tail=None, warm_std=None, noise_beta=0.0)
COMPARED = ('actions', 'action', 'score', 'certificate', 'feasible', 'n_feasible', 'mean', 'std', 'history_score',
            'history_certificate', 'history_feasible', 'candidates', 'scores', 'certificates', 'ranks')

_FIRST = {}


def _first(iterations=2):
    """A cold plan of the scene at seed 11, shared: the previous control step of the warm starts."""
    if iterations not in _FIRST:
        alg = _alg('reach')
        _FIRST[iterations] = _plan(alg, iterations=iterations, threshold=_middle_threshold(alg))
    return _FIRST[iterations]


def _same(a, b, names=COMPARED):
    for k in names:
        assert_bits(getattr(a, k), getattr(b, k), k)


# ------------------------------------------------------------------ 1. off is off
def test_every_new_argument_off_is_the_call_without_them(monkeypatch):
    alg = _alg('reach')
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_sample_ar', 'drpo_plan_shift'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    kw = dict(iterations=2, temperature=0.5, steps=2)
    a, b = _plan(alg, seed=5, **kw), _plan(alg, seed=5, **kw, **OFF)
    _same(a, b)
    assert calls == ['drpo_plan_sample'] * 4
    assert (b.noise_beta, b.warm_started, b.shift) == (0.0, False, None)
    assert all(getattr(b, f) is None for f in ops.PlanResult.FILTER_FIELDS)


# ------------------------------------------------------------------ 2. one warm iteration, re-run in public
@pytest.mark.parametrize('beta', [0.0, 0.5])
@pytest.mark.parametrize('shift', [0, 1, H])
def test_a_warm_iteration_is_shift_sample_imagine(shift, beta, monkeypatch):
    alg, res1 = _alg('reach'), _first()
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_sample_ar', 'drpo_plan_shift'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    res = _plan(alg, seed=23, iterations=1, warm_start=res1, shift=shift, noise_beta=beta, warm_std=0.2,
                init_std=0.4, threshold=res1.threshold)
    assert calls == ['drpo_plan_shift', 'drpo_plan_sample' if beta == 0 else 'drpo_plan_sample_ar']
    assert (res.noise_beta, res.warm_started, res.shift) == (beta, True, shift)
    noise = drpo_amd.DeviceNoise(23)
    start = ops.plan_shift(res1.mean, res1.std, res1.actions, shift=shift, fresh_std=0.4, std_floor=0.2)
    cand = ops.plan_sample(*start, N, noise.seed, noise.next(), corr=beta)
    A = alg.action_dim
    assert_bits(res.candidates, cand.reshape(P, N, H, A), 'candidates')
    # candidate 0 is the shifted best sequence, not the shifted mean
    assert_bits(res.candidates[:, 0, :H - shift], res1.actions[:, shift:], 'candidate 0')
    if shift < H:
        assert not torch.equal(res1.actions[:, shift:], res1.mean[:, shift:])
    assert float(start[1].min()) >= np.float32(0.2) and (shift == 0 or bool((start[1][:, H - shift:] == np.float32(0.4)).all()))
    im = alg.imagine(_states(alg).repeat_interleave(N, 0), horizon=H, actions=cand, lookahead=True, deterministic=True,
                     noise=drpo_amd.DeviceNoise(99), **RUN)
    torch.cuda.synchronize()
    assert_bits(res.scores.reshape(-1), im.value_lookahead[:, H].contiguous(), 'scores')
    assert_bits(res.certificates.reshape(-1), im.certificate_lookahead[:, H].max(dim=-1).values, 'certificates')


def test_tail_and_steps_reach_the_shift():
    alg, K = _alg('reach'), 2
    res1 = _plan(alg, iterations=1, steps=K)
    tail = torch.full((P, alg.action_dim), 0.25, device=DEV)
    res = _plan(alg, seed=23, iterations=1, steps=K, warm_start=res1, tail=tail)
    assert_bits(res.candidates[:, 0, 0], res1.actions[:, 1], 'the kept step')
    assert_bits(res.candidates[:, 0, 1], tail, 'the fresh step')
    # any object with mean, std and actions will do, CPU tensors too
    class Prev:
        mean, std, actions = res1.mean.cpu(), res1.std.cpu().numpy(), res1.actions.cpu()
    again = _plan(alg, seed=23, iterations=1, steps=K, warm_start=Prev, tail=tail.cpu())
    _same(res, again)


# ------------------------------------------------------------------ 3. the incumbent argument
@pytest.mark.parametrize('beta', [0.0, 0.5])
def test_replanning_at_the_same_states_is_no_worse(beta):
    alg, res1 = _alg('reach'), _first()
    res = _plan(alg, seed=29, iterations=2, warm_start=res1, shift=0, warm_std=0.0, noise_beta=beta,
                threshold=res1.threshold)
    f1, s1, c1 = res1.feasible.cpu(), res1.score.cpu(), res1.certificate.cpu()
    hf, hs, hc = res.history_feasible.cpu(), res.history_score.cpu(), res.history_certificate.cpu()
    for p in range(P):
        was = _key(f1[p], s1[p], c1[p])
        for i in range(2):
            assert _key(hf[i, p], hs[i, p], hc[i, p]) >= was, (p, i)
            was = _key(hf[i, p], hs[i, p], hc[i, p])
    print('keys before and after:', [_key(f1[p], s1[p], c1[p]) for p in range(P)],
          [_key(hf[1, p], hs[1, p], hc[1, p]) for p in range(P)])


# ------------------------------------------------------------------ 4. reset
def test_reset_states_start_cold():
    alg, res1 = _alg('reach'), _first()
    kw = dict(seed=31, iterations=1, threshold=res1.threshold, noise_beta=0.5)
    cold, warm = _plan(alg, **kw), _plan(alg, warm_start=res1, **kw)
    every = _plan(alg, warm_start=res1, reset=torch.ones(P, dtype=torch.bool, device=DEV), **kw)
    _same(every, cold)
    assert every.warm_started and not cold.warm_started
    mask = torch.tensor([True, False, False, True, False])
    some = _plan(alg, warm_start=res1, reset=mask, **kw)                    # (a CPU mask: plan moves it)
    for p in range(P):
        want = cold if mask[p] else warm
        for k in ('candidates', 'scores', 'certificates', 'ranks', 'actions', 'mean', 'std'):
            assert_bits(getattr(some, k)[p], getattr(want, k)[p], f'{k}[{p}]')
    assert not torch.equal(cold.candidates, warm.candidates)
    # with a tail the cold states start from it
    tail = torch.full((P, alg.action_dim), -0.5, device=DEV)
    tailed = _plan(alg, warm_start=res1, reset=mask.to(DEV), tail=tail, **kw)
    from_tail = _plan(alg, init=tail.unsqueeze(1).repeat(1, H, 1), **kw)
    for p in (0, 3):
        assert_bits(tailed.candidates[p], from_tail.candidates[p], f'candidates[{p}]')
        assert_bits(tailed.scores[p], from_tail.scores[p], f'scores[{p}]')


# ------------------------------------------------------------------ 5. streams
def test_the_same_seed_gives_the_same_bits():
    alg, res1 = _alg('reach'), _first()
    kw = dict(iterations=3, temperature=0.5, momentum=0.25, warm_start=res1, noise_beta=0.75, warm_std=0.1,
              reset=torch.tensor([False, True, False, False, False]))
    a, b, c = _plan(alg, seed=5, **kw), _plan(alg, seed=5, **kw), _plan(alg, seed=6, **kw)
    _same(a, b)
    assert not torch.equal(a.candidates, c.candidates)
    # one iteration, correlated against white: other candidates from the same draws
    ar, white = (_plan(alg, seed=5, **dict(kw, iterations=1, noise_beta=b)) for b in (0.75, 0.0))
    assert not torch.equal(ar.candidates, white.candidates)
    assert_bits(ar.candidates[:, :, 0], white.candidates[:, :, 0], 'step 0: u_0 = z_0')


def test_the_controller_leaves_the_training_state_alone(monkeypatch):
    from test_gpu_imagine_lookahead import _virtual
    alg = _drifting_quadrotor_alg(16)
    alg.imagine()                                            # (so that imagine's private stream exists)
    torch.cuda.synchronize()
    before = _virtual(alg)
    ctrs = (alg.noise.ctr, alg._imagine_noise.ctr)
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_sample_ar', 'drpo_plan_shift', 'drpo_plan_refit', 'drpo_rollout',
                 'drpo_rollout_trajectories', 'drpo_rollout_trajectories_given'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    ctl = alg.mpc(horizon=H, candidates=N, iterations=2, noise_beta=0.5, **RUN)
    s = _states(alg)
    for _ in range(3):
        a = ctl.act(s)
    torch.cuda.synchronize()
    assert a.shape == (P, alg.action_dim) and a.device.type == 'cuda' and ctl.steps == 3
    it = ['drpo_plan_sample_ar', 'drpo_rollout_trajectories_given', 'drpo_plan_refit'] * 2
    assert calls == it + (['drpo_plan_shift'] + it) * 2
    assert (alg.noise.ctr, alg._imagine_noise.ctr) == ctrs
    assert alg._plan_noise.ctr == 3 * 2 * 2                  # plan's private stream: a sample and an imagine per iteration
    after = _virtual(alg)
    assert before[1:] == after[1:]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    # a given noise object is the one the controller draws from
    mine = drpo_amd.DeviceNoise(3)
    alg.mpc(horizon=H, candidates=N, iterations=1, noise=mine, **RUN).act(s)
    assert mine.ctr == 2 and alg._plan_noise.ctr == 12


# ------------------------------------------------------------------ 6. the controller
def test_the_controllers_second_act_is_a_warm_plan():
    alg = _alg('reach')
    thr = _first().threshold
    kw = dict(horizon=H, candidates=N, iterations=2, threshold=thr, noise_beta=0.5, temperature=0.5, **RUN)
    ctl = alg.mpc(fallback=None, shift=1, warm_std=0.15, noise=drpo_amd.DeviceNoise(41), **kw)
    s1 = _states(alg)
    a1 = ctl.act(s1)
    first = ctl.last
    s2 = first.imagined.states[torch.arange(P, device=DEV) * N + first.ranks.argmin(dim=1), 1].contiguous()
    mask = torch.tensor([False, False, True, False, False], device=DEV)
    a2 = ctl.act(s2, reset=mask)
    torch.cuda.synchronize()
    assert ctl.steps == 2 and ctl.last is not first and ctl.last.warm_started and ctl.last.shift == 1
    noise = drpo_amd.DeviceNoise(41)
    by_hand1 = alg.plan(s1, noise=noise, **kw)
    by_hand2 = alg.plan(s2, warm_start=by_hand1, shift=1, warm_std=0.15, reset=mask, noise=noise, **kw)
    torch.cuda.synchronize()
    _same(first, by_hand1)
    _same(ctl.last, by_hand2)
    assert_bits(a1, by_hand1.action, 'the first action')
    assert_bits(a2, by_hand2.action, 'the second action')
    # another P, and reset(): cold again
    ctl.act(s2[:3])
    assert not ctl.last.warm_started and ctl.steps == 3
    ctl.act(s2[:3])
    assert ctl.last.warm_started
    ctl.reset()
    ctl.act(s2[:3])
    assert not ctl.last.warm_started and ctl.steps == 5


def test_what_the_controller_hands_out():
    alg = _alg('reach')
    s = _states(alg)
    safe = alg.solver.actor_safe.act(s, eval=True)
    kw = dict(horizon=H, candidates=N, iterations=1, **RUN)

    def ctl(**k):
        c = alg.mpc(noise=drpo_amd.DeviceNoise(7), **dict(kw, **k))
        a = c.act(s)
        torch.cuda.synchronize()
        return a, c.last
    a, res = ctl(threshold=-INF)                         # no row is feasible: the safe actor's action
    assert not bool(res.feasible.any())
    assert_bits(a, safe, "fallback='safe' at -inf")
    a, res = ctl(threshold=INF)
    assert bool(res.feasible.all())
    assert_bits(a, res.action, "fallback='safe' at +inf")
    assert not torch.equal(a, safe)
    a, res = ctl(threshold=-INF, fallback=None)
    assert_bits(a, res.action, 'fallback=None at -inf')
    a, res = ctl(threshold=INF, safety_filter=True)
    assert res.safe_action is not None
    assert_bits(a, res.safe_action, 'safety_filter=True')
    a, res = ctl(threshold=-INF, safety_filter=True)
    assert_bits(a, safe, "safety_filter=True, fallback='safe' at -inf")
    a, res = ctl(threshold=-INF, safety_filter=True, fallback=None)
    assert_bits(a, res.safe_action, 'safety_filter=True, fallback=None at -inf')
    # a threshold between the states' least certificates (the candidates of a seed do not depend on
    # it): the select is per state
    least = ctl(threshold=INF)[1].certificates.min(dim=1).values.sort().values
    assert float(least[P // 2]) < float(least[P // 2 + 1])
    a, res = ctl(threshold=float(least[P // 2]))
    f = res.feasible
    assert int(f.sum()) == P // 2 + 1
    assert_bits(a[f], res.action[f], 'the feasible states')
    assert_bits(a[~f], safe[~f], 'the others')


# ------------------------------------------------------------------ 7. on the environment
def test_evaluate_with_a_controller(monkeypatch):
    import drpo_amd.smbpo as smbpo
    from pr_env import PointRobot, TorchEnv
    alg = _width_alg('point-robot', 64, 64)
    alg._eval_env = ProductEnv([TorchEnv(PointRobot(id=i), DEV) for i in range(2)], max_episode_steps=6)
    monkeypatch.setattr(smbpo, 'N_EVAL_TRAJ', 3)
    ctrs = (alg.noise.ctr, int(alg.steps_sampled.item()), len(alg.replay_buffer))
    ctl = alg.mpc(candidates=8, iterations=1, horizon=3, members=0)
    masks = []
    real = ctl.act
    monkeypatch.setattr(ctl, 'act', lambda states, reset=None: (masks.append(reset.cpu().tolist()), real(states, reset))[1])
    ev = alg.evaluate(controller=ctl)
    assert set(ev) == {'eval return mean', 'eval return std', 'eval length mean', 'eval length std',
                       'eval violation mean'}
    assert all(np.isfinite(v) for v in ev.values()), ev
    # both envs run into the time limit at step 5 and are reset together; the third episode ends the run at step 11
    assert ctl.steps == 12 and ev['eval length mean'] == 6.0
    assert masks == [[True, True]] + [[False, False]] * 5 + [[True, True]] + [[False, False]] * 5
    assert ctl.last.warm_started and ctl.last.shift == 1
    assert (alg.noise.ctr, int(alg.steps_sampled.item()), len(alg.replay_buffer)) == ctrs
    # the default loop is the shielded policy's, as before
    plain = alg.evaluate()
    assert set(plain) == set(ev) and ctl.steps == 12
    rec = RecordingController(alg.action_dim)
    alg.evaluate(controller=rec)
    assert rec.masks == masks
