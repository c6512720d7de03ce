"""Receding-horizon control on the planner without a GPU: the definitions of drpo_plan_sample_ar
and drpo_plan_shift on examples worked by hand (plan_mpc_helpers' references, which the GPU tests
hold the kernels to), the two structs and every refusal of the two entry points (calls that fail
before any launch; pointers are dummies the host never dereferences), every Python refusal of the
new arguments of SMBPO.plan and of SMBPO.mpc, and the reset masks that
sample_episodes_batched(controller=) hands to a controller."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib, ops, sampling
from drpo_amd.envs import ProductEnv
from plan_mpc_helpers import (RecordingController, ScriptedEnv, assert_bits, fma_f32, plan_sample_ar_reference,
                              plan_shift_reference, round_f32)
from test_host_logic import make_smbpo
from test_rollout_traj_checks import EINVAL, OK, P, _err

NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------ 1. the definitions, by hand
def test_ar_definition_by_hand():
    """corr = innov = 0.5, K 3, z = [1, -2, 4] (every number dyadic, every step exact):
    u = [1, 0.5 - 1 = -0.5, -0.25 + 2 = 1.75]; x = 0.25 + 0.5 u = [0.75, 0, 1.125], clamped at 1.
    Candidate 0 is the incumbent; the second dimension runs z = [-4, 0, 0]: u = [-4, -2, -1],
    x = [-1.75, -0.75, -0.25], clamped at -1."""
    z = torch.tensor([[[[9.0, 9.0], [9.0, 9.0], [9.0, 9.0]], [[1.0, -4.0], [-2.0, 0.0], [4.0, 0.0]]]])   # [1, 2, 3, 2]
    mean, std = torch.full((1, 3, 2), 0.25), torch.full((1, 3, 2), 0.5)
    inc = torch.tensor([[[0.125, -0.0], [NAN, 2.0], [-3.0, 0.5]]])
    x, u = plan_sample_ar_reference(z, mean, std, inc, corr=0.5, innov=0.5)
    assert x.shape == u.shape == (2, 3, 2) and x.dtype == np.float32
    assert_bits(x[0], inc[0], 'candidate 0')                  # unclamped, NaN and -0.0 as they are
    assert u[1].tolist() == [[1.0, -4.0], [-0.5, -2.0], [1.75, -1.0]]
    assert x[1].tolist() == [[0.75, -1.0], [0.0, -0.75], [1.0, -0.25]]
    # corr 0, innov 1: white noise, u = z
    w, uw = plan_sample_ar_reference(z, mean, std, inc, corr=0.0, innov=1.0, lo=-INF, hi=INF)
    assert uw[1].tolist() == z[0, 1].tolist() and w[1].tolist() == [[0.75, -1.75], [-0.75, 0.25], [2.25, 0.25]]
    # a NaN mean stays through the clamp
    bad = mean.clone()
    bad[0, 1, 0] = NAN
    y, _ = plan_sample_ar_reference(z, bad, std, inc, corr=0.5, innov=0.5)
    assert math.isnan(y[1, 1, 0]) and y[1, 0, 0] == 0.75


def test_the_exact_fma_rounds_once():
    """4097 * 16773121 = 2^36 + 1, so a * b = 2^-24 + 2^-60 exactly and a * b + 1 lies just above
    the middle of 1 and the next float32: one rounding goes up. Float64 drops the 2^-60, lands on
    the middle, and the second rounding takes the tie to the even 1.0."""
    a, b = np.float32(4097 * 2.0 ** -30), np.float32(16773121 * 2.0 ** -30)
    assert float(a) * float(b) == 2.0 ** -24 + 2.0 ** -60
    assert fma_f32(a, b, 1.0) == np.nextafter(np.float32(1), np.float32(2))
    assert np.float32(np.float64(a) * np.float64(b) + 1.0) == np.float32(1)
    assert round_f32(Fraction(3, 2)) == 1.5 and round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == 1.0   # a tie: even
    assert round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == np.float32(1 + 2.0 ** -22)                 # a tie: even
    assert math.isnan(fma_f32(NAN, 1, 1)) and fma_f32(INF, 1, 1) == INF
    assert math.copysign(1, fma_f32(-0.0, 1.0, -0.0)) == -1 and math.copysign(1, fma_f32(-0.0, 1.0, 0.0)) == 1


@pytest.mark.parametrize('with_tail', [False, True])
def test_shift_definition_by_hand(with_tail):
    """P 2, K 3, A 1, shift 1, floor 0.125, fresh 0.75; state 1 is reset."""
    mean = torch.tensor([[[1.0], [2.0], [3.0]], [[4.0], [5.0], [6.0]]])
    std = torch.tensor([[[0.5], [0.0625], [0.25]], [[0.5], [0.5], [0.5]]])
    inc = torch.tensor([[[-1.0], [-2.0], [-3.0]], [[-4.0], [-5.0], [-6.0]]])
    tail = torch.tensor([[9.0], [8.0]]) if with_tail else None
    m, s, i = plan_shift_reference(mean, std, inc, shift=1, fresh_std=0.75, std_floor=0.125,
                                   reset=torch.tensor([False, True]), tail=tail)
    last, cold = (9.0, 8.0) if with_tail else (None, 0.0)
    assert m[:, :, 0].tolist() == [[2.0, 3.0, last or 3.0], [cold] * 3]
    assert i[:, :, 0].tolist() == [[-2.0, -3.0, last or -3.0], [cold] * 3]
    assert s[:, :, 0].tolist() == [[0.125, 0.25, 0.75], [0.75] * 3]        # 0.0625 raised to the floor
    # without the mask state 1 shifts as well; shift K keeps nothing, shift 0 everything
    m2, s2, _ = plan_shift_reference(mean, std, inc, shift=1, fresh_std=0.75, std_floor=0.0, tail=tail)
    assert m2[1, :, 0].tolist() == [5.0, 6.0, 8.0 if with_tail else 6.0] and s2[0, :, 0].tolist() == [0.0625, 0.25, 0.75]
    m3, s3, i3 = plan_shift_reference(mean, std, inc, shift=3, fresh_std=0.75, std_floor=0.0, tail=tail)
    assert m3[0, :, 0].tolist() == [last or 3.0] * 3 and i3[1, :, 0].tolist() == [8.0 if with_tail else -6.0] * 3
    assert (s3 == 0.75).all()
    m0, s0, i0 = plan_shift_reference(mean, std, inc, shift=0, fresh_std=0.75, std_floor=0.0, tail=tail)
    for got, want, k in ((m0, mean, 'mean'), (s0, std, 'std'), (i0, inc, 'incumbent')):
        assert_bits(got, want, k)


# ------------------------------------------------------------------ 2. structs, version, refusals
def test_struct_layouts_and_version():
    L = _lib.lib()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_abi_sizeof(b'drpo_plan_sample_ar_t') == ctypes.sizeof(_abi.PlanSampleAr) \
        == ctypes.sizeof(_abi.PlanSample) + 2 * 8
    assert L.drpo_abi_sizeof(b'drpo_plan_shift_t') == ctypes.sizeof(_abi.PlanShift) == 4 * 4 + 2 * 4 + 8 * ptr
    assert [f[0] for f in _abi.PlanSampleAr._fields_][:-2] == [f[0] for f in _abi.PlanSample._fields_]
    assert L.drpo_version() >= 15            # the version that added the entry points


AR_POINTERS = ('mean', 'std', 'incumbent', 'cand')


def _ar(**kw):
    d = _abi.PlanSampleAr()
    d.P, d.N, d.K, d.A, d.lo, d.hi, d.seed, d.ctr, d.corr, d.innov = 5, 37, 3, 2, -1.0, 1.0, 1, 2, 0.5, 0.5
    for f in AR_POINTERS:
        setattr(d, f, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call_ar(d):
    return _lib.lib().drpo_plan_sample_ar(None if d is None else ctypes.byref(d), None)


def test_ar_refuses_null_pointers():
    who = 'drpo_plan_sample_ar:'
    assert _call_ar(None) == EINVAL
    assert _err().startswith(who) and 'null descriptor' in _err()
    for f in AR_POINTERS:
        assert _call_ar(_ar(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null pointer' in _err()


@pytest.mark.parametrize('kw, fragment', [
    # what drpo_plan_sample refuses, in its words
    ({'N': 1}, 'N=1 outside 2..1024'), ({'N': 0}, 'outside 2..1024'), ({'N': 1025}, 'N=1025 outside 2..1024'),
    ({'N': -4}, 'outside 2..1024'), ({'K': 0}, 'K=0, need K >= 1'), ({'K': -1}, 'need K >= 1'),
    ({'A': 0}, 'A=0, need A >= 1'), ({'P': -1}, 'P=-1 is negative'), ({'lo': 0.5, 'hi': 0.25}, 'clamp'),
    ({'lo': math.nan}, 'clamp'), ({'hi': math.nan}, 'clamp'),
    ({'P': 2 ** 31 - 1, 'N': 1024, 'K': 128, 'A': 64}, 'exceed one grid'),
    # and its own
    ({'corr': 1.0}, 'corr 1 outside [0, 1)'), ({'corr': -0.25}, 'corr'), ({'corr': math.nan}, 'corr'),
    ({'corr': math.inf}, 'corr'),
    ({'innov': 0.0}, 'innov 0 outside (0, 1]'), ({'innov': -0.5}, 'innov'), ({'innov': 1.5}, 'innov'),
    ({'innov': math.nan}, 'innov'),
    ({'P': 0, 'corr': 1.0}, 'corr'), ({'P': 0, 'innov': 0.0}, 'innov'),        # before the P == 0 return
])
def test_ar_refuses_before_any_launch(kw, fragment):
    assert _call_ar(_ar(**kw)) == EINVAL
    assert _err().startswith('drpo_plan_sample_ar:') and fragment in _err(), _err()


def test_ar_of_no_state_is_ok_without_a_launch():
    for kw in ({}, {'N': 2}, {'N': 1024}, {'corr': 0.0, 'innov': 1.0}, {'corr': 0.999}, {'innov': 1e-3},
               {'lo': -math.inf, 'hi': math.inf}):
        assert _call_ar(_ar(P=0, **kw)) == OK, kw


SHIFT_INPUTS, SHIFT_OUTPUTS = ('mean', 'std', 'incumbent'), ('mean_out', 'std_out', 'incumbent_out')
SHIFT_OPTIONAL = ('reset', 'tail')


def _shift(**kw):
    d = _abi.PlanShift()
    d.P, d.K, d.A, d.shift, d.fresh_std, d.std_floor = 5, 3, 2, 1, 0.5, 0.05
    for j, f in enumerate(SHIFT_INPUTS + SHIFT_OPTIONAL + SHIFT_OUTPUTS):
        setattr(d, f, P + 0x100 * j)             # distinct dummies: an output equal to an input is refused
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call_shift(d):
    return _lib.lib().drpo_plan_shift(None if d is None else ctypes.byref(d), None)


def test_shift_refuses_null_pointers_and_aliases():
    who = 'drpo_plan_shift:'
    assert _call_shift(None) == EINVAL
    assert _err().startswith(who) and 'null descriptor' in _err()
    for f in SHIFT_INPUTS + SHIFT_OUTPUTS:
        assert _call_shift(_shift(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null pointer' in _err()
    for o in SHIFT_OUTPUTS:
        for i in SHIFT_INPUTS + SHIFT_OPTIONAL:
            d = _shift(P=0)
            setattr(d, o, getattr(d, i))
            assert _call_shift(d) == EINVAL, (o, i)
            assert _err().startswith(who) and 'aliases an input' in _err()


@pytest.mark.parametrize('kw, fragment', [
    ({'P': -1}, 'P=-1 is negative'), ({'K': 0}, 'K=0, need K >= 1'), ({'A': 0}, 'A=0, need A >= 1'),
    ({'A': -3}, 'need A >= 1'),
    ({'shift': -1}, 'shift=-1 outside 0..K=3'), ({'shift': 4}, 'shift=4 outside 0..K=3'),
    ({'fresh_std': 0.0}, 'fresh_std'), ({'fresh_std': -0.5}, 'fresh_std'), ({'fresh_std': math.inf}, 'fresh_std'),
    ({'fresh_std': math.nan}, 'fresh_std'),
    ({'std_floor': -0.01}, 'std_floor'), ({'std_floor': math.nan}, 'std_floor'),
    ({'P': 2 ** 31 - 1, 'K': 2 ** 20, 'A': 64}, 'exceed one grid'),
    ({'P': 0, 'shift': 4}, 'shift'), ({'P': 0, 'fresh_std': 0.0}, 'fresh_std'),      # before the P == 0 return
])
def test_shift_refuses_before_any_launch(kw, fragment):
    assert _call_shift(_shift(**kw)) == EINVAL
    assert _err().startswith('drpo_plan_shift:') and fragment in _err(), _err()


def test_shift_of_no_state_is_ok_without_a_launch():
    for kw in ({}, {'shift': 0}, {'shift': 3}, {'reset': None}, {'tail': None}, {'reset': None, 'tail': None},
               {'std_floor': 0.0}, {'std_floor': math.inf}, {'K': 1, 'shift': 1}):
        assert _call_shift(_shift(P=0, **kw)) == OK, kw


# ------------------------------------------------------------------ 3. the Python refusals
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


@pytest.fixture
def seen(monkeypatch):
    calls = []
    for name in ('plan_sample', 'plan_shift', 'plan_refit', '_terminal_critics', 'rollout_trajectories', 'lookahead'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    return calls


class _Warm:
    """any object with mean, std and actions"""

    def __init__(self, shape=(4, 3, 2), **kw):
        self.mean, self.std, self.actions = (torch.zeros(shape) for _ in range(3))
        for k, v in kw.items():
            if v is None:
                delattr(self, k)
            else:
                setattr(self, k, v)


W = _Warm()


@pytest.mark.parametrize('kw, match', [
    ({'noise_beta': 1.0}, 'noise_beta'), ({'noise_beta': -0.1}, 'noise_beta'), ({'noise_beta': math.nan}, 'noise_beta'),
    ({'noise_beta': '0.5'}, 'noise_beta'), ({'noise_beta': None}, 'noise_beta'), ({'noise_beta': True}, 'noise_beta'),
    ({'warm_start': W, 'init': 'policy'}, 'warm_start together with init'),
    ({'warm_start': W, 'init': torch.zeros(4, 3, 2)}, 'warm_start together with init'),
    ({'warm_start': _Warm((4, 2, 2))}, 'warm_start'), ({'warm_start': _Warm((3, 3, 2))}, 'warm_start'),
    ({'warm_start': _Warm(std=torch.zeros(4, 3))}, 'warm_start: its std'),
    ({'warm_start': _Warm(actions=None)}, 'warm_start: its actions is missing'),
    ({'warm_start': _Warm(mean=[[0.0]])}, 'warm_start: its mean'),
    ({'warm_start': 3}, 'warm_start'), ({'warm_start': torch.zeros(4, 3, 2)}, 'warm_start'),
    ({'warm_start': W, 'steps': 2}, 'warm_start'),                           # another K
    ({'warm_start': W, 'shift': 4}, 'shift'), ({'warm_start': W, 'shift': -1}, 'shift'),
    ({'warm_start': W, 'shift': 1.0}, 'shift'), ({'warm_start': W, 'shift': True}, 'shift'),
    ({'shift': 4}, 'shift'), ({'shift': None}, 'shift'), ({'warm_start': W, 'steps': 1, 'shift': 2}, 'shift'),
    ({'reset': torch.zeros(4, dtype=torch.bool)}, 'reset without warm_start'),
    ({'tail': torch.zeros(4, 2)}, 'tail without warm_start'), ({'warm_std': 0.1}, 'warm_std without warm_start'),
    ({'warm_start': W, 'reset': torch.zeros(3, dtype=torch.bool)}, 'reset'),
    ({'warm_start': W, 'reset': torch.zeros(4, 1, dtype=torch.bool)}, 'reset'),
    ({'warm_start': W, 'reset': torch.zeros(4)}, 'reset'), ({'warm_start': W, 'reset': [True] * 4}, 'reset'),
    ({'warm_start': W, 'tail': torch.zeros(4, 3)}, 'tail'), ({'warm_start': W, 'tail': torch.zeros(3, 2)}, 'tail'),
    ({'warm_start': W, 'tail': torch.zeros(4)}, 'tail'), ({'warm_start': W, 'tail': 0.0}, 'tail'),
    ({'warm_start': W, 'warm_std': -0.1}, 'warm_std'), ({'warm_start': W, 'warm_std': math.nan}, 'warm_std'),
    ({'warm_start': W, 'warm_std': 'wide'}, 'warm_std'),
])
def test_plan_refuses_before_any_device_work(alg, seen, kw, match):
    s = torch.zeros(4, alg.state_dim)
    assert alg.action_dim == 2
    with pytest.raises(ValueError, match=match):
        alg.plan(s, **dict({'horizon': 3, 'candidates': 8}, **kw))
    assert seen == [] and alg.__dict__.get('_plan_noise') is None


def test_plan_still_has_no_halt_and_no_shield(alg, seen):
    for kw in ({'halt': 0.5}, {'shield': True}):
        with pytest.raises(TypeError):
            alg.plan(torch.zeros(4, alg.state_dim), warm_start=W, **kw)
        with pytest.raises(TypeError):
            alg.mpc(**kw)
    assert seen == []


@pytest.mark.parametrize('kw, match', [
    ({'states': torch.zeros(4, 11)}, 'states'), ({'init': 'policy'}, 'init'), ({'warm_start': W}, 'warm_start'),
    ({'reset': torch.zeros(4, dtype=torch.bool)}, 'reset'),
    ({'fallback': 'policy'}, 'fallback'), ({'fallback': True}, 'fallback'),
    ({'shift': 4}, 'shift'), ({'shift': 1.5}, 'shift'), ({'shift': 2, 'steps': 1}, 'shift'),
    ({'warm_std': -1.0}, 'warm_std'), ({'warm_std': math.nan}, 'warm_std'),
    ({'noise_beta': 1.0}, 'noise_beta'), ({'candidates': 1}, 'candidates'), ({'iterations': 0}, 'iterations'),
    ({'members': 'each'}, 'members'), ({'horizon': 129}, 'horizon'), ({'lookahead': False}, 'lookahead'),
    ({'threshold': math.nan}, 'threshold'), ({'safety_filter': 'soft'}, 'safety_filter'),
    ({'tail': torch.zeros(4, 3)}, 'tail'), ({'tail': torch.zeros(2)}, 'tail'),
])
def test_mpc_refuses_at_construction(alg, seen, kw, match):
    with pytest.raises(ValueError, match=match):
        alg.mpc(**dict({'horizon': 3, 'candidates': 8}, **kw))
    assert seen == [] and alg.__dict__.get('_plan_noise') is None


def test_mpc_builds_a_controller_without_device_work(alg, seen, monkeypatch):
    c = alg.mpc(horizon=3, candidates=8, iterations=1, noise_beta=0.5, warm_std=0.2, shift=2, fallback=None,
                tail=torch.zeros(4, 2))
    assert isinstance(c, ops.PlanController) and c.last is None and c.steps == 0
    assert (c.fallback, c.shift, c.warm_std) == (None, 2, 0.2)
    assert alg.mpc().fallback == 'safe' and alg.mpc().shift == 1 and alg.mpc().warm_std is None
    assert seen == [] and alg.__dict__.get('_plan_noise') is None
    monkeypatch.setattr(alg, 'env_params', None)
    with pytest.raises(NotImplementedError, match='constraint functions on the device'):
        alg.mpc()


def test_the_controller_starts_cold_then_warm(alg, monkeypatch):
    """act() without a device: plan is recorded. Cold on the first call, after reset() and when P
    changes; else warm from the last result with the mask handed through."""
    calls = []

    def plan(states, **kw):
        calls.append(kw)
        n = len(states)
        return ops.PlanResult(**dict({k: None for k in ops.PlanResult.FIELDS}, actions=torch.zeros(n, 3, 2),
                                     action=torch.full((n, 2), float(len(calls))),
                                     feasible=torch.ones(n, dtype=torch.bool)))
    monkeypatch.setattr(alg, 'plan', plan)
    c = ops.PlanController(alg, None, 2, 0.25, dict(horizon=3, candidates=8))
    s4, s5, mask = torch.zeros(4, alg.state_dim), torch.zeros(5, alg.state_dim), torch.tensor([True, False, False, True])
    a = c.act(s4, reset=mask)
    assert a.shape == (4, 2) and calls[-1] == dict(horizon=3, candidates=8) and c.steps == 1
    first = c.last
    assert c.act(s4, reset=mask).tolist() == [[2.0, 2.0]] * 4
    assert calls[-1] == dict(horizon=3, candidates=8, warm_start=first, shift=2, warm_std=0.25, reset=mask)
    c.act(s5)
    assert calls[-1] == dict(horizon=3, candidates=8)                  # P changed
    c.act(s5)
    assert calls[-1]['warm_start'] is not None and calls[-1]['reset'] is None
    c.reset()
    assert c.last is None
    c.act(s5)
    assert calls[-1] == dict(horizon=3, candidates=8) and c.steps == 5
    # a tail starts the cold plan too: what a reset state gets
    c = ops.PlanController(alg, None, 1, None, dict(horizon=3, steps=2, tail=torch.full((4, 2), 0.5)))
    c.act(s4)
    assert set(calls[-1]) == {'horizon', 'steps', 'init'} and calls[-1]['init'].tolist() == [[[0.5] * 2] * 2] * 4
    c.act(s4)
    assert 'init' not in calls[-1] and calls[-1]['tail'].shape == (4, 2)


# ------------------------------------------------------------------ 4. the evaluation loop
def _episodes(monkeypatch, controller):
    """3 envs, T = 4: env 0 ends at its step 2, env 2 at its step 3, env 1 runs to the time limit."""
    env = ProductEnv([ScriptedEnv([2, None]), ScriptedEnv([None, None]), ScriptedEnv([3, None])], max_episode_steps=4)
    graph = []

    def shielded(policy, states, *a, **kw):
        graph.append(('shielded_actions', a, tuple(kw)))
        return torch.zeros(len(states), 2)
    monkeypatch.setattr(sampling, 'shielded_actions', shielded)
    kw = {} if controller is None else {'controller': controller}
    trajs = sampling.sample_episodes_batched(env, 'policy', 5, eval=True, safe_shield_threshold=-0.2,
                                             shield_type='safe', **kw)
    return trajs, graph


def test_the_reset_masks_of_the_evaluation_loop(monkeypatch):
    ctl = RecordingController(2)
    trajs, graph = _episodes(monkeypatch, ctl)
    assert graph == []                                   # the shielded policy does not run
    # env 0 ends at step 1, env 2 at step 2, env 1 runs out of time at step 3
    assert ctl.masks[0] == [True, True, True]
    assert ctl.masks[1] == [False, False, False]
    assert ctl.masks[2] == [True, False, False]
    assert ctl.masks[3] == [False, False, True]
    assert ctl.masks[4] == [False, True, False]
    # afterwards true exactly for the envs reset at the previous step: their state is a reset's zeros
    for m, s in zip(ctl.masks[1:], ctl.states[1:]):
        assert m == [bool((row == 0).all()) for row in s]
    assert [len(t) for t in trajs] == [2, 3, 4, 4, 4] and len(ctl.masks) == 7


def test_without_a_controller_the_loop_is_as_before(monkeypatch):
    trajs, graph = _episodes(monkeypatch, None)
    assert [len(t) for t in trajs] == [2, 3, 4, 4, 4]
    assert graph == [('shielded_actions', (True, -0.2, 'safe'), ())] * 7
    with_ctl, _ = _episodes(monkeypatch, RecordingController(2))
    for a, b in zip(trajs, with_ctl):
        for k in ('states', 'next_states', 'rewards', 'dones'):
            assert torch.equal(a.get(k), b.get(k)), k


def test_evaluate_hands_the_controller_through(alg, monkeypatch):
    seen_kw = []

    def fake(env, policy, n, **kw):
        seen_kw.append(kw)
        raise StopIteration
    monkeypatch.setattr(sampling, 'sample_episodes_batched', fake)
    ctl = object()
    for kw in ({}, {'controller': ctl}):
        with pytest.raises(StopIteration):
            alg.evaluate(**kw)
    assert 'controller' not in seen_kw[0] and seen_kw[1]['controller'] is ctl
    assert set(seen_kw[1]) - {'controller'} == set(seen_kw[0])


# ------------------------------------------------------------------ 5. the result
def test_plan_result_keeps_its_fields_and_names_the_new_ones():
    fields = ('actions', 'action', 'score', 'certificate', 'feasible', 'n_feasible', 'mean', 'std', 'history_score',
              'history_certificate', 'history_feasible', 'candidates', 'scores', 'certificates', 'ranks', 'imagined',
              'threshold', 'lookahead_kind')
    assert ops.PlanResult.FIELDS == fields
    assert ops.PlanResult.MPC_FIELDS == ('noise_beta', 'warm_started', 'shift')
    base = {k: i for i, k in enumerate(fields)}
    r = ops.PlanResult(**base)
    assert r.noise_beta is None and r.warm_started is None and r.shift is None
    r = ops.PlanResult(**base, noise_beta=0.5, warm_started=True, shift=2, safe_action=7)
    assert (r.noise_beta, r.warm_started, r.shift, r.safe_action, r.actions) == (0.5, True, 2, 7, 0)
