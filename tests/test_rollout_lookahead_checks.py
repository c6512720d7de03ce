"""The model-based lookahead without a GPU: the definition on an example worked by hand
(lookahead_helpers.lookahead_reference, which the GPU tests hold the kernel to bit for bit), the
struct and every refusal of drpo_rollout_lookahead (calls that fail before any launch; pointers
are dummies the host never dereferences), the Python refusals of imagine(lookahead=), and the
group 'lookahead' of ImaginedRollout."""
import ctypes
import math

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib, ops
from lookahead_helpers import (COST, NAN, QNAN_BITS, REACH, SCALES, assert_synthetic_shows_every_case, bits,
                               lookahead_reference, synthetic, weights)
from test_host_logic import make_smbpo
from test_rollout_host import _run
from test_rollout_traj_checks import EINVAL, OK, P, _err

WHO = 'drpo_rollout_lookahead:'
H = 3


# ------------------------------------------------------------------ 1. the definition, by hand
def _example():
    """3 rows, H 3, C 2, discount 0.5, reward_scale 1, alive_bonus 1, constraint_scale 10,
    constraint_offset 0.5. Every number is dyadic, so every step below is exact.

    Row 0 ends at step 1 (length 2, terminated); its terminal inputs are 100 and NaN and must
    not show. r' = [2, 3]; h' = [3.0, -5.0], [-2.5, 1.75] (0.25 -> 2.5 + 0.5; -0.5 -> -5).
    Row 1 lives to the horizon. r' = [1, 0, 1.5]; h' = [-1.25, 5.5], [0, -10], [5.5, 3.0].
    Row 2 has length 0 (halted at step 0): every entry is its terminal bootstrap."""
    x = dict(
        rewards=torch.tensor([[1.0, 2.0, 0.0], [0.0, -1.0, 0.5], [0.0, 0.0, 0.0]]),
        constraint_values=torch.tensor([[[0.25, -0.5], [-0.25, 0.125], [0.0, 0.0]],
                                        [[-0.125, 0.5], [0.0, -1.0], [0.5, 0.25]],
                                        [[0.0, 0.0]] * 3]),
        dones=torch.tensor([[False, True, False], [False] * 3, [False] * 3]),
        violations=torch.tensor([[False, True, False], [True, False, True], [False] * 3]),
        lengths=torch.tensor([2, 3, 0], dtype=torch.int32),
        terminated=torch.tensor([True, False, False]),
        step_q=torch.tensor([[4.0, 8.0, 0.0], [2.0, -4.0, 8.0], [0.0, 0.0, 0.0]]),
        step_qc=torch.tensor([[[1.0, -1.0], [2.0, -6.0], [0.0, 0.0]],
                              [[0.5, 0.25], [-1.0, 7.0], [6.0, 2.0]],
                              [[0.0, 0.0]] * 3]),
        terminal_q=torch.tensor([100.0, 16.0, 5.0]),
        terminal_qc=torch.tensor([[NAN, NAN], [-3.0, 4.0], [0.75, -0.5]]))
    scales = dict(reward_scale=1.0, alive_bonus=1.0, constraint_scale=10.0, constraint_offset=0.5)
    # row 0: 4 | 2 + 8/2 | 2 + 3/2, no bootstrap | the same
    # row 1: 2 | 1 - 4/2 | 1 + 0 + 8/4 | 1 + 0 + 1.5/4 + 16/8
    value = [[4.0, 6.0, 3.5, 3.5], [2.0, -1.0, 3.0, 3.375], [5.0] * 4]
    # reachability, x <- h'/2 + max(h', x)/2 from the bootstrap backwards (done: x <- h')
    # row 0, k 1: from [2, -6]: [3/2 + 3/2, -5/2 - 5/2]; k 2: step 1 is done: [-2.5, 1.75], then
    #   [3/2 + 3/2, -5/2 + 1.75/2]
    # row 1, k 1: from [-1, 7]: [-0.625 - 0.5, 2.75 + 3.5]; k 2: from [6, 2]: [0 + 3, -5 + 1], then
    #   [-0.625 + 1.5, 2.75 + 2.75]; k 3: from [-3, 4]: [5.5, 1.5 + 2], [0 + 2.75, -5 + 1.75],
    #   [-0.625 + 1.375, 2.75 + 2.75]
    reach = [[[1.0, -1.0], [3.0, -5.0], [3.0, -1.625], [3.0, -1.625]],
             [[0.5, 0.25], [-1.125, 6.25], [0.875, 5.5], [0.75, 5.5]],
             [[0.75, -0.5]] * 4]
    # cost, x <- v + x/2 (done: x <- v), v = the violation bit
    # row 0, k 1: 0 + [2, -6]/2; k 2: step 1 is done: 1, then 0 + 1/2
    # row 1, k 1: 1 + [-1, 7]/2; k 2: [6, 2]/2 = [3, 1], 1 + [1.5, 0.5]; k 3: 1 + [-3, 4]/2 =
    #   [-0.5, 3], [-0.25, 1.5], 1 + [-0.125, 0.75]
    cost = [[[1.0, -1.0], [1.0, -3.0], [0.5, 0.5], [0.5, 0.5]],
            [[0.5, 0.25], [0.5, 4.5], [2.5, 1.5], [0.875, 1.75]],
            [[0.75, -0.5]] * 4]
    return x, scales, np.array(value, np.float32), np.array(reach, np.float32), np.array(cost, np.float32)


@pytest.mark.parametrize('mode', [REACH, COST], ids=['reachability', 'cost'])
def test_reference_on_the_example_worked_by_hand(mode):
    x, scales, value, reach, cost = _example()
    v, c = lookahead_reference(**x, gamma=0.5, mode=mode, **scales)
    assert v.dtype == c.dtype == np.float32 and v.shape == (3, H + 1) and c.shape == (3, H + 1, 2)
    assert np.array_equal(bits(v), bits(value)), v
    want = reach if mode == REACH else cost
    assert np.array_equal(bits(c), bits(want)), c


def test_reference_edges():
    """Lengths are clamped; a NaN bootstrap of a live row shows as the canonical NaN and stays out of
    a terminated row; reward_scale 0 means unscaled; the weights are imagine's."""
    x, scales, value, reach, _ = _example()
    x['lengths'] = torch.tensor([2, 200, -3], dtype=torch.int32)
    v, c = lookahead_reference(**x, gamma=0.5, mode=REACH, **scales)
    assert np.array_equal(bits(v), bits(value)) and np.array_equal(bits(c), bits(reach))
    assert not np.isnan(v[0]).any() and not np.isnan(c[0]).any()
    x['terminal_qc'][1, 0] = NAN
    v2, c2 = lookahead_reference(**x, gamma=0.5, mode=REACH, **scales)
    assert (bits(c2[1, 3, 0:1]) == QNAN_BITS).all() and np.array_equal(bits(c2[1, :3]), bits(c[1, :3]))
    assert np.array_equal(bits(c2[1, :, 1]), bits(c[1, :, 1]))
    v3, _ = lookahead_reference(**x, gamma=0.5, mode=REACH, **dict(scales, reward_scale=0.0))
    assert np.array_equal(bits(v3), bits(v))
    w = weights(0.99, 10)
    assert w.dtype == np.float64 and len(w) == 11
    assert np.array_equal(w[:10], np.power(np.float64(0.99), np.arange(10, dtype=np.float64)))


@pytest.mark.parametrize('Hs, C', [(1, 1), (3, 2), (128, 2)])
def test_synthetic_rows_show_every_case(Hs, C):
    x, cases = synthetic(37, Hs, C)
    assert_synthetic_shows_every_case(x, cases, Hs, C)
    if Hs > 3:
        return
    for mode in (REACH, COST):
        v, c = lookahead_reference(**x, gamma=0.99, mode=mode, **SCALES)
        assert np.isnan(v[cases['nan_boot']]).any() and np.isnan(c[cases['nan_boot']]).any()
        assert np.isinf(v[cases['pinf_boot']]).any()
        assert not np.isnan(v[cases['nan_dead']]).any() and not np.isnan(c[cases['nan_dead']]).any()
        assert np.isnan(c[cases['nan_step'], 0]).all() and not np.isnan(v[cases['nan_step'], 0])
        n = np.clip(x['lengths'].numpy(), 0, Hs)
        for i in range(37):                                   # entries beyond a length repeat the one at it
            assert np.array_equal(bits(v[i, n[i]:]), np.repeat(bits(v[i, n[i]:n[i] + 1]), Hs + 1 - n[i]))


# ------------------------------------------------------------------ 2. the struct and the refusals
def _desc(**kw):
    d = _abi.RolloutLookahead()
    d.B, d.H, d.C, d.mode, d.gamma = 37, H, 2, 0, 0.99
    d.reward_scale, d.alive_bonus, d.constraint_scale, d.constraint_offset = 1.0, 1.0, 10.0, 0.0
    for f in INPUTS + ('violations', 'value', 'certificate'):
        setattr(d, f, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


INPUTS = ('rewards', 'constraint_values', 'dones', 'lengths', 'terminated', 'weights', 'step_q', 'step_qc',
          'terminal_q', 'terminal_qc')


def _call(d):
    return _lib.lib().drpo_rollout_lookahead(None if d is None else ctypes.byref(d), None)


def test_struct_layout_and_version():
    L = _lib.lib()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_abi_sizeof(b'drpo_rollout_lookahead_t') == ctypes.sizeof(_abi.RolloutLookahead) == \
        4 * 4 + 5 * 8 + 13 * ptr
    assert L.drpo_version() >= 12            # the version that added the entry point


def test_refuses_a_null_descriptor_or_input():
    assert _call(None) == EINVAL
    assert _err().startswith(WHO) and 'null descriptor' in _err()
    for f in INPUTS:
        assert _call(_desc(**{f: None})) == EINVAL, f
        assert _err().startswith(WHO) and 'null input pointer' in _err()
    assert _call(_desc(mode=1, violations=None)) == EINVAL
    assert _err().startswith(WHO) and 'null violations in cost mode' in _err()


@pytest.mark.parametrize('field, value, fragment', [
    ('H', 0, 'H=0 outside 1..128'), ('H', 129, 'H=129 outside 1..128'), ('H', -1, 'outside 1..128'),
    ('C', 0, 'C=0, need C >= 1'), ('C', -2, 'need C >= 1'), ('mode', 2, 'mode 2'), ('mode', -1, 'mode -1'),
    ('gamma', math.nan, 'gamma'), ('gamma', math.inf, 'gamma'), ('gamma', -0.01, 'gamma'), ('gamma', 1.01, 'gamma'),
    ('B', -1, 'B=-1 is negative'),
])
def test_refuses_before_any_launch(field, value, fragment):
    assert _call(_desc(**{field: value})) == EINVAL
    assert _err().startswith(WHO) and fragment in _err(), _err()


def test_an_empty_batch_is_ok_without_a_launch():
    L = _lib.lib()
    assert L.drpo_abi_const(b'DRPO_ROLLOUT_FUSED_MAX_H') == 128
    for kw in ({}, {'H': 128}, {'gamma': 0.0}, {'gamma': 1.0}, {'mode': 1}, {'violations': None},
               {'value': None}, {'certificate': None}):
        assert _call(_desc(B=0, **kw)) == OK, kw


# ------------------------------------------------------------------ 3. the Python refusals
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


def test_imagine_refuses_before_any_device(alg, monkeypatch):
    seen = []
    monkeypatch.setattr(ops, 'rollout_trajectories', lambda *a, **kw: seen.append(kw))
    monkeypatch.setattr(ops, 'lookahead', lambda *a, **kw: seen.append(a[3:]))
    s = torch.zeros(4, alg.state_dim)
    for bad in ('x', 'mean', 'Bound', 1, 0.5, ('bound',)):
        with pytest.raises(ValueError, match='lookahead: '):
            alg.imagine(s, lookahead=bad)
    assert seen == []
    for off in (None, False):
        alg.imagine(s, lookahead=off)
    assert len(seen) == 2 and all(isinstance(kw, dict) for kw in seen)     # the rollout alone
    seen.clear()
    assert alg.solver.distributional_qc
    alg.imagine(s, lookahead=True, discount=0.5)
    alg.imagine(s, lookahead='bound')
    assert seen[1] == ('mean', 0.5) and seen[3] == ('bound', float(alg.solver.discount))
    monkeypatch.setattr(alg.solver, 'distributional_qc', False)
    with pytest.raises(ValueError, match='needs a distributional constraint critic'):
        alg.imagine(s, lookahead='bound')
    assert ops._lookahead_request(alg, True) == 'mean'


# ------------------------------------------------------------------ 4. the group of ImaginedRollout
IR = ops.ImaginedRollout
TENSORS6 = ('step_q', 'step_qc', 'terminal_q', 'terminal_qc', 'value_lookahead', 'certificate_lookahead')


def _with_lookahead(seed):
    im = _run(seed, ('shield',))
    g = torch.Generator().manual_seed(100 + seed)
    shapes = {'step_q': (2, H), 'step_qc': (2, H, 2), 'terminal_q': (2,), 'terminal_qc': (2, 2),
              'value_lookahead': (2, H + 1), 'certificate_lookahead': (2, H + 1, 2)}
    im.set_group('lookahead', lookahead_kind='bound', **{k: torch.rand(shapes[k], generator=g) for k in TENSORS6})
    return im


def test_the_group_is_beside_groups_not_in_it():
    assert set(IR.GROUPS) == {'shield', 'linear', 'uncertainty'}
    assert IR.LOOKAHEAD_GROUP == {'lookahead': (TENSORS6, ('lookahead_kind',))}
    assert set(IR._ALL_GROUPS) == set(IR.GROUPS) | {'halt', 'lookahead'}
    plain = _run(1, ())
    assert all(getattr(plain, k) is None for k in TENSORS6 + ('lookahead_kind',))
    with pytest.raises(AssertionError):
        plain.set_group('lookahead', step_q=torch.zeros(2, H))


def test_stack_with_and_without_the_group():
    runs = [_with_lookahead(seed) for seed in (1, 2, 3)]
    out = IR.stack(runs)
    for k in TENSORS6:
        want = torch.stack([getattr(r, k) for r in runs])
        assert getattr(out, k).shape == (3,) + tuple(getattr(runs[0], k).shape) and torch.equal(getattr(out, k), want), k
    assert out.lookahead_kind == 'bound' and out.shield_threshold == 0.5
    assert torch.equal(out.certificate, torch.stack([r.certificate for r in runs]))
    out = IR.stack([_run(seed, ('shield',)) for seed in (1, 2, 3)])
    assert all(getattr(out, k) is None for k in TENSORS6 + ('lookahead_kind',)) and out.certificate is not None
