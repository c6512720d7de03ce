"""halt_helpers.cut_reference on a hand-written 4 x 3 example, no GPU: the reference the GPU
tests of halted rollouts compare with, checked against values worked out by hand.

B 4, H 3, S = A = C = 1, threshold 0.5, weights (1, 0.5, 0.25):
  row 0  natural length 3, scores .1 .2 .7      halted at 2
  row 1  natural length 3, scores .1 nan .1     a NaN halts: at 1; its violation at step 2 is cut off
  row 2  natural length 2 (done at 1), scores .5 .4 9   equal to the threshold does not halt, and
                                                the 9 lies beyond the row's length: unchanged
  row 3  natural length 1 (done and violation at 0), scores inf . .   halted at 0: length 0"""
import math

import torch

from drpo_amd import ops
from halt_helpers import assert_cut, cut_reference

NAN, INF = float('nan'), float('inf')


def _example():
    length = torch.tensor([3, 3, 2, 1], dtype=torch.int32)
    B, H = 4, 3
    steps = torch.arange(H)
    mask = steps[None] < length[:, None]
    smask = torch.arange(H + 1)[None] <= length[:, None]
    i = torch.arange(B, dtype=torch.float32)[:, None]
    states = torch.where(smask, 10 * i + torch.arange(H + 1), torch.zeros(())).reshape(B, H + 1, 1)
    t = steps.float()[None]
    actions = torch.where(mask, 0.5 * i - 0.125 * t, torch.zeros(())).reshape(B, H, 1)
    rewards = torch.where(mask, (i + 1) + 0.25 * t, torch.zeros(()))
    cv = torch.where(mask, t - i, torch.zeros(())).reshape(B, H, 1)
    dones = torch.tensor([[0, 0, 0], [0, 0, 0], [0, 1, 0], [1, 0, 0]], dtype=torch.bool)
    viol = torch.tensor([[0, 0, 0], [0, 0, 1], [0, 0, 0], [1, 0, 0]], dtype=torch.bool)
    w = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)
    im = ops.ImaginedRollout(
        [0] * H, states=states, actions=actions, rewards=rewards, constraint_values=cv, dones=dones, violations=viol,
        lengths=length, returns=(rewards.double() * w).sum(-1).float(),
        max_constraint=torch.tensor([[2.0], [1.0], [-1.0], [-3.0]]),
        first_violation=torch.tensor([-1, 2, -1, 0], dtype=torch.int32),
        terminated=torch.tensor([False, False, True, True]))
    dis = torch.where(mask, 0.1 * (t + 1).expand(B, H), torch.zeros(()))
    im.set_group('uncertainty', disagreement=dis, epistemic=2 * dis, aleatoric=3 * dis,
                 max_disagreement=dis.max(-1).values)
    scores = torch.tensor([[.1, .2, .7], [.1, NAN, .1], [.5, .4, 9.], [INF, .0, .0]])
    return im, scores, w


def test_cut_reference_on_the_hand_written_example():
    im, scores, w = _example()
    ref = cut_reference(im, scores, 0.5, w)
    f = torch.float32
    want = {
        'halted_at': torch.tensor([2, 1, -1, 0], dtype=torch.int32),
        'lengths': torch.tensor([2, 1, 2, 0], dtype=torch.int32),
        'states': torch.tensor([[0, 1, 2, 0], [10, 11, 0, 0], [20, 21, 22, 0], [30, 0, 0, 0]], dtype=f).unsqueeze(-1),
        'actions': torch.tensor([[0, -.125, 0], [.5, 0, 0], [1., .875, 0], [0, 0, 0]], dtype=f).unsqueeze(-1),
        'rewards': torch.tensor([[1, 1.25, 0], [2, 0, 0], [3, 3.25, 0], [0, 0, 0]], dtype=f),
        'constraint_values': torch.tensor([[0, 1, 0], [-1, 0, 0], [-2, -1, 0], [0, 0, 0]], dtype=f).unsqueeze(-1),
        'dones': torch.tensor([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=torch.bool),
        'violations': torch.zeros(4, 3, dtype=torch.bool),
        'returns': torch.tensor([1.625, 2.0, 4.625, 0.0], dtype=f),
        'max_constraint': torch.tensor([[1.0], [-1.0], [-1.0], [-INF]], dtype=f),
        'first_violation': torch.tensor([-1, -1, -1, -1], dtype=torch.int32),
        'terminated': torch.tensor([False, False, True, False]),
        'disagreement': torch.tensor([[.1, .2, 0], [.1, 0, 0], [.1, .2, 0], [0, 0, 0]], dtype=f),
        'max_disagreement': torch.tensor([.2, .1, .2, 0], dtype=f),
    }
    want['epistemic'], want['aleatoric'] = 2 * want['disagreement'], 3 * want['disagreement']
    assert set(ref) == set(want)
    for k, v in want.items():
        assert ref[k].dtype == v.dtype and ref[k].shape == v.shape, k
        assert torch.equal(ref[k], v), (k, ref[k], v)
    # the row the cut leaves alone is the unhalted row, bit for bit
    for k in ('states', 'actions', 'rewards', 'constraint_values', 'returns', 'max_constraint'):
        assert torch.equal(ref[k][2], getattr(im, k)[2]), k


def test_limits_of_the_threshold():
    im, scores, w = _example()
    scores = torch.nan_to_num(scores, nan=0.3, posinf=0.3)
    none = cut_reference(im, scores, INF, w)
    assert none['halted_at'].tolist() == [-1] * 4
    for k in ('states', 'rewards', 'returns', 'max_constraint', 'first_violation', 'terminated', 'lengths'):
        assert torch.equal(none[k], getattr(im, k)), k
    every = cut_reference(im, scores, -1.0, w)
    assert every['halted_at'].tolist() == [0] * 4 and every['lengths'].tolist() == [0] * 4
    assert torch.equal(every['states'][:, 0], im.states[:, 0]) and not every['states'][:, 1:].any()
    assert all(math.isinf(x) and x < 0 for x in every['max_constraint'].reshape(-1).tolist())
    assert not every['returns'].any() and not every['terminated'].any()


def test_assert_cut_compares_bits():
    im, scores, w = _example()
    ref = cut_reference(im, torch.nan_to_num(scores, nan=0.3), INF, w)     # (a NaN halts under any threshold)
    ref.pop('halted_at')
    assert_cut(im, ref)
    ref['returns'] = ref['returns'] + 1e-6 * ref['returns']
    try:
        assert_cut(im, ref)
    except AssertionError as e:
        assert 'returns' in str(e)
    else:
        raise AssertionError('a changed bit went unnoticed')
