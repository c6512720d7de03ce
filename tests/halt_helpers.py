"""What the tests of halted rollouts share (tests/test_rollout_halt_reference.py,
tests/test_gpu_rollout_halt.py): the host-side reference of the cut and its comparison.

cut_reference applies the one definition of halting to an UNHALTED ImaginedRollout, in torch
on the CPU. With score[i, t], the row's natural length len_i and a threshold thr (compared in
float32, as the kernel compares it):

  c_i          the first t < len_i with not (score[i, t] <= thr): a NaN halts, equality does not
  halted_at    c_i, or -1 if there is none;  the new length is c_i if halted, len_i otherwise
  steps t >= the new length do not exist: zero in every per-step tensor; states keeps
  states[i, new length], the state the row halted at (its start state for length 0)
  returns      sum over the kept steps of weights[t] * rewards[i, t], accumulated in step order
               in float64 and rounded to float32 once: the kernel's own order, so equal to the bit
  max_constraint  over the kept steps, -inf for length 0;  first_violation -1 unless before the
               cut;  terminated False for a halted row
  the optional groups' [B, H] tensors are zero at and beyond the new lengths, max_disagreement
  the largest kept disagreement (0 for length 0)."""
import types

import torch

CORE = ('states', 'actions', 'rewards', 'constraint_values', 'dones', 'violations', 'lengths', 'returns',
        'max_constraint', 'first_violation', 'terminated')
STEP_GROUPS = ('interventions', 'certificate', 'blend', 'disagreement', 'epistemic', 'aleatoric')


def cut_reference(im, scores, thr, weights=None):
    """The tensors of ``im`` (one unhalted run) as they look under the cut, as a dict of CPU
    tensors: CORE, 'halted_at', and those of STEP_GROUPS / 'max_disagreement' that ``im`` has.
    scores: [B, H]; weights: H float64 per-step weights of ``returns`` (default ones)."""
    H = im.rewards.shape[-1]
    length = im.lengths.detach().cpu().long()
    B = len(length)
    sc = scores.detach().cpu().float()
    assert tuple(sc.shape) == (B, H)
    thr32 = torch.tensor(float(thr), dtype=torch.float32)
    steps = torch.arange(H)
    over = ~(sc <= thr32) & (steps[None] < length[:, None])
    halted = over.any(-1)
    first = over.to(torch.int64).argmax(-1)
    newlen = torch.where(halted, first, length)
    mask = steps[None] < newlen[:, None]
    t = {k: getattr(im, k).detach().cpu() for k in CORE}
    out = {'halted_at': torch.where(halted, first, torch.full_like(first, -1)).to(torch.int32),
           'lengths': newlen.to(torch.int32)}
    smask = torch.arange(H + 1)[None] <= newlen[:, None]
    out['states'] = torch.where(smask[..., None], t['states'], torch.zeros_like(t['states']))
    for k in ('actions', 'constraint_values'):
        out[k] = torch.where(mask[..., None], t[k], torch.zeros_like(t[k]))
    for k in ('rewards', 'dones', 'violations'):
        out[k] = torch.where(mask, t[k], torch.zeros_like(t[k]))
    w = torch.ones(H, dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    acc = torch.zeros(B, dtype=torch.float64)
    for s in range(H):
        acc = torch.where(mask[:, s], acc + w[s] * t['rewards'][:, s].double(), acc)
    out['returns'] = acc.float()
    neg = torch.full_like(t['constraint_values'], float('-inf'))
    out['max_constraint'] = torch.where(mask[..., None], t['constraint_values'], neg).max(dim=1).values
    viol = out['violations'].bool()
    out['first_violation'] = torch.where(viol.any(-1), viol.to(torch.int64).argmax(-1),
                                         torch.full_like(first, -1)).to(torch.int32)
    out['terminated'] = t['terminated'] & ~halted
    for k in STEP_GROUPS:
        v = getattr(im, k, None)
        if v is not None:
            v = v.detach().cpu()
            out[k] = torch.where(mask, v, torch.zeros_like(v))
    if 'disagreement' in out:
        out['max_disagreement'] = out['disagreement'].max(dim=-1).values
    return out


def run_of(im, e):
    """Run ``e`` of a stacked ImaginedRollout (members='each'), as cut_reference reads one."""
    names = CORE + STEP_GROUPS + ('max_disagreement', 'halted_at')
    return types.SimpleNamespace(**{k: (None if getattr(im, k, None) is None else getattr(im, k)[e]) for k in names})


def _bits(x):
    x = x.detach().cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def assert_cut(im, ref):
    """Every tensor of the reference, bit for bit (float32 as int32)."""
    for k, want in ref.items():
        got = getattr(im, k)
        assert got is not None, k
        got = got.detach().cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, want.dtype, got.shape, want.shape)
        assert torch.equal(_bits(got), _bits(want)), k
