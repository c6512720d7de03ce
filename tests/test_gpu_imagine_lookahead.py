"""SMBPO.imagine(lookahead=) and ops.lookahead: what the two critics say along imagined
trajectories and at their ends.

Scenes (imagine_helpers): _scene(16) / _scene(32), B 72, H 3, C 2, every natural length, rows
ended and rows cut by the horizon; _action_scene, whose members disagree, for halt=; and one
scene built here with a constrained_fcn='cost' solver (one critic output).

Tolerances. The critics' values come from existing kernels, the stand-alone forwards: against
the oracle's networks at the run's own rows the project's forward tolerance 1e-4 + 1e-4 |ref|
(imagine_helpers). Everything else is bit for bit (float32 as int32): the scan against
lookahead_helpers.lookahead_reference applied to the run's own tensors and its own step_* /
terminal_* (ordered double arithmetic on both sides), the identities, and every tensor the
post-pass must leave alone."""
import random

import numpy as np
import pytest
import torch

import bench
import drpo_amd
from drpo_amd import ops
from gpu_helpers import DEV, _drifting_quadrotor_alg
from imagine_helpers import (B, H, SEED, TENSORS, _action_scene, _assert_every_length, _imagine, _params, _scene,
                             assert_same, bits)
from lookahead_helpers import COST, REACH, assert_bits, lookahead_reference
from oracle import drpo_oracle as O

pytestmark = pytest.mark.gpu

LOOK = ops.ImaginedRollout.LOOKAHEAD_GROUP['lookahead'][0]
SCAN_INPUTS = ('rewards', 'constraint_values', 'dones', 'violations', 'lengths', 'terminated', 'step_q', 'step_qc',
               'terminal_q', 'terminal_qc')
SCALE_NAMES = ('reward_scale', 'alive_bonus', 'constraint_scale', 'constraint_offset')


def _fwd_tol(ref):
    return 1e-4 + 1e-4 * ref.abs()


def _scales(alg, **kw):
    return dict({k: float(getattr(alg, k)) for k in SCALE_NAMES}, **kw)


def check_scan(alg, im, gamma=None, **scales):
    """value_lookahead and certificate_lookahead of one run against the reference on the run's own tensors"""
    gamma = float(alg.solver.discount if gamma is None else gamma)
    mode = REACH if alg.solver.constrained_fcn == 'reachability' else COST
    x = {k: getattr(im, k).detach().cpu() for k in SCAN_INPUTS}
    want_v, want_c = lookahead_reference(**x, gamma=gamma, mode=mode, **_scales(alg, **scales))
    assert_bits(im.value_lookahead, want_v, 'value_lookahead')
    assert_bits(im.certificate_lookahead, want_c, 'certificate_lookahead')
    return want_v, want_c


def check_layout(alg, im, kind, b=B, h=H):
    C = alg.solver.constraint_critic.output_dim
    shapes = {'step_q': (b, h), 'step_qc': (b, h, C), 'terminal_q': (b,), 'terminal_qc': (b, C),
              'value_lookahead': (b, h + 1), 'certificate_lookahead': (b, h + 1, C)}
    for k in LOOK:
        v = getattr(im, k)
        assert v.dtype == torch.float32 and tuple(v.shape) == shapes[k] and v.is_contiguous(), k
    assert im.lookahead_kind == kind
    mask, term = im.mask, im.terminated
    assert not bool(bits(im.step_q)[~mask.cpu()].any()) and not bool(bits(im.step_qc)[~mask.cpu()].any())
    assert not bool(bits(im.terminal_q)[term.cpu()].any()) and not bool(bits(im.terminal_qc)[term.cpu()].any())


def check_networks(alg, im, kind, policy=None):
    """step_q, step_qc, terminal_q and terminal_qc against the oracle's critics at the run's own rows"""
    P, cc = _params(alg), alg.solver.constraint_critic
    C = cc.output_dim
    policy = alg.actor if policy is None else policy
    b, h = im.rewards.shape

    def q_ref(s, a):
        return torch.min(torch.stack(O.critic_all(P, 'critic.', s, a)), 0).values

    def qc_ref(s, a):
        q = O.cons_critic(P, 'constraint_critic.', s, a, 'uncertainty' if kind == 'bound' else 'mean',
                          std_ratio=cc.std_ratio, rng=O.LiveRNG(), lmin=cc.log_std_min, lmax=cc.log_std_max)
        return q.reshape(len(s), C)

    def close(name, got, ref, keep):
        err = (got.cpu() - ref).abs()
        ok = err <= _fwd_tol(ref)
        print(f'{name}: {int(keep.sum())} values in {float(ref[keep].min()):.4f} .. {float(ref[keep].max()):.4f}, '
              f'max |d| {float(err[keep].max()):.3g}')
        assert bool(ok[keep].all()), (name, float(err[keep].max()))
    mask = im.mask.cpu()
    s = im.states[:, :h].reshape(b * h, -1).cpu()
    a = im.actions.reshape(b * h, -1).cpu()
    close('step_q', im.step_q, q_ref(s, a).reshape(b, h), mask)
    close('step_qc', im.step_qc, qc_ref(s, a).reshape(b, h, C), mask.unsqueeze(-1).expand(b, h, C))
    at = im.lengths.long().reshape(b, 1, 1).expand(b, 1, im.states.shape[-1])
    last = torch.gather(im.states, 1, at).reshape(b, -1)
    alive = ~im.terminated.cpu()
    assert bool(alive.any())
    a_pol, a_safe = policy.act(last, eval=True).cpu(), alg.actor_safe.act(last, eval=True).cpu()
    close('terminal_q', im.terminal_q, q_ref(last.cpu(), a_pol), alive)
    close('terminal_qc', im.terminal_qc, qc_ref(last.cpu(), a_safe), alive.unsqueeze(-1).expand(b, C))


def check_identities(im):
    n = im.lengths.cpu().numpy()
    v, c = bits(im.value_lookahead).numpy(), bits(im.certificate_lookahead).numpy()
    live0 = n > 0
    assert np.array_equal(v[live0, 0], bits(im.step_q).numpy()[live0, 0])
    assert np.array_equal(c[live0, 0], bits(im.step_qc).numpy()[live0, 0])
    assert np.array_equal(c[~live0, 0], bits(im.terminal_qc).numpy()[~live0])
    for i in range(len(n)):                                    # entries beyond a length repeat the one at it
        assert (v[i, n[i]:] == v[i, n[i]]).all() and (c[i, n[i]:] == c[i, n[i]]).all(), i


# ------------------------------------------------------------------ 2. the scenes
@pytest.mark.parametrize('kind', [True, 'bound'], ids=['mean', 'bound'])
@pytest.mark.parametrize('rpt', [16, 32])
def test_lookahead_on_the_scenes(rpt, kind):
    alg = _scene(rpt)
    name = 'mean' if kind is True else 'bound'
    im = _imagine(alg, lookahead=kind)
    _assert_every_length(im)
    check_layout(alg, im, name)
    check_networks(alg, im, name)
    want_v, want_c = check_scan(alg, im)
    check_identities(im)
    assert len(np.unique(want_v)) > B and len(np.unique(want_c)) > B       # not a constant
    # in the rewards' own units the value expansion of a terminated row ends in its return
    gamma = float(alg.solver.discount)
    kept = {k: getattr(im, k) for k in LOOK}
    ops.lookahead(alg, alg.actor, im, name, gamma, reward_scale=1, alive_bonus=0)
    torch.cuda.synchronize()
    check_scan(alg, im, reward_scale=1.0, alive_bonus=0.0)
    for k in ('step_q', 'step_qc', 'terminal_q', 'terminal_qc', 'certificate_lookahead'):
        assert torch.equal(bits(getattr(im, k)), bits(kept[k])), k
    n, term = im.lengths.cpu().numpy(), im.terminated.cpu().numpy()
    v, ret = bits(im.value_lookahead).numpy(), bits(im.returns).numpy()
    for i in np.flatnonzero(term):
        assert (v[i, n[i]:] == ret[i]).all(), i


def test_bound_and_mean_differ_where_they_should():
    alg = _scene(16)
    mean, bound = _imagine(alg, lookahead=True), _imagine(alg, lookahead='bound')
    assert_same(mean, bound)
    for k in ('step_q', 'terminal_q', 'value_lookahead'):
        assert torch.equal(bits(getattr(mean, k)), bits(getattr(bound, k))), k
    live = mean.mask
    assert bool((bound.step_qc[live] > mean.step_qc[live]).all())          # mean + std_ratio * std, std > 0
    assert not torch.equal(bits(mean.certificate_lookahead), bits(bound.certificate_lookahead))


# ------------------------------------------------------------------ 3. nothing else moves
def _virtual(alg):
    vb = alg.virt_buffer._module
    return {k: getattr(vb, k).clone() for k in ops._VB_FIELDS if torch.is_tensor(getattr(vb, k))}, \
        int(vb._pointer.item()), int(alg.steps_sampled.item())


@pytest.mark.parametrize('kind', [True, 'bound'], ids=['mean', 'bound'])
def test_lookahead_is_a_post_pass(kind):
    a, b = _drifting_quadrotor_alg(16), _drifting_quadrotor_alg(16)
    before = _virtual(b)
    kw = dict(shield=True, uncertainty=True)
    plain = a.imagine(**kw)
    im = b.imagine(lookahead=kind, **kw)
    torch.cuda.synchronize()
    _assert_every_length(im)
    assert_same(plain, im)
    assert_same(plain, im, ('interventions', 'certificate', 'disagreement', 'epistemic', 'aleatoric', 'max_disagreement'))
    assert plain.shield_threshold == im.shield_threshold and plain.members == im.members
    assert all(getattr(plain, k) is None for k in LOOK + ('lookahead_kind',)) and im.step_q is not None
    # the trainer's stream and imagine's private one stand where the plain call left them
    assert (a.noise.ctr, a._imagine_noise.ctr) == (b.noise.ctr, b._imagine_noise.ctr)
    assert_same(a.imagine(), b.imagine())
    assert_same(a.imagine(noise=a.noise), b.imagine(noise=b.noise))
    # given a noise object it advances as the plain call advances it
    na, nb = drpo_amd.DeviceNoise(5), drpo_amd.DeviceNoise(5)
    assert_same(a.imagine(noise=na), b.imagine(noise=nb, lookahead=kind))
    assert na.ctr == nb.ctr
    after = _virtual(b)
    assert before[1:] == after[1:]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k


# ------------------------------------------------------------------ 4. composition
_ACTION = {}


def _disagreeing():
    if 'v' not in _ACTION:
        _ACTION['v'] = _action_scene(DEV)[0]
    return _ACTION['v']


def test_under_halt_it_runs_on_the_cut_trajectories():
    from test_gpu_rollout_halt import _between_live_scores
    alg = _disagreeing()
    thr = _between_live_scores(_imagine(alg, uncertainty=True))
    cut = _imagine(alg, halt=thr)
    im = _imagine(alg, halt=thr, lookahead=True)
    assert_same(cut, im)
    assert_same(cut, im, ('halted_at', 'disagreement', 'max_disagreement'))
    n = im.lengths.cpu().numpy()
    print(f'halt at {thr:.6g}: lengths {sorted(set(n.tolist()))}, {int((n == 0).sum())} rows of length 0')
    assert (n == 0).any() and (n > 0).any()
    check_layout(alg, im, 'mean')
    check_networks(alg, im, 'mean')
    check_scan(alg, im)
    check_identities(im)
    # a row of length 0: every entry is its terminal bootstrap
    zero = np.flatnonzero(n == 0)
    w0q = bits((im.terminal_q.double() * 1.0 + 0.0).float()).numpy()
    assert (bits(im.value_lookahead).numpy()[zero] == w0q[zero, None]).all()
    assert (bits(im.certificate_lookahead).numpy()[zero] == bits(im.terminal_qc).numpy()[zero, None]).all()


@pytest.mark.parametrize('form', ['actionsH', 'shield'])
def test_other_forms_of_the_call(form):
    alg = _scene(16)
    acts = (torch.rand(B, H, alg.action_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    kw = {'actionsH': dict(actions=acts), 'shield': dict(shield=True)}[form]
    plain = _imagine(alg, **kw)
    im = _imagine(alg, lookahead=True, **kw)
    assert_same(plain, im)
    assert im.given_steps == (H if form == 'actionsH' else 0)
    if form == 'shield':
        assert_same(plain, im, ('interventions', 'certificate'))
    check_layout(alg, im, 'mean')
    check_networks(alg, im, 'mean')
    check_scan(alg, im)
    check_identities(im)


def test_members_each_stacks_the_lookahead():
    alg = _scene(16)
    elites = list(alg.model_ensemble._elite_inds)
    E = len(elites)
    each = _imagine(alg, members='each', lookahead='bound', seed=77)
    assert each.lookahead_kind == 'bound'
    C = alg.solver.constraint_critic.output_dim
    assert each.step_q.shape == (E, B, H) and each.step_qc.shape == (E, B, H, C)
    assert each.terminal_q.shape == (E, B) and each.terminal_qc.shape == (E, B, C)
    assert each.value_lookahead.shape == (E, B, H + 1) and each.certificate_lookahead.shape == (E, B, H + 1, C)
    for k, member in enumerate(elites):
        one = _imagine(alg, members=member, lookahead='bound', seed=77)
        for name in TENSORS + LOOK:
            assert torch.equal(bits(getattr(each, name)[k]), bits(getattr(one, name))), (k, name)


def _cost_scene():
    """_drifting_quadrotor_alg(16) with a constrained_fcn='cost' solver: the certificate is one
    discounted violation count (one critic output for the two constraints)."""
    random.seed(11)
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON,
                         extra={'sac_cfg': {'constrained_fcn': 'cost', 'distributional_qc': False,
                                            'qc_under_uncertainty': False, 'mlp_multiplier': False}})
    rep = bench.synth_replay('quadrotor', 400, np.random.RandomState(0))
    rep['states'][:, 2] = np.linspace(0.6, 1.6, 400, dtype=np.float32)
    rep['states'][:, [0, 4]] *= 0.1
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    _, diff, _ = alg.model_ensemble.views()
    diff[-1][1][..., 2] = 0.1
    alg.rollout_engine, alg.rows_per_tile = 2, 16
    return alg


def test_a_cost_solver():
    alg = _cost_scene()
    assert alg.solver.constrained_fcn == 'cost' and alg.solver.constraint_critic.output_dim == 1 and alg.con_dim == 2
    im = _imagine(alg, lookahead=True)
    _assert_every_length(im)
    assert bool(im.violations.any())
    check_layout(alg, im, 'mean')
    check_networks(alg, im, 'mean')
    check_scan(alg, im)
    check_identities(im)
    with pytest.raises(ValueError, match='needs a distributional constraint critic'):
        alg.imagine(lookahead='bound')
