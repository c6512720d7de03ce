"""The ensemble's disagreement through the Python layers: BatchedGaussianEnsemble.disagreement,
SMBPO.imagine(uncertainty=) and SMBPO.model_rollout_error(uncertainty=True).

Scene: _drifting_quadrotor_alg(16) (B 72, H 3, rows dying at steps 0, 1 and 2), elites
[3, 0, 6, 2, 5]. Its steady mode zeroes the diff head's output layer, which makes the seven
members one model; here that layer gets small per-member weights back (0.003 N(0, 1), seeded:
a prediction moves by ~1e-2, a tenth of the drift that ends the rows), so the members disagree
and by an amount that depends on the row.

Tolerances. Between calls everything is compared bit for bit (float32 as int32). Against
float64, test_gpu_ens_spread's error model with its reference built from what the model's own
head returns: d = mu - [s, 0] and lv of _forward_all. mu = D + s was rounded once, so every d of
the reference is off by up to 2^-24 (|s| + |d|): |s| is added to the |d| of every term. lv is the
kernel's own float32 clamp of the same raw value (one definition, lv_clamp), so what is left of
the aleatoric error is the exp's: exp_arg is |lv| / 2, no larger than the a_l / 2 of the model."""
import numpy as np
import pytest
import torch

import drpo_amd
from gpu_helpers import (C_LIBM, DEV, SPREAD_OUTPUTS as OUTPUTS, _drifting_quadrotor_alg, f64,
                         spread_statistics as statistics, within)
from imagine_helpers import (B, EP_LEN, H, TENSORS, _action_scene, _assert_every_length, _episode_inputs, assert_same,
                             bits)

pytestmark = pytest.mark.gpu

ELITES = [3, 0, 6, 2, 5]
UNC = ('disagreement', 'epistemic', 'aleatoric')


def _scene():
    alg = _drifting_quadrotor_alg(16)
    m = alg.model_ensemble
    _, diff, _ = m.views()
    W = diff[-1][0]
    g = torch.Generator().manual_seed(23)
    W.add_(0.003 * torch.randn(W.shape, generator=g).to(DEV))
    m._elite_inds = list(ELITES)
    return alg


@pytest.fixture(scope='module')
def alg():
    return _scene()


def _check_spread(tag, sp, m, s, a, members, w):
    """sp against the float64 statistics of the head's own outputs (module docstring)"""
    mu, lv = m._forward_all(s.unsqueeze(0), a.unsqueeze(0))
    s0 = torch.cat([f64(s), torch.zeros(len(s), 1, dtype=torch.float64)], -1)
    d, lv = (f64(mu) - s0)[members], f64(lv)[members]
    ref, model = statistics(d, lv, lv.abs() / 2, s0, f64(w), d.abs() + s0.abs())
    for k in OUTPUTS:
        terms, exp_arg = model[k]
        within(f'disagreement() {k} {tag}', getattr(sp, k), ref[k], terms, C_LIBM, exp_arg)
    return ref


def _same_spread(a, b):
    for k in OUTPUTS:
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k


def test_disagreement_of_replay_rows(alg):
    m = alg.model_ensemble
    S = alg.state_dim
    s, a = (x[2:400:5][:B].contiguous() for x in alg.replay_buffer.get('states', 'actions'))
    assert len(s) == B
    norm = m.state_normalizer
    w = torch.cat([1.0 / (norm.std + norm.epsilon), torch.zeros(1, device=DEV)])
    sp = m.disagreement(s, a)
    torch.cuda.synchronize()
    assert sp.members == ELITES and sp.mean.shape == (B, S + 1) and sp.disagreement.shape == (B,)
    ref = _check_spread('elites', sp, m, s, a, ELITES, w)
    assert float(ref['disagreement'].min()) > 0 and float(ref['disagreement'].max()) > float(ref['disagreement'].min())
    _same_spread(m.disagreement(s, a, members=list(m._elite_inds)), sp)
    every = m.disagreement(s, a, members='all')
    assert every.members == list(range(7))
    _check_spread('all', every, m, s, a, list(range(7)), w)
    assert bool((every.disagreement >= sp.disagreement).all())          # more pairs, the elites' among them
    eng = m.engine
    try:
        eng.spread_chunk_rows = 16                                       # 4 chunks of 16 rows and one of 8
        _same_spread(m.disagreement(s, a), sp)
    finally:
        del eng.spread_chunk_rows
    assert eng.spread_chunk_rows == 65536
    ones = m.disagreement(s, a, scale=torch.ones(S))
    _check_spread('scale of ones', ones, m, s, a, ELITES, torch.cat([torch.ones(S), torch.zeros(1)]))
    _same_spread(m.disagreement(s, a, scale=torch.cat([torch.ones(S), torch.zeros(1)]).to(DEV)), ones)


def _check_uncertainty_layout(im, shape):
    """present, float32, of the rollout's shape, zero at and beyond the lengths"""
    mask = im.mask
    assert mask.shape == shape
    for k in UNC:
        v = getattr(im, k)
        assert v.shape == shape and v.dtype == torch.float32, k
        assert torch.equal(bits(v[~mask]), torch.zeros(int((~mask).sum()), dtype=torch.int32)), k
        assert bool((v[mask] > 0).all()), k
    assert im.max_disagreement.shape == shape[:-1]
    assert torch.equal(bits(im.max_disagreement), bits(torch.where(mask, im.disagreement, 0).max(-1).values))


def test_imagine_uncertainty_is_a_post_pass():
    a, b = _scene(), _scene()
    plain = a.imagine(noise=drpo_amd.DeviceNoise(7))
    im = b.imagine(uncertainty=True, noise=drpo_amd.DeviceNoise(7))
    torch.cuda.synchronize()
    _assert_every_length(im)
    assert_same(plain, im)
    assert all(getattr(plain, k) is None for k in UNC + ('max_disagreement',))
    assert_same(a.imagine(), b.imagine())                              # no counter of the trainer moved
    _check_uncertainty_layout(im, (B, H))
    mask = im.mask
    m = b.model_ensemble
    sp = m.disagreement(im.states[:, :H][mask], im.actions[mask])
    for k in UNC:
        assert torch.equal(bits(getattr(im, k)[mask]), bits(getattr(sp, k))), k
    # first_uncertain against a loop, at the median live disagreement
    dis, length = im.disagreement.cpu().numpy(), im.lengths.cpu().numpy()
    thr = float(np.median(dis[mask.cpu().numpy()]))
    want = np.full(B, -1, np.int32)
    for i in range(B):
        for t in range(int(length[i])):
            if dis[i, t] > thr:
                want[i] = t
                break
    got = im.first_uncertain(thr)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert (want == -1).any() and (want >= 0).any()
    assert np.array_equal(im.first_uncertain(float('inf')).cpu().numpy(), np.full(B, -1, np.int32))
    assert np.array_equal(im.first_uncertain(-1.0).cpu().numpy(), np.zeros(B, np.int32))
    with pytest.raises(ValueError, match='first_uncertain needs'):
        plain.first_uncertain(thr)
    every = b.imagine(uncertainty='all', noise=drpo_amd.DeviceNoise(7))
    assert_same(plain, every)
    assert bool((every.disagreement >= im.disagreement).all()) and not torch.equal(every.disagreement, im.disagreement)


@pytest.mark.parametrize('form', ['actions1', 'actionsH', 'shield', 'linear', 'deterministic'])
def test_other_forms_of_the_call(alg, form):
    acts = torch.rand(B, H, alg.action_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1
    kw = {'actions1': dict(actions=acts[:, :1].contiguous()), 'actionsH': dict(actions=acts), 'shield': dict(shield=True),
          'linear': dict(shield='linear'), 'deterministic': dict(deterministic=True, model_noise=False)}[form]
    plain = alg.imagine(noise=drpo_amd.DeviceNoise(11), **kw)
    im = alg.imagine(uncertainty=True, noise=drpo_amd.DeviceNoise(11), **kw)
    torch.cuda.synchronize()
    assert_same(plain, im)
    if 'shield' in kw:
        assert torch.equal(plain.interventions, im.interventions)
        assert torch.equal(bits(plain.certificate), bits(im.certificate))
    _check_uncertainty_layout(im, (B, H))


def test_members_each_stacks_the_uncertainty(alg):
    each = alg.imagine(members='each', uncertainty=True, noise=drpo_amd.DeviceNoise(77))
    torch.cuda.synchronize()
    _check_uncertainty_layout(each, (5, B, H))
    assert not torch.equal(each.disagreement[0], each.disagreement[1])
    for k, member in enumerate(ELITES):
        one = alg.imagine(members=member, uncertainty=True, noise=drpo_amd.DeviceNoise(77))
        for name in TENSORS + UNC + ('max_disagreement',):
            assert torch.equal(bits(getattr(each, name)[k]), bits(getattr(one, name))), (k, name)


def test_model_rollout_error_with_uncertainty():
    """The replay of test_model_rollout_error_on_episodes_the_model_made: two episodes member 3
    imagined, so the buffer holds real 2-step segments."""
    alg, rep, _ = _action_scene(DEV, scale=3.0)
    s0, seq = _episode_inputs(rep)
    im = alg.imagine(states=s0[:1].to(DEV), actions=seq[:1].contiguous().to(DEV), members=3, model_noise=False,
                     horizon=EP_LEN)
    assert int(im.lengths[0]) == EP_LEN
    alg.replay_buffer.extend(states=im.states[0, :EP_LEN], actions=im.actions[0], next_states=im.states[0, 1:],
                             rewards=im.rewards[0], dones=im.dones[0], violations=im.violations[0],
                             constraint_values=im.constraint_values[0])
    plain = alg.model_rollout_error(horizon=2, members=0)
    err = alg.model_rollout_error(horizon=2, members=0, uncertainty=True)
    torch.cuda.synchronize()
    n = EP_LEN - 1
    assert plain.disagreement is None and plain.epistemic is None
    assert err.disagreement.shape == err.epistemic.shape == err.alive.shape == (n, 2)
    assert torch.equal(plain.starts, err.starts) and torch.equal(plain.alive, err.alive)
    for k in ('state_error', 'reward_error'):
        assert torch.equal(bits(getattr(plain, k)), bits(getattr(err, k))), k
    assert_same(plain.imagined, err.imagined)
    alive = err.alive
    assert int(alive.sum()) >= n
    for k in ('disagreement', 'epistemic'):
        assert torch.equal(torch.isnan(getattr(err, k)), ~alive), k
    s = alg.replay_buffer.get('states')
    state_std = s.std(dim=0)
    state_std[state_std < 1e-7] = 1.0
    ri = err.imagined
    sp = alg.model_ensemble.disagreement(ri.states[:, :2][alive], ri.actions[alive], scale=1.0 / (state_std + 1e-7))
    assert torch.equal(bits(err.disagreement[alive]), bits(sp.disagreement))
    assert torch.equal(bits(err.epistemic[alive]), bits(sp.epistemic))
    assert bool((sp.disagreement > 0).all())
