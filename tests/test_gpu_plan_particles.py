"""SMBPO.plan(particles=) and imagine(particles=): planning over ensemble particles, on
test_gpu_plan's scene and sizes (imagine_helpers._action_scene: 7 members, elites 3, 0, 6, 2, 5;
P 5, N 32, H 3, model_noise=False, so that a row is a function of its start state, its actions
and its member alone).

Everything is bit for bit (float32 as int32): one particle is the fixed member; a plan's member
values are column H of the public imagine(actions=, members=m_j, lookahead=True), its scores,
certificates and ranks the helper's aggregation and order of them; imagine(particles=) is the
stack of the per-member runs at the same seed and counter. The monotonicity check compares float32
keys the kernel itself stored."""
import numpy as np
import pytest
import torch

import drpo_amd
from drpo_amd import _lib, ops
from gpu_helpers import DEV, _drifting_quadrotor_alg
from imagine_helpers import MEMBER
from plan_helpers import INF, assert_bits, bits, plan_order
from plan_particles_helpers import particle_aggregate
from test_gpu_plan import H, N, P, _alg, _key, _states

pytestmark = pytest.mark.gpu

PARTS = [3, 0, 6]
FIELDS = ('actions', 'action', 'score', 'certificate', 'feasible', 'n_feasible', 'mean', 'std', 'history_score',
          'history_certificate', 'history_feasible', 'candidates', 'scores', 'certificates', 'ranks')


def _plan(alg, seed=11, **kw):
    res = alg.plan(_states(alg), H,
                   **dict(dict(candidates=N, noise=drpo_amd.DeviceNoise(seed), model_noise=False), **kw))
    torch.cuda.synchronize()
    return res


def _middle_threshold(alg, **kw):
    c = _plan(alg, iterations=1, threshold=INF, **kw).certificates
    return float(c.flatten().sort().values[c.numel() // 2])


# ------------------------------------------------------------------ 1. one particle is the fixed member
@pytest.mark.parametrize('filt', [None, True, 'linear'], ids=['plain', 'filter', 'linear-filter'])
def test_one_particle_is_the_fixed_member(filt):
    alg = _alg('reach')
    kw = dict(iterations=2, temperature=0.5, momentum=0.25, steps=2, safety_filter=filt,
              threshold=_middle_threshold(alg, members=MEMBER))
    a, b = _plan(alg, members=MEMBER, **kw), _plan(alg, particles=[MEMBER], **kw)
    for k in FIELDS:
        assert_bits(getattr(b, k), getattr(a, k), k)
    assert (b.threshold, b.lookahead_kind, b.filter_threshold) == (a.threshold, a.lookahead_kind, a.filter_threshold)
    for k in ops.ImaginedRollout.TENSORS + (('interventions', 'certificate') if filt else ()):
        assert_bits(getattr(b.imagined, k)[0], getattr(a.imagined, k), 'imagined.' + k)
    assert b.imagined.rewards.shape == (1, P * N, H) and b.imagined.particle_launches == 1
    if filt:
        assert_bits(b.executed_actions[0], a.executed_actions, 'executed_actions')
        assert_bits(b.interventions[0], a.interventions, 'interventions')
        assert_bits(b.safe_action, a.safe_action, 'safe_action')
    # what the particles add; and a call without them says nothing of them
    assert (b.particles, b.risk, b.cert_risk) == ([MEMBER], 'mean', 'max')
    assert_bits(b.member_scores[0], a.scores, 'member_scores')
    assert_bits(b.member_certificates[0], a.certificates, 'member_certificates')
    assert not bool(b.score_spread.any())
    assert all(getattr(a, k) is None for k in ops.PlanResult.PARTICLE_FIELDS)


# ------------------------------------------------------------------ 2. the last iteration, re-run in public
@pytest.mark.parametrize('risk, T', [('mean', 3), ('worst', 1), (('cvar', 0.5), 2)], ids=['mean', 'worst', 'cvar'])
@pytest.mark.parametrize('cert_risk', ['max', 'mean'])
def test_member_values_are_imagines_and_the_aggregate_is_the_helpers(risk, T, cert_risk):
    alg = _alg('reach')
    thr = _middle_threshold(alg, particles=PARTS, risk=risk, cert_risk=cert_risk)
    res = _plan(alg, iterations=2, particles=PARTS, risk=risk, cert_risk=cert_risk, threshold=thr)
    A, G = alg.action_dim, len(PARTS)
    assert res.member_scores.shape == res.member_certificates.shape == (G, P, N) and res.score_spread.shape == (P, N)
    assert (res.particles, res.risk, res.cert_risk) == (PARTS, risk, cert_risk)
    assert res.imagined.rewards.shape == (G, P * N, H) and res.imagined.particle_launches == G
    cand = res.candidates.reshape(P * N, H, A)
    for j, m in enumerate(PARTS):
        im = alg.imagine(_states(alg).repeat_interleave(N, 0), horizon=H, actions=cand, lookahead=True,
                         deterministic=True, noise=drpo_amd.DeviceNoise(99), members=m, model_noise=False)
        torch.cuda.synchronize()
        assert_bits(res.member_scores[j].reshape(-1), im.value_lookahead[:, H].contiguous(), f'member_scores[{j}]')
        assert_bits(res.member_certificates[j].reshape(-1), im.certificate_lookahead[:, H].max(dim=-1).values,
                    f'member_certificates[{j}]')
        assert_bits(res.imagined.states[j], im.states, f'imagined.states[{j}]')
    ms, mc = res.member_scores.cpu().numpy().reshape(G, -1), res.member_certificates.cpu().numpy().reshape(G, -1)
    s, c, sp = particle_aggregate(ms, mc, T, 0 if cert_risk == 'max' else 1)
    assert_bits(res.scores.reshape(-1), s, 'scores')
    assert_bits(res.certificates.reshape(-1), c, 'certificates')
    assert_bits(res.score_spread.reshape(-1), sp, 'score_spread')
    s, c, nf = s.reshape(P, N), c.reshape(P, N), res.n_feasible.cpu().numpy()
    for p in range(P):
        order, cls, _ = plan_order(s[p], c[p], thr)
        assert res.ranks[p].cpu().tolist() == [order.index(n) for n in range(N)], p
        assert nf[p] == cls.count(0)
        assert_bits(res.actions[p], res.candidates[p, order[0]], f'actions[{p}]')
        assert bits(res.score)[p] == bits(s)[p, order[0]] and bits(res.certificate)[p] == bits(c)[p, order[0]]
    assert 0 < int(nf.sum()) < P * N                       # the threshold divides the candidates
    assert float(res.score_spread.max()) > 0               # the members disagree
    assert (ms[0] != ms[1]).any() and (ms[1] != ms[2]).any()


def test_the_risks_order_as_they_should():
    alg = _alg('reach')
    runs = {r: _plan(alg, iterations=1, particles=PARTS, risk=r, threshold=INF)
            for r in ('mean', 'worst', ('cvar', 0.5))}
    for r in runs.values():          # the same candidates and member values; another aggregate
        assert_bits(r.member_scores, runs['mean'].member_scores, 'member_scores')
    assert_bits(runs['worst'].scores, runs['mean'].member_scores.min(dim=0).values, 'worst: the minimum')
    assert bool((runs['worst'].scores <= runs[('cvar', 0.5)].scores).all())
    assert bool((runs[('cvar', 0.5)].scores <= runs['mean'].scores).all())
    tight, loose = (_plan(alg, iterations=1, particles=PARTS, cert_risk=c, threshold=INF) for c in ('max', 'mean'))
    assert_bits(tight.certificates, tight.member_certificates.max(dim=0).values, 'max: every member certifies')
    assert bool((loose.certificates <= tight.certificates).all())
    assert not torch.equal(loose.certificates, tight.certificates)


# ------------------------------------------------------------------ 3. what the iterations promise
@pytest.mark.parametrize('risk', ['mean', ('cvar', 0.5)], ids=['mean', 'cvar'])
def test_the_incumbents_key_never_decreases(risk):
    alg = _alg('reach')
    thr = _middle_threshold(alg, particles=PARTS, risk=risk)
    res = _plan(alg, iterations=4, particles=PARTS, risk=risk, threshold=thr, temperature=1.0)
    f, s, c = res.history_feasible.cpu(), res.history_score.cpu(), res.history_certificate.cpu()
    keys = [[_key(f[i, p], s[i, p], c[i, p]) for p in range(P)] for i in range(4)]
    for i in range(3):
        for p in range(P):
            assert keys[i + 1][p] >= keys[i][p], (i, p, keys[i][p], keys[i + 1][p])
    print('keys of the first and the last iteration:', keys[0], keys[3])
    assert_bits(res.history_score[3], res.score, 'score')


# ------------------------------------------------------------------ 4. nothing else moves
def test_plan_particles_leaves_the_training_state_alone(monkeypatch):
    from test_gpu_imagine_lookahead import _virtual
    alg = _drifting_quadrotor_alg(16)
    alg.imagine()                                            # (so that imagine's private stream exists)
    torch.cuda.synchronize()
    before = _virtual(alg)
    ctrs = (alg.noise.ctr, alg._imagine_noise.ctr)
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_refit', 'drpo_plan_refit_particles', 'drpo_rollout_trajectories_given',
                 'drpo_rollout_lookahead', 'drpo_rollout', 'drpo_rollout_trajectories'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    parts = [int(m) for m in alg.model_ensemble._elite_inds][:3]
    noise = drpo_amd.DeviceNoise(4)
    res = alg.plan(_states(alg), H, candidates=N, iterations=2, init='policy', particles=parts, noise=noise)
    torch.cuda.synchronize()
    # the policy's run under the first particle; per iteration one sample launch, one run per particle, one refit
    assert calls == ['drpo_rollout_trajectories'] + (['drpo_plan_sample'] + ['drpo_rollout_trajectories_given'] * 3 +
                                                     ['drpo_plan_refit_particles']) * 2
    assert noise.ctr == 1 + 2 * 2                            # as without particles: the particles share a counter
    assert (alg.noise.ctr, alg._imagine_noise.ctr) == ctrs and alg.__dict__.get('_plan_noise') is None
    after = _virtual(alg)
    assert before[1:] == after[1:]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    assert res.imagined.step_q is None and res.imagined.value_lookahead is None


# ------------------------------------------------------------------ 5. behind the shield
@pytest.mark.parametrize('filt', [True, 'linear'])
def test_the_filtered_first_action_is_the_same_under_every_member(filt):
    alg = _alg('reach')
    a_safe_thr = _middle_threshold(alg, particles=PARTS)
    # a shield threshold between the proposals' certificates, so that it steps in at some first steps and not at others
    probe = _plan(alg, iterations=1, particles=PARTS, safety_filter=INF if filt is True else ('linear', INF))
    mid = float(probe.imagined.certificate[0, :, 0].flatten().sort().values[P * N // 2])
    res = _plan(alg, iterations=2, particles=PARTS, threshold=a_safe_thr,
                safety_filter=mid if filt is True else ('linear', mid))
    G, A = len(PARTS), alg.action_dim
    assert res.executed_actions.shape == (G, P, H, A) and res.interventions.shape == (G, P, H)
    assert res.safe_action.shape == (P, A) and res.filter_threshold == float(np.float32(mid))
    for j in range(G):
        assert_bits(res.executed_actions[j, :, 0].contiguous(), res.safe_action.contiguous(), f'group {j}, step 0')
        assert torch.equal(res.interventions[j, :, 0], res.interventions[0, :, 0])
    # over all rows too: step 0's proposal, certificate and executed action do not depend on the member
    im = res.imagined
    assert torch.equal(im.actions[:, :, 0], im.actions[:1, :, 0].expand(G, -1, -1))
    assert torch.equal(im.interventions[:, :, 0], im.interventions[:1, :, 0].expand(G, -1))
    assert 0 < int(im.interventions[0, :, 0].sum()) < P * N       # the shield steps in at some and not at others
    assert not torch.equal(im.states[0, :, 1], im.states[1, :, 1])   # and the members differ from step 1 on
    # the best row's executed actions are its trajectory's under each member
    rows = torch.arange(P, device=DEV) * N + res.ranks.argmin(dim=1)
    assert_bits(res.executed_actions, im.actions[:, rows], 'executed_actions')


# ------------------------------------------------------------------ 6. the controller
def test_mpc_with_particles_acts_cold_and_warm():
    alg = _alg('reach')
    noise = drpo_amd.DeviceNoise(31)
    ctl = alg.mpc(horizon=H, candidates=N, iterations=2, particles=PARTS, risk='worst', noise=noise, threshold=INF,
                  fallback=None)
    s = _states(alg)
    a0 = ctl.act(s)
    first = ctl.last
    a1 = ctl.act(s)
    torch.cuda.synchronize()
    assert a0.shape == a1.shape == (P, alg.action_dim) and ctl.steps == 2
    assert (first.warm_started, ctl.last.warm_started, ctl.last.shift) == (False, True, 1)
    assert first.particles == ctl.last.particles == PARTS and ctl.last.risk == 'worst'
    assert_bits(a0, first.action, 'the cold action')
    # the cold call is plan's; the warm one starts from the first one's best sequence, moved one step
    cold = _plan(alg, seed=31, iterations=2, particles=PARTS, risk='worst', threshold=INF)
    assert_bits(cold.actions, first.actions, 'cold')
    assert_bits(cold.member_scores, first.member_scores, 'cold member_scores')
    assert noise.ctr == 2 * 2 * 2
    assert ctl.last.member_scores.shape == (len(PARTS), P, N)
    assert_bits(a1, ctl.last.action, 'the warm action')


# ------------------------------------------------------------------ 7. imagine(particles=) on the per-member launches
@pytest.mark.parametrize('kw', [dict(deterministic=True), dict(model_noise=True), dict(shield=True),
                                dict(shield='linear', deterministic=True), dict(halt=0.5)],
                         ids=['recorded', 'philox', 'shield', 'linear', 'halt'])
def test_imagine_particles_is_the_stack_of_the_members_runs(kw):
    alg = _alg('reach')
    s = _states(alg).repeat_interleave(4, 0)                 # 20 rows: not a multiple of the tile
    given = {} if 'shield' in kw or 'halt' in kw else \
        {'actions': torch.rand(len(s), 2, alg.action_dim, device=DEV) - 0.5}
    parts = [2, 2, 5]
    im = alg.imagine(s, horizon=H, particles=parts, noise=drpo_amd.DeviceNoise(8), uncertainty=True, lookahead=True,
                     **given, **kw)
    runs = [alg.imagine(s, horizon=H, members=m, noise=drpo_amd.DeviceNoise(8), uncertainty=True, lookahead=True,
                        **given, **kw) for m in parts]
    torch.cuda.synchronize()
    assert im.particle_launches == 3 and im.members == [r.members for r in runs] and runs[0].particle_launches is None
    names = ops.ImaginedRollout.TENSORS + tuple(k for per_run, _ in ops.ImaginedRollout._ALL_GROUPS.values()
                                                for k in per_run if getattr(runs[0], k) is not None)
    assert {'disagreement', 'value_lookahead'} <= set(names)
    for k in names:
        assert_bits(getattr(im, k), torch.stack([getattr(r, k) for r in runs]), k)
    assert torch.equal(im.states[0], im.states[1])           # the same member twice: the same run
    if 'halt' not in kw:                                     # (the halt cuts these rows before the members part)
        assert not torch.equal(im.states[0], im.states[2])


def test_imagine_particles_elites_is_members_each():
    alg = _alg('reach')
    s = _states(alg)
    a, b = (alg.imagine(s, horizon=H, noise=drpo_amd.DeviceNoise(8), lookahead=True, **kw)
            for kw in (dict(members='each'), dict(particles='elites')))
    torch.cuda.synchronize()
    for k in ops.ImaginedRollout.TENSORS + ('value_lookahead', 'certificate_lookahead'):
        assert_bits(getattr(b, k), getattr(a, k), k)
    assert a.members == b.members
    assert (a.particle_launches, b.particle_launches) == (None, len(alg.model_ensemble._elite_inds))
