"""Imagined rollouts under the shielded controller (SMBPO.imagine(shield=),
ops.rollout_trajectories(shield=), drpo_rollout_trajectories_shielded: the SH
instantiations of rollout_persist_kernel; the shield of src/smbpo.py:124-136).

The scene is gpu_helpers._drifting_quadrotor_alg: B 72 (four full 16-row tiles
and one of 8, or two 32-row tiles and one of 8), H 3, S 12, A 2, C 2, rows leaving at
steps 0, 1 and 2 while others survive. The safe actor starts as a copy of the actor, so
its mean action tanh(mu) differs from the actor's sample tanh(mu + std * eps) by 0.28 on
average (CPU oracle).

Tolerances: between calls of the kernel everything is compared bit for bit (float32 as
int32). Against the oracle |d| <= 2e-4 + 2e-4 |ref|, the oracle tolerance of
test_gpu_imagine.py. The safe actor's action against the stand-alone op at the project's
forward tolerance 1e-4 + 1e-4 |ref| (tanhf there, fast_tanh in the kernel)."""
import numpy as np
import pytest
import torch

import drpo_amd
from drpo_amd import envs, ops
from drpo_amd.policy import SquashedGaussianPolicy
from gpu_helpers import DEV, ProgramQuadrotor, _drifting_quadrotor_alg, _fill, _no_host_env, _width_alg
from imagine_helpers import (B, H, INF, MEMBER, PRE, SEED, TENSORS, _assert_every_length, _params, _scene,
                             _teacher_inputs, _tol, assert_same, bits, check_certificate_at_step_0,
                             check_replay_and_safe_action, oracle_qc)
from oracle import drpo_oracle as O

pytestmark = pytest.mark.gpu


def oracle_shield_step(P, alg, s, eps_a_t):
    """(a_perf, q, a_safe) of one step from states s under the recorded action draws."""
    mu, std = O.policy_params(P, 'actor.net.', s)
    a_perf = torch.tanh(mu + std * eps_a_t)
    return (a_perf, oracle_qc(P, alg, s, a_perf, alg.solver.distributional_qc),
            O.policy_mean(P, 'actor_safe.net.', s))


def _alg16():
    return _scene(16)


# ------------------------------------------------------------------ 1 / 2. the two ends
def check_threshold_plus_inf(alg, **kw):
    """Nothing intervenes: the SH kernel's actor and member phases are the parent's and no
    draw moved. Returns the shielded run."""
    base = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), **kw)
    sh = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), shield=INF, **dict({'members': base.members}, **kw))
    torch.cuda.synchronize()
    assert base.interventions is None and base.certificate is None and base.shield_threshold is None
    assert sh.shield_threshold == INF and sh.members == base.members
    assert_same(base, sh)
    assert sh.interventions.dtype == torch.bool and sh.certificate.dtype == torch.float32
    assert sh.interventions.shape == sh.certificate.shape == sh.rewards.shape
    assert not bool(sh.interventions.any())
    assert torch.equal(sh.certificate != 0, sh.mask)
    return sh


def check_threshold_minus_inf(alg, **kw):
    """Everything alive intervenes: the member path sees the selected action and nothing
    else (the replay under the run's own actions, K = H), and the action is the safe actor's."""
    im = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), shield=-INF, **kw)
    torch.cuda.synchronize()
    assert torch.equal(im.interventions, im.mask)
    assert torch.equal(im.certificate != 0, im.mask)
    check_replay_and_safe_action(alg, im, **kw)
    return im


@pytest.mark.parametrize('rpt', [16, 32])
def test_threshold_plus_inf_is_the_unshielded_run_bit_for_bit(rpt):
    sh = check_threshold_plus_inf(_scene(rpt))
    _assert_every_length(sh)


@pytest.mark.parametrize('rpt', [16, 32])
def test_threshold_minus_inf_takes_the_safe_action_everywhere(rpt):
    im = check_threshold_minus_inf(_scene(rpt))
    _assert_every_length(im)


# ------------------------------------------------------------------ 3. teacher-forced against the oracle
def oracle_open_loop(P, alg, s, eps_a, eps_m, thr):
    """The oracle alone, open loop: policy -> certificate -> select -> ens_forward1 -> env
    functions. Per step (alive, intervening, not intervening, within the margin of thr)."""
    fn = O.env_fns('quadrotor')
    alive = torch.ones(len(s), dtype=torch.bool)
    counts = []
    for t in range(H):
        a_perf, q, a_safe = oracle_shield_step(P, alg, s, eps_a[t])
        iv = q > thr
        near = (q - thr).abs() <= 2 * _tol(q)
        a = torch.where(iv.unsqueeze(1), a_safe, a_perf)
        mean, lv = O.ens_forward1(P, PRE, s, a, MEMBER)
        s = (mean + torch.exp(lv).sqrt() * eps_m[t])[:, :-1]
        done = torch.as_tensor(np.asarray(fn(s)[0])).reshape(-1).bool()
        counts.append((int(alive.sum()), int((alive & iv).sum()), int((alive & ~iv).sum()), int((alive & near).sum())))
        alive = alive & ~done
    return counts


def test_threshold_inside_the_range_teacher_forced_against_the_oracle():
    """Recorded draws (eps_layout 1), member 3, thr = the median over the 72 start states of
    the oracle's certificate at step 0; every step checked from the kernel's own states.

    The scene as it is (raw initial critic weights, nothing scaled) meets both conditions on
    the inputs. The CPU oracle alone, open loop (alive, intervening, not intervening, within
    2 * (2e-4 + 2e-4 |q|) of thr): step 0 (72, 36, 36, 1), step 1 (65, 30, 35, 0), step 2
    (55, 22, 33, 3); thr 1.9230, the certificate spans 1.834 .. 2.028 over the start states
    (standard deviation 0.036)."""
    alg = _alg16()
    P = _params(alg)
    s, eps_a, eps_m = _teacher_inputs(alg)
    thr = float(oracle_shield_step(P, alg, s, eps_a[0])[1].median())
    counts = oracle_open_loop(P, alg, s, eps_a, eps_m, thr)
    print('oracle open loop:', counts, 'thr', thr)
    for n, iv, niv, near in counts:          # conditions on the inputs, not measurements
        assert iv >= 0.1 * n and niv >= 0.1 * n, counts
    assert sum(c[3] for c in counts) <= 0.1 * sum(c[0] for c in counts), counts

    im = ops.rollout_trajectories(alg, alg.actor, s.to(DEV), drpo_amd.DeviceNoise(5), members=MEMBER,
                                  eps_a=eps_a.to(DEV).contiguous(), eps_m=eps_m.to(DEV).contiguous(), eps_layout=1,
                                  shield=thr)
    torch.cuda.synchronize()
    assert im.shield_threshold == thr
    cert, iv_k, acts, mask = im.certificate.cpu(), im.interventions.cpu(), im.actions.cpu(), im.mask.cpu()
    assert torch.equal(iv_k, cert > thr)                     # the kernel's own values, every row
    assert not bool(cert[~mask].any()) and not bool(iv_k[~mask].any())
    excluded = alive_pairs = 0
    for t in range(H):
        live = mask[:, t]
        a_perf, q, a_safe = oracle_shield_step(P, alg, im.states[:, t].cpu(), eps_a[t])
        err = (cert[:, t] - q).abs()[live]
        assert bool((err <= _tol(q)[live]).all()), (t, float(err.max()))
        clear = live & ((q - thr).abs() > 2 * _tol(q))
        assert torch.equal(iv_k[:, t][clear], (q > thr)[clear]), t
        excluded += int((live & ~clear).sum())
        alive_pairs += int(live.sum())
        n_iv = int(iv_k[:, t][live].sum())
        assert n_iv >= 0.1 * int(live.sum()) and int(live.sum()) - n_iv >= 0.1 * int(live.sum()), (t, n_iv)
        ref = torch.where(iv_k[:, t].unsqueeze(1), a_safe, a_perf)
        aerr = (acts[:, t] - ref).abs()[live]
        print(f'step {t}: alive {int(live.sum())}, intervening {n_iv}, certificate max |d| {float(err.max()):.3g}, '
              f'action max |d| {float(aerr.max()):.3g}')
        assert bool((aerr <= _tol(ref)[live]).all()), (t, float(aerr.max()))
    assert excluded <= 0.1 * alive_pairs, (excluded, alive_pairs)
    assert int((im.lengths < H).sum()) >= 1, 'no row ended before the horizon'


# ------------------------------------------------------------------ 4. the other paths
def test_constraint_program_env(monkeypatch):
    """PG x SH: the quadrotor through its constraint program (env id 4)."""
    _no_host_env(monkeypatch)
    with monkeypatch.context() as mp:
        mp.setattr(envs, 'ShapeEnv', ProgramQuadrotor)
        alg = _drifting_quadrotor_alg(16)
    assert alg.env_params['env_id'] == 4
    sh = check_threshold_plus_inf(alg)
    _assert_every_length(sh)
    check_certificate_at_step_0(alg, sh, alg.solver.distributional_qc)
    check_threshold_minus_inf(alg)


def test_generic_widths():
    """Actor, critic and model 64 wide on the point robot (C = 1): the runtime-K layers,
    neither the paired heads nor the LDS-resident actor; 40 start states (two full tiles
    and one of 8)."""
    alg = _width_alg('point-robot', 64, 64)
    rep = _fill(alg, 'point-robot', 8000, 3)
    m = alg.model_ensemble
    mean, std = O.normalizer_fit(torch.from_numpy(rep['states']))
    m.state_normalizer.mean.copy_(mean)
    m.state_normalizer.std.copy_(std)
    m._elite_inds = [2, 0, 1]
    cc = alg.constraint_critic
    assert cc.hidden_dim != 256 and cc.output_dim == 1
    assert m.hidden_dim != 200 and alg.actor.spec.dims[1] != 256
    s40 = alg.replay_buffer.get('states')[::200].clone()
    assert len(s40) == 40
    sh = check_threshold_plus_inf(alg, states=s40)
    assert sh.certificate.shape == (40, alg.horizon)
    check_certificate_at_step_0(alg, sh, alg.solver.distributional_qc)
    check_threshold_minus_inf(alg, states=s40)


def test_mean_only_certificate(monkeypatch):
    """distributional_qc = False: the certificate is the mean head's maximum, no log-std head."""
    alg = _alg16()
    monkeypatch.setattr(alg.solver, 'distributional_qc', False)
    sh = check_threshold_plus_inf(alg)
    check_certificate_at_step_0(alg, sh, alg.solver.distributional_qc)
    check_threshold_minus_inf(alg)
    monkeypatch.undo()
    dist = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), shield=INF, members=sh.members)
    live = sh.mask
    assert bool((dist.certificate[live] > sh.certificate[live]).all())      # the bound adds std_ratio * std > 0


def test_members_each():
    """members='each': one launch per elite member with common draws, stacked; each slice
    is the single-member call. The threshold is any value inside the certificate's range."""
    alg = _alg16()
    probe = alg.imagine(noise=drpo_amd.DeviceNoise(77), shield=INF, members=MEMBER)
    thr = float(probe.certificate[:, 0].median())
    each = alg.imagine(members='each', noise=drpo_amd.DeviceNoise(77), shield=thr)
    E = len(alg.model_ensemble._elite_inds)
    assert each.states.shape == (E, B, H + 1, alg.state_dim)
    assert each.interventions.shape == each.certificate.shape == (E, B, H)
    assert each.interventions.dtype == torch.bool and each.shield_threshold == thr
    for k, member in enumerate(alg.model_ensemble._elite_inds):
        one = alg.imagine(members=int(member), noise=drpo_amd.DeviceNoise(77), shield=thr)
        for name in TENSORS:
            assert torch.equal(bits(getattr(each, name)[k]), bits(getattr(one, name))), (k, name)
        assert torch.equal(each.interventions[k], one.interventions)
        assert torch.equal(bits(each.certificate[k]), bits(one.certificate))
        n_iv, n_live = int(one.interventions[:, 0].sum()), B
        assert 0 < n_iv < n_live, (k, n_iv)


# ------------------------------------------------------------------ 5. refusals
def test_refusals(monkeypatch):
    alg = _alg16()
    A = alg.action_dim
    assert alg.imagine(shield=None).interventions is None
    assert alg.imagine(shield=False).interventions is None
    assert alg.imagine(shield=True).shield_threshold == alg.safe_shield_threshold
    with pytest.raises(ValueError, match='shield with actions'):
        alg.imagine(actions=torch.zeros(B, 1, A, device=DEV), shield=True)
    with pytest.raises(ValueError, match='shield with a recorded tape'):
        alg.imagine(noise=drpo_amd.TapeNoise([]), shield=0.0)
    narrow = SquashedGaussianPolicy.create(alg.state_dim, A, 64, 2, 'actor_safe_64', DEV)
    monkeypatch.setattr(alg.solver, 'actor_safe', narrow)
    with pytest.raises(ValueError, match='safe actor'):
        alg.imagine(shield=True)
