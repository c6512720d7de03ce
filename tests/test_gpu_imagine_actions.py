"""Imagined rollouts under given actions (SMBPO.imagine(actions=), ops.rollout_trajectories,
drpo_rollout_trajectories_given: the GA instantiations of rollout_persist_kernel) and the
k-step open-loop model error built on them (SMBPO.model_rollout_error).

Tolerances: between calls of the kernel everything is compared bit for bit (float32 as
int32). Against the oracle's member forward |d| <= 2e-4 + 2e-4 |ref|, the oracle tolerance
of test_gpu_imagine.py; constraint values to 1e-6 as there. The one-step error against
model_ensemble.means: the project's forward tolerance 1e-4 + 1e-4 |ref| on each predicted
component, carried through the error norm by the triangle inequality.

Tests 3 and 5 run imagine_helpers._action_scene (its docstring says how the scene makes the
actions matter). Counts of the CPU oracle alone (open loop from the start states, member 3,
actions and draws as in the tests) are in the tests' docstrings."""
import numpy as np
import pytest
import torch

import drpo_amd
from drpo_amd import envs, ops
from drpo_amd.sampling import episode_segments
from gpu_helpers import DEV, ProgramQuadrotor, _drifting_quadrotor_alg, _fill, _no_host_env, _width_alg
from imagine_helpers import (B, EP2_LEN, EP_LEN, H, MEMBER, PRE, TENSORS, _action_scene, _assert_every_length,
                             _episode_inputs, assert_same, bits)
from oracle import drpo_oracle as O

pytestmark = pytest.mark.gpu


def _replay_equal(alg, ks, noise_seed=1234, **kw):
    """imagine, then imagine again under its own first K actions: the same trajectories."""
    im = alg.imagine(noise=drpo_amd.DeviceNoise(noise_seed), **kw)
    torch.cuda.synchronize()
    assert im.given_steps == 0
    for K in ks:
        re = alg.imagine(actions=im.actions[:, :K].contiguous(), members=im.members,
                         noise=drpo_amd.DeviceNoise(noise_seed), **kw)
        torch.cuda.synchronize()
        assert re.given_steps == K and re.members == im.members
        assert_same(im, re)
    return im


# ------------------------------------------------------------------ 1. replay, bit for bit
@pytest.mark.parametrize('rpt', [16, 32])
def test_replay_under_own_actions_bit_for_bit(rpt):
    """K = 3: no actor in the whole horizon (and no LDS-resident actor weights at 16-row
    tiles). K = 1, 2: the switch back to the actor, whose draws must not have moved."""
    alg = _drifting_quadrotor_alg(rpt)
    im = _replay_equal(alg, [1, 2, 3])
    _assert_every_length(im)
    assert im.states.shape == (B, H + 1, alg.state_dim)


def test_replay_under_own_actions_constraint_program(monkeypatch):
    _no_host_env(monkeypatch)
    with monkeypatch.context() as mp:
        mp.setattr(envs, 'ShapeEnv', ProgramQuadrotor)
        alg = _drifting_quadrotor_alg(16)
    assert alg.env_params['env_id'] == 4
    _assert_every_length(_replay_equal(alg, [2]))


# ------------------------------------------------------------------ 2. generic widths
def test_replay_under_own_actions_generic_widths():
    """Actor 64, model 64: neither the paired heads nor the LDS-resident actor."""
    alg = _width_alg('point-robot', 64, 64)
    rep = _fill(alg, 'point-robot', 8000, 3)
    m = alg.model_ensemble
    mean, std = O.normalizer_fit(torch.from_numpy(rep['states']))
    m.state_normalizer.mean.copy_(mean)
    m.state_normalizer.std.copy_(std)
    m._elite_inds = [2, 0, 1]
    assert m.hidden_dim != 200 and alg.actor.spec.dims[1] != 256
    s40 = alg.replay_buffer.get('states')[::200].clone()          # two full tiles and one of 8
    assert len(s40) == 40
    Hw = alg.horizon
    im = _replay_equal(alg, [1, Hw], states=s40)
    assert im.actions.shape == (40, Hw, alg.action_dim) and bool(im.actions.abs().sum() > 0)


# ------------------------------------------------------------------ 3. the actions drive the model
def _teacher_inputs(rep):
    """72 start states over the whole z range, actions uniform in [-1, 1), model draws."""
    g = torch.Generator().manual_seed(7)
    s = torch.from_numpy(rep['states'][2:400:5][:B].copy())
    a = torch.rand(B, H, 2, generator=g) * 2 - 1
    eps_m = 0.02 * torch.randn(H, B, s.shape[1] + 1, generator=g)
    return s, a, eps_m


def oracle_open_loop(P, s, a, m, eps_m=None):
    """The oracle alone, open loop: per step (rows alive at its start, rows done in it)."""
    fn = O.env_fns('quadrotor')
    alive = torch.ones(len(s), dtype=torch.bool)
    counts, states = [], [s]
    for t in range(a.shape[1]):
        mean, lv = O.ens_forward1(P, PRE, s, a[:, t], m)
        x = mean if eps_m is None else mean + torch.exp(lv).sqrt() * eps_m[t]
        s = x[:, :-1]
        done = torch.as_tensor(np.asarray(fn(s)[0])).reshape(-1).bool()
        counts.append((int(alive.sum()), int((alive & done).sum())))
        alive = alive & ~done
        states.append(s)
    return counts, states


_SCENE = {}


def _scene():
    if not _SCENE:
        _SCENE['v'] = _action_scene(DEV)
    return _SCENE['v']


def _check_teacher_forced(alg, P, re, s, a, eps_m):
    S, C = alg.state_dim, alg.con_dim
    length = re.lengths.cpu()
    assert torch.equal(bits(re.states[:, 0]), bits(s))
    acts = re.actions.cpu()
    for t in range(H):
        live = length > t
        assert int(live.sum()) >= 16, (t, int(live.sum()))
        assert torch.equal(bits(acts[live, t]), bits(a[live, t])), t
        assert not acts[~live, t].any(), t
        st = re.states[:, t].cpu()
        mean, lv = O.ens_forward1(P, PRE, st, a[:, t], MEMBER)
        ref = mean if eps_m is None else mean + torch.exp(lv).sqrt() * eps_m[t]
        got = torch.cat([re.states[:, t + 1].cpu(), re.rewards[:, t].cpu().unsqueeze(1)], dim=1)
        err = (got - ref).abs()[live]
        print(f'step {t}: alive {int(live.sum())}, max |d| {float(err.max()):.3g}')
        assert bool((err <= 2e-4 + 2e-4 * ref.abs()[live]).all()), (t, float(err.max()))
        done, viol, h = alg.check_constraints(re.states[:, t + 1])
        lv_ = live.to(DEV)
        assert torch.equal(done[lv_], re.dones[:, t][lv_]) and torch.equal(viol[lv_], re.violations[:, t][lv_])
        np.testing.assert_allclose(re.constraint_values[:, t][lv_].cpu().numpy(),
                                   h.reshape(len(s), C)[lv_].cpu().numpy(), rtol=0, atol=1e-6)
    assert int((length < H).sum()) >= 1, 'no row ended before the horizon'


def test_given_actions_drive_the_member_forward():
    """imagine(states, actions, member 3, model_noise=False) against the oracle's member
    forward, step by step on the kernel's own states (teacher-forced).

    The CPU oracle alone, open loop (alive at the start of the step, done in it):
    step 0 (72, 10), step 1 (62, 14), step 2 (48, 20); a against -a moves a row's next
    state by 0.045 (largest component, mean over the rows)."""
    alg, rep, P = _scene()
    s, a, _ = _teacher_inputs(rep)
    counts, _ = oracle_open_loop(P, s, a, MEMBER)
    assert all(n >= 16 for n, _ in counts) and sum(d for _, d in counts[:-1]) >= 1, counts
    sd, ad = s.to(DEV), a.to(DEV)
    re = alg.imagine(states=sd, actions=ad, members=MEMBER, model_noise=False)
    free = alg.imagine(states=sd, members=MEMBER, model_noise=False)
    torch.cuda.synchronize()
    assert re.given_steps == H and free.given_steps == 0
    _check_teacher_forced(alg, P, re, s, a, None)
    assert not torch.equal(re.states, free.states)
    # other actions, other trajectories: the model reads them
    other = alg.imagine(states=sd, actions=-ad, members=MEMBER, model_noise=False)
    live = (re.lengths > 0) & (other.lengths > 0)
    d = (re.states[:, 1] - other.states[:, 1]).abs().amax(dim=1)[live]
    assert float(d.mean()) > 50 * 2e-4, float(d.mean())


def test_given_actions_with_recorded_model_draws():
    """The same with model noise from recorded draws (eps_layout 1): the oracle step is
    mean + exp(lv).sqrt() * eps_m[t].

    The CPU oracle alone, open loop: step 0 (72, 8), step 1 (64, 17), step 2 (47, 23)."""
    alg, rep, P = _scene()
    s, a, eps_m = _teacher_inputs(rep)
    counts, _ = oracle_open_loop(P, s, a, MEMBER, eps_m)
    assert all(n >= 16 for n, _ in counts) and sum(d for _, d in counts[:-1]) >= 1, counts
    eps_a = torch.zeros(H, B, alg.action_dim, device=DEV)
    re = ops.rollout_trajectories(alg, alg.actor, s.to(DEV), drpo_amd.DeviceNoise(5), members=MEMBER, eps_a=eps_a,
                                  eps_m=eps_m.to(DEV).contiguous(), eps_layout=1, actions=a.to(DEV))
    torch.cuda.synchronize()
    assert re.given_steps == H
    _check_teacher_forced(alg, P, re, s, a, eps_m)


# ------------------------------------------------------------------ 4. small and odd
def test_small_and_odd_shapes_and_side_effects(monkeypatch):
    alg = _drifting_quadrotor_alg(16)
    S, A = alg.state_dim, alg.action_dim
    alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(9))       # the buffer holds rows, its pointer is not 0
    torch.cuda.synchronize()
    vb = alg.virt_buffer._module
    before = {f: getattr(vb, f).clone() for f in ops._VB_FIELDS}
    n_before, steps_before = len(alg.virt_buffer), int(alg.steps_sampled)
    assert n_before > 0
    replay = alg.replay_buffer.get('states')
    g = torch.Generator().manual_seed(3)

    s5 = replay[[0, 100, 200, 300, 399]].clone()
    a5 = (torch.rand(5, A, generator=g) * 2 - 1).to(DEV)
    x = alg.imagine(states=s5, actions=a5, horizon=1, noise=drpo_amd.DeviceNoise(5))          # [B, A]: K = 1
    y = alg.imagine(states=s5, actions=a5.reshape(5, 1, A), horizon=1, noise=drpo_amd.DeviceNoise(5))
    z = alg.imagine(states=s5, actions=a5.cpu().numpy(), horizon=1, noise=drpo_amd.DeviceNoise(5))
    torch.cuda.synchronize()
    assert x.given_steps == y.given_steps == z.given_steps == 1
    assert x.states.shape == (5, 2, S) and x.actions.shape == (5, 1, A)
    assert torch.equal(bits(x.actions[:, 0]), bits(a5)) and torch.equal(bits(x.states[:, 0]), bits(s5))
    assert (x.lengths == 1).all() and 0 < int(x.terminated.sum()) < 5
    assert_same(x, y)
    assert_same(x, z)

    # replay start states: rollout_batch_size rows of actions
    aB = (torch.rand(B, 2, A, generator=g) * 2 - 1).to(DEV)
    r1 = alg.imagine(actions=aB, noise=drpo_amd.DeviceNoise(21))
    r0 = alg.imagine(noise=drpo_amd.DeviceNoise(21))
    torch.cuda.synchronize()
    assert r1.given_steps == 2 and r1.states.shape == (B, H + 1, S)
    assert torch.equal(bits(r1.states[:, 0]), bits(r0.states[:, 0]))     # the same draw of start states
    live = r1.mask[:, :2]
    assert torch.equal(bits(r1.actions[:, :2][live]), bits(aB[live])) and not bool(r1.actions[:, :2][~live].any())
    assert set(r1.lengths.cpu().tolist()) == {1, 2, 3}

    # members='each': elite k is the single-member call, the same actions for every member
    each = alg.imagine(actions=aB, members='each', noise=drpo_amd.DeviceNoise(77))
    assert each.given_steps == 2 and each.states.shape == (5, B, H + 1, S)
    for k, member in enumerate(alg.model_ensemble._elite_inds):
        one = alg.imagine(actions=aB, members=int(member), noise=drpo_amd.DeviceNoise(77))
        for name in TENSORS:
            assert torch.equal(bits(getattr(each, name)[k]), bits(getattr(one, name))), (k, name)
    alg.imagine(actions=aB, deterministic=True, model_noise=False)

    with pytest.raises(ValueError, match='1 <= K <= horizon 3'):
        alg.imagine(actions=torch.zeros(B, H + 1, A, device=DEV))
    with pytest.raises(ValueError, match='5 rows for 72 trajectories'):
        alg.imagine(actions=a5)
    with pytest.raises(ValueError, match='71 rows for 72 trajectories'):
        alg.imagine(actions=aB[:71].contiguous())
    with pytest.raises(ValueError, match='is not \\[B, K, 2\\]'):
        alg.imagine(actions=torch.zeros(B, 2, A + 1, device=DEV))
    with pytest.raises(ValueError, match='tape'):
        alg.imagine(actions=aB, noise=drpo_amd.TapeNoise([]))
    torch.cuda.synchronize()
    for f in ops._VB_FIELDS:
        assert torch.equal(getattr(vb, f), before[f]), f
    assert len(alg.virt_buffer) == n_before and int(alg.steps_sampled) == steps_before

    monkeypatch.setattr(alg, 'env_params', None)             # an env on the host round trip
    with pytest.raises(NotImplementedError, match='ConstraintProgram'):
        alg.imagine(actions=aB)
    with pytest.raises(NotImplementedError, match='ConstraintProgram'):
        alg.model_rollout_error(1)


# ------------------------------------------------------------------ 5. model_rollout_error
def test_model_rollout_error_on_episodes_the_model_made():
    """The replay is the model's own: an episode of 12 steps and one of 6 imagined under
    member 3 without model noise, appended to the 400 unlinked synthetic rows. Open loop
    from any of their states under the same member and actions, the same kernel gives the
    same bits: errors exactly 0.

    The scene's weights are scaled by 3 here, not 6: at 6 the model amplifies z along its
    own trajectory and no row lives 12 steps. The CPU oracle alone: the 12-step row is alive
    at every step, its largest constraint value over the 12 steps is -0.196 (z climbs from
    0.65 to 1.22); members 0 and 3 differ by 0.009 in the first next state."""
    alg, rep, P = _action_scene(DEV, scale=3.0)
    s0, seq = _episode_inputs(rep)
    counts, _ = oracle_open_loop(P, s0[:1], seq[:1], MEMBER)
    assert all(c == (1, 0) for c in counts), counts
    n0 = len(alg.replay_buffer)
    for i, n in ((0, EP_LEN), (1, EP2_LEN)):
        im = alg.imagine(states=s0[i:i + 1].to(DEV), actions=seq[i:i + 1, :n].contiguous().to(DEV), members=MEMBER,
                         model_noise=False, horizon=n)
        assert int(im.lengths[0]) == n and not bool(im.terminated[0])
        alg.replay_buffer.extend(states=im.states[0, :n], actions=im.actions[0], next_states=im.states[0, 1:],
                                 rewards=im.rewards[0], dones=im.dones[0], violations=im.violations[0],
                                 constraint_values=im.constraint_values[0])
    buf = alg.replay_buffer.get(as_dict=True)
    starts = episode_segments(buf['states'], buf['next_states'], buf['dones'], 4)
    assert starts.tolist() == [n0 + i for i in range(EP_LEN - 3)] + [n0 + EP_LEN + i for i in range(EP2_LEN - 3)]
    sd_before = {k: v.clone() for k, v in alg.state_dict().items()}
    vb_len, steps = len(alg.virt_buffer), int(alg.steps_sampled)

    r = alg.model_rollout_error(horizon=4, members=MEMBER)
    torch.cuda.synchronize()
    assert torch.equal(r.starts.cpu(), starts.cpu())
    assert r.imagined.given_steps == 4 and r.imagined.members == [MEMBER] * 4
    assert r.state_error.shape == r.reward_error.shape == r.alive.shape == (len(starts), 4)
    assert bool(r.alive.all())
    assert bool((r.state_error == 0).all()) and bool((r.reward_error == 0).all())
    assert bool((r.deciles(3) == 0).all()) and r.deciles(3).shape == (11,)

    other = alg.model_rollout_error(horizon=4, members=0)
    assert bool(other.alive[:, 0].all()) and bool((other.state_error[:, 0] > 0).all())
    assert float(other.deciles(0)[0]) > 0 and other.deciles(3).shape == (11,)

    each = alg.model_rollout_error(horizon=4, members='each', max_segments=5)
    assert each.state_error.shape == (5, 5, 4)
    assert each.starts.tolist() == [starts[(i * 12) // 5].item() for i in range(5)]
    assert bool((each.state_error[0] == 0).all())                             # elite 0 is member 3
    assert bool((each.state_error[1][each.alive[1]] > 0).all())

    with pytest.raises(ValueError, match='no episode segment of 13 steps'):
        alg.model_rollout_error(horizon=13)
    for k, v in alg.state_dict().items():                                     # nothing of the training state moved
        assert torch.equal(v, sd_before[k]), k
    assert len(alg.virt_buffer) == vb_len and int(alg.steps_sampled) == steps


def test_model_rollout_error_one_step_is_the_evaluate_models_error():
    """horizon 1 on the random replay: every row is a segment, 72 evenly spaced ones are
    kept, and the error is evaluate_models' (src/smbpo.py:327-336) for that member."""
    alg, rep, P = _scene()
    r = alg.model_rollout_error(horizon=1, members=MEMBER)
    torch.cuda.synchronize()
    n = len(alg.replay_buffer)
    assert r.starts.tolist() == [(i * n) // B for i in range(B)]
    states, actions, next_states = alg.replay_buffer.get('states', 'actions', 'next_states')
    state_std = states.std(dim=0)
    state_std[state_std < 1e-7] = 1.0
    with torch.no_grad():
        pred = alg.model_ensemble.means(states, actions)[0][MEMBER]
    scale = state_std + 1e-7
    want = torch.norm((pred - next_states) / scale, dim=1)[r.starts]
    bound = torch.norm((1e-4 + 1e-4 * pred.abs()) / scale, dim=1)[r.starts]
    alive = r.alive[:, 0]
    assert int(alive.sum()) >= 16
    err = (r.state_error[:, 0] - want).abs()
    print('one-step error: max |d|', float(err[alive].max()), 'smallest bound', float(bound.min()))
    assert bool((err[alive] <= bound[alive]).all()), float(err[alive].max())
    assert bool(torch.isnan(r.state_error[:, 0][~alive]).all())
