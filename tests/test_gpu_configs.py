"""HIP path vs the CPU oracle at the EXACT BASELINE config shapes:

  config 1  cartpole     E=3  H=5  B=256
  config 2  quadrotor    E=7  H=10 B=4096
  config 3  point-robot  E=7  H=20 B=8192
  config 4  tracking     E=8  H=40 B=16384
  config 5  quadrotor    E=32 H=80 B=65536   (global batch, on one GPU here)

Per config, with reference default widths (actor/critics 256, model 200) and the
env's reference JSON hyper-parameters:

* a full rollout (B x H) by the production fused-horizon engine vs the oracle driven
  by live reference RNG calls (the recorded draws re-indexed by original row).
  Regime: the diff head's state rows are scaled by 1e-3 (the reward row keeps full
  scale, so the whole member MLP is exercised through it) and the log-var bias is
  -20 (std clamps to e^-5): trajectories drift slowly and (almost) no row finishes,
  so a threshold-straddling fp32 rounding -- which at 5.2 M transitions with rows
  dying every step would flip some done flag -- is practically excluded; the row
  count must still equal the oracle's exactly;
* the same shape with the raw random weights (rows die every step): structural
  properties of the HIP output (per-step survivor chaining in reference order,
  flags == the env constraint functions of next_state, action bounds);
* the same shape with the raw random weights, TEACHER-FORCED against the oracle:
  every horizon step of the production fused engine (16- or 32-row tiles, ordered
  emit) is compared with one oracle step started from the HIP's own states of that
  step (a sample of <= 2048 rows per step, all rows' ordering by survivor chaining),
  so the member MLP's state outputs are checked at full scale while rows die,
  without divergence accumulating over the horizon;
* one update_critic + update_actor_and_alpha + update_multiplier at the full B vs
  the oracle with its draws replayed;
* a full-width (hidden 200) fit(steps=3) at the config's E vs the oracle.

Tolerances (fp32): rollout floats |d| <= 2e-4 + 2e-4|ref|; violation flags exact
except where the oracle's constraint value is within 1e-5 of 0 (the flag is that
value's sign); losses rtol 1e-4 (2e-4 at B=65536); parameters after one Adam step
|d| <= 3e-5 + 1e-4|ref| (elements whose reference gradient sign is below fp32
noise: |d| <= 2 lr, at most 1e-4 of all elements); fit losses rtol 1e-4, fit parameters |d| <= 5e-5 + 2e-4|ref|,
elites exact.
"""
import numpy as np
import pytest
import torch

import bench
import drpo_amd
from fake_envs import ENVS
from gpu_helpers import DEV, COMP, _fill, original_row_tape
from oracle import drpo_oracle as O

pytestmark = pytest.mark.gpu

CFGS = [1, 2, 3, 4, 5]


def _alg(c, B=None, seed=5):
    cd = bench.CONFIGS[c]
    env = cd['env']
    B = B or cd['B']
    torch.manual_seed(seed)
    alg = bench.make_alg(DEV, B, cd['H'], cd['E'], seed, bench.ENV_JSON[env], env=env)
    return alg, cd


def _oracle_threads():
    torch.set_num_threads(max(4, min(16, torch.get_num_threads() * 4)))


def _close(got, ref, tol, msg):
    g = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    r = ref.detach().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert g.shape == r.shape, (msg, g.shape, r.shape)
    bad = np.abs(g.astype(np.float64) - r) > tol + tol * np.abs(r)
    assert not bad.any(), (msg, int(bad.sum()), float(np.abs(g - r).max()))


@pytest.mark.parametrize('c', CFGS)
def test_config_rollout_vs_oracle(c):
    alg, cd = _alg(c)
    env, B, H = cd['env'], cd['B'], cd['H']
    rep = _fill(alg, env, 100000, 3)
    m = alg.model_ensemble
    st = torch.from_numpy(rep['states'])
    mean, std = O.normalizer_fit(st)
    m.state_normalizer.mean.copy_(mean)
    m.state_normalizer.std.copy_(std)
    _, diff, logv = m.views()
    S = alg.state_dim
    diff[-1][0][:, :S].mul_(1e-3)
    diff[-1][1][:, :S].mul_(1e-3)
    logv[-1][1].fill_(-20.0)
    E = m.ensemble_size
    m._elite_inds = sorted({0, E // 2, E - 1, 1, E - 2})[:min(5, E)]
    sd = {k: v.detach().cpu() for k, v in alg.state_dict().items()}
    P = {k[len('solver.'):]: v for k, v in sd.items() if k.startswith('solver.actor.')}
    P.update({k: v for k, v in sd.items() if k.startswith('model_ensemble.')})
    _oracle_threads()
    torch.manual_seed(c)
    live = O.LiveRNG()
    ref = O.rollout(P, 'actor.net.', 'model_ensemble.', m._elite_inds, st, env, B, H, live)
    n = len(ref['states'])
    assert n >= 0.95 * B * H, 'regime: (almost) no row may finish'
    tape = drpo_amd.TapeNoise(original_row_tape(live.entries, ref, B))
    del live
    from drpo_amd import ops
    out = ops.rollout(alg, alg.actor, None, tape, eps_layout=1)
    torch.cuda.synchronize()
    assert tape.done()
    assert len(out) == n
    got = out.get(as_dict=True)
    for k in ('states', 'actions', 'next_states', 'rewards', 'constraint_values'):
        _close(got[k], ref[k].reshape(got[k].shape), 2e-4, f'config {c} {k}')
    assert torch.equal(got['dones'].cpu(), ref['dones'])
    hv = ref['constraint_values'].reshape(n, -1)
    marginal = (hv.abs() < 1e-5).any(1)
    vg, vr = got['violations'].cpu(), ref['violations']
    assert torch.equal(vg[~marginal], vr[~marginal]), f'config {c} violations'


def _dying_rows_properties(alg, env, B, H):
    """Raw random weights: rows finish at every step. The output must chain: step t+1's
    states are step t's next_states of the rows that did not finish, in order."""
    _fill(alg, env, 100000, 4)
    m = alg.model_ensemble
    m.state_normalizer.fit(alg.replay_buffer.get('states'))
    m._elite_inds = list(range(min(5, m.ensemble_size)))
    out = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(99, rank=0))
    torch.cuda.synchronize()
    n = len(out)
    got = out.get(as_dict=True)
    assert B <= n <= B * H
    d = got['dones'].cpu().numpy()
    start, alive = 0, B
    steps = 0
    while start < n:
        seg = slice(start, start + alive)
        nd = ~d[seg]
        nxt = int(nd.sum())
        if start + alive < n:
            assert torch.equal(got['states'][start + alive:start + alive + nxt], got['next_states'][seg][nd]), \
                f'step {steps} survivors'
        start += alive
        alive = nxt
        steps += 1
        if alive == 0:
            break
    assert start == n and steps <= H
    from drpo_amd import ops
    dn, vl, h = ops.env_constraints(alg.env_params, got['next_states'])
    assert torch.equal(dn, got['dones']) and torch.equal(vl, got['violations'])
    assert torch.equal(h, got['constraint_values'])
    assert (got['actions'].abs() <= 1).all() and torch.isfinite(got['next_states']).all()


@pytest.mark.parametrize('c', CFGS)
def test_config_rollout_dying_rows_properties(c):
    alg, cd = _alg(c, seed=7)
    _dying_rows_properties(alg, cd['env'], cd['B'], cd['H'])


def test_rollout_dying_rows_scan_emit_small():
    """The scan + emit + finalize tail at its smallest shape: quadrotor, E = 7, B = 4100 in
    16-row tiles (257 tiles, the last with 4 rows), H = 32: 257 x 32 = 8224 counts, just
    above the single-launch emit's 8192. Rows die within a few steps, so whole tiles exit
    early and leave zeroed later counts."""
    env, B, H = 'quadrotor', 4100, 32
    torch.manual_seed(7)
    alg = bench.make_alg(DEV, B, H, 7, 7, bench.ENV_JSON[env], env=env)
    _dying_rows_properties(alg, env, B, H)


def _sac_batch(alg, env, jsn, B, seed):
    rng = np.random.RandomState(seed)
    rep = bench.synth_replay(env, 20000, rng, DEV, alg.env_params)
    idx = rng.randint(0, 20000, B)
    C = alg.con_dim
    h = torch.from_numpy(rep['constraint_values'])[idx].reshape(B, -1) * jsn.get('constraint_scale', 10.0)
    h = h + (h > 0).float() * jsn.get('constraint_offset', 0.0)
    d = torch.from_numpy(rep['dones'])[idx]
    batch = (torch.from_numpy(rep['states'])[idx], torch.from_numpy(rep['actions'])[idx],
             torch.from_numpy(rep['next_states'])[idx],
             torch.from_numpy(rep['rewards'])[idx] * jsn['reward_scale'] + jsn['alive_bonus'],
             d, torch.from_numpy(rep['violations'])[idx], h if C > 1 else h[:, 0])
    return batch


def _eff_grads(orc):
    """Each parameter's last effective Adam gradient (clipped + coupled L2) in the oracle."""
    return {k: st['g'] for opt in orc.opt.values() for k, st in opt.items() if 'g' in st}


def _check_params(sol, P, msg, grads=None, lr=3e-4, atol=3e-5, rtol=1e-4):
    """Parameters after an Adam step vs the oracle. Adam's first step moves an element
    by ~lr * sign(g) whatever |g| is (for |g| >> eps), g = clipped grad + 1e-4 * param
    (coupled L2), so an element whose reference g is below fp32 summation noise
    (|g| <= 1e-3 * rms of its tensor's g, e.g. a gradient cancelling the weight-decay
    term) may legitimately differ by up to 2 lr; such elements are counted separately
    and must stay a tiny minority."""
    sd = sol.state_dict()
    bad, weak = [], 0
    for k, exp in P.items():
        if k not in sd:
            continue
        got, e = sd[k].detach().cpu().numpy(), exp.numpy()
        err = np.abs(got - e) - (atol + rtol * np.abs(e))
        fail = err > 0
        if fail.any() and grads is not None and k in grads:
            g = grads[k].numpy()
            rms = float(np.sqrt(np.mean(g.astype(np.float64) ** 2)))
            ill = np.abs(g) <= 1e-3 * rms
            ok = ill & (np.abs(got - e) <= 2.05 * lr + atol)
            weak += int((fail & ok).sum())
            fail &= ~ok
        if fail.any():
            bad.append((k, float(np.abs(got - e).max()), int(fail.sum()), e.size))
    assert not bad, f'{msg}: {bad[:6]}'
    total = sum(v.numel() for v in P.values())
    assert weak <= 1e-4 * total + 8, f'{msg}: {weak} ill-conditioned elements'
    if weak:   # reported in the run's warnings summary (the carve-out's count, per check)
        import warnings
        warnings.warn(f'{msg}: {weak} of {total} elements inside the 2 lr ill-conditioned carve-out')
    return weak


@pytest.mark.parametrize('c', CFGS)
def test_config_sac_update_vs_oracle(c):
    alg, cd = _alg(c)
    env, B = cd['env'], cd['B']
    jsn = bench.ENV_JSON[env]
    sol = alg.solver
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim
    sd = {k: v.detach().cpu().clone() for k, v in alg.state_dict().items()}
    Ps = {k[len('solver.'):]: v for k, v in sd.items() if k.startswith('solver.') and
          not k.startswith('solver.model_ensemble') and k != 'solver.total_updates'}
    sc = jsn['sac_cfg']
    orc = O.SSACOracle(Ps, dict(batch_size=B, target_entropy=sc['target_entropy'], penalty_lb=sc['penalty_lb'],
                                penalty_ub=sc['penalty_ub'], actor_lr=sc['actor_lr'], actor_lr_end=sc['actor_lr_end'],
                                std_ratio=sc['constraint_critic_cfg']['std_ratio'],
                                updates_per_training=sol.updates_per_training), C, A)
    batch = _sac_batch(alg, env, jsn, B, 4)
    dev_batch = [x.to(DEV) for x in batch]
    rtol = 2e-4 if B > 32768 else 1e-4
    lr_max = max(sol.critic_lr, sol.actor_lr, sol.multiplier_lr)   # earlier steps' deviations persist
    _oracle_threads()
    torch.manual_seed(c)
    live = O.LiveRNG()
    lq_ref, lqc_ref = orc.update_critic(*batch, live)
    tape = drpo_amd.TapeNoise(live.entries)
    lq, lqc = sol.update_critic(*dev_batch, noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    np.testing.assert_allclose(lq.item(), float(lq_ref), rtol=rtol)
    np.testing.assert_allclose(lqc.item(), float(lqc_ref), rtol=rtol)
    _check_params(sol, orc.P, f'config {c} after update_critic', _eff_grads(orc), lr_max)
    live = O.LiveRNG()
    orc.update_actor_and_alpha(batch[0], live)
    tape = drpo_amd.TapeNoise(live.entries)
    sol.update_actor_and_alpha(dev_batch[0], noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    np.testing.assert_allclose(sol.log_alpha.item(), float(orc.log_alpha), rtol=1e-5, atol=1e-6)
    _check_params(sol, orc.P, f'config {c} after update_actor_and_alpha', _eff_grads(orc), lr_max)
    live = O.LiveRNG()
    orc.update_multiplier(batch[0], live)
    tape = drpo_amd.TapeNoise(live.entries)
    sol.update_multiplier(dev_batch[0], noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    _check_params(sol, orc.P, f'config {c} after update_multiplier', _eff_grads(orc), lr_max)


@pytest.mark.parametrize('c', CFGS)
def test_config_full_width_fit_vs_oracle(c):
    alg, cd = _alg(c, B=256)
    env = cd['env']
    m = alg.model_ensemble
    assert m.hidden_dim == 200 and m.ensemble_size == cd['E']
    _fill(alg, env, 30000, 6)
    buf = {k: v.cpu() for k, v in alg.replay_buffer.get(as_dict=True).items()}
    P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _oracle_threads()
    torch.manual_seed(c)
    live = O.LiveRNG()
    opt = {}
    ref_losses, ref_elites = O.ens_fit(P, '', opt, buf, 3, m.ensemble_size, m.batch_size, m.holdout_size,
                                       m.num_elites, live)
    tape = drpo_amd.TapeNoise(live.entries)
    losses = m.fit(alg.replay_buffer, steps=3, noise=tape)
    assert tape.done()
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    assert m._elite_inds == ref_elites
    sd = m.state_dict()
    for k in O.ens_param_keys(P, ''):
        got, e = sd[k].cpu().numpy(), P[k].numpy()
        err = np.abs(got - e) - (5e-5 + 2e-4 * np.abs(e))
        assert not (err > 0).any(), (k, float(np.abs(got - e).max()))


def test_fit_head_hidden_layers_2_vs_oracle():
    """A model with head_hidden_layers=2 (a config option; the reference default is 1)
    is outside drpo_mlp_backward_ens's shapes: the fit must take the separate NLL launch
    + generic backward (FitPlan.fused, from drpo_ens_fit_paths), not raise from the fused one."""
    cd = bench.CONFIGS[2]
    torch.manual_seed(11)
    alg = bench.make_alg(DEV, 256, cd['H'], cd['E'], 11, bench.ENV_JSON[cd['env']], env=cd['env'],
                         extra={'model_cfg': {'head_hidden_layers': 2}})
    m = alg.model_ensemble
    assert m.head_hidden_layers == 2
    assert not m.engine.fit_plan().fused
    _fill(alg, cd['env'], 30000, 8)
    buf = {k: v.cpu() for k, v in alg.replay_buffer.get(as_dict=True).items()}
    P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _oracle_threads()
    live = O.LiveRNG()
    ref_losses, ref_elites = O.ens_fit(P, '', {}, buf, 3, m.ensemble_size, m.batch_size, m.holdout_size,
                                       m.num_elites, live)
    tape = drpo_amd.TapeNoise(live.entries)
    losses = m.fit(alg.replay_buffer, steps=3, noise=tape)
    assert tape.done()
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    assert m._elite_inds == ref_elites
    sd = m.state_dict()
    for k in O.ens_param_keys(P, ''):
        got, e = sd[k].cpu().numpy(), P[k].numpy()
        err = np.abs(got - e) - (5e-5 + 2e-4 * np.abs(e))
        assert not (err > 0).any(), (k, float(np.abs(got - e).max()))


_RAGGED = {}


def _ragged_case(env, hhl):
    """One model [hidden 200, E=2, batch = holdout = 20 rows] per (env, head_hidden_layers)
    with its start state and the oracle's fit(steps=2) from it, computed once."""
    key = (env, hhl)
    if key not in _RAGGED:
        torch.manual_seed(13)
        alg = bench.make_alg(DEV, 256, 5, 2, 13, bench.ENV_JSON[env], env=env,
                             extra={'model_cfg': {'ensemble_size': 2, 'num_elites': 2, 'batch_size': 20,
                                                  'holdout_size': 20, 'head_hidden_layers': hhl}})
        m = alg.model_ensemble
        assert (m.hidden_dim, m.ensemble_size, m.batch_size, m.holdout_size) == (200, 2, 20, 20)
        assert m.head_hidden_layers == hhl
        _fill(alg, env, 3000, 9)
        buf = {k: v.cpu() for k, v in alg.replay_buffer.get(as_dict=True).items()}
        P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        m.optimizer._ensure_state()
        start = [m.group.data.clone(), m.optimizer.m.clone(), m.optimizer.v.clone(), m.optimizer.step_count]
        _oracle_threads()
        live = O.LiveRNG()
        ref_losses, ref_elites = O.ens_fit(P, '', {}, buf, 2, 2, 20, 20, 2, live)
        _RAGGED[key] = (alg, start, P, ref_losses, ref_elites, live.entries)
    return _RAGGED[key]


# (env, head_hidden_layers, engine switches, expected fit_fb, expected fit_path)
RAGGED_CASES = [
    ('cartpole', 1, {}, True, 'fused'),
    ('cartpole', 1, {'fit_fb_enabled': False}, False, 'fused'),
    ('cartpole', 1, {'fused_adam': False}, True, 'separate'),
    ('cartpole', 1, {'split_bwd': False}, False, 'fused'),
    ('cartpole', 2, {}, False, 'separate'),
    ('tracking', 1, {}, False, 'fused'),
    ('tracking', 1, {'split_bwd': False}, False, 'fused'),
]


@pytest.mark.parametrize('env,hhl,switches,fit_fb,fit_path', RAGGED_CASES,
                         ids=[f'{e}-h{h}-' + ('-'.join(s) or 'production') for e, h, s, _, _ in RAGGED_CASES])
def test_fit_ragged_tile_vs_oracle(env, hhl, switches, fit_fb, fit_path):
    """fit(steps=2) at batch = holdout = 20 rows per member (one full 16-row tile plus a
    4-row tile: the smallest shape at which the tile's partial write-out and the padded
    NLL rows can go wrong), hidden width 200, E = 2, on tape noise against the oracle: on
    cartpole (S + 1 <= 16) through every way the step can run (the one-launch step, forward +
    fused-NLL backward split and paired, the separate Adam step, and the separate NLL launch
    of head_hidden_layers = 2), and on tracking (S + 1 > 16) split and paired. Tolerances of
    test_fit_head_hidden_layers_2_vs_oracle, every element compared."""
    alg, start, P, ref_losses, ref_elites, entries = _ragged_case(env, hhl)
    m = alg.model_ensemble
    eng, g = m.engine, m.group
    assert (m.state_dim + 1 <= 16) == (env == 'cartpole')
    g.data.copy_(start[0])
    m.optimizer.m.copy_(start[1])
    m.optimizer.v.copy_(start[2])
    m.optimizer.step_count = start[3]
    g.mark_dirty()
    g.ensure_packed()
    eng.ws.clear()
    eng.wg_ws.clear()
    tape = drpo_amd.TapeNoise(entries)
    try:
        for k, v in switches.items():
            setattr(eng, k, v)
        losses = m.fit(alg.replay_buffer, steps=2, noise=tape)
    finally:
        eng.fit_fb_enabled = eng.fused_adam = eng.split_bwd = True
    assert tape.done()
    assert (eng.fit_fb, eng.fit_path) == (fit_fb, fit_path)
    print('ragged fit', env, hhl, switches, 'loss rel err',
          float(np.max(np.abs(np.asarray(losses) - ref_losses) / np.abs(ref_losses))))
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    assert m._elite_inds == ref_elites
    sd = m.state_dict()
    for k in O.ens_param_keys(P, ''):
        got, e = sd[k].cpu().numpy(), P[k].numpy()
        err = np.abs(got - e) - (5e-5 + 2e-4 * np.abs(e))
        print('ragged fit', k, 'max excess over tolerance', float(err.max()))
        assert not (err > 0).any(), (k, float(np.abs(got - e).max()))


def _flags_marginal(fns, s2, flags, n_probe=6, rel=1e-5):
    """Rows whose (done, violation) flags flip under +-rel perturbations of next_state:
    there the flag is decided by fp32 rounding, not by the kernel's arithmetic."""
    g = torch.Generator().manual_seed(0)
    marg = torch.zeros(len(s2), dtype=torch.bool)
    for _ in range(n_probe):
        u = torch.rand(s2.shape, generator=g) * 2 - 1
        d, v, _ = fns(s2 + rel * (1 + s2.abs()) * u)
        marg |= (d != flags[0]) | (v != flags[1])
    return marg


@pytest.mark.parametrize('c', CFGS)
def test_config_rollout_teacher_forced_dying_rows(c):
    """Raw random weights at the config's exact shape (rows die every step). The fused
    engine runs on recorded original-row draws; then, for every step t, one oracle
    step (actor sample, elite member sample, env constraint fns) is computed from the
    HIP's own step-t states and compared row by row: actions, next states, rewards,
    constraint values |d| <= 2e-4 + 2e-4|ref|, done / violation flags exact except
    rows whose flags flip under a 1e-5 relative perturbation. Step t+1's rows must be
    step t's surviving next states in batch order, exactly (the 32-row-tile emit)."""
    alg, cd = _alg(c, seed=7)
    env, B, H = cd['env'], cd['B'], cd['H']
    rep = _fill(alg, env, 100000, 4)
    m = alg.model_ensemble
    st = torch.from_numpy(rep['states'])
    mean, std = O.normalizer_fit(st)
    m.state_normalizer.mean.copy_(mean)
    m.state_normalizer.std.copy_(std)
    E = m.ensemble_size
    m._elite_inds = sorted({0, E // 2, E - 1, 1, E - 2})[:min(5, E)]
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim
    S1 = S + 1
    g = torch.Generator().manual_seed(100 + c)
    init = np.random.RandomState(c).choice(len(st), B, replace=False)
    ks = [int(k) for k in np.random.RandomState(50 + c).randint(0, len(m._elite_inds), H)]
    eps_a = [torch.randn(B, A, generator=g).numpy() for _ in range(H)]
    eps_m = [torch.randn(B, S1, generator=g).numpy() for _ in range(H)]
    entries = [('np_choice', init)]
    for t in range(H):
        entries += [('normal', eps_a[t]), ('choice', np.array(ks[t])), ('randn_like', eps_m[t])]
    tape = drpo_amd.TapeNoise(entries)
    from drpo_amd import ops
    out = ops.rollout(alg, alg.actor, None, tape, eps_layout=1)
    torch.cuda.synchronize()
    assert tape.done()
    n = len(out)
    got = {k: v.cpu() for k, v in out.get(as_dict=True).items()}
    assert B <= n <= B * H
    sd = {k: v.detach().cpu() for k, v in alg.state_dict().items()}
    P = {k[len('solver.'):]: v for k, v in sd.items() if k.startswith('solver.actor.')}
    P.update({k: v for k, v in sd.items() if k.startswith('model_ensemble.')})
    fns = O.env_fns(env)
    _oracle_threads()
    ids = np.arange(B)
    off, steps, checked, marginal_total = 0, 0, 0, 0
    assert torch.equal(got['states'][:B], st[init]), 'step-0 states = replay rows of the initial draw'
    rs = np.random.RandomState(c)
    while off < n:
        nt = len(ids)
        seg = slice(off, off + nt)
        sel = np.sort(rs.choice(nt, min(nt, 2048), replace=False))
        s_t = got['states'][seg][sel]
        rng = O.TapeRNG([('normal', eps_a[steps][ids[sel]]), ('choice', np.array(ks[steps])),
                         ('randn_like', eps_m[steps][ids[sel]])])
        a_ref, _, _, _ = O.policy_sample(P, 'actor.net.', s_t, rng)
        s2_ref, r_ref = O.ens_sample(P, 'model_ensemble.', s_t, a_ref, m._elite_inds, rng)
        assert rng.done()
        msg = f'config {c} step {steps}'
        _close(got['actions'][seg][sel], a_ref, 2e-4, msg + ' actions')
        _close(got['next_states'][seg][sel], s2_ref, 2e-4, msg + ' next_states')
        _close(got['rewards'][seg][sel], r_ref, 2e-4, msg + ' rewards')
        s2_hip = got['next_states'][seg][sel]
        d_o, v_o, h_o = fns(s2_hip)
        _close(got['constraint_values'][seg][sel], h_o.reshape(got['constraint_values'][seg][sel].shape), 2e-4,
               msg + ' constraint values')
        dg, vg = got['dones'][seg][sel], got['violations'][seg][sel]
        bad = (dg != d_o) | (vg != v_o)
        if bad.any():
            marg = _flags_marginal(fns, s2_hip, (d_o, v_o))
            assert not (bad & ~marg).any(), (msg, 'flags', int((bad & ~marg).sum()))
            marginal_total += int(bad.sum())
        checked += len(sel)
        dn = got['dones'][seg].numpy().astype(bool)
        nxt = int((~dn).sum())
        if off + nt < n:
            assert torch.equal(got['states'][off + nt:off + nt + nxt], got['next_states'][seg][~dn]), \
                msg + ' survivors (ordered emit)'
        ids = ids[~dn]
        off += nt
        steps += 1
        if len(ids) == 0:
            break
    assert off == n and steps <= H
    assert marginal_total <= 4, marginal_total
    print(f'config {c}: {n} rows over {steps} steps, {checked} teacher-forced rows checked')


@pytest.mark.parametrize('c', [2])
def test_fit_fused_adam_matches_separate_step(c):
    """The fit's Adam fused into the weight-gradient launch (drpo_mlp_wgrad_adam) against
    the separate drpo_optim_step launch, both on the split-heads backward: the same
    per-element arithmetic, so parameters, Adam moments and both packed mirrors are
    bitwise equal after 3 production-noise steps. The paired backward (one workgroup per
    row tile, trunk dZ by the concatenated-K product) differs only in summation order."""
    from drpo_amd.rng import DeviceNoise
    alg, cd = _alg(c, B=256)
    m = alg.model_ensemble
    eng = m.engine
    _fill(alg, cd['env'], 30000, 7)
    g = m.group
    m.optimizer._ensure_state()
    start = [g.data.clone(), m.optimizer.m.clone(), m.optimizer.v.clone(), m.optimizer.step_count]

    def run(fused, split):
        g.data.copy_(start[0])
        m.optimizer.m.copy_(start[1])
        m.optimizer.v.copy_(start[2])
        m.optimizer.step_count = start[3]
        g.mark_dirty()
        g.ensure_packed()
        eng.fused_adam = fused
        eng.split_bwd = split
        eng.ws.clear()
        eng.wg_ws.clear()
        losses = m.fit(alg.replay_buffer, steps=3, noise=DeviceNoise(1234))
        torch.cuda.synchronize()
        out = [g.data.clone(), m.optimizer.m.clone(), m.optimizer.v.clone(), g.packed.clone(), g.packedT.clone(),
               g.grad.clone()]
        return losses, out

    try:
        l_f, o_f = run(True, True)
        l_s, o_s = run(False, True)
        l_p, o_p = run(False, False)
    finally:
        eng.split_bwd = True
        eng.fused_adam = True
    assert l_f == l_s
    for a, b, what in zip(o_f, o_s, ['data', 'm', 'v', 'packed', 'packedT', 'grad']):
        assert torch.equal(a, b), what
    assert int((o_f[5] != 0).sum()) == 0           # the gradient is left zeroed
    np.testing.assert_allclose(l_p, l_f, rtol=1e-5)
    _close(o_p[0], o_f[0].cpu().numpy(), 2e-5, 'paired vs split backward: parameters')


@pytest.mark.parametrize('c', [1, 2, 3])
def test_fit_fb_matches_two_launches(c):
    """The fit step's forward + NLL + backward-data as ONE launch (drpo_ens_fit_fb,
    csrc/fit.hip) against the split-heads forward + drpo_mlp_backward_ens it replaces:
    the same saves (x, trunk y's, heads' hidden y's), every dZ the weight gradients read
    (trunk dz + dz2, both heads) and the step losses, from the same start and minibatch
    (one step, production noise). The trunk and hidden layers take the same MFMA order
    (bitwise); the heads' output layers are reduced split-K over the 4 waves that own the
    hidden columns instead of the separate forward's order, so D / log-var and everything
    downstream differ by summation order only: rtol 2e-5 on the saves, 1e-4 of each
    tensor's max-abs on the dZ."""
    from drpo_amd.rng import DeviceNoise
    alg, cd = _alg(c, B=256)
    m = alg.model_ensemble
    eng = m.engine
    _fill(alg, cd['env'], 30000, 8)
    g = m.group
    m.optimizer._ensure_state()
    start = [g.data.clone(), m.optimizer.m.clone(), m.optimizer.v.clone(), m.optimizer.step_count]
    names = ['fit.x', 'fit.sy00', 'fit.sy01', 'fit.sy10', 'fit.sy20'] + \
        [f'fit.dz{j}{l}' for j in range(3) for l in range(2)] + ['fit.dzb0', 'fit.dzb1']

    def run(fb):
        g.data.copy_(start[0])
        m.optimizer.m.copy_(start[1])
        m.optimizer.v.copy_(start[2])
        m.optimizer.step_count = start[3]
        g.mark_dirty()
        g.ensure_packed()
        eng.fit_fb_enabled = fb
        eng.ws.clear()
        eng.wg_ws.clear()
        losses = m.fit(alg.replay_buffer, steps=1, noise=DeviceNoise(4321))
        torch.cuda.synchronize()
        assert eng.fit_fb == fb and eng.fit_path == 'fused'
        return losses, {k: eng.ws[k].clone() for k in names}

    try:
        l_f, o_f = run(True)
        l_s, o_s = run(False)
    finally:
        eng.fit_fb_enabled = True
    np.testing.assert_allclose(l_f, l_s, rtol=2e-5)
    for k in names:
        a, b = o_f[k].cpu().numpy(), o_s[k].cpu().numpy()
        assert np.isfinite(a).all(), k
        if k.startswith('fit.dz'):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-4 * float(np.abs(b).max()) + 1e-30, err_msg=k)
        else:
            np.testing.assert_allclose(a, b, rtol=2e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize('fb', [True, False])
def test_fit_step_tight_log_var_bounds_vs_oracle(fb):
    """The fused flavour of the NLL (nll_element with the hardware sp_grad: fit_fb_body when fb, else
    ens_upstream inside drpo_mlp_backward_ens) with a good share of elements OUTSIDE each log-variance
    bound, where the bound-gradient shares cmn / cmx and the clamp's slopes are not ~0 / ~1 as they are
    at the initial bounds [-10, 1]: the bounds are set to the 30 % / 70 % quantiles of the initial raw
    log-variance outputs, per column. One fit step on recorded draws against O.ens_fit: the step loss
    (rtol 1e-4, test_config_full_width_fit_vs_oracle) and every parameter's gradient, the log-var
    bounds' included, read back from Adam's first moment after its first step (0.1 x the effective
    gradient on both sides) with the gradient tolerance of test_gpu_ensemble.py."""
    alg, cd = _alg(2, B=256)
    m = alg.model_ensemble
    eng = m.engine
    _fill(alg, cd['env'], 30000, 9)
    buf = {k: v.cpu() for k, v in alg.replay_buffer.get(as_dict=True).items()}
    P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _oracle_threads()
    E = m.ensemble_size

    def raw_log_var(s, a):
        x = torch.cat([O.normalize(P, '', s), a], dim=-1)
        return O._batched(P, 'log_var_head.', O._batched(P, 'trunk.', x, True), False)
    P['state_normalizer.mean'], P['state_normalizer.std'] = O.normalizer_fit(buf['states'])
    raw = raw_log_var(buf['states'][:2048].repeat(E, 1, 1), buf['actions'][:2048].repeat(E, 1, 1))
    flat = raw.reshape(-1, raw.shape[-1])
    lo, hi = torch.quantile(flat, 0.3, dim=0), torch.quantile(flat, 0.7, dim=0)
    P['min_log_var'], P['max_log_var'] = lo.clone(), hi.clone()
    m.min_log_var.data.copy_(lo.to(DEV))
    m.max_log_var.data.copy_(hi.to(DEV))
    torch.manual_seed(17)
    live = O.LiveRNG()
    opt = {}
    P0 = {k: v.clone() for k, v in P.items()}
    ref_losses, _ = O.ens_fit(P, '', opt, buf, 1, E, m.batch_size, m.holdout_size, m.num_elites, live)
    idx = torch.as_tensor(np.asarray(live.entries[0][1])).long().reshape(E, -1)
    P, P_after = P0, P                           # the shares: the oracle's raw outputs on the step's minibatch
    raw = raw_log_var(buf['states'][idx], buf['actions'][idx])
    below, above = (raw < lo).float().mean().item(), (raw > hi).float().mean().item()
    print(f'tight log-var bounds (fb={fb}): {below:.3f} of the elements below min_log_var, {above:.3f} above max_log_var')
    assert below >= 0.10 and above >= 0.10
    tape = drpo_amd.TapeNoise(live.entries)
    m.optimizer._ensure_state()
    eng.ws.clear()
    eng.wg_ws.clear()
    try:
        eng.fit_fb_enabled = fb
        losses = m.fit(alg.replay_buffer, steps=1, noise=tape)
        torch.cuda.synchronize()
    finally:
        eng.fit_fb_enabled = True
    assert tape.done()
    assert eng.fit_fb == fb and eng.fit_path == 'fused'
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    bad = []
    for k in O.ens_param_keys(P_after, ''):
        got = m.group.view(k, m.optimizer.m).cpu().numpy()
        exp = opt[k]['m'].numpy()
        tol = 1e-5 * np.abs(exp).max() + 1e-3 * np.abs(exp)
        if (np.abs(got - exp) > tol).any():
            bad.append((k, float(np.abs(got - exp).max()), float(np.abs(exp).max())))
    assert not bad, bad
    for k in ('min_log_var', 'max_log_var'):
        assert np.abs(opt[k]['m'].numpy()).min() > 0


@pytest.mark.parametrize('c', [2])
def test_multiplier_post_chain_matches_separate_launch(c):
    """The MLPMultiplier forward chained behind the constraint bound in the same
    workgroups (drpo_mlp_fwd_t.post: no 'a.mult' / 'm.mult' launch) against its own
    launch (SACEngine.post_mult = False), at the reference widths (256: the bound is formed
    in-kernel): the same layers on the same [s, bound] rows, so two actor and two
    multiplier updates leave bitwise the same parameters."""
    from drpo_amd.rng import DeviceNoise

    def run(post):
        alg, cd = _alg(c, B=1024)
        sol = alg.solver
        sol.engine.post_mult = post
        assert sol.mlp_multiplier
        g = torch.Generator().manual_seed(5)
        noise = DeviceNoise(11)
        for _ in range(2):
            obs = torch.randn(1024, alg.state_dim, generator=g).to(DEV)
            sol.update_actor_and_alpha(obs, noise=noise)
            sol.update_multiplier(obs, noise=noise)
        torch.cuda.synchronize()
        assert sol.engine._ccb_fused() and sol.engine._post_mult() == post
        return {k: v.detach().clone() for k, v in sol.state_dict().items()}

    a = run(True)
    b = run(False)
    for k in a:
        assert torch.equal(a[k], b[k]), k
