"""End to end at hidden widths other than the reference defaults (actor / critics /
multiplier 256, model 200), against the CPU oracle: (SAC hidden, model hidden) = (64, 64),
(128, 128), (144, 96) at E = 3, B = 256, H = 4.

hidden_dim is a user setting, and every fast path tests for its own shapes (the paired twin
critics and policies: 256; the constraint bound formed in the forward launch, the
multiplier's post chain and the actor update's fused forward + backward: a 256-wide
constraint critic; the fit's fused NLL backward and one-launch step: 200 | 256; the
rollout's paired model heads: 200; its LDS-resident actor: 256). At any other width the
generic trunk and one-head-at-a-time code runs; these tests hold it to the same oracle and
tolerances as the default widths, and assert that the generic path is the one that ran.

* rollout, engines 1 (per step) and 2 (fused horizon), against O.rollout on its recorded
  draws (engine 2: re-indexed by original row): point-robot (rows die; S + 1 <= 16, the
  split-K model output layers) and tracking (S + 1 = 52 > 16, the wide ones). Floats
  |d| <= 2e-4 + 2e-4 |ref| (test_gpu_rollout.py), flags and row counts exact;
* one update_critic + update_actor_and_alpha + update_multiplier against O.SSACOracle with
  the checks and tolerances of test_gpu_configs.py::test_config_sac_update_vs_oracle;
* fit(steps=3) against O.ens_fit with the tolerances of
  test_gpu_configs.py::test_config_full_width_fit_vs_oracle.
"""
import numpy as np
import pytest
import torch

import bench
import drpo_amd
from drpo_amd import _abi
from gpu_helpers import (DEV, COMP, WIDTH_B as B, WIDTH_E as E, WIDTH_H as H, _width_alg as _alg, close,
                         original_row_tape)
from oracle import drpo_oracle as O
from test_gpu_configs import _check_params, _eff_grads, _fill, _sac_batch

pytestmark = pytest.mark.gpu

WIDTHS = [(64, 64), (128, 128), (144, 96)]    # (actor / critic / multiplier hidden, model hidden)
assert (E, B, H) == (3, 256, 4)


_ROLLOUT = {}


def _rollout_case(env, hid, mh):
    """The trainer with a replay and a fitted normaliser, and the oracle's rollout with its
    recorded draws, once per (env, widths) for both engines."""
    key = (env, hid, mh)
    if key not in _ROLLOUT:
        alg = _alg(env, hid, mh)
        rep = _fill(alg, env, 8000, 3)
        m = alg.model_ensemble
        st = torch.from_numpy(rep['states'])
        mean, std = O.normalizer_fit(st)
        m.state_normalizer.mean.copy_(mean)
        m.state_normalizer.std.copy_(std)
        m._elite_inds = [2, 0, 1]
        sd = {k: v.detach().cpu() for k, v in alg.state_dict().items()}
        P = {k[len('solver.'):]: v for k, v in sd.items() if k.startswith('solver.actor.')}
        P.update({k: v for k, v in sd.items() if k.startswith('model_ensemble.')})
        torch.manual_seed(17)
        live = O.LiveRNG()
        ref = O.rollout(P, 'actor.net.', 'model_ensemble.', m._elite_inds, st, env, B, H, live)
        _ROLLOUT[key] = (alg, ref, live.entries)
    return _ROLLOUT[key]


@pytest.mark.parametrize('engine', [1, 2])
@pytest.mark.parametrize('hid,mh', WIDTHS)
@pytest.mark.parametrize('env', ['point-robot', 'tracking'])
def test_width_rollout_vs_oracle(env, hid, mh, engine):
    from drpo_amd import ops
    alg, ref, entries = _rollout_case(env, hid, mh)
    assert (alg.state_dim + 1 <= 16) == (env == 'point-robot')
    n = len(ref['states'])
    if env == 'point-robot':
        assert B < n < B * H, 'regime: rows must die during the horizon'
    alg.rollout_engine = engine
    if engine == 1:
        tape = drpo_amd.TapeNoise(entries)
        out = ops.rollout(alg, alg.actor, None, tape)
    else:
        tape = drpo_amd.TapeNoise(original_row_tape(entries, ref, B))
        out = ops.rollout(alg, alg.actor, None, tape, eps_layout=1)
    torch.cuda.synchronize()
    assert tape.done()
    assert len(out) == n
    got = out.get(as_dict=True)
    for k in COMP:
        close(got[k], ref[k], tol=2e-4, msg=f'{env} {hid}/{mh} engine {engine} {k}')


def _assert_generic_sac_path(sol, prof):
    """The update ran none of the 256-wide fast paths: no pair job, no in-launch constraint
    bound, no post chain, no fused forward + backward launch."""
    eng = sol.engine
    from drpo_amd.mlp_desc import pairable
    n = eng.nets
    assert not pairable(n['q0'], n['q1']) and not pairable(n['actor'], n['safe'])
    assert not eng._ccb_fused() and not eng._post_mult() and not eng._fb_actor(True)
    assert 'mlp_fb' not in prof and not any(k.startswith('a.fb') for k in eng.desc)
    multi = 0
    for key, d in eng.desc.items():
        if isinstance(d, tuple) and len(d) == 4 and isinstance(d[0], _abi.MlpFwd * d[2]):
            for j in range(d[2]):
                job = d[0][j]
                assert not job.pair and not job.ccb_out and job.post.nl == 0, key
                multi += 1
    assert multi > 0, 'no multi-job forward seen'


@pytest.mark.parametrize('hid,mh', WIDTHS)
def test_width_sac_update_vs_oracle(hid, mh):
    from drpo_amd.mlp_desc import LaunchProfiler
    env = 'point-robot'
    alg = _alg(env, hid, mh)
    jsn = bench.ENV_JSON[env]
    sol = alg.solver
    A, C = alg.action_dim, alg.con_dim
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
    rtol = 1e-4
    lr_max = max(sol.critic_lr, sol.actor_lr, sol.multiplier_lr)
    sol.engine.profiler = LaunchProfiler()
    torch.manual_seed(hid)
    live = O.LiveRNG()
    lq_ref, lqc_ref = orc.update_critic(*batch, live)
    tape = drpo_amd.TapeNoise(live.entries)
    lq, lqc = sol.update_critic(*dev_batch, noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    np.testing.assert_allclose(lq.item(), float(lq_ref), rtol=rtol)
    np.testing.assert_allclose(lqc.item(), float(lqc_ref), rtol=rtol)
    _check_params(sol, orc.P, f'{hid} after update_critic', _eff_grads(orc), lr_max)
    live = O.LiveRNG()
    orc.update_actor_and_alpha(batch[0], live)
    tape = drpo_amd.TapeNoise(live.entries)
    sol.update_actor_and_alpha(dev_batch[0], noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    np.testing.assert_allclose(sol.log_alpha.item(), float(orc.log_alpha), rtol=1e-5, atol=1e-6)
    _check_params(sol, orc.P, f'{hid} after update_actor_and_alpha', _eff_grads(orc), lr_max)
    live = O.LiveRNG()
    orc.update_multiplier(batch[0], live)
    tape = drpo_amd.TapeNoise(live.entries)
    sol.update_multiplier(dev_batch[0], noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    _check_params(sol, orc.P, f'{hid} after update_multiplier', _eff_grads(orc), lr_max)
    prof = sol.engine.profiler.summarise()
    sol.engine.profiler = None
    _assert_generic_sac_path(sol, prof)


@pytest.mark.parametrize('hid,mh', WIDTHS)
def test_width_fit_vs_oracle(hid, mh):
    env = 'point-robot'
    alg = _alg(env, hid, mh)
    m = alg.model_ensemble
    assert not m.engine.fit_plan().fused
    _fill(alg, env, 30000, 6)
    buf = {k: v.cpu() for k, v in alg.replay_buffer.get(as_dict=True).items()}
    P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(mh)
    live = O.LiveRNG()
    ref_losses, ref_elites = O.ens_fit(P, '', {}, buf, 3, m.ensemble_size, m.batch_size, m.holdout_size,
                                       m.num_elites, live)
    tape = drpo_amd.TapeNoise(live.entries)
    losses = m.fit(alg.replay_buffer, steps=3, noise=tape)
    assert tape.done()
    assert not m.engine.fit_fb and m.engine.fit_path == 'separate'
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    assert m._elite_inds == ref_elites
    sd = m.state_dict()
    for k in O.ens_param_keys(P, ''):
        got, e = sd[k].cpu().numpy(), P[k].numpy()
        err = np.abs(got - e) - (5e-5 + 2e-4 * np.abs(e))
        assert not (err > 0).any(), (k, float(np.abs(got - e).max()))
