"""The actor update's pass through the frozen critics as ONE forward + backward launch
('a.fb', drpo_mlp_fb_multi; SACEngine.fb_actor) against the two launches it replaces
('a.f2' + 'a.b'): two identically seeded engines, production DeviceNoise, all nets 256
wide. The forward is the same code, the backward the same products in the same order,
and a mask select differs from a multiply by 0 / 1 at most in the sign of a zero, so
every compared value must be EQUAL (assert_array_equal), not close.

Shapes: quadrotor (S = 12, A = 2, C = 2) and point-robot (S = 11, A = 2, C = 1) dims;
B = 40 (two full 16-row tiles and a ragged 8-row one) and B = 16 (one tile)."""
import numpy as np
import pytest
import torch

import bench
from gpu_helpers import DEV

pytestmark = pytest.mark.gpu

CALLS = 3          # DeviceNoise(7) picks critic k = 1, 0, 1 over these calls
WATCHED = ('a.dA', 'a.dAc', 'a.dAs', 'a.sqc', 'a.multx')


def _solver(env, B, fb, sac=None):
    torch.manual_seed(3)
    alg = bench.make_alg(DEV, B, 2, 2, 3, bench.ENV_JSON[env], extra={'sac_cfg': sac} if sac else None, env=env)
    alg.solver.engine.fb_actor = fb
    return alg, alg.solver


def _actor_updates(env, B, fb, sac=None):
    """CALLS update_actor_and_alpha calls; per call the watched workspaces and the alpha-loss
    partials, at the end the state dict and the descriptor keys that ran."""
    from drpo_amd.rng import DeviceNoise
    alg, sol = _solver(env, B, fb, sac)
    eng = sol.engine
    noise = DeviceNoise(7)
    g = torch.Generator().manual_seed(5)
    per_call = []
    for _ in range(CALLS):
        obs = torch.randn(B, alg.state_dim, generator=g).to(DEV)
        sol.update_actor_and_alpha(obs, noise=noise)
        torch.cuda.synchronize()
        snap = {k: eng.ws[k].cpu().numpy().copy() for k in WATCHED if k in eng.ws}
        snap['alpha_sum'] = eng.alpha_sum[:(B + 15) // 16].cpu().numpy().copy()
        per_call.append(snap)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in sol.state_dict().items() if torch.is_tensor(v)}
    return per_call, sd, set(eng.desc), set(eng.ws)


def _assert_equal_runs(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert x.keys() == y.keys()
        for k in x:
            assert np.isfinite(x[k]).all(), (i, k)
            np.testing.assert_array_equal(x[k], y[k], err_msg=f'call {i}: {k}')
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        np.testing.assert_array_equal(a[1][k], b[1][k], err_msg=k)


@pytest.mark.parametrize('B', [40, 16])
@pytest.mark.parametrize('env', ['quadrotor', 'point-robot'])
def test_fused_actor_pass_equals_the_two_launches(env, B):
    fused = _actor_updates(env, B, True)
    split = _actor_updates(env, B, False)
    # both critics were picked, and each engine ran its own path
    assert {'a.fb.0', 'a.fb.1'} <= fused[2] and not any(k.startswith(('a.f2', 'a.b.')) for k in fused[2])
    assert {'a.f2.011', 'a.f2.111', 'a.b.01', 'a.b.11'} <= split[2] and not any(k.startswith('a.fb') for k in split[2])
    for k in WATCHED:
        assert k in fused[0][0], k
    # the gradients are not trivially zero
    assert all(np.abs(fused[0][-1][k]).max() > 0 for k in ('a.dA', 'a.dAc', 'a.dAs'))
    # no hidden-layer save of the frozen critics is allocated on the fused path
    assert not any(k.startswith(('a.q0.sy', 'a.q1.sy')) and not k.endswith('.sy2') for k in fused[3])
    assert not any(k.startswith(('a.cc.0.', 'a.cc2.0.', 'a.cc.1.sy0', 'a.cc.2.sy0', 'a.cc2.1.sy0', 'a.cc2.2.sy0'))
                   for k in fused[3])
    _assert_equal_runs(fused, split)


def test_scalar_multiplier_keeps_the_two_launches():
    """An engine the fused launch must refuse (no MLP multiplier) runs 'a.f2' + 'a.b' with
    the switch on, and matches the switch off."""
    sac = {'mlp_multiplier': False}
    on = _actor_updates('quadrotor', 40, True, sac)
    off = _actor_updates('quadrotor', 40, False, sac)
    for run in (on, off):
        assert not any(k.startswith('a.fb') for k in run[2])
        assert any(k.startswith('a.f2.') for k in run[2]) and any(k.startswith('a.b.') for k in run[2])
    _assert_equal_runs(on, off)
