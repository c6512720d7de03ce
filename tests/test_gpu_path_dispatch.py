"""Which launches the engines pick, pinned: the SAC update's launch sequence and the model
fit's plan, for shapes on and off the fused paths. The engines take their shape verdicts from
the library's path queries (include/drpo_hip.h); the literals below were recorded by running
these same bodies on the commit before the queries existed, where Python predicates made the
choice (profiles/path_queries/README.md), on one MI355X."""
import pytest
import torch

import bench
from drpo_amd.mlp_desc import LaunchProfiler
from drpo_amd.rng import DeviceNoise
from gpu_helpers import DEV, _fill

pytestmark = pytest.mark.gpu

B = 32      # two 16-row tiles


def _widths(hid):
    return {'hidden_dim': hid, 'critic_cfg': {'hidden_dim': hid}, 'constraint_critic_cfg': {'hidden_dim': hid},
            'mlp_multiplier_cfg': {'hidden_dim': hid}}


def sac_launches(env, hid, fb):
    """(kind, key) of every MLP launch of one update_solver(actor, multiplier) at B rows"""
    torch.manual_seed(3)
    alg = bench.make_alg(DEV, B, 2, 2, 3, bench.ENV_JSON[env], extra={'sac_cfg': _widths(hid)}, env=env)
    rows = _fill(alg, env, 512, 3)
    alg.virt_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rows.items()})
    eng = alg.solver.engine
    eng.fb_actor = fb
    eng.profiler = LaunchProfiler()
    alg.update_solver(update_actor=True, update_multiplier=True, noise=DeviceNoise(7))
    torch.cuda.synchronize()
    return [(r[0], r[1]) for r in eng.profiler.recs]


CRITIC = [('mlp_fwd', 'c.f.d+a'), ('mlp_bwd', 'c.b1'), ('mlp_wgrad', 'c.wg1f')]
ACTOR_TAIL = [('mlp_bwd', 'a.bpi'), ('mlp_wgrad', 'a.wgf')]
MULT_TAIL = [('mlp_bwd', 'm.bmult'), ('mlp_wgrad', 'm.wgf')]
SAC_LAUNCHES = {
    # the reference widths: pair jobs, the bound and the multiplier in the forward launch
    ('quadrotor', 256, True): CRITIC + [('mlp_fb', 'a.fb.1')] + ACTOR_TAIL + [
        ('mlp_fwd', 'm.f1.d'), ('mlp_fwd', 'm.f21')] + MULT_TAIL,
    ('quadrotor', 256, False): CRITIC + [('mlp_fwd', 'a.f2.111'), ('mlp_bwd', 'a.b.11')] + ACTOR_TAIL + [
        ('mlp_fwd', 'm.f1.d'), ('mlp_fwd', 'm.f21')] + MULT_TAIL,
    # 64-wide nets: none of the fused paths, whatever the switch says
    ('point-robot', 64, True): CRITIC + [('mlp_fwd', 'a.f2.110'), ('mlp_fwd', 'a.mult'), ('mlp_bwd', 'a.b.11')]
    + ACTOR_TAIL + [('mlp_fwd', 'm.f1.d'), ('mlp_fwd', 'm.f20'), ('mlp_fwd', 'm.mult')] + MULT_TAIL,
    ('point-robot', 64, False): CRITIC + [('mlp_fwd', 'a.f2.110'), ('mlp_fwd', 'a.mult'), ('mlp_bwd', 'a.b.11')]
    + ACTOR_TAIL + [('mlp_fwd', 'm.f1.d'), ('mlp_fwd', 'm.f20'), ('mlp_fwd', 'm.mult')] + MULT_TAIL,
}


@pytest.mark.parametrize('env,hid,fb', list(SAC_LAUNCHES))
def test_sac_update_runs_the_recorded_launches(env, hid, fb):
    got = sac_launches(env, hid, fb)
    print(got)
    assert got == SAC_LAUNCHES[(env, hid, fb)]


MODELS = {'reference': {}, 'two hidden head layers': {'head_hidden_layers': 2}, 'hidden 128': {'hidden_dim': 128}}


def fit_model(model, fit_fb):
    """The engine of an E = 3, b = 32 model with the fit switches at their defaults but fit_fb_enabled"""
    torch.manual_seed(3)
    cfg = dict(MODELS[model], batch_size=B, holdout_size=B)
    alg = bench.make_alg(DEV, B, 2, 3, 3, bench.QUAD_JSON, extra={'model_cfg': cfg})
    eng = alg.model_ensemble.engine
    assert (eng.fused_adam, eng.split_bwd, eng.fit_fb_enabled) == (True, True, True)
    eng.fit_fb_enabled = fit_fb
    return eng


FIT_PLANS = {
    ('reference', True): (True, True, 'fused'),
    ('reference', False): (True, False, 'fused'),
    ('two hidden head layers', True): (False, False, 'separate'),
    ('two hidden head layers', False): (False, False, 'separate'),
    ('hidden 128', True): (False, False, 'separate'),
    ('hidden 128', False): (False, False, 'separate'),
}


@pytest.mark.parametrize('model,fit_fb', list(FIT_PLANS))
def test_fit_plan_is_the_recorded_one(model, fit_fb):
    plan = fit_model(model, fit_fb).fit_plan()
    got = (plan.fused, plan.fb, plan.path)
    print(got)
    assert got == FIT_PLANS[(model, fit_fb)]
