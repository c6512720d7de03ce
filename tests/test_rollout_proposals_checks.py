"""Host-side checks of drpo_rollout_trajectories_proposed (csrc/rollout.hip) and of the Python
surfaces above it, imagine(proposals=) and plan(safety_filter=), no GPU: every C call here is
refused before any launch (descriptors and dummy pointers: test_rollout_traj_checks.py's,
test_rollout_given_checks.py's, test_rollout_shield_checks.py's and
test_rollout_linear_checks.py's), every Python refusal happens before anything touches a device
(the trainer is on the CPU here: a call that got further raises DrpoError, not ValueError), and
plan's loop runs on the host over stand-ins for its four launches."""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch

import drpo_amd
from drpo_amd import _lib, ops
from test_host_logic import make_smbpo
from test_rollout_given_checks import _given
from test_rollout_linear_checks import _linear
from test_rollout_shield_checks import _shield
from test_rollout_traj_checks import EINVAL, P, _desc, _err, _out

WHO = 'drpo_rollout_trajectories_proposed:'
H = 3
TAPE, DEVICE = drpo_amd.TapeNoise([]), drpo_amd.DeviceNoise(1)


def _call(d, g, s, lin, t):
    by = lambda x: None if x is None else ctypes.byref(x)   # noqa: E731
    return _lib.lib().drpo_rollout_trajectories_proposed(ctypes.byref(d), by(g), by(s), by(lin), by(t), None)


# ------------------------------------------------------------------ the entry point
def test_version():
    assert _lib.lib().drpo_version() >= 14            # the version that added the entry point


@pytest.mark.parametrize('linear', [False, True])
def test_refuses_the_other_entry_points_calls(linear):
    lin = _linear() if linear else None
    for g in (None, _given(0), _given(0, None)):
        assert _call(_desc(H=H), g, _shield(), lin, _out()) == EINVAL
        assert _err().startswith(WHO) and 'no given actions' in _err(), _err()
    assert _call(_desc(H=H), _given(2), None, lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'null shield' in _err(), _err()


@pytest.mark.parametrize('K', [1, 33, 0, -1])
def test_refuses_candidates_outside_2_to_32(K):
    assert _call(_desc(H=H), _given(2), _shield(), _linear(K), _out()) == EINVAL
    assert _err() == f'{WHO} linear shield candidates {K} outside 2..32'


@pytest.mark.parametrize('steps, actions, fragment', [
    (H + 1, P, 'given steps 4 outside [0, horizon 3]'),
    (-1, P, 'given steps -1 outside [0, horizon 3]'),
    (2, None, 'given steps 2 need actions'),
])
@pytest.mark.parametrize('linear', [False, True])
def test_every_check_of_the_given_call_applies(linear, steps, actions, fragment):
    assert _call(_desc(H=H), _given(steps, actions), _shield(), _linear() if linear else None, _out()) == EINVAL
    assert _err().startswith(WHO) and fragment in _err(), _err()


@pytest.mark.parametrize('steps', [1, H])
@pytest.mark.parametrize('linear', [False, True])
def test_every_check_of_the_shielded_call_applies(linear, steps):
    """Valid proposals add no refusal: the shield's and the trajectory call's, under this name."""
    lin, g = (_linear() if linear else None), _given(steps)
    assert _call(_desc(H=H), g, _shield(Hc=257), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'hidden width 257 outside 1..256' in _err()
    assert _call(_desc(H=H), g, _shield(sW2=None), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'null safe-actor pointer' in _err()
    assert _call(_desc(H=H), g, _shield(zW1=None), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'distributional shield needs the log-std head' in _err()
    assert _call(_desc(H=H), g, _shield(), lin, _out(ret=P)) == EINVAL
    assert _err() == WHO + ' ret needs weights'
    assert _call(_desc(H=H), g, _shield(), lin, _out(len=None)) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    d = _desc(H=H)
    d.engine = 1
    assert _call(d, g, _shield(), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'fused engine only' in _err()
    d = _desc(H=H)
    d.rows_per_tile = 8
    assert _call(d, g, _shield(), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'rows_per_tile must be 16 or 32' in _err()


# ------------------------------------------------------------------ ops: the request
ACTIONS = torch.zeros(4, 1, 2)
REQUESTS = [
    ((DEVICE, None, None, None), False),
    ((DEVICE, ACTIONS, None, None), False),
    ((TAPE, None, None, None), False),
    ((DEVICE, None, None, 0.5), False),
    ((DEVICE, None, ACTIONS, 0.5), True),
    ((DEVICE, None, ACTIONS, -float('inf')), True),
    ((DEVICE, None, ACTIONS, None), 'proposals without shield.*actions='),
    ((DEVICE, ACTIONS, ACTIONS, 0.5), 'proposals with actions'),
    ((DEVICE, ACTIONS, ACTIONS, None), 'proposals with actions'),
    ((TAPE, None, ACTIONS, 0.5), 'proposals with a recorded tape'),
]


@pytest.mark.parametrize('args, want', REQUESTS, ids=[str(i) for i in range(len(REQUESTS))])
def test_proposal_request(args, want):
    if isinstance(want, str):
        with pytest.raises(ValueError, match=want):
            ops._proposal_request(*args)
    else:
        assert ops._proposal_request(*args) is want


def test_proposals_are_checked_as_actions_are_under_their_own_name():
    for bad in (torch.zeros(4, 1, 2, dtype=torch.float64), [[0.0, 0.0]], torch.zeros(4, 2, 2)[:, :1]):
        with pytest.raises(ValueError, match='^proposals: a contiguous float32 tensor'):
            ops._given_actions(bad, 4, H, 2, 'proposals')
        with pytest.raises(ValueError, match='^actions: a contiguous float32 tensor'):
            ops._given_actions(bad, 4, H, 2)
    assert ops._given_actions(None, 4, H, 2, 'proposals') == (None, 0)


# ------------------------------------------------------------------ imagine(proposals=)
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


@pytest.fixture
def device_work(monkeypatch):
    """Everything rollout_trajectories does first when it starts on its inputs."""
    calls = []
    for mod, name in ((_lib, 'require_device'), (ops, '_start_states'), (ops, '_shield_desc'), (ops, '_rollout_static')):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **kw: calls.append(_n))
    return calls


def test_imagine_refuses_before_any_device_work(alg, device_work):
    B, A = alg.rollout_batch_size, alg.action_dim
    s, p = torch.zeros(B, alg.state_dim), torch.zeros(B, 1, A)
    for shield in (None, False):
        with pytest.raises(ValueError, match='proposals without shield.*actions='):
            alg.imagine(s, proposals=p, shield=shield)
    for shield in (None, True, 0.5, 'linear', ('linear', 0.0, 5)):
        with pytest.raises(ValueError, match='proposals with actions'):
            alg.imagine(s, proposals=p, actions=p, shield=shield)
    for shield in (True, 'linear'):
        with pytest.raises(ValueError, match='proposals with a recorded tape'):
            alg.imagine(s, proposals=p, shield=shield, noise=drpo_amd.TapeNoise([]))
    # the shield's own refusals stay the shield's
    with pytest.raises(ValueError, match='shield_candidates'):
        alg.imagine(s, proposals=p, shield=('linear', 0.0, 33))
    with pytest.raises(ValueError, match='shield: '):
        alg.imagine(s, proposals=p, shield='safe')
    # and the old spelling keeps its verdict
    with pytest.raises(ValueError, match='shield with actions'):
        alg.imagine(s, actions=p, shield=True)
    assert device_work == []


def test_the_shield_request_sees_no_actions(alg, monkeypatch):
    """_shield_request keeps its signature and is asked with actions=None for the new form; a
    valid call gets past every refusal and stops where the compute path asks for device tensors."""
    seen = []
    real = ops._shield_request
    monkeypatch.setattr(ops, '_shield_request', lambda *a: (seen.append(a), real(*a))[1])
    B, A = alg.rollout_batch_size, alg.action_dim
    s = torch.zeros(B, alg.state_dim)
    for shield, want in ((True, (alg.safe_shield_threshold, None)), (0.25, (0.25, None)), ('linear', (alg.safe_shield_threshold, 11)),
                         (('linear', 0.5, 4), (0.5, 4))):
        for p in (torch.zeros(B, 2, A), torch.zeros(B, A)):
            seen.clear()
            with pytest.raises(_lib.DrpoError, match='no CPU fallback'):
                alg.imagine(s, proposals=p, shield=shield, shield_uncertainty=False)
            (a,) = seen
            assert len(a) == 6 and a[0] is alg and a[2] is None and a[3:] == (float(want[0]), want[1], False)


# ------------------------------------------------------------------ plan(safety_filter=)
@pytest.fixture
def seen(monkeypatch):
    calls = []
    for name in ('plan_sample', 'plan_refit', '_terminal_critics', 'rollout_trajectories', 'lookahead'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    return calls


@pytest.mark.parametrize('bad', [
    'safe', '', 'Linear', (), ('safe', 0.0), ('linear', 0.0, 11, 1), ('linear', 0.0, 1), ('linear', 0.0, 33),
    ('linear', 0.0, 11.0), ('linear', 0.0, True), ('linear', math.nan), ('linear', 'low'), ['linear', True],
    math.nan, {}, 1 + 2j,
], ids=str)
def test_plan_refuses_the_filter_before_any_device_work(alg, seen, bad):
    with pytest.raises(ValueError, match='safety_filter'):
        alg.plan(torch.zeros(4, alg.state_dim), horizon=3, candidates=8, safety_filter=bad)
    assert seen == [] and alg.__dict__.get('_plan_noise') is None


def test_plan_keeps_its_refusals(alg, seen):
    with pytest.raises(TypeError):
        alg.plan(torch.zeros(4, alg.state_dim), shield=True, safety_filter=True)
    with pytest.raises(TypeError):
        alg.plan(torch.zeros(4, alg.state_dim), proposals=torch.zeros(4, 3, 2))
    with pytest.raises(ValueError, match='recorded tape'):
        alg.plan(torch.zeros(4, alg.state_dim), horizon=3, candidates=8, safety_filter=True, noise=drpo_amd.TapeNoise([]))
    assert seen == []


PP, N, K = 4, 8, 2


def _host_plan(alg, monkeypatch, **kw):
    """alg.plan on the host over stand-ins for the sample launch, imagine, the terminal critics and
    the refit. Returns (the result, imagine's keyword arguments per iteration, the stand-in run,
    the candidates of the last iteration)."""
    A = alg.action_dim
    g = torch.Generator().manual_seed(3)
    im = SimpleNamespace(actions=torch.rand(PP * N, H, A, generator=g), interventions=torch.rand(PP * N, H, generator=g) < 0.5,
                         shield_threshold='the run\'s threshold')
    best = torch.tensor([3, 0, 7, 5], dtype=torch.int32)
    runs, cands = [], []

    def sample(mean, std, incumbent, n, seed, ctr):
        cands.append(torch.rand(PP * n, K, A, generator=g))
        return cands[-1]

    def refit(alg_, im_, tq, tqc, cand, mean, std, gamma, **_):
        z = torch.zeros(PP)
        return {'mean': mean, 'std': std, 'best_actions': cand.reshape(PP, N, K, A)[torch.arange(PP), best.long()],
                'best': best, 'n_feasible': best, 'best_score': z, 'best_cert': z, 'best_feasible': z > 0,
                'score': torch.zeros(PP, N), 'cert': torch.zeros(PP, N), 'rank': torch.zeros(PP, N, dtype=torch.int32)}
    monkeypatch.setattr(ops, 'plan_sample', sample)
    monkeypatch.setattr(ops, '_terminal_critics', lambda *a: (None, None))
    monkeypatch.setattr(ops, 'plan_refit', refit)
    monkeypatch.setattr(alg, 'imagine', lambda *a, **k: (runs.append(k), im)[1])
    res = alg.plan(torch.zeros(PP, alg.state_dim), H, candidates=N, iterations=2, steps=K, members=0,
                   noise=drpo_amd.DeviceNoise(2), **kw)
    return res, runs, im, cands[-1], best


@pytest.mark.parametrize('off', [{}, {'safety_filter': None}, {'safety_filter': False}], ids=['default', 'None', 'False'])
def test_off_means_off(alg, monkeypatch, off):
    """Without a filter the planner's runs are imagine(actions=) as before, with no new keyword,
    and the result's new fields are None; without proposals imagine hands ops no new keyword
    either, and the new entry point is not reached."""
    res, runs, im, cand, _ = _host_plan(alg, monkeypatch, **off)
    assert len(runs) == 2
    for k in runs:
        assert set(k) == {'actions', 'members', 'deterministic', 'model_noise', 'discount', 'noise'}
    assert runs[-1]['actions'] is cand
    assert all(getattr(res, f) is None for f in ops.PlanResult.FILTER_FIELDS)
    assert res.actions.shape == (PP, K, alg.action_dim) and res.imagined is im


def test_imagine_without_proposals_is_the_call_it_was(alg, monkeypatch):
    got = []
    monkeypatch.setattr(ops, 'rollout_trajectories', lambda *a, **kw: (got.append(kw), SimpleNamespace())[1])
    reached = []
    monkeypatch.setattr(_lib.lib(), 'drpo_rollout_trajectories_proposed', lambda *a: reached.append(a))
    B, A = alg.rollout_batch_size, alg.action_dim
    s = torch.zeros(B, alg.state_dim)
    for kw in ({}, {'actions': torch.zeros(B, 1, A)}, {'shield': True}, {'shield': 'linear'}, {'proposals': None, 'shield': 0.5}):
        alg.imagine(s, members=0, noise=drpo_amd.DeviceNoise(2), **kw)
        assert 'proposals' not in got[-1], kw
    assert set(got[0]) == {'members', 'weights', 'horizon', 'actions', 'shield_uncertainty'}
    p = torch.zeros(B, 1, A)
    alg.imagine(s, members=0, noise=drpo_amd.DeviceNoise(2), proposals=p, shield=0.5)
    assert got[-1]['proposals'] is p and got[-1]['actions'] is None and got[-1]['shield'] == 0.5
    assert reached == []


@pytest.mark.parametrize('spelling, shield', [
    (True, 'default'), (0.25, 0.25), (-math.inf, -math.inf), (math.inf, math.inf), (1, 1.0),
    ('linear', ('linear', 'default')), (('linear',), ('linear', 'default')), (('linear', None, 5), ('linear', 'default', 5)),
    (('linear', 0.5), ('linear', 0.5)), (['linear', 0.5, 32], ('linear', 0.5, 32)),
], ids=str)
def test_the_filter_runs_the_candidates_as_proposals(alg, monkeypatch, spelling, shield):
    default = float(alg.safe_shield_threshold)
    want = default if shield == 'default' else \
        tuple(default if x == 'default' else x for x in shield) if isinstance(shield, tuple) else shield
    res, runs, im, cand, best = _host_plan(alg, monkeypatch, safety_filter=spelling, threshold=0.75)
    assert len(runs) == 2
    for k in runs:
        assert set(k) == {'proposals', 'shield', 'members', 'deterministic', 'model_noise', 'discount', 'noise'}
        assert k['shield'] == want and type(k['shield']) is type(want)
    assert runs[-1]['proposals'] is cand
    assert res.threshold == 0.75                                   # the planner's own constraint is a separate argument
    rows = torch.arange(PP) * N + best.long()
    assert torch.equal(res.executed_actions, im.actions[rows]) and res.executed_actions.shape == (PP, H, alg.action_dim)
    assert torch.equal(res.safe_action, im.actions[rows][:, 0])
    assert torch.equal(res.interventions, im.interventions[rows])
    assert res.filter_threshold == im.shield_threshold
    # the incumbent and the result's actions stay proposals, copied
    assert torch.equal(res.actions, cand.reshape(PP, N, K, -1)[torch.arange(PP), best.long()])
    assert torch.equal(res.action, res.actions[:, 0])


def test_plan_result_names_its_filter_fields():
    assert ops.PlanResult.FILTER_FIELDS == ('executed_actions', 'safe_action', 'interventions', 'filter_threshold')
    base = {k: i for i, k in enumerate(ops.PlanResult.FIELDS)}
    r = ops.PlanResult(**base)
    assert all(getattr(r, f) is None for f in ops.PlanResult.FILTER_FIELDS)
    r = ops.PlanResult(**base, executed_actions=1, safe_action=2, interventions=3, filter_threshold=4)
    assert (r.executed_actions, r.safe_action, r.interventions, r.filter_threshold) == (1, 2, 3, 4)
    with pytest.raises(AssertionError):
        ops.PlanResult(**base, executed=1)
