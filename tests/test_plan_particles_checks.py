"""Planning over ensemble particles without a GPU: the definition of drpo_plan_refit_particles on
an example worked by hand (plan_particles_helpers.plan_particles_reference, which the GPU tests hold
the kernel to), the struct, the constant, every refusal of the entry point (calls that fail before
any launch; pointers are dummies the host never dereferences) and every Python refusal of
plan / imagine / mpc(particles=, risk=, cert_risk=)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib, ops
from drpo_amd.rng import TapeNoise
from lookahead_helpers import COST, NAN, QNAN_BITS, REACH
from plan_helpers import INF, SCALES, THRESHOLD, assert_bits, bits, plan_refit_reference
from plan_particles_helpers import (assert_particles_synthetic_shows_every_case, particle_aggregate,
                                    plan_particles_reference, synthetic_particles)
from test_host_logic import make_smbpo
from test_plan_checks import REFIT_INPUTS, REFIT_ROW_OUTPUTS, REFIT_STATE_OUTPUTS, _example
from test_rollout_traj_checks import EINVAL, OK, P, _err

f32 = lambda v: np.asarray(v, np.float32)


# ------------------------------------------------------------------ 1. the definition, by hand
def _particles_example():
    """G 3, P 1, N 4, H 2. Member 0 is test_plan_checks._example (reachability: scores 4.5, 4, 4.5,
    3.5, certs -1.25, 3, -0.5, 0). Members 1 and 2 have rows of length 0 that are not terminated:
    a row's score is its terminal_q and its cert its terminal_qc.
      member 1: scores 4.5, 1, NaN, 2.5; certs -0.5, -1, -1, -0.75
      member 2: scores 1.5, 2, 3, 3.5;   certs -2, -0.5, -0.25, -1
    Row 0: members (4.5, 4.5, 1.5), a tie: the order is j = 2, 0, 1; T 1: 1.5, T 2: (1.5 + 4.5) / 2 = 3,
      T 3: 10.5 / 3 = 3.5. The mean is 3.5, the deviations 1, 1, -2: spread sqrt(6 / 3).
    Row 1: (4, 1, 2): 1; 1.5; 7 / 3. Row 2: a NaN member: NaN for every T, and a NaN spread.
    Row 3: (3.5, 2.5, 3.5): 2.5; 3; 9.5 / 3.
    Cert, max: -0.5, 3, -0.25, 0; mean: -3.75 / 3 = -1.25, 1.5 / 3 = 0.5, -1.75 / 3, -1.75 / 3.
    At threshold -0.25 under max: row 0 is feasible; row 2 would be but its score is NaN (invalid);
      rows 3 and 1 follow by cert ascending: ranks 0, 2, 3, 1.
    Under mean: rows 0, 3 are feasible (row 2 invalid): by score at T 3: 3.5 > 9.5 / 3: ranks 0, 2, 3, 1."""
    x0, scales, cand, mean_in, std_in, _, _, _ = _example()
    z = lambda *s, **kw: torch.zeros(*s, **kw)
    other = lambda q, qc: dict(rewards=z(4, 2), constraint_values=z(4, 2, 1), dones=z(4, 2, dtype=torch.bool),
                               violations=z(4, 2, dtype=torch.bool), lengths=z(4, dtype=torch.int32),
                               terminated=z(4, dtype=torch.bool), terminal_q=torch.tensor(q),
                               terminal_qc=torch.tensor(qc).reshape(4, 1))
    runs = [x0, other([4.5, 1.0, NAN, 2.5], [-0.5, -1.0, -1.0, -0.75]),
            other([1.5, 2.0, 3.0, 3.5], [-2.0, -0.5, -0.25, -1.0])]
    x = {k: torch.cat([r[k] for r in runs]) for k in x0}
    return x, scales, cand, mean_in, std_in


@pytest.mark.parametrize('T, score', [(1, [1.5, 1.0, NAN, 2.5]), (2, [3.0, 1.5, NAN, 3.0]),
                                      (3, [3.5, 7.0 / 3.0, NAN, 9.5 / 3.0])])
@pytest.mark.parametrize('cert_mode', [0, 1], ids=['max', 'mean'])
def test_reference_on_the_example_worked_by_hand(T, score, cert_mode):
    x, scales, cand, mean_in, std_in = _particles_example()
    out = plan_particles_reference(x, cand, mean_in, std_in, G=3, N=4, score_tail=T, cert_mode=cert_mode, gamma=0.5,
                                   mode=REACH, scales=scales, threshold=-0.25, elites=1, temperature=INF,
                                   momentum=0.0, min_std=0.0)
    assert_bits(out['member_score'], f32([[[4.5, 4.0, 4.5, 3.5]], [[4.5, 1.0, NAN, 2.5]], [[1.5, 2.0, 3.0, 3.5]]]),
                'member_score')
    assert_bits(out['member_cert'], f32([[[-1.25, 3.0, -0.5, 0.0]], [[-0.5, -1.0, -1.0, -0.75]],
                                         [[-2.0, -0.5, -0.25, -1.0]]]), 'member_cert')
    assert_bits(out['score'], f32([score]), 'score')
    assert bits(out['score'])[0, 2] == QNAN_BITS
    cert = [[-0.5, 3.0, -0.25, 0.0], [-1.25, 0.5, -1.75 / 3.0, -1.75 / 3.0]][cert_mode]
    assert_bits(out['cert'], f32([cert]), 'cert')
    spread = [math.sqrt(2.0), math.sqrt((25.0 / 9 + 16.0 / 9 + 1.0 / 9) / 3), NAN, None]
    got = out['score_spread'][0]
    assert bits(got)[0] == bits(f32(spread[0])) and bits(got)[2] == QNAN_BITS
    assert abs(float(got[1]) - spread[1]) <= 2.0 ** -23 * spread[1]       # (7/3 is not dyadic: another float64 path)
    if cert_mode == 0:
        assert out['n_feasible'].tolist() == [1] and out['rank'].tolist() == [[0, 2, 3, 1]]
    else:
        assert out['n_feasible'].tolist() == [2]
        # T 1: 1.5 < 2.5 and T 2: 3 == 3 (the lower n) put row 0 ahead or behind row 3
        assert out['rank'].tolist() == [{1: [1, 2, 3, 0], 2: [0, 2, 3, 1], 3: [0, 2, 3, 1]}[T]]
    assert out['best_feasible'].tolist() == [True]


def test_reference_rules():
    x, scales, cand, mean_in, std_in = _particles_example()
    kw = dict(N=4, gamma=0.5, mode=REACH, scales=scales, threshold=-0.25, elites=2, temperature=INF, momentum=0.5,
              min_std=0.3125)
    # G 1 is plan_refit_reference, whatever T and the cert mode
    one = {k: v[:4] for k, v in x.items()}
    want = plan_refit_reference(one, cand, mean_in, std_in, **kw)
    for cert_mode in (0, 1):
        got = plan_particles_reference(one, cand, mean_in, std_in, G=1, score_tail=1, cert_mode=cert_mode, **kw)
        for k in want:
            assert_bits(got[k], want[k], k)
        assert_bits(got['member_score'][0], want['score'], 'member_score')
        assert_bits(got['member_cert'][0], want['cert'], 'member_cert')
        assert not got['score_spread'].any()
    # a NaN certificate stays under the maximum and under the mean; +-inf members
    s, c, sp = particle_aggregate(f32([[1.0, INF, INF, 2.0], [2.0, 1.0, -INF, -INF]]),
                                  f32([[NAN, -1.0, -1.0, INF], [-1.0, NAN, -2.0, -INF]]), 2, 0)
    assert bits(c).tolist() == [QNAN_BITS, QNAN_BITS] + bits(f32([-1.0, INF])).tolist()
    assert bits(s).tolist() == bits(f32([1.5, INF])).tolist() + [QNAN_BITS] + bits(f32([-INF])).tolist()
    assert (bits(sp)[1:] == QNAN_BITS).all() and sp[0] == 0.5
    assert bits(particle_aggregate(f32([[1.0], [2.0]]), f32([[INF], [-INF]]), 1, 1)[1])[0] == QNAN_BITS
    # the tail: T 1 is the minimum, T G the ordered mean
    ms = f32([[3.0, 0.1], [1.0, 0.2], [2.0, 0.3]])
    assert particle_aggregate(ms, ms, 1, 0)[0].tolist() == f32([1.0, 0.1]).tolist()
    assert particle_aggregate(ms, ms, 3, 0)[0][0] == 2.0
    m = (np.float64(ms[0, 1]) + np.float64(ms[1, 1]) + np.float64(ms[2, 1])) / 3.0
    assert bits(particle_aggregate(ms, ms, 3, 0)[0])[1] == bits(f32(m))


@pytest.mark.parametrize('G, N, T, cert_mode', [(2, 2, 1, 0), (3, 37, 2, 1), (7, 37, 7, 0), (32, 64, 16, 0)])
def test_synthetic_particles_show_every_case(G, N, T, cert_mode):
    x, cand, mean_in, std_in = synthetic_particles(G, N, 3, 3, 2, 2)
    for mode in (REACH, COST):
        ref = plan_particles_reference(x, cand, mean_in, std_in, G=G, N=N, score_tail=T, cert_mode=cert_mode,
                                       gamma=0.99, mode=mode, scales=SCALES, threshold=THRESHOLD, elites=max(1, N // 4),
                                       temperature=INF, momentum=0.0, min_std=0.05)
        assert_particles_synthetic_shows_every_case(ref, G, N, T, cert_mode)


# ------------------------------------------------------------------ 2. struct, constant, refusals
def test_struct_layout_and_constant():
    L = _lib.lib()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_abi_sizeof(b'drpo_plan_refit_particles_t') == ctypes.sizeof(_abi.PlanRefitParticles) \
        == ctypes.sizeof(_abi.PlanRefit) + 4 * 4 + 3 * ptr
    # the shared prefix: drpo_plan_refit_t's fields at drpo_plan_refit_t's offsets
    for name, _ in _abi.PlanRefit._fields_:
        assert getattr(_abi.PlanRefitParticles, name).offset == getattr(_abi.PlanRefit, name).offset, name
    c = lambda name: L.drpo_abi_const(name.encode())
    assert c('DRPO_PLAN_MAX_PARTICLES') == _abi.PLAN_MAX_PARTICLES == ops.PLAN_MAX_PARTICLES == 32
    assert 'drpo_plan_refit_particles' in _abi.PROTOTYPES
    assert L.drpo_version() >= 16            # the version that added the entry point


def _refit(**kw):
    d = _abi.PlanRefitParticles()
    d.P, d.N, d.H, d.K, d.A, d.C, d.mode, d.elites = 5, 37, 3, 3, 2, 2, 0, 4
    d.gamma, d.reward_scale, d.alive_bonus, d.constraint_scale, d.constraint_offset = 0.99, 1.0, 1.0, 10.0, 0.0
    d.temperature, d.momentum, d.min_std, d.threshold = math.inf, 0.0, 0.05, -0.1
    d.G, d.score_tail, d.cert_mode = 3, 2, 0
    for f in REFIT_INPUTS + ('violations',) + REFIT_STATE_OUTPUTS + REFIT_ROW_OUTPUTS + PARTICLE_OUTPUTS:
        setattr(d, f, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


PARTICLE_OUTPUTS = ('member_score', 'member_cert', 'score_spread')


def _call(d):
    return _lib.lib().drpo_plan_refit_particles(None if d is None else ctypes.byref(d), None)


def test_refit_particles_refuses_null_pointers():
    who = 'drpo_plan_refit_particles:'
    assert _call(None) == EINVAL
    assert _err().startswith(who) and 'null descriptor' in _err()
    for f in REFIT_INPUTS:
        assert _call(_refit(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null input pointer' in _err()
    for f in REFIT_STATE_OUTPUTS:
        assert _call(_refit(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null per-state output pointer' in _err()
    assert _call(_refit(mode=1, violations=None)) == EINVAL
    assert _err().startswith(who) and 'null violations in cost mode' in _err()


@pytest.mark.parametrize('kw, fragment', [
    # what drpo_plan_refit refuses
    ({'N': 1}, 'N=1 outside 2..1024'), ({'N': 1025}, 'N=1025 outside 2..1024'), ({'P': -1}, 'P=-1 is negative'),
    ({'P': 2 ** 31 - 1, 'N': 1024}, 'exceed int32'),
    ({'H': 0}, 'H=0 outside 1..128'), ({'H': 129, 'K': 129}, 'H=129 outside 1..128'),
    ({'K': 0}, 'K=0 outside 1..H=3'), ({'K': 4}, 'K=4 outside 1..H=3'), ({'A': 0}, 'A=0, need A >= 1'),
    ({'C': 0}, 'C=0, need C >= 1'), ({'mode': 2}, 'mode 2'), ({'mode': -1}, 'mode -1'),
    ({'gamma': math.nan}, 'gamma'), ({'gamma': 1.01}, 'gamma'), ({'gamma': -0.01}, 'gamma'),
    ({'elites': 0}, 'elites=0 outside 1..N=37'), ({'elites': 38}, 'elites=38 outside 1..N=37'),
    ({'temperature': 0.0}, 'temperature'), ({'temperature': -1.0}, 'temperature'),
    ({'temperature': math.nan}, 'temperature'),
    ({'momentum': 1.0}, 'momentum'), ({'momentum': -0.1}, 'momentum'), ({'momentum': math.nan}, 'momentum'),
    ({'min_std': -0.1}, 'min_std'), ({'min_std': math.inf}, 'min_std'), ({'min_std': math.nan}, 'min_std'),
    ({'threshold': math.nan}, 'threshold is NaN'),
    # and its own
    ({'G': 0}, 'G=0 outside 1..32'), ({'G': 33, 'score_tail': 33}, 'G=33 outside 1..32'),
    ({'G': -1}, 'G=-1 outside 1..32'),
    ({'score_tail': 0}, 'score_tail=0 outside 1..G=3'), ({'score_tail': 4}, 'score_tail=4 outside 1..G=3'),
    ({'cert_mode': 2}, 'cert_mode 2'), ({'cert_mode': -1}, 'cert_mode -1'),
    ({'P': 2 ** 20, 'N': 1024, 'G': 4, 'score_tail': 1}, 'G*P*N = 4294967296 rows exceed int32'),
    ({'P': 2 ** 16, 'N': 1024, 'G': 32}, 'G*P*N'),
])
def test_refit_particles_refuses_before_any_launch(kw, fragment):
    assert _call(_refit(**kw)) == EINVAL
    assert _err().startswith('drpo_plan_refit_particles:') and fragment in _err(), _err()


def test_refit_particles_of_no_state_is_ok_without_a_launch():
    for kw in ({}, {'G': 1, 'score_tail': 1}, {'G': 32, 'score_tail': 32}, {'G': 32, 'score_tail': 1}, {'cert_mode': 1},
               {'mode': 1}, {'violations': None}, dict.fromkeys(REFIT_ROW_OUTPUTS + PARTICLE_OUTPUTS, None)):
        assert _call(_refit(P=0, **kw)) == OK, kw


# ------------------------------------------------------------------ 3. the Python refusals
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


@pytest.fixture
def seen(monkeypatch):
    calls = []
    for name in ('plan_sample', 'plan_refit', '_terminal_critics', 'rollout_trajectories', 'lookahead'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    return calls


def _bad_particles(alg):
    E = alg.model_ensemble.ensemble_size
    return [({'particles': 'each'}, 'particles'), ({'particles': 'all'}, 'particles'),
            ({'particles': []}, 'particles: 0'),
            ({'particles': [0] * 33}, 'particles: 33'), ({'particles': [E]}, 'not a member index'),
            ({'particles': [-1]}, 'not a member index'), ({'particles': [0.0]}, 'not a member index'),
            ({'particles': [True]}, 'not a member index'), ({'particles': 3}, 'particles'),
            ({'particles': [0], 'members': 0}, 'particles together with members'),
            ({'particles': 'elites', 'members': [0, 0, 0]}, 'particles together with members'),
            ({'particles': [0], 'noise': TapeNoise([])}, 'recorded tape')]


def test_plan_refuses_before_any_device_work(alg, seen):
    s = torch.zeros(4, alg.state_dim)
    bad = _bad_particles(alg) + [
        ({'particles': [0, 1], 'risk': 'best'}, 'risk'), ({'particles': [0, 1], 'risk': ('cvar', 0.0)}, 'risk'),
        ({'particles': [0, 1], 'risk': ('cvar', 1.5)}, 'risk'),
        ({'particles': [0, 1], 'risk': ('cvar', math.nan)}, 'risk'),
        ({'particles': [0, 1], 'risk': ('cvar',)}, 'risk'), ({'particles': [0, 1], 'risk': ('var', 0.5)}, 'risk'),
        ({'particles': [0, 1], 'risk': 0.5}, 'risk'), ({'particles': [0, 1], 'risk': None}, 'risk'),
        ({'particles': [0, 1], 'cert_risk': 'worst'}, 'cert_risk'),
        ({'particles': [0, 1], 'cert_risk': None}, 'cert_risk'),
        ({'particles': [0, 1], 'cert_risk': 0}, 'cert_risk'),
        ({'risk': 'worst'}, 'without particles'), ({'risk': ('cvar', 0.5)}, 'without particles'),
        ({'cert_risk': 'mean'}, 'without particles'), ({'members': 0, 'risk': 'worst'}, 'without particles'),
        ({'members': 'each'}, 'members'),                       # 'each' stays refused: it is particles='elites'
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            alg.plan(s, **dict({'horizon': 3, 'candidates': 8}, **kw))
        with pytest.raises(ValueError, match=match):
            alg.mpc(**dict({'horizon': 3, 'candidates': 8}, **kw))
    assert seen == [] and alg.__dict__.get('_plan_noise') is None


def test_the_checks_resolve_the_tail_and_the_cert_mode(alg, monkeypatch):
    import inspect
    s = torch.zeros(4, alg.state_dim)
    E = alg.model_ensemble.ensemble_size
    assert E >= 3

    def resolve(**kw):
        bound = inspect.signature(alg.plan).bind(s, horizon=3, candidates=8, **kw)
        bound.apply_defaults()
        q = alg._plan_checks(**bound.arguments)
        return q['parts'], q['score_tail'], q['cert_mode']
    assert resolve() == (None, None, 0)
    assert resolve(particles=[2, 0, 2]) == ([2, 0, 2], 3, 0)
    assert resolve(particles=np.array([1, 2]), risk='worst', cert_risk='mean') == ([1, 2], 1, 1)
    monkeypatch.setattr(alg.model_ensemble, '_elite_inds', [2, 0, 1], raising=False)     # (a fit sets them)
    assert resolve(particles='elites') == ([2, 0, 1], 3, 0)
    seven = [0, 1, 2] * 2 + [0]
    for alpha, T in ((0.5, 4), (1.0, 7), (0.01, 1), (0.3, 3), (np.float32(0.5), 4)):
        assert resolve(particles=seven, risk=('cvar', alpha)) == (seven, T, 0), alpha
    assert resolve(particles=[0] * 32, risk=('cvar', 0.5))[1] == 16
    c = alg.mpc(horizon=3, candidates=8, particles=[0, 1], risk=('cvar', 0.5), cert_risk='mean')
    assert c.plan_kwargs['particles'] == [0, 1] and c.plan_kwargs['risk'] == ('cvar', 0.5)


def test_imagine_refuses_before_any_device_work(alg, monkeypatch):
    calls = []
    for mod, name in ((_lib, 'require_device'), (ops, '_start_states'), (ops, '_rollout_static'),
                      (ops, 'rollout_trajectories')):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **kw: calls.append(_n))
    s = torch.zeros(alg.rollout_batch_size, alg.state_dim)
    for kw, match in _bad_particles(alg) + [({'particles': [0], 'members': 'each'}, 'particles together with members')]:
        with pytest.raises(ValueError, match=match):
            alg.imagine(s, **kw)
    assert calls == []


def test_plan_result_names_its_particle_fields():
    assert ops.PlanResult.PARTICLE_FIELDS == ('particles', 'risk', 'cert_risk', 'member_scores', 'member_certificates',
                                              'score_spread')
    r = ops.PlanResult(**{k: i for i, k in enumerate(ops.PlanResult.FIELDS)})
    assert all(getattr(r, k) is None for k in ops.PlanResult.PARTICLE_FIELDS)
    r = ops.PlanResult(**{k: i for i, k in enumerate(ops.PlanResult.FIELDS)}, particles=[1, 2], risk='worst',
                       cert_risk='max', member_scores=1, member_certificates=2, score_spread=3)
    assert r.particles == [1, 2] and r.score_spread == 3 and r.safe_action is None


def test_stacked_runs_flatten_run_major():
    spec = ops._traj_spec(3, 2, 4, 2, 1)
    runs = [ops.ImaginedRollout(m, 1, **{n: torch.full(shape, float(m)).to(dtype) for n, shape, dtype, _ in spec})
            for m in (5, 6)]
    im = ops.ImaginedRollout.stack(runs)
    flat = im.flat_runs()
    assert im.particle_launches is None and flat.given_steps == 1
    assert flat.rewards.shape == (6, 2) and flat.states.shape == (6, 3, 4) and flat.lengths.shape == (6,)
    assert flat.rewards[:3].eq(5).all() and flat.rewards[3:].eq(6).all()
    assert flat.rewards.data_ptr() == im.rewards.data_ptr()            # views: no copy
