"""Planning on the model without a GPU: the definition of drpo_plan_refit on an example worked by
hand (plan_helpers.plan_refit_reference, which the GPU tests hold the kernel to), the synthetic
candidates, the two structs and every refusal of drpo_plan_sample / drpo_plan_refit (calls that
fail before any launch; pointers are dummies the host never dereferences), the constants, and
every Python refusal of SMBPO.plan."""
import ctypes
import math

import numpy as np
import pytest
import torch

import rng_model
from drpo_amd import _abi, _lib, ops
from drpo_amd.rng import TapeNoise
from lookahead_helpers import COST, NAN, QNAN_BITS, REACH
from plan_helpers import (INF, P_STATES, SCALES, THRESHOLD, assert_bits, assert_plan_synthetic_shows_every_case, bits,
                          plan_order, plan_refit_reference, plan_sample_reference, synthetic_plan)
from test_host_logic import make_smbpo
from test_rollout_traj_checks import EINVAL, OK, P, _err


# ------------------------------------------------------------------ 1. the definition, by hand
def _example():
    """P 1, N 4, H 2, K 2, A 1, C 1; discount 0.5, reward_scale 1, alive_bonus 1, constraint_scale
    10, constraint_offset 0.5, threshold -0.25. Every number is dyadic, so every step is exact.

    Row 0 lives to the horizon: r' = [2, 3], score 2 + 3/2 + 4/4 = 4.5; h' = [-1.25, -2.5], from the
      bootstrap -1: -1.25 + max(-2.5, -1)/2 = -1.75, then -0.625 + max(-1.25, -1.75)/2 = -1.25; cost:
      -1/2, then -1/4 (equal to the threshold: feasible).
    Row 1 ends at step 0 (terminated; its NaN terminal inputs must not show): score r' = 4;
      h' = 2.5 + 0.5 = 3, done: cert 3; cost: a violation at a done step: 1.
    Row 2 has length 0: score and cert are its bootstraps 4.5 (the tie with row 0) and -0.5.
    Row 3: r' = [1, 1], score 1 + 1/2 + 8/4 = 3.5; h' = [0, -5], from 0.25: -2.5 + 0.25/2 = -2.375,
      then 0 + max(0, -2.375)/2 = 0; cost: 0.25/2 = 0.125, then 1 + 0.0625."""
    x = dict(rewards=torch.tensor([[1.0, 2.0], [3.0, 0.0], [0.0, 0.0], [0.0, 0.0]]),
             constraint_values=torch.tensor([[[-0.125], [-0.25]], [[0.25], [0.0]], [[0.0], [0.0]], [[0.0], [-0.5]]]),
             dones=torch.tensor([[False, False], [True, False], [False, False], [False, False]]),
             violations=torch.tensor([[False, False], [True, False], [False, False], [True, False]]),
             lengths=torch.tensor([2, 1, 0, 2], dtype=torch.int32),
             terminated=torch.tensor([False, True, False, False]),
             terminal_q=torch.tensor([4.0, NAN, 4.5, 8.0]),
             terminal_qc=torch.tensor([[-1.0], [NAN], [-0.5], [0.25]]))
    scales = dict(reward_scale=1.0, alive_bonus=1.0, constraint_scale=10.0, constraint_offset=0.5)
    cand = torch.tensor([[[0.5], [-0.5]], [[1.0], [1.0]], [[-0.5], [0.25]], [[0.0], [0.0]]])
    mean_in, std_in = torch.tensor([[[1.0], [1.0]]]), torch.tensor([[[0.25], [0.125]]])
    score = [4.5, 4.0, 4.5, 3.5]
    cert = {REACH: [-1.25, 3.0, -0.5, 0.0], COST: [-0.25, 1.0, -0.5, 1.0625]}
    # feasible rows 0 and 2 (equal scores: the lower n first), then by cert ascending
    rank = {REACH: [0, 3, 1, 2], COST: [0, 2, 1, 3]}
    return x, scales, cand, mean_in, std_in, score, cert, rank


@pytest.mark.parametrize('mode', [REACH, COST], ids=['reachability', 'cost'])
@pytest.mark.parametrize('elites', [2, 3])
def test_reference_on_the_example_worked_by_hand(mode, elites):
    x, scales, cand, mean_in, std_in, score, cert, rank = _example()
    out = plan_refit_reference(x, cand, mean_in, std_in, N=4, gamma=0.5, mode=mode, scales=scales, threshold=-0.25,
                               elites=elites, temperature=INF, momentum=0.5, min_std=0.3125)
    f32 = lambda v: np.asarray(v, np.float32)
    assert_bits(out['score'], f32([score]), 'score')
    assert_bits(out['cert'], f32([cert[mode]]), 'cert')
    assert out['rank'].tolist() == [rank[mode]]
    assert out['best'].tolist() == [0] and out['n_feasible'].tolist() == [2]        # elites 3: Ke = n_feasible
    assert out['weight'].tolist() == [[1.0, 0.0, 1.0, 0.0]]
    assert_bits(out['best_score'], f32([4.5]), 'best_score')
    assert_bits(out['best_cert'], f32([cert[mode][0]]), 'best_cert')
    assert out['best_feasible'].tolist() == [True]
    assert_bits(out['best_actions'], f32([[[0.5], [-0.5]]]), 'best_actions')
    # m = [0, -0.125]; v = [0.25, 0.375^2]; mean = m/2 + 1/2; std = [0.5, 0.375]/2 + [0.25, 0.125]/2, floor 0.3125
    assert_bits(out['mean'], f32([[[0.5], [0.4375]]]), 'mean')
    assert_bits(out['std'], f32([[[0.375], [0.3125]]]), 'std')


def test_reference_rules():
    x, scales, cand, mean_in, std_in, score, cert, rank = _example()
    kw = dict(N=4, gamma=0.5, mode=REACH, scales=scales, elites=2, temperature=INF, momentum=0.0, min_std=0.0)
    # lengths are clamped as read
    y = dict(x, lengths=torch.tensor([200, 1, -3, 2], dtype=torch.int32))
    a, b = plan_refit_reference(x, cand, mean_in, std_in, threshold=-0.25, **kw), \
        plan_refit_reference(y, cand, mean_in, std_in, threshold=-0.25, **kw)
    for k in a:
        assert_bits(a[k], b[k], k)
    # no feasible row: the least certificates are the elites, keyed by -cert
    none = plan_refit_reference(x, cand, mean_in, std_in, threshold=-INF, **kw)
    assert none['n_feasible'].tolist() == [0] and none['rank'].tolist() == [[0, 3, 1, 2]]
    assert none['best'].tolist() == [0] and none['best_feasible'].tolist() == [False]
    assert none['weight'].tolist() == [[1.0, 0.0, 1.0, 0.0]]
    # every row feasible: the argmax of the score, ties to the lower n
    every = plan_refit_reference(x, cand, mean_in, std_in, threshold=INF, **kw)
    assert every['n_feasible'].tolist() == [4] and every['rank'].tolist() == [[0, 2, 1, 3]]
    # a finite temperature: exp((key - best) / T) over the elites, in double
    warm = plan_refit_reference(x, cand, mean_in, std_in, threshold=INF, **dict(kw, elites=4, temperature=0.5))
    want = [1.0, math.exp(-1.0), 1.0, math.exp(-2.0)]
    assert_bits(warm['weight'], np.asarray([want], np.float64).astype(np.float32), 'weight')
    m0 = (0.5 + want[1] * 1.0 + -0.5) / (1.0 + want[1] + 1.0 + want[3])
    assert abs(float(warm['mean'][0, 0, 0]) - m0) <= 2 ** -23 * abs(m0)
    # no valid row: mean and std pass through, best 0
    z = dict(x, terminal_q=torch.full((4,), NAN), terminated=torch.zeros(4, dtype=torch.bool))
    dead = plan_refit_reference(z, cand, mean_in, std_in, threshold=0.0, **kw)
    assert dead['best'].tolist() == [0] and dead['n_feasible'].tolist() == [0] and dead['rank'].tolist() == [[0, 1, 2, 3]]
    assert_bits(dead['mean'], mean_in.numpy(), 'mean')
    assert_bits(dead['std'], std_in.numpy(), 'std')
    assert (bits(dead['score']) == QNAN_BITS).all() and not dead['weight'].any()
    # -0.0 and 0.0 tie
    order, cls, key = plan_order(np.float32([0.0, -0.0, 0.0]), np.float32([-1, -1, -1]), 0.0)
    assert order == [0, 1, 2] and cls == [0, 0, 0]


@pytest.mark.parametrize('N, H, C, elites', [(2, 1, 1, 1), (2, 3, 2, 2), (37, 3, 2, 9), (37, 1, 1, 37), (256, 3, 1, 64)])
def test_synthetic_candidates_show_every_case(N, H, C, elites):
    x, cand, mean_in, std_in = synthetic_plan(N, H, H, 2, C)
    for mode in (REACH, COST):
        ref = plan_refit_reference(x, cand, mean_in, std_in, N=N, gamma=0.99, mode=mode, scales=SCALES,
                                   threshold=THRESHOLD, elites=elites, temperature=INF, momentum=0.0, min_std=0.05)
        assert_plan_synthetic_shows_every_case(x, ref, N, H, elites)
        for p in range(P_STATES):
            assert sorted(ref['rank'][p].tolist()) == list(range(N))
        # the mutation check's two wrong definitions give other answers on these rows
        flipped = plan_refit_reference(x, cand, mean_in, std_in, N=N, gamma=0.99, mode=mode, scales=SCALES,
                                       threshold=THRESHOLD, elites=elites, temperature=INF, momentum=0.0, min_std=0.05,
                                       flip_ties=True)
        blind = plan_refit_reference(x, cand, mean_in, std_in, N=N, gamma=0.99, mode=mode, scales=SCALES,
                                     threshold=THRESHOLD, elites=elites, temperature=INF, momentum=0.0, min_std=0.05,
                                     ignore_feasibility=True)
        assert (flipped['rank'] != ref['rank']).any() and (blind['rank'] != ref['rank']).any()
        assert (blind['n_feasible'] != ref['n_feasible']).any()


def test_sample_reference():
    g = torch.Generator().manual_seed(4)
    mean, std, inc = torch.rand(3, 2, 2, generator=g) - 0.5, torch.rand(3, 2, 2, generator=g), \
        torch.rand(3, 2, 2, generator=g)
    x, radius = plan_sample_reference(mean, std, inc, N=5, seed=77, ctr=3)
    assert x.shape == radius.shape == (15, 2, 2) and x.dtype == np.float64
    assert np.array_equal(x.reshape(3, 5, 2, 2)[:, 0], inc.numpy().astype(np.float64))
    assert (np.abs(x) <= 1.0).all() and (radius > 0).all()
    # element (r, t, a) draws normal_at((r K + t) A + a): row 7, t 1, a 0 is index 30
    z, _ = rng_model.normal_at(77, 3, _abi.PLAN_SITE, np.arange(30, 31))
    want = min(max(float(std[1, 1, 0]) * z[0] + float(mean[1, 1, 0]), -1.0), 1.0)
    assert x[7, 1, 0] == want
    wide, _ = plan_sample_reference(mean, std * 100, inc, N=5, seed=77, ctr=3, lo=-0.25, hi=0.5)
    drawn = wide.reshape(3, 5, 2, 2)[:, 1:]
    assert (drawn == -0.25).any() and (drawn == 0.5).any() and ((drawn >= -0.25) & (drawn <= 0.5)).all()
    other, _ = plan_sample_reference(mean, std, inc, N=5, seed=77, ctr=4)
    assert not np.array_equal(other, x)


# ------------------------------------------------------------------ 2. structs, constants, refusals
def test_struct_layouts_constants_and_version():
    L = _lib.lib()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_abi_sizeof(b'drpo_plan_sample_t') == ctypes.sizeof(_abi.PlanSample) == 4 * 4 + 2 * 4 + 2 * 8 + 4 * ptr
    assert L.drpo_abi_sizeof(b'drpo_plan_refit_t') == ctypes.sizeof(_abi.PlanRefit) == 8 * 4 + 8 * 8 + 8 + 24 * ptr
    assert L.drpo_version() >= 13            # the version that added the entry points
    c = lambda name: L.drpo_abi_const(name.encode())
    assert c('DRPO_PLAN_MAX_CANDIDATES') == _abi.PLAN_MAX_CANDIDATES == ops.PLAN_MAX_CANDIDATES == 1024
    assert c('DRPO_PLAN_SITE') == _abi.PLAN_SITE == ops.PLAN_SITE


def test_the_site_is_no_other_sites():
    """DESIGN's counter table: the normal_at sites, the gather's and the batch sampler's third word,
    and the rollout engines' q = 0..16."""
    taken = set(rng_model.NORMAL_AT_SITES) | {rng_model.SITE_GATHER, rng_model.SITE_SAMPLE_BATCH} | set(range(17))
    assert _abi.PLAN_SITE not in taken and 0 < _abi.PLAN_SITE < 2 ** 32


def _sample(**kw):
    d = _abi.PlanSample()
    d.P, d.N, d.K, d.A, d.lo, d.hi, d.seed, d.ctr = 5, 37, 3, 2, -1.0, 1.0, 1, 2
    for f in SAMPLE_POINTERS:
        setattr(d, f, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


SAMPLE_POINTERS = ('mean', 'std', 'incumbent', 'cand')


def _call_sample(d):
    return _lib.lib().drpo_plan_sample(None if d is None else ctypes.byref(d), None)


def test_sample_refuses_null_pointers():
    who = 'drpo_plan_sample:'
    assert _call_sample(None) == EINVAL
    assert _err().startswith(who) and 'null descriptor' in _err()
    for f in SAMPLE_POINTERS:
        assert _call_sample(_sample(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null pointer' in _err()


@pytest.mark.parametrize('kw, fragment', [
    ({'N': 1}, 'N=1 outside 2..1024'), ({'N': 0}, 'outside 2..1024'), ({'N': 1025}, 'N=1025 outside 2..1024'),
    ({'N': -4}, 'outside 2..1024'), ({'K': 0}, 'K=0, need K >= 1'), ({'K': -1}, 'need K >= 1'),
    ({'A': 0}, 'A=0, need A >= 1'), ({'P': -1}, 'P=-1 is negative'), ({'lo': 0.5, 'hi': 0.25}, 'clamp'),
    ({'lo': math.nan}, 'clamp'), ({'hi': math.nan}, 'clamp'),
    ({'P': 2 ** 31 - 1, 'N': 1024, 'K': 128, 'A': 64}, 'exceed one grid'),
])
def test_sample_refuses_before_any_launch(kw, fragment):
    assert _call_sample(_sample(**kw)) == EINVAL
    assert _err().startswith('drpo_plan_sample:') and fragment in _err(), _err()


def test_sample_of_no_state_is_ok_without_a_launch():
    for kw in ({}, {'N': 2}, {'N': 1024}, {'lo': 0.0, 'hi': 0.0}, {'lo': -math.inf, 'hi': math.inf}):
        assert _call_sample(_sample(P=0, **kw)) == OK, kw


REFIT_INPUTS = ('rewards', 'constraint_values', 'dones', 'lengths', 'terminated', 'weights', 'terminal_q',
                'terminal_qc', 'cand', 'mean_in', 'std_in')
REFIT_STATE_OUTPUTS = ('mean_out', 'std_out', 'best_actions', 'best', 'n_feasible', 'best_score', 'best_cert',
                       'best_feasible')
REFIT_ROW_OUTPUTS = ('score', 'cert', 'rank', 'weight')


def _refit(**kw):
    d = _abi.PlanRefit()
    d.P, d.N, d.H, d.K, d.A, d.C, d.mode, d.elites = 5, 37, 3, 3, 2, 2, 0, 4
    d.gamma, d.reward_scale, d.alive_bonus, d.constraint_scale, d.constraint_offset = 0.99, 1.0, 1.0, 10.0, 0.0
    d.temperature, d.momentum, d.min_std, d.threshold = math.inf, 0.0, 0.05, -0.1
    for f in REFIT_INPUTS + ('violations',) + REFIT_STATE_OUTPUTS + REFIT_ROW_OUTPUTS:
        setattr(d, f, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call_refit(d):
    return _lib.lib().drpo_plan_refit(None if d is None else ctypes.byref(d), None)


def test_refit_refuses_null_pointers():
    who = 'drpo_plan_refit:'
    assert _call_refit(None) == EINVAL
    assert _err().startswith(who) and 'null descriptor' in _err()
    for f in REFIT_INPUTS:
        assert _call_refit(_refit(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null input pointer' in _err()
    for f in REFIT_STATE_OUTPUTS:
        assert _call_refit(_refit(**{f: None})) == EINVAL, f
        assert _err().startswith(who) and 'null per-state output pointer' in _err()
    assert _call_refit(_refit(mode=1, violations=None)) == EINVAL
    assert _err().startswith(who) and 'null violations in cost mode' in _err()


@pytest.mark.parametrize('kw, fragment', [
    ({'N': 1}, 'N=1 outside 2..1024'), ({'N': 1025}, 'N=1025 outside 2..1024'), ({'P': -1}, 'P=-1 is negative'),
    ({'P': 2 ** 31 - 1, 'N': 1024}, 'exceed int32'),
    ({'H': 0}, 'H=0 outside 1..128'), ({'H': 129, 'K': 129}, 'H=129 outside 1..128'),
    ({'K': 0}, 'K=0 outside 1..H=3'), ({'K': 4}, 'K=4 outside 1..H=3'), ({'A': 0}, 'A=0, need A >= 1'),
    ({'C': 0}, 'C=0, need C >= 1'), ({'mode': 2}, 'mode 2'), ({'mode': -1}, 'mode -1'),
    ({'gamma': math.nan}, 'gamma'), ({'gamma': 1.01}, 'gamma'), ({'gamma': -0.01}, 'gamma'),
    ({'elites': 0}, 'elites=0 outside 1..N=37'), ({'elites': 38}, 'elites=38 outside 1..N=37'),
    ({'temperature': 0.0}, 'temperature'), ({'temperature': -1.0}, 'temperature'), ({'temperature': math.nan}, 'temperature'),
    ({'momentum': 1.0}, 'momentum'), ({'momentum': -0.1}, 'momentum'), ({'momentum': math.nan}, 'momentum'),
    ({'min_std': -0.1}, 'min_std'), ({'min_std': math.inf}, 'min_std'), ({'min_std': math.nan}, 'min_std'),
    ({'threshold': math.nan}, 'threshold is NaN'),
])
def test_refit_refuses_before_any_launch(kw, fragment):
    assert _call_refit(_refit(**kw)) == EINVAL
    assert _err().startswith('drpo_plan_refit:') and fragment in _err(), _err()


def test_refit_of_no_state_is_ok_without_a_launch():
    for kw in ({}, {'H': 128, 'K': 128}, {'K': 1}, {'elites': 37}, {'elites': 1}, {'temperature': 0.01},
               {'threshold': math.inf}, {'threshold': -math.inf}, {'mode': 1}, {'violations': None}, {'momentum': 0.25},
               {'min_std': 0.0}, dict.fromkeys(REFIT_ROW_OUTPUTS, None)):
        assert _call_refit(_refit(P=0, **kw)) == OK, kw


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


@pytest.mark.parametrize('kw, match', [
    ({'members': 'each'}, 'members'), ({'members': 'all'}, 'members'),
    ({'candidates': 1}, 'candidates'), ({'candidates': 1025}, 'candidates'), ({'candidates': 8.0}, 'candidates'),
    ({'candidates': True}, 'candidates'),
    ({'steps': 0}, 'steps'), ({'steps': 4}, 'steps'), ({'steps': 1.5}, 'steps'),
    ({'horizon': 0}, 'horizon'), ({'horizon': 129}, 'horizon'),
    ({'iterations': 0}, 'iterations'), ({'iterations': 2.0}, 'iterations'),
    ({'elites': 0}, 'elites'), ({'elites': 9}, 'elites'), ({'elites': 2.5}, 'elites'),
    ({'temperature': 0.0}, 'temperature'), ({'temperature': -1.0}, 'temperature'), ({'temperature': math.nan}, 'temperature'),
    ({'temperature': None}, 'temperature'),
    ({'momentum': 1.0}, 'momentum'), ({'momentum': -0.5}, 'momentum'), ({'momentum': math.nan}, 'momentum'),
    ({'min_std': -1.0}, 'min_std'), ({'min_std': math.inf}, 'min_std'), ({'min_std': math.nan}, 'min_std'),
    ({'init_std': 0.0}, 'init_std'), ({'init_std': -0.5}, 'init_std'), ({'init_std': math.inf}, 'init_std'),
    ({'init_std': math.nan}, 'init_std'),
    ({'threshold': math.nan}, 'threshold'), ({'threshold': 'low'}, 'threshold'),
    ({'lookahead': None}, 'lookahead'), ({'lookahead': False}, 'lookahead'), ({'lookahead': 'mean'}, 'lookahead'),
    ({'init': 'actor'}, 'init'), ({'init': 3}, 'init'), ({'init': torch.zeros(4, 3)}, 'init: shape'),
    ({'init': torch.zeros(4, 2, 2)}, 'init: shape'), ({'init': torch.zeros(3, 3, 2)}, 'init: shape'),
    ({'noise': TapeNoise([])}, 'recorded tape'),
])
def test_plan_refuses_before_any_device_work(alg, seen, kw, match):
    s = torch.zeros(4, alg.state_dim)
    assert alg.action_dim == 2
    with pytest.raises(ValueError, match=match):
        alg.plan(s, **dict({'horizon': 3, 'candidates': 8}, **kw))
    assert seen == [] and alg.__dict__.get('_plan_noise') is None


def test_plan_refuses_the_rest(alg, seen, monkeypatch):
    with pytest.raises(ValueError, match='start states'):
        alg.plan(None)
    with pytest.raises(TypeError):
        alg.plan(torch.zeros(4, alg.state_dim), halt=0.5)               # not an argument: out of scope
    with pytest.raises(TypeError):
        alg.plan(torch.zeros(4, alg.state_dim), shield=True)
    assert alg.solver.distributional_qc
    monkeypatch.setattr(alg.solver, 'distributional_qc', False)
    with pytest.raises(ValueError, match='needs a distributional constraint critic'):
        alg.plan(torch.zeros(4, alg.state_dim), lookahead='bound')
    monkeypatch.setattr(alg, 'env_params', None)
    with pytest.raises(NotImplementedError, match='constraint functions on the device'):
        alg.plan(torch.zeros(4, alg.state_dim))
    assert seen == []


def test_plan_result_names_its_fields():
    fields = ('actions', 'action', 'score', 'certificate', 'feasible', 'n_feasible', 'mean', 'std', 'history_score',
              'history_certificate', 'history_feasible', 'candidates', 'scores', 'certificates', 'ranks', 'imagined',
              'threshold', 'lookahead_kind')
    assert ops.PlanResult.FIELDS == fields
    r = ops.PlanResult(**{k: i for i, k in enumerate(fields)})
    assert r.actions == 0 and r.lookahead_kind == len(fields) - 1
    with pytest.raises(AssertionError):
        ops.PlanResult(actions=1)
