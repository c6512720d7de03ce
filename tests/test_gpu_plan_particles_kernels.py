"""drpo_plan_refit_particles (csrc/plan.hip) against plan_particles_helpers' float64 reference, bit for
bit on every output (float32 compared as int32; integers as they are).

P 5 start states of G member-major runs (plan_particles_helpers.synthetic_particles: plan_helpers'
synthetic candidates per member, edited where the members must differ: member orders that change
from candidate to candidate, equal member scores, +-inf, a NaN in one member, a row that one
member alone does not certify; with plan_helpers' states without a feasible and without a valid
row. Both asserts on the reference hold the inputs to that before anything is compared). CASES
reach G 1, 2, 3, 7, 32; N 2, 64, 257 (two passes of the 256 lanes, the second of one lane) and
1024 with G 32 once (four passes on 32 KB of member scores: 54,304 bytes of LDS; the maximum, at
H 128, is 1,016 bytes more, and its reference would take minutes); H 1, 5, 128; T 1, a middle value
and G; both cert modes, both modes. Every case runs at temperature inf, where the weights are
exactly 1 and both sides' refit is ordered double sums, correctly rounded divisions and square
roots: mean, std and weight are compared exactly too. Outputs start as a sentinel: every element
is written.

G 1 against drpo_plan_refit on identical inputs, at a finite temperature too: the same device code."""
import ctypes

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib
from gpu_helpers import DEV
from lookahead_helpers import COST, REACH, weights
from plan_helpers import (INF, PER_ROW, PER_STATE, SCALES, THRESHOLD, assert_bits,
                          assert_plan_synthetic_shows_every_case, plan_scores, synthetic_plan)
from plan_particles_helpers import (assert_particles_synthetic_shows_every_case, plan_particles_reference,
                                    synthetic_particles)

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ISENTINEL = -77
GAMMA = 0.99
MIN_STD = 0.05
PARTICLE_OUT = ('member_score', 'member_cert', 'score_spread')

# (G, N, H, K, A, C, mode, T, cert_mode, elites, momentum)
R, Cm = REACH, COST
CASES = [
    (1, 2, 1, 1, 1, 1, R, 1, 0, 1, 0.0), (1, 64, 5, 5, 2, 2, Cm, 1, 1, 16, 0.25),
    (2, 2, 5, 1, 2, 2, Cm, 1, 0, 2, 0.0), (2, 64, 1, 1, 5, 1, R, 2, 1, 16, 0.25),
    (2, 257, 5, 5, 2, 2, R, 1, 1, 64, 0.0), (3, 64, 5, 5, 2, 2, R, 2, 0, 16, 0.0),
    (3, 257, 1, 1, 1, 2, Cm, 3, 0, 257, 0.25), (3, 2, 128, 128, 2, 1, R, 1, 1, 1, 0.0),
    (7, 64, 128, 1, 2, 1, Cm, 4, 0, 16, 0.0), (7, 257, 5, 5, 2, 1, R, 7, 1, 64, 0.25),
    (7, 2, 1, 1, 1, 2, R, 1, 0, 2, 0.0),
    (7, 64, 5, 5, 5, 2, Cm, 1, 1, 1, 0.0), (32, 64, 5, 1, 2, 2, R, 16, 0, 16, 0.0),
    (32, 2, 128, 128, 1, 1, Cm, 32, 1, 1, 0.25), (32, 257, 1, 1, 2, 1, Cm, 1, 0, 64, 0.0),
    (32, 1024, 1, 1, 2, 1, R, 8, 0, 256, 0.0),
]


def _id(c):
    G, N, H, K, A, C, mode, T, cm, elites, mom = c
    return f'G{G}-N{N}-H{H}-K{K}-A{A}-C{C}-{"reach" if mode == REACH else "cost"}-T{T}-{"max" if cm == 0 else "mean"}' \
           f'-e{elites}-m{mom}'


def _launch(x, cand, mean_in, std_in, G, N, mode, T, cert_mode, elites, temperature, mom, particles=True,
            optional=True):
    """One drpo_plan_refit_particles call (particles=False: drpo_plan_refit) on CPU tensors: a dict of
    the outputs (None for one not given)."""
    P, K, A = mean_in.shape
    H = x['rewards'].shape[1]
    C = x['terminal_qc'].shape[-1]
    dev = {k: v.to(DEV).contiguous() for k, v in x.items()}
    dev.update(cand=cand.to(DEV).contiguous(), mean_in=mean_in.to(DEV).contiguous(), std_in=std_in.to(DEV).contiguous())
    w = torch.from_numpy(weights(GAMMA, H)).to(DEV)
    f = lambda *s: torch.full(s, SENTINEL, device=DEV)
    i = lambda *s: torch.full(s, ISENTINEL, dtype=torch.int32, device=DEV)
    out = {'mean_out': f(P, K, A), 'std_out': f(P, K, A), 'best_actions': f(P, K, A), 'best': i(P), 'n_feasible': i(P),
           'best_score': f(P), 'best_cert': f(P), 'best_feasible': torch.full((P,), 77, dtype=torch.uint8, device=DEV),
           'score': f(P, N) if optional else None, 'cert': f(P, N) if optional else None,
           'rank': i(P, N) if optional else None, 'weight': f(P, N) if optional else None}
    d = _abi.PlanRefitParticles() if particles else _abi.PlanRefit()
    if particles:
        d.G, d.score_tail, d.cert_mode = G, T, cert_mode
        out.update(member_score=f(G, P, N) if optional else None, member_cert=f(G, P, N) if optional else None,
                   score_spread=f(P, N) if optional else None)
    d.P, d.N, d.H, d.K, d.A, d.C, d.mode, d.elites = P, N, H, K, A, C, mode, elites
    d.gamma, d.temperature, d.momentum, d.min_std, d.threshold = GAMMA, temperature, mom, MIN_STD, THRESHOLD
    for k, v in SCALES.items():
        setattr(d, k, v)
    for k, v in dev.items():
        setattr(d, k, v.data_ptr())
    if mode == REACH:
        d.violations = None                                   # may be null there
    d.weights = w.data_ptr()
    for k, v in out.items():
        setattr(d, k, None if v is None else v.data_ptr())
    fn = _lib.lib().drpo_plan_refit_particles if particles else _lib.lib().drpo_plan_refit
    _lib.check(fn(ctypes.byref(d), _lib.stream()), 'plan_refit_particles')
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, optional=True):
    for k in PER_STATE + ('best_actions',) + ((PER_ROW + PARTICLE_OUT) if optional else ()):
        g = got[k].astype(bool) if k == 'best_feasible' else got[k]
        assert k != 'best_feasible' or set(np.unique(got[k]).tolist()) <= {0, 1}
        assert_bits(g, ref[k], k)
    assert_bits(got['mean_out'], ref['mean'], 'mean')
    assert_bits(got['std_out'], ref['std'], 'std')


def _reference(case):
    G, N, H, K, A, C, mode, T, cm, elites, mom = case
    x, cand, mean_in, std_in = synthetic_particles(G, N, H, K, A, C)
    ref = plan_particles_reference(x, cand, mean_in, std_in, G=G, N=N, score_tail=T, cert_mode=cm, gamma=GAMMA,
                                   mode=mode, scales=SCALES, threshold=THRESHOLD, elites=elites, temperature=INF,
                                   momentum=mom, min_std=MIN_STD)
    return x, cand, mean_in, std_in, ref


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_refit_particles_equals_the_reference(case):
    G, N, H, K, A, C, mode, T, cm, elites, mom = case
    x, cand, mean_in, std_in, ref = _reference(case)
    if G == 1:          # plan_helpers' own rows
        assert_plan_synthetic_shows_every_case(x, ref, N, H, elites)
    assert_particles_synthetic_shows_every_case(ref, G, N, T, cm)
    got = _launch(x, cand, mean_in, std_in, G, N, mode, T, cm, elites, INF, mom)
    _compare(got, ref)
    for k, v in got.items():        # every element written
        assert not (v == (SENTINEL if v.dtype == np.float32 else 77 if v.dtype == np.uint8 else ISENTINEL)).any(), k


def test_cases_reach_what_they_should():
    seen = lambda i: {c[i] for c in CASES}
    assert seen(0) == {1, 2, 3, 7, 32} and seen(1) == {2, 64, 257, 1024} and seen(2) == {1, 5, 128}
    assert seen(5) == {1, 2} and seen(6) == {REACH, COST} and seen(8) == {0, 1}
    assert [c[:2] for c in CASES if c[1] == 1024] == [(32, 1024)]
    for G in (2, 3, 7, 32):
        mine = [c for c in CASES if c[0] == G]
        assert {c[8] for c in mine} == {0, 1} and {c[6] for c in mine} == {REACH, COST}, G
        assert 1 in {c[7] for c in mine}, G
    assert {c[7] for c in CASES if c[0] == 7} == {1, 4, 7} and {c[7] for c in CASES if c[0] == 32} == {1, 8, 16, 32}
    assert {c[7] for c in CASES if c[0] == 3} == {1, 2, 3} and {c[7] for c in CASES if c[0] == 2} == {1, 2}
    assert any(c[2] == 128 and c[0] > 1 and c[1] > 2 for c in CASES)
    # the dynamic LDS of the largest case, and of the largest launch the entry point admits
    lds = lambda N, H, G: 8 * (H + 1 + N) + 4 * 3 * N + 16 + N + 4 * 256 * G
    assert lds(1024, 1, 32) == 54304 and lds(1024, 128, 32) == 55320 < 65536


@pytest.mark.parametrize('temperature', [INF, 0.5])
@pytest.mark.parametrize('N, H, K, A, C, mode',
                         [(64, 5, 5, 2, 2, REACH), (257, 5, 1, 2, 1, COST), (1024, 1, 1, 5, 2, REACH)])
def test_one_particle_is_the_refit_launch(N, H, K, A, C, mode, temperature):
    x, cand, mean_in, std_in = synthetic_plan(N, H, K, A, C)
    elites = max(1, N // 4)
    want = _launch(x, cand, mean_in, std_in, 1, N, mode, 1, 0, elites, temperature, 0.25, particles=False)
    for cert_mode in (0, 1):
        got = _launch(x, cand, mean_in, std_in, 1, N, mode, 1, cert_mode, elites, temperature, 0.25)
        for k in want:
            assert_bits(got[k], want[k], k)
        assert_bits(got['member_score'][0], want['score'], 'member_score')
        assert_bits(got['member_cert'][0], want['cert'], 'member_cert')
        # the spread of one value: 0, or NaN where the value is not finite
        finite = np.isfinite(want['score'])
        assert not got['score_spread'][finite].any() and np.isnan(got['score_spread'][~finite]).all()


def test_refit_particles_without_the_optional_outputs():
    case = (3, 64, 5, 5, 2, 2, R, 2, 0, 16, 0.0)
    G, N, H, K, A, C, mode, T, cm, elites, mom = case
    x, cand, mean_in, std_in, ref = _reference(case)
    got = _launch(x, cand, mean_in, std_in, G, N, mode, T, cm, elites, INF, mom, optional=False)
    assert all(got[k] is None for k in PER_ROW + PARTICLE_OUT)
    _compare(got, ref, optional=False)
