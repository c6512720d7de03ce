"""drpo_plan_refit and drpo_plan_sample (csrc/plan.hip) against plan_helpers' float64 references.

Refit. P 5 start states (plan_helpers.synthetic_plan, built by position: a state with no feasible
row, with exactly one, equal scores, no valid row, a cert equal to the threshold, NaN scores and
certs among valid rows, lengths 0..H terminated and not; assert_plan_synthetic_shows_every_case
holds the inputs to that before anything is compared). CASES is 30 of the products of N 2, 37, 256,
1024; H 1, 3, 128; K 1, H; A 1, 2, 5; C 1, 2; both modes; elites 1, N/4, N; temperature inf, 1,
0.01; momentum 0, 0.25. They reach: one partial pass of the 256 lanes (N 2, 37), one full pass and
four (N 256, 1024), the longest chain (H 128, with N 37 once: its reference is the slow one), a
refit of more (t, a) than lanes (K 128, A 5: 640) and of fewer, every elites rule (1, fewer feasible
rows than elites, all rows), and each temperature and momentum with each N.

Exact (float32 compared as int32; integers as they are): score, cert, rank, best, n_feasible, best_score,
best_cert, best_feasible, best_actions, and at temperature inf the mean and the weights (ordered
double sums and one correctly rounded division on both sides). At a finite temperature the two
sides' double exp may differ by an ulp: a weight by one float32 ulp, and a weighted mean of |a| <= 1
by about N 2^-52 before its rounding to float32, so |mean - ref| <= 2^-23 |ref| + 1e-12. The std
always: 2^-23 |ref| + 1e-6 (the root of that absolute error in the variance, at v = 0 too). Outputs
start as a sentinel: every element is written.

Sample. Candidate 0 is the incumbent's bits; the others |cand - ref| <= std C_HW 2^-24 m + ulp32(ref)
with the Box-Muller radius m, as test_gpu_rng_streams.py bounds a normal; the clamp at lo / hi
under a large std."""
import ctypes

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib
from gpu_helpers import C_HW, DEV, U32, ulp32
from lookahead_helpers import COST, REACH, weights
from plan_helpers import (INF, P_STATES, PER_ROW, PER_STATE, SCALES, THRESHOLD, assert_bits,
                          assert_plan_synthetic_shows_every_case, plan_refit_reference, plan_sample_reference,
                          plan_scores, synthetic_plan)

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ISENTINEL = -77
GAMMA = 0.99
MIN_STD = 0.05

# (N, H, K, A, C, mode, elites, temperature, momentum)
R, Cm = REACH, COST
CASES = [
    (2, 1, 1, 1, 1, R, 1, INF, 0.0), (2, 1, 1, 2, 2, Cm, 2, INF, 0.25), (2, 3, 3, 5, 2, R, 1, 1.0, 0.0),
    (2, 3, 1, 1, 1, Cm, 2, 0.01, 0.25), (2, 128, 128, 2, 1, R, 2, INF, 0.0), (2, 128, 1, 5, 2, Cm, 1, 1.0, 0.25),
    (37, 1, 1, 1, 2, R, 9, INF, 0.0), (37, 1, 1, 5, 1, Cm, 37, 1.0, 0.25), (37, 3, 3, 2, 2, R, 1, INF, 0.25),
    (37, 3, 3, 2, 2, Cm, 9, 0.01, 0.0), (37, 3, 1, 5, 1, R, 37, INF, 0.0), (37, 3, 3, 1, 1, Cm, 9, 1.0, 0.0),
    (37, 128, 128, 5, 1, R, 9, INF, 0.25), (256, 1, 1, 2, 1, R, 64, INF, 0.0), (256, 3, 3, 5, 2, Cm, 256, 1.0, 0.25),
    (256, 3, 1, 1, 2, R, 1, 0.01, 0.0), (256, 3, 3, 2, 1, Cm, 64, INF, 0.25), (1024, 1, 1, 1, 1, Cm, 256, INF, 0.0),
    (1024, 3, 3, 2, 2, R, 1024, 1.0, 0.0), (1024, 3, 1, 5, 1, R, 1, INF, 0.25), (1024, 3, 3, 5, 2, Cm, 256, 0.01, 0.25),
    (37, 3, 3, 5, 2, R, 37, 0.01, 0.25), (256, 1, 1, 5, 2, Cm, 1, 1.0, 0.0), (2, 3, 3, 2, 1, R, 2, INF, 0.25),
    (37, 1, 1, 2, 1, R, 1, 0.01, 0.0), (256, 3, 3, 1, 1, R, 256, INF, 0.0), (1024, 1, 1, 2, 2, R, 1, 1.0, 0.25),
    (37, 3, 1, 1, 2, Cm, 37, INF, 0.25), (2, 128, 128, 1, 2, R, 1, 0.01, 0.0), (256, 3, 1, 2, 2, Cm, 64, 0.01, 0.0),
]


def _id(c):
    N, H, K, A, C, mode, elites, T, mom = c
    return f'N{N}-H{H}-K{K}-A{A}-C{C}-{"reach" if mode == REACH else "cost"}-e{elites}-T{T}-m{mom}'


_INPUTS, _SCORES = {}, {}


def _inputs(N, H, K, A, C):
    key = (N, H, K, A, C)
    if key not in _INPUTS:
        _INPUTS[key] = synthetic_plan(N, H, K, A, C)
    return _INPUTS[key]


def _scores(N, H, K, A, C, mode):
    """the reference's scores, once per set of rows and mode, left unchanged"""
    key = (N, H, K, A, C, mode)
    if key not in _SCORES:
        _SCORES[key] = plan_scores(_inputs(N, H, K, A, C)[0], gamma=GAMMA, mode=mode, scales=SCALES)
    return _SCORES[key]


def _launch(x, cand, mean_in, std_in, N, mode, elites, T, mom, threshold=THRESHOLD, per_row=True, alias=False):
    """One drpo_plan_refit call on CPU tensors: a dict of the outputs (None for one not given)."""
    P, K, A = mean_in.shape
    B, H = x['rewards'].shape
    C = x['terminal_qc'].shape[-1]
    dev = {k: v.to(DEV).contiguous() for k, v in x.items()}
    dev.update(cand=cand.to(DEV).contiguous(), mean_in=mean_in.to(DEV).contiguous(), std_in=std_in.to(DEV).contiguous())
    w = torch.from_numpy(weights(GAMMA, H)).to(DEV)
    f = lambda *s: torch.full(s, SENTINEL, device=DEV)
    i = lambda *s: torch.full(s, ISENTINEL, dtype=torch.int32, device=DEV)
    out = {'mean_out': dev['mean_in'] if alias else f(P, K, A), 'std_out': dev['std_in'] if alias else f(P, K, A),
           'best_actions': f(P, K, A), 'best': i(P), 'n_feasible': i(P), 'best_score': f(P), 'best_cert': f(P),
           'best_feasible': torch.full((P,), 77, dtype=torch.uint8, device=DEV),
           'score': f(P, N) if per_row else None, 'cert': f(P, N) if per_row else None,
           'rank': i(P, N) if per_row else None, 'weight': f(P, N) if per_row else None}
    d = _abi.PlanRefit()
    d.P, d.N, d.H, d.K, d.A, d.C, d.mode, d.elites = P, N, H, K, A, C, mode, elites
    d.gamma, d.temperature, d.momentum, d.min_std, d.threshold = GAMMA, T, mom, MIN_STD, threshold
    for k, v in SCALES.items():
        setattr(d, k, v)
    for k, v in dev.items():
        setattr(d, k, v.data_ptr())
    if mode == REACH:
        d.violations = None                                   # may be null there
    d.weights = w.data_ptr()
    for k, v in out.items():
        setattr(d, k, None if v is None else v.data_ptr())
    _lib.check(_lib.lib().drpo_plan_refit(ctypes.byref(d), _lib.stream()), 'plan_refit')
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, T, per_row=True):
    for k in PER_STATE + ('best_actions',) + (PER_ROW[:3] if per_row else ()):
        g = got[k].astype(bool) if k == 'best_feasible' else got[k]
        assert k != 'best_feasible' or set(np.unique(got[k]).tolist()) <= {0, 1}
        assert_bits(g, ref[k], k)
    mean, std = got['mean_out'].astype(np.float64), got['std_out'].astype(np.float64)
    rm, rs = ref['mean'].astype(np.float64), ref['std'].astype(np.float64)
    if np.isinf(T):
        assert_bits(got['mean_out'], ref['mean'], 'mean')
        if per_row:
            assert_bits(got['weight'], ref['weight'], 'weight')
    else:
        err = np.abs(mean - rm)
        print(f'mean: max |d| {err.max():.3g}, {int((err > 0).sum())} of {err.size} differ')
        assert (err <= 2.0 ** -23 * np.abs(rm) + 1e-12).all(), float(err.max())
        if per_row:
            werr = np.abs(got['weight'].astype(np.float64) - ref['weight'].astype(np.float64))
            assert (werr <= 2.0 ** -23 * ref['weight'] + 2.0 ** -149).all(), float(werr.max())
    err = np.abs(std - rs)
    print(f'std: max |d| {err.max():.3g}, {int((err > 0).sum())} of {err.size} differ')
    assert (err <= 2.0 ** -23 * np.abs(rs) + 1e-6).all(), float(err.max())
    assert (std >= np.float32(MIN_STD)).all()


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_refit_equals_the_reference(case):
    N, H, K, A, C, mode, elites, T, mom = case
    x, cand, mean_in, std_in = _inputs(N, H, K, A, C)
    ref = plan_refit_reference(x, cand, mean_in, std_in, N=N, gamma=GAMMA, mode=mode, scales=SCALES,
                               threshold=THRESHOLD, elites=elites, temperature=T, momentum=mom, min_std=MIN_STD,
                               scores=_scores(N, H, K, A, C, mode))
    assert_plan_synthetic_shows_every_case(x, ref, N, H, elites)
    got = _launch(x, cand, mean_in, std_in, N, mode, elites, T, mom)
    _compare(got, ref, T)
    # every element written
    for k, v in got.items():
        assert not (v == (SENTINEL if v.dtype == np.float32 else 77 if v.dtype == np.uint8 else ISENTINEL)).any(), k


def test_cases_reach_what_they_should():
    seen = lambda i: {c[i] for c in CASES}
    assert seen(0) == {2, 37, 256, 1024} and seen(1) == {1, 3, 128} and seen(3) == {1, 2, 5} and seen(4) == {1, 2}
    assert seen(5) == {REACH, COST} and seen(7) == {INF, 1.0, 0.01} and seen(8) == {0.0, 0.25}
    assert all(c[2] in (1, c[1]) for c in CASES) and {c[2] == c[1] for c in CASES if c[1] > 1} == {True, False}
    assert all(c[6] in (1, max(1, c[0] // 4), c[0]) for c in CASES)
    for N in (2, 37, 256, 1024):
        mine = [c for c in CASES if c[0] == N]
        assert {c[6] for c in mine} == {1, max(1, N // 4), N} and {c[7] for c in mine} == {INF, 1.0, 0.01}
        assert {c[8] for c in mine} == {0.0, 0.25} and {c[5] for c in mine} == {REACH, COST}
    assert any(c[2] * c[3] > 256 for c in CASES) and any(c[1] == 128 and c[0] > 2 for c in CASES)


@pytest.mark.parametrize('threshold', [-INF, INF], ids=['none-feasible', 'all-feasible'])
def test_refit_at_the_infinite_thresholds(threshold):
    N, H, K, A, C = 37, 3, 3, 2, 2
    x, cand, mean_in, std_in = _inputs(N, H, K, A, C)
    ref = plan_refit_reference(x, cand, mean_in, std_in, N=N, gamma=GAMMA, mode=REACH, scales=SCALES,
                               threshold=threshold, elites=9, temperature=1.0, momentum=0.0, min_std=MIN_STD,
                               scores=_scores(N, H, K, A, C, REACH))
    got = _launch(x, cand, mean_in, std_in, N, REACH, 9, 1.0, 0.0, threshold=threshold)
    _compare(got, ref, 1.0)
    valid = ~np.isnan(ref['score']) & ~np.isnan(ref['cert'])
    assert got['n_feasible'].tolist() == ([0] * P_STATES if threshold < 0 else valid.sum(1).tolist())


def test_refit_without_the_per_row_outputs_and_in_place():
    N, H, K, A, C = 256, 3, 3, 5, 2
    x, cand, mean_in, std_in = _inputs(N, H, K, A, C)
    ref = plan_refit_reference(x, cand, mean_in, std_in, N=N, gamma=GAMMA, mode=COST, scales=SCALES,
                               threshold=THRESHOLD, elites=64, temperature=INF, momentum=0.25, min_std=MIN_STD,
                               scores=_scores(N, H, K, A, C, COST))
    got = _launch(x, cand, mean_in.clone(), std_in.clone(), N, COST, 64, INF, 0.25, per_row=False, alias=True)
    assert all(got[k] is None for k in PER_ROW)
    _compare(got, ref, INF, per_row=False)                  # mean_out / std_out alias their inputs


# ------------------------------------------------------------------ the sample launch
def _sample(mean, std, inc, N, seed, ctr, lo=-1.0, hi=1.0):
    P, K, A = mean.shape
    dev = [t.to(DEV).contiguous() for t in (mean, std, inc)]
    cand = torch.full((P * N, K, A), SENTINEL, device=DEV)
    d = _abi.PlanSample()
    d.P, d.N, d.K, d.A, d.lo, d.hi, d.seed, d.ctr = P, N, K, A, lo, hi, seed, ctr
    d.mean, d.std, d.incumbent, d.cand = (t.data_ptr() for t in dev + [cand])
    _lib.check(_lib.lib().drpo_plan_sample(ctypes.byref(d), _lib.stream()), 'plan_sample')
    torch.cuda.synchronize()
    return cand.cpu()


@pytest.mark.parametrize('N, K, A', [(2, 1, 1), (37, 3, 2), (256, 128, 5), (1024, 1, 5)])
def test_sample_equals_the_reference(N, K, A):
    P = P_STATES
    g = torch.Generator().manual_seed(N + K + A)
    mean, std = torch.rand(P, K, A, generator=g) - 0.5, torch.rand(P, K, A, generator=g) * 0.5 + 0.05
    inc = torch.rand(P, K, A, generator=g) * 4 - 2                    # copied as it is, outside the clamp too
    inc[0, 0, 0] = float('nan')
    seed, ctr = 0x1234567890ABCDEF, 7 + (1 << 32)                     # only ctr's low 32 bits enter
    got = _sample(mean, std, inc, N, seed, ctr)
    assert not (got == SENTINEL).any()
    assert_bits(got.reshape(P, N, K, A)[:, 0].contiguous(), inc.numpy(), 'candidate 0')
    ref, radius = plan_sample_reference(mean, std, inc, N=N, seed=seed, ctr=7)
    sd = np.broadcast_to(std.numpy().astype(np.float64)[:, None], (P, N, K, A)).reshape(P * N, K, A)
    bound = sd * C_HW * U32 * radius + ulp32(torch.from_numpy(ref)).numpy()
    err = np.abs(got.numpy().astype(np.float64) - ref).reshape(P, N, K, A)[:, 1:]
    print(f'sample: max err / bound {(err / bound.reshape(P, N, K, A)[:, 1:]).max():.3g}')
    assert (err <= bound.reshape(P, N, K, A)[:, 1:]).all()
    drawn = got.reshape(P, N, K, A)[:, 1:]
    assert float(drawn.min()) >= -1.0 and float(drawn.max()) <= 1.0 and drawn.std() > 0.05
    assert not torch.equal(_sample(mean, std, inc, N, seed, 8), got)   # another counter: other draws


def test_sample_clamps_at_lo_and_hi():
    P, N, K, A = P_STATES, 37, 3, 2
    mean, std, inc = torch.zeros(P, K, A), torch.full((P, K, A), 50.0), torch.zeros(P, K, A)
    got = _sample(mean, std, inc, N, 5, 1, lo=-0.25, hi=0.5).reshape(P, N, K, A)[:, 1:]
    assert float(got.min()) == -0.25 and float(got.max()) == 0.5
    assert int((got == -0.25).sum()) > got.numel() // 3 and int((got == 0.5).sum()) > got.numel() // 3
    ref, _ = plan_sample_reference(mean, std, inc, N=N, seed=5, ctr=1, lo=-0.25, hi=0.5)
    same = (got.numpy() == ref.reshape(P, N, K, A)[:, 1:])
    assert same.mean() > 0.97          # all but the few draws that land inside [lo, hi], which are rounded
