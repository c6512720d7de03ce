"""drpo_plan_sample_ar and drpo_plan_shift (csrc/plan.hip) against plan_mpc_helpers' references,
bit for bit (float32 as int32).

The normals come off the white launch itself: drpo_plan_sample with mean 0, std 1 and an infinite
clamp returns z (fmaf(1, z, 0) is z), and the AR launch draws at the same indices and site. The
reference then runs the float64 recursion on those z, rounds u to float32 once and evaluates the
fused multiply-add exactly (rationals, one rounding), so every comparison is of bits and no
tolerance enters. Outputs sit between guard bands of a sentinel that no launch may touch."""
import ctypes

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib, ops
from gpu_helpers import C_HW, DEV, U32, ulp32
from plan_mpc_helpers import INF, assert_bits, plan_sample_ar_reference, plan_shift_reference

pytestmark = pytest.mark.gpu

P = 3
SENTINEL = -777.25
GUARD = 67                   # floats on either side of an output (odd: the output is not 16-byte aligned)
SEED, CTR = 0x1234567890ABCDEF, 7
NAN = float('nan')
SHAPES = [(2, 1, 1), (3, 5, 2), (37, 7, 3), (2, 128, 1)]       # (37, 7, 3): 333 lanes, two workgroups, the last partial


def _guarded(n):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf, n, msg):
    b = buf.cpu()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), f'{msg}: a guard band was written'
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), f'{msg}: an element was not written'


def _sample(mean, std, inc, N, *, corr=None, innov=None, lo=-1.0, hi=1.0, seed=SEED, ctr=CTR):
    """One launch on CPU tensors: drpo_plan_sample (corr None) or drpo_plan_sample_ar; cand on the CPU."""
    Pn, K, A = mean.shape
    dev = [t.to(DEV).contiguous() for t in (mean, std, inc)]
    n = Pn * N * K * A
    buf, cand = _guarded(n)
    d = _abi.PlanSample() if corr is None else _abi.PlanSampleAr()
    d.P, d.N, d.K, d.A, d.lo, d.hi, d.seed, d.ctr = Pn, N, K, A, lo, hi, seed, ctr
    d.mean, d.std, d.incumbent, d.cand = (t.data_ptr() for t in dev + [cand])
    if corr is None:
        _lib.check(_lib.lib().drpo_plan_sample(ctypes.byref(d), _lib.stream()), 'plan_sample')
    else:
        d.corr, d.innov = corr, innov
        _lib.check(_lib.lib().drpo_plan_sample_ar(ctypes.byref(d), _lib.stream()), 'plan_sample_ar')
    torch.cuda.synchronize()
    _guards_untouched(buf, n, 'cand')
    return cand.cpu().reshape(Pn * N, K, A)


_Z = {}


def _z(N, K, A):
    """The normals of (SEED, CTR) as the white launch draws them, [P, N, K, A]; computed once per shape."""
    if (N, K, A) not in _Z:
        zero, one = torch.zeros(P, K, A), torch.ones(P, K, A)
        _Z[N, K, A] = _sample(zero, one, zero, N, lo=-INF, hi=INF).reshape(P, N, K, A)
    return _Z[N, K, A]


def _inputs(N, K, A):
    g = torch.Generator().manual_seed(N + K + A)
    mean, std = torch.rand(P, K, A, generator=g) - 0.5, torch.rand(P, K, A, generator=g) * 0.5 + 0.05
    inc = torch.rand(P, K, A, generator=g) * 4 - 2                    # copied as it is, outside the clamp too
    return mean, std, inc


# ------------------------------------------------------------------ the AR launch
@pytest.mark.parametrize('N, K, A', SHAPES)
def test_the_white_launch_returns_z(N, K, A):
    z = _z(N, K, A)
    drawn = z[:, 1:]
    assert torch.isfinite(drawn).all() and (z[:, 0] == 0).all()
    if drawn.numel() > 500:
        assert abs(float(drawn.mean())) < 0.15 and 0.85 < float(drawn.std()) < 1.15
    # it is the generator of the CPU model (float64 there: within the bound test_gpu_plan_kernels holds
    # the white launch to, at std 1)
    import rng_model
    ref, radius = rng_model.normal_at(SEED, CTR, _abi.PLAN_SITE, np.arange(z.numel()))
    bound = C_HW * U32 * radius + ulp32(torch.from_numpy(ref)).numpy()
    err = np.abs(ref - z.numpy().astype(np.float64).reshape(-1))
    assert (err <= bound).reshape(z.shape)[:, 1:].all()


@pytest.mark.parametrize('corr, innov', [(0.5, 0.5), (0.9, float(np.sqrt(1 - 0.81)))], ids=['dyadic', 'unit'])
@pytest.mark.parametrize('N, K, A', SHAPES)
def test_ar_unit_scale_is_the_float64_recursion(N, K, A, corr, innov):
    """mean 0, std 1: the launch returns (float)u."""
    z = _z(N, K, A)
    zero, one = torch.zeros(P, K, A), torch.ones(P, K, A)
    got = _sample(zero, one, zero, N, corr=corr, innov=innov, lo=-INF, hi=INF)
    ref, u32 = plan_sample_ar_reference(z, zero, one, zero, corr=corr, innov=innov, lo=-INF, hi=INF)
    assert_bits(got.reshape(P, N, K, A)[:, 1:], u32.reshape(P, N, K, A)[:, 1:], '(float)u')
    assert_bits(got, ref, 'cand')
    if K > 1:
        assert not torch.equal(got, z.reshape(got.shape))


@pytest.mark.parametrize('N, K, A', SHAPES)
def test_ar_equals_the_reference(N, K, A):
    z = _z(N, K, A)
    mean, std, inc = _inputs(N, K, A)
    inc[0, 0, 0] = NAN
    corr, innov = 0.75, float(np.sqrt(1 - 0.75 ** 2))
    got = _sample(mean, std, inc, N, corr=corr, innov=innov)
    ref, _ = plan_sample_ar_reference(z, mean, std, inc, corr=corr, innov=innov)
    assert_bits(got, ref, 'cand')
    drawn = got.reshape(P, N, K, A)[:, 1:]
    assert float(drawn.min()) >= -1.0 and float(drawn.max()) <= 1.0
    if K >= 7 and N >= 37:
        # the noise is correlated along the steps, and of unit variance
        u = (_sample(torch.zeros(P, K, A), torch.ones(P, K, A), torch.zeros(P, K, A), N, corr=corr, innov=innov,
                     lo=-INF, hi=INF).reshape(P, N, K, A)[:, 1:]).numpy().astype(np.float64)
        lag1 = float((u[:, :, 1:] * u[:, :, :-1]).mean())
        assert 0.6 < lag1 < 0.9 and 0.85 < float(u.std()) < 1.15, (lag1, u.std())


@pytest.mark.parametrize('N, K, A', SHAPES)
def test_ar_without_correlation_is_the_white_launch(N, K, A):
    mean, std, inc = _inputs(N, K, A)
    inc[0, 0, 0] = NAN
    assert_bits(_sample(mean, std, inc, N, corr=0.0, innov=1.0), _sample(mean, std, inc, N), 'cand')
    wide = std * 100                                                     # most draws at the clamp
    assert_bits(_sample(mean, wide, inc, N, corr=0.0, innov=1.0, lo=-0.25, hi=0.5),
                _sample(mean, wide, inc, N, lo=-0.25, hi=0.5), 'cand, clamped')


def test_ar_clamps_and_keeps_a_nan():
    N, K, A = 37, 7, 3
    mean, std, inc = torch.zeros(P, K, A), torch.full((P, K, A), 50.0), torch.zeros(P, K, A)
    mean[1, 2, 0] = NAN                                # a NaN mean: the selects of the clamp let it through
    got = _sample(mean, std, inc, N, corr=0.5, innov=0.5, lo=-0.25, hi=0.5).reshape(P, N, K, A)[:, 1:]
    assert torch.isnan(got[1, :, 2, 0]).all()
    rest = got[~torch.isnan(got)]
    assert float(rest.min()) == -0.25 and float(rest.max()) == 0.5
    assert int((rest == -0.25).sum()) > rest.numel() // 3 and int((rest == 0.5).sum()) > rest.numel() // 3
    ref, _ = plan_sample_ar_reference(_z(N, K, A), mean, std, inc, corr=0.5, innov=0.5, lo=-0.25, hi=0.5)
    assert_bits(got, ref.reshape(P, N, K, A)[:, 1:], 'cand')


def test_ar_candidate_0_keeps_every_bit():
    N, K, A = 3, 5, 2
    mean, std, _ = _inputs(N, K, A)
    inc = torch.zeros(P, K, A)
    raw = inc.view(torch.int32)
    raw[0, 0, 0] = 0x7FC12345            # a NaN with a payload
    raw[0, 1, 1] = -(1 << 31)            # -0.0
    raw[1, 4, 0] = 0x7F800001            # a signalling NaN
    inc[2] = 7.5                         # outside the clamp
    got = _sample(mean, std, inc, N, corr=0.5, innov=0.5).reshape(P, N, K, A)
    assert_bits(got[:, 0], inc, 'candidate 0')
    assert not torch.isnan(got[:, 1:]).any()


def test_ops_plan_sample_takes_the_launch_its_corr_names(monkeypatch):
    N, K, A = 37, 7, 3
    mean, std, inc = (t.to(DEV) for t in _inputs(N, K, A))
    calls = []
    for name in ('drpo_plan_sample', 'drpo_plan_sample_ar'):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _f=real, _n=name: (calls.append(_n), _f(*a))[1])
    white = ops.plan_sample(mean, std, inc, N, SEED, CTR)
    also = ops.plan_sample(mean, std, inc, N, SEED, CTR, corr=0.0)
    ar = ops.plan_sample(mean, std, inc, N, SEED, CTR, corr=0.75)
    torch.cuda.synchronize()
    assert calls == ['drpo_plan_sample', 'drpo_plan_sample', 'drpo_plan_sample_ar']
    assert_bits(white, _sample(*_inputs(N, K, A), N), 'white')
    assert_bits(also, white, 'corr=0')
    assert_bits(ar, _sample(*_inputs(N, K, A), N, corr=0.75, innov=float(np.sqrt(1 - 0.75 ** 2))), 'corr=0.75')


# ------------------------------------------------------------------ the shift launch
def _shift_inputs(Pn, K, A):
    g = torch.Generator().manual_seed(Pn * 100 + K * 10 + A)
    mean, inc = torch.rand(Pn, K, A, generator=g) - 0.5, torch.rand(Pn, K, A, generator=g) * 4 - 2
    # std below, at and above the floor 0.25
    std = torch.tensor([0.125, 0.25, 0.5, 0.0, 0.2499999])[torch.randint(0, 5, (Pn, K, A), generator=g)]
    flat_m, flat_i, flat_s = mean.view(-1), inc.view(-1), std.view(-1)
    flat_m[0], flat_i[-1] = NAN, -0.0
    if flat_m.numel() > 4:
        flat_m[3], flat_i[2], flat_s[1], flat_s[4] = -0.0, NAN, NAN, 0.25
    tail = torch.rand(Pn, A, generator=g) - 0.5
    tail.view(-1)[0] = -0.0
    reset = torch.arange(Pn) % 3 == 1 if Pn > 1 else torch.tensor([True])
    return mean, std, inc, reset, tail


def _shift(mean, std, inc, shift, reset, tail, fresh_std=0.75, std_floor=0.25):
    Pn, K, A = mean.shape
    n = Pn * K * A
    keep = [t.to(DEV).contiguous() for t in (mean, std, inc)]
    outs = [_guarded(n) for _ in range(3)]
    d = _abi.PlanShift()
    d.P, d.K, d.A, d.shift, d.fresh_std, d.std_floor = Pn, K, A, shift, fresh_std, std_floor
    d.mean, d.std, d.incumbent = (t.data_ptr() for t in keep)
    if reset is not None:
        keep.append(reset.to(DEV).contiguous())
        d.reset = keep[-1].data_ptr()
    if tail is not None:
        keep.append(tail.to(DEV).contiguous())
        d.tail = keep[-1].data_ptr()
    d.mean_out, d.std_out, d.incumbent_out = (o[1].data_ptr() for o in outs)
    _lib.check(_lib.lib().drpo_plan_shift(ctypes.byref(d), _lib.stream()), 'plan_shift')
    torch.cuda.synchronize()
    for (buf, _), k in zip(outs, ('mean_out', 'std_out', 'incumbent_out')):
        # (fresh_std and the inputs never equal the sentinel, so every element shows as written)
        _guards_untouched(buf, n, k)
    return [o[1].cpu().reshape(Pn, K, A) for o in outs]


@pytest.mark.parametrize('with_tail', [False, True], ids=['repeat', 'tail'])
@pytest.mark.parametrize('with_reset', [False, True], ids=['all-warm', 'reset'])
@pytest.mark.parametrize('Pn, K, A', [(7, 5, 9), (1, 1, 1), (2, 128, 2)])
def test_shift_equals_the_reference(Pn, K, A, with_reset, with_tail):
    mean, std, inc, reset, tail = _shift_inputs(Pn, K, A)
    reset, tail = reset if with_reset else None, tail if with_tail else None
    for shift in sorted({0, 1, K - 1, K}):
        got = _shift(mean, std, inc, shift, reset, tail)
        ref = plan_shift_reference(mean, std, inc, shift=shift, fresh_std=0.75, std_floor=0.25, reset=reset, tail=tail)
        for g, r, k in zip(got, ref, ('mean_out', 'std_out', 'incumbent_out')):
            assert_bits(g, r, f'{k}, shift {shift}')
    if not with_reset and K > 1:        # the inputs show the floor: kept steps below, at and above it
        low = plan_shift_reference(mean, std, inc, shift=1, fresh_std=0.75, std_floor=0.25)[1][:, :K - 1]
        assert (low[~np.isnan(low)] >= 0.25).all() and (low == 0.25).any() and (low == 0.5).any()


def test_ops_plan_shift_returns_fresh_tensors():
    mean, std, inc, reset, tail = _shift_inputs(7, 5, 9)
    dev = [t.to(DEV) for t in (mean, std, inc)]
    before = [t.clone() for t in dev]
    out = ops.plan_shift(*dev, shift=2, fresh_std=0.75, std_floor=0.25, reset=reset.to(DEV), tail=tail.to(DEV))
    torch.cuda.synchronize()
    ref = plan_shift_reference(mean, std, inc, shift=2, fresh_std=0.75, std_floor=0.25, reset=reset, tail=tail)
    for g, r, k in zip(out, ref, ('mean', 'std', 'incumbent')):
        assert_bits(g, r, k)
    for t, b in zip(dev, before):
        assert_bits(t, b, 'an input')
    assert len({t.data_ptr() for t in list(out) + dev}) == 6
    plain = ops.plan_shift(*dev, shift=0, fresh_std=0.75, std_floor=0.0)
    assert_bits(plain[0], mean, 'shift 0: mean')
    assert_bits(plain[2], inc, 'shift 0: incumbent')
