"""The float64 references of tests/optim_reference.py against torch itself (no GPU): adam_ref
against one step of a float64 torch.optim.Adam whose state was preloaded, clip_coef_ref against
torch.nn.utils.clip_grad_norm_, scalar_grad_ref against float64 autograd of the three scalar
losses it stands for (src/ssac.py:470-479,556-563)."""
import math

import pytest
import torch

from drpo_amd.optim import Adam
from optim_reference import (adam_ref, adam_terms, clip_coef_ref, ens_reduce_f32, ens_reduce_ref, scalar_grad_ref,
                             strided16_f32, sums_block_f32, sums_bound)

LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8


def state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g, dtype=torch.float64)
    gr = torch.randn(n, generator=g, dtype=torch.float64) * 0.1
    m = torch.randn(n, generator=g, dtype=torch.float64) * 0.01
    v = torch.rand(n, generator=g, dtype=torch.float64) * 0.01
    return p, gr, m, v


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_adam_ref_is_torch_adam(t, wd):
    p0, g, m0, v0 = state(257, 10 * t + int(wd > 0))
    ours = Adam(None, LR, weight_decay=wd, betas=BETAS, eps=EPS, tensor=torch.zeros(1))
    ours.step_count = t - 1
    lr_over_bc1, bc2_sqrt = ours.step_scalars()
    assert ours.step_count == t
    p, m, v = adam_ref(p0, g, m0, v0, lr_over_bc1, bc2_sqrt, BETAS, EPS, wd)
    for foreach in (False, True):
        w = torch.nn.Parameter(p0.clone())
        w.grad = g.clone()
        opt = torch.optim.Adam([w], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=foreach)
        opt.state[w] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m0.clone(), 'exp_avg_sq': v0.clone()}
        opt.step()
        st = opt.state[w]
        assert float(st['step']) == t
        for got, ref, what in ((p, w.detach(), 'p'), (m, st['exp_avg'], 'm'), (v, st['exp_avg_sq'], 'v')):
            rel = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
            assert rel <= 1e-12, (what, foreach, rel)
        assert not torch.equal(w.detach(), p0)


@pytest.mark.parametrize('max_norm,scale', [(0.5, 1.0), (0.5, 1 / 3), (100.0, 1.0), (100.0, 0.5)])
def test_clip_coef_ref_is_clip_grad_norm(max_norm, scale):
    """The summed gradient G with the mean's scale folded into the coefficient, as drpo_optim_step
    does it, against clip_grad_norm_ of the mean gradient G * scale; norms above and below max_norm."""
    _, G, _, _ = state(1000, 5)
    w = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    w.grad = G * scale
    total = torch.nn.utils.clip_grad_norm_([w], max_norm)
    coef = clip_coef_ref(float((G * G).sum()), max_norm, scale)
    assert (coef < 1.0) == (float(total) > max_norm) == (max_norm == 0.5)
    ref = w.grad
    rel = ((G * scale * coef - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    assert rel <= 1e-12, rel


@pytest.mark.parametrize('kind,p', [(0, -5.0), (0, 1.5), (1, -30.0), (1, 2.0), (2, 0.3)])
def test_scalar_grad_ref_is_autograd(kind, p):
    """kind 0: alpha_loss = -mean(exp(log_alpha) * x); kind 1: -mean(softplus(lam) * x); kind 2:
    -mean(log_alpha * x); x the per-row factor whose tile sums the kernels hand over."""
    g = torch.Generator().manual_seed(kind)
    x = torch.randn(512, generator=g)
    partials = x.view(32, 16).sum(1)                          # float32 tile sums
    q = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    c = (q.exp(), torch.nn.functional.softplus(q), q)[kind]
    (-(c * partials.double().sum()) / 512).backward()
    ref, terms = scalar_grad_ref(kind, p, partials, 512)
    assert abs(ref - float(q.grad)) <= 1e-12 * abs(float(q.grad))
    assert terms >= abs(ref)


def test_bounds_reduce_to_the_plain_sums():
    part = torch.tensor([1.5, -2.0, 0.25])
    assert sums_bound(part) == (-0.25, 9, 3.75)
    assert sums_bound(torch.zeros(0)) == (0.0, 8, 0.0) and sums_bound(torch.zeros(257))[1] == 10
    r = ens_reduce_ref(torch.ones(2, 17), torch.ones(2, 17, 3), -torch.ones(2, 17, 3), [0.0, -1.0, 2.0],
                       [1.0, 1.0, 1.0], 0.5, 0.25, 0.125)
    assert r['mse'][0].tolist() == [17.0, 17.0] and r['mse'][1] == 2 + 4
    assert float(r['loss'][0]) == 34.0 + 0.5 * (3.0 - 1.0) and r['loss'][1] == 6 + 2 + 6 + 2
    assert r['gmin'][0].tolist() == [0.125 + 34 - 0.125] * 3 and r['gmax'][0].tolist() == [0.125 - 34 + 0.125] * 3
    assert r['gmin'][1] == 3 + 4 + 2 and r['gmin'][2].tolist() == [0.125 + 34 + 0.125] * 3
    # a gradient known exactly and no state: the terms are the update's own magnitudes
    T_p, T_m, T_v = adam_terms(1.0, 2.0, 0.0, 0.0, 2.0, 0.03, math.sqrt(0.001), BETAS, 0.0, 0.0)
    assert abs(float(T_m) - 0.2) < 1e-15 and abs(float(T_v) - 0.001 * 12) < 1e-15
    assert abs(float(T_p) - (1 + 0.03 * (0.2 + 0.2 * (1 + 12 / 8)) / 2.0)) < 1e-12


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 1000])
def test_exact_order_models_sum(n):
    """Small integers add without rounding in any order, so the ordered float32 models must give the exact
    sum; on random data they stay inside the derived bounds they are a special case of."""
    g = torch.Generator().manual_seed(n)
    k = torch.randint(-50, 50, (n,), generator=g).float()
    assert float(sums_block_f32(k)) == float(k.sum()) and float(strided16_f32(k)) == float(k.sum())
    x = torch.randn(n, generator=g) * 100
    ref, c, terms = sums_bound(x)
    assert abs(float(sums_block_f32(x)) - ref) <= c * 2.0 ** -24 * terms
    assert abs(float(strided16_f32(x)) - ref) <= (-(-n // 16) + 4) * 2.0 ** -24 * terms


def test_exact_order_model_of_the_reduction():
    g = torch.Generator().manual_seed(1)
    Z, nbx, S1 = 5, 19, 3
    ints = lambda *shape: torch.randint(-9, 9, shape, generator=g).float()
    mse, mn, mx, lo, hi = ints(Z, nbx), ints(Z, nbx, S1), ints(Z, nbx, S1), ints(S1), ints(S1)
    emse, egmin, egmax, eloss = ens_reduce_f32(mse, mn, mx, lo, hi, 0.5, 0.25)
    r = ens_reduce_ref(mse, mn, mx, lo, hi, 0.5, None, 0.25)
    assert emse.tolist() == r['mse'][0].tolist()
    assert egmin.tolist() == r['gmin'][0].tolist() and egmax.tolist() == r['gmax'][0].tolist()
    assert float(eloss[0]) == float(eloss[1]) == float(r['loss'][0])
