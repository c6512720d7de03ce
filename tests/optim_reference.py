"""Float64 restatements of what the optimizer launch (csrc/optim.hip) and the riders on the
weight-gradient launch (csrc/wgrad.hip, csrc/ens_nll.hpp) compute, and the error models the GPU
tests hold the kernels to. No GPU, no library: tests/test_optim_reference.py pins the
restatements to torch.optim.Adam and torch.nn.utils.clip_grad_norm_ themselves.

Every bound is gpu_helpers.error_ratio's

    bound = c * 2^-24 * terms (+ 2^-126)

with ``terms`` the sum of the absolute terms of the float64 formula and ``c`` the number of
float32 roundings on the longest path to the result. The functions here return (c, terms) or
the terms alone; the tests hand them to gpu_helpers.within.

Fixed-order sums. A sum the kernels spread over L lanes and finish with a log2(L')-level tree
adds ceil(N / L) values per lane in order, then one value per tree level: at most
ceil(N / L) + levels roundings on any path, each relative to a partial sum that the absolute
terms bound (lane_sum_roundings). The first add of a lane (0 + x) is exact, so the count is
one too many: kept, the issue's count.

Propagation through Adam (adam_terms). With the gradient g known to C * 2^-24 * t_g (t_g >= |g|:
its own absolute terms, scaled so that the constant is the C of the comparison), weight decay
wd, a = lr / bc1 and the float32 formulas of adam_step (csrc/common.hpp)

    ge = g + wd p0            t_ge = t_g + wd |p0|
    m' = m0 + (1 - b1)(ge - m0)
    v' = b2 v0 + (1 - b2) ge^2
    p' = p0 - a m' / denom,   denom = sqrt(v') / sqrt(bc2) + eps

the absolute terms are

    T_m = |m0| + (1 - b1)(|m0| + t_ge)
    T_v = b2 |v0| + (1 - b2)(ge^2 + 2 |ge| t_ge)      (d(ge^2) = 2 |ge| d(ge))
    T_p = |p0| + a (T_m + |m'| (1 + T_v / (2 v'))) / denom

T_p: the quotient m' / denom moves by (d m' + |m'| d denom / denom) / denom; d denom / denom is
at most the relative error of sqrt(v'), half that of v' (T_v / (2 v')), and the 1 stands for the
quotient's, the product's and the subtraction's own roundings, each relative to a |m'| / denom.
"""
import math

import torch

U32 = 2.0 ** -24


def f32(x):
    """the float32 nearest to x, as a Python float (what a c_float field of a descriptor holds)"""
    return float(torch.tensor(x, dtype=torch.float64).float().double())


def adam_ref(p, g, m, v, lr_over_bc1, bc2_sqrt, betas, eps, wd, coef=1.0, scale=1.0):
    """torch.optim.Adam's single-tensor update with coupled weight decay on float64 tensors, the
    gradient being g * scale (the data-parallel mean) * coef (the clip coefficient). The scalars
    are those of drpo_amd.optim.Adam.step_scalars(). Returns the new (p, m, v)."""
    b1, b2 = betas
    ge = g * scale * coef + wd * p
    m = m + (ge - m) * (1 - b1)
    v = v * b2 + (1 - b2) * ge * ge
    p = p - lr_over_bc1 * (m / (v.sqrt() / bc2_sqrt + eps))
    return p, m, v


def clip_coef_ref(sumsq, max_norm, scale=1.0):
    """clip_grad_norm_'s coefficient for a gradient whose SUMMED form has sum of squares sumsq and
    whose mean is scale times the sum: min(1, max_norm / (sqrt(sumsq) * scale + 1e-6))"""
    return min(1.0, max_norm / (math.sqrt(float(sumsq)) * scale + 1e-6))


def scalar_grad_ref(kind, p, partials, rows):
    """Gradient of a scalar parameter from device loss partials: -c(p) * sum(partials) / rows with
    c = exp(p) (kind 0: the SAC temperature), sigmoid(p) (kind 1: the scalar multiplier's softplus)
    or 1 (kind 2: the log-alpha loss). Returns (gradient, absolute terms c(p) sum|partials| / rows)."""
    part = torch.as_tensor(partials).double()
    c = {0: math.exp(p), 1: 1.0 / (1.0 + math.exp(-p)), 2: 1.0}[kind]
    return -c * float(part.sum()) / rows, c * float(part.abs().sum()) / rows


def lane_sum_roundings(n, lanes, levels):
    """roundings on the longest path of a sum of n values over ``lanes`` strided lanes and a
    ``levels``-level tree"""
    return -(-n // lanes) + levels


def sums_bound(part):
    """drpo_mlp_wgrad_sums (sums_block): 256 strided lanes, then block_tree_sum's 8 levels.
    Returns (float64 sum of the float32 partials, c, terms)."""
    part = torch.as_tensor(part).double()
    return float(part.sum()), lane_sum_roundings(part.numel(), 256, 8), float(part.abs().sum())


def ens_reduce_ref(mse_part, min_part, max_part, minlv, maxlv, weight, gscale, g0):
    """ens_loss_reduce_block in float64 from float32 partials mse [Z][nbx], min / max [Z][nbx][S1] and
    the bounds: a dict of (value, c, terms) for 'mse' [Z], 'loss', 'gmin' [S1], 'gmax' [S1]. g0: what
    gmin / gmax held before, one number or a pair of [S1] tensors (gmin's, gmax's).

    mse[z]: a 16-lane strided sum of nbx values and a 4-level xor tree. gmin[c] / gmax[c]: the same
    over the Z * nbx partials of column c, then the -/+ gscale * weight and the g0 +. loss: thread 0
    adds the Z member sums and the 2 * S1 bounds in order, then the difference, the product and the
    final sum (Z + 2 S1 + 2), on top of a member sum's own roundings."""
    mse_part, min_part, max_part = (torch.as_tensor(x).double() for x in (mse_part, min_part, max_part))
    minlv, maxlv = torch.as_tensor(minlv).double(), torch.as_tensor(maxlv).double()
    Z, nbx = mse_part.shape
    S1 = minlv.numel()
    gw = (1.0 if gscale is None else gscale) * weight
    c_mse = lane_sum_roundings(nbx, 16, 4)
    c_g = lane_sum_roundings(Z * nbx, 16, 4) + 2
    mse = mse_part.sum(1)
    out = {'mse': (mse, c_mse, mse_part.abs().sum(1))}
    loss = mse.sum() + weight * (maxlv.sum() - minlv.sum())
    out['loss'] = (loss, c_mse + Z + 2 * S1 + 2,
                   mse_part.abs().sum() + weight * (maxlv.abs().sum() + minlv.abs().sum()))
    g0min, g0max = (torch.as_tensor(x, dtype=torch.float64) for x in (g0 if isinstance(g0, tuple) else (g0, g0)))
    out['gmin'] = (g0min + min_part.sum((0, 1)) - gw, c_g, g0min.abs() + min_part.abs().sum((0, 1)) + gw)
    out['gmax'] = (g0max + max_part.sum((0, 1)) + gw, c_g, g0max.abs() + max_part.abs().sum((0, 1)) + gw)
    return out


def adam_terms(p0, g, m0, v0, t_g, lr_over_bc1, bc2_sqrt, betas, eps, wd):
    """(T_p, T_m, T_v) of the module docstring for float64 tensors (or floats) p0, g, m0, v0 and the
    gradient's terms t_g; evaluated at the float64 update itself"""
    p0, g, m0, v0, t_g = (torch.as_tensor(x, dtype=torch.float64) for x in (p0, g, m0, v0, t_g))
    b1, b2 = betas
    ge = g + wd * p0
    t_ge = t_g + wd * p0.abs()
    _, m1, v1 = adam_ref(p0, g, m0, v0, lr_over_bc1, bc2_sqrt, betas, eps, wd)
    T_m = m0.abs() + (1 - b1) * (m0.abs() + t_ge)
    T_v = b2 * v0.abs() + (1 - b2) * (ge * ge + 2 * ge.abs() * t_ge)
    denom = v1.sqrt() / bc2_sqrt + eps
    rel_v = torch.where(v1 > 0, T_v / (2 * v1.clamp_min(1e-300)), torch.zeros_like(v1))
    T_p = p0.abs() + lr_over_bc1 * (T_m + m1.abs() * (1 + rel_v)) / denom
    return T_p, T_m, T_v


# ---------------------------------------------------------------------------
# Exact-order models. The kernels' sums have one fixed order and nothing but float32 adds (no
# product next to them for the compiler to contract into an fma), so numpy float32 in the same order
# gives the same bits. The derived bounds above are worst cases -- every rounding of the longest path
# aligned, no cancellation -- and random signs leave the measured error at a hundredth of them; these
# models are what a single wrong rounding path cannot pass.
# ---------------------------------------------------------------------------
def _f32(x):
    import numpy as np
    return np.ascontiguousarray(torch.as_tensor(x).detach().cpu().float().numpy(), dtype=np.float32)


def sums_block_f32(part):
    """sums_block (csrc/wgrad.hip): lane t adds part[t], part[t + 256], ... in order from 0.f; then
    block_tree_sum: red[t] += red[t + w] for w = 128, 64, ..., 1. Returns a numpy float32."""
    import numpy as np
    part = _f32(part).reshape(-1)
    red = np.zeros(256, np.float32)
    for j0 in range(0, part.size, 256):
        chunk = part[j0:j0 + 256]
        red[:chunk.size] = red[:chunk.size] + chunk
    w = 128
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w >>= 1
    return red[0]


def strided16_f32(vals):
    """ens_loss_reduce_block's sum of vals [..., N] over the last axis: lane l of 16 adds vals[l],
    vals[l + 16], ... in order from 0.f; then the xor tree m += shfl_xor(m, o) for o = 8, 4, 2, 1
    (lane 0's result). Returns numpy float32 [...]."""
    import numpy as np
    v = _f32(vals)
    lanes = np.zeros(v.shape[:-1] + (16,), np.float32)
    for q0 in range(0, v.shape[-1], 16):
        chunk = v[..., q0:q0 + 16]
        lanes[..., :chunk.shape[-1]] = lanes[..., :chunk.shape[-1]] + chunk
    idx = np.arange(16)
    for o in (8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ o]
    return lanes[..., 0]


def ens_reduce_f32(mse_part, min_part, max_part, minlv, maxlv, weight, g0):
    """ens_loss_reduce_block in its own order, float32, for gscale == NULL (gw = 1.f * weight, exact):
    mse [Z], gmin / gmax [S1] = g0 + (sum -/+ weight), and the two values the loss may take: thread 0's
    in-order sums, then tot + weight * (smax - smin) either as a product and a sum or contracted into
    one fma (the compiler's choice)."""
    import numpy as np
    mse = strided16_f32(mse_part)
    Z, nbx, S1 = _f32(min_part).shape
    w, g0 = np.float32(weight), np.float32(g0)
    a0 = strided16_f32(_f32(min_part).reshape(Z * nbx, S1).T)
    a1 = strided16_f32(_f32(max_part).reshape(Z * nbx, S1).T)
    gmin, gmax = g0 + (a0 - w), g0 + (a1 + w)
    tot = np.float32(0)
    for z in range(Z):
        tot = tot + mse[z]
    smax, smin = np.float32(0), np.float32(0)
    for hi, lo in zip(_f32(maxlv), _f32(minlv)):
        smax, smin = smax + hi, smin + lo
    d = smax - smin
    loss = (np.float32(tot + w * d), np.float32(np.float64(w) * np.float64(d) + np.float64(tot)))
    return mse, gmin, gmax, loss
