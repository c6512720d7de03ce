"""The row-wise launches against float64 at the edges of their formulas.

Each test calls a C entry point (or its thin ops.py wrapper) on a prescribed table of inputs --
saturated, clamped, flushed, tied -- and compares with a float64 evaluation of the reference's
formula written here with torch on the CPU; gradients come from float64 autograd of that
formula. Tolerances are per element, gpu_helpers.error_ratio:

    bound = c * 2^-24 * (sum |terms of the formula| + |value| * max |exp argument|)

with c = 8 for the libm kernels and c = 32 for the hardware-transcendental ones (cc_std). Where
an inner sum feeds a product (diff = t - (D + s) in the NLL, 1 - t^2 in the multiplier) its
absolute terms are carried through the product. The exps INSIDE a softplus do not scale the
value: exp(-|x|) with a relative error of 2^-24 |x| moves log1p(exp(-|x|)) by at most
2^-24 |x| e^-|x| <= 2^-24 / e, one of the c operations; the exp argument of the model is that
of the outer exp (the log-std / log-variance) or of a sigmoid far in its tail.

Measured error / bound per quantity: profiles/rowwise_edges/README.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib, ops
from gpu_helpers import C_HW, C_LIBM, U32, f64, sp64, ulp32, within

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


def dev(x, dtype=torch.float32):
    return torch.as_tensor(x).to(dtype).contiguous().to(DEV)


def f32(v):
    """the float32 nearest to v, as a Python float"""
    return float(np.float32(v))


# ---------------------------------------------------------------------------
# 1. Normalizer: drpo_normalizer_fit, drpo_normalize
# ---------------------------------------------------------------------------
NORM_S = [1, 3, 17, 128, 129, 256]           # lanes = 256 // S: 256, 85 (+1 idle thread), 15, 2, 1 (+127 idle), 1
NORM_N = [1, 2, 37, 2047, 2048, 2049, 5000]  # around the NORM_ROWS = 2048 block edge, and three blocks
NORM_CASES = sorted({(S, N) for S in NORM_S for N in (2049, 5000)} | {(17, N) for N in NORM_N})
CONSTANTS = [0.0, 1000.1, 1e4 + 0.3, -7.77]


def norm_columns(N, S):
    """[N][S] float32; the nine column kinds cycled over the S columns"""
    g = torch.Generator().manual_seed(1000 * S + N)
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0).double()
    cols = []
    for c in range(S):
        k = c % 9
        z = torch.randn(N, generator=g, dtype=torch.float64)
        if k == 0:
            col = z
        elif k == 1:
            col = 1e3 + 1e-2 * z
        elif k == 2:
            col = -1e4 + 1e-1 * z
        elif k <= 6:
            col = torch.full((N,), CONSTANTS[k - 3], dtype=torch.float64)
        elif k == 7:
            col = 2.5e-7 * sign        # true std under the 1e-6 threshold -> 1.0
        else:
            col = 4e-6 * sign          # kept
        cols.append(col.float())
    return torch.stack(cols, 1).contiguous()


def norm_reference(X):
    """float64 two-pass mean and unbiased std of the float32 data; std cast to float32, then
    std[std < 1e-6] = 1 (src/normalization.py:18-20)"""
    X = X.double()
    N = X.shape[0]
    mean = X.sum(0) / N
    if N > 1:
        std64 = (((X - mean) ** 2).sum(0) / (N - 1)).sqrt()
    else:
        std64 = torch.full_like(mean, float('nan'))
    std = std64.float()
    std[std < 1e-6] = 1.0
    return mean, std64, std


@pytest.mark.parametrize('S,N', NORM_CASES)
def test_normalizer_fit(S, N):
    """Mean within 1 ulp, std within 2 ulp of the float64 two-pass reference, exactly 1.0 where the
    reference is 1.0, NaN at N = 1. The one-pass sums of x and x^2 this kernel used before gave, at
    N = 5000, std 1.811e-4 for the column constant at float32(1000.1) (S = 129, 256), 1.099e-3 for
    float32(1e4 + 0.3) and 1.09e-6 for -7.77 (S = 128), and offset-column stds up to 115 ulp off:
    13 of these 19 cases were red (profiles/rowwise_edges/README.md)."""
    X = norm_columns(N, S)
    mean_ref, std64, std_ref = norm_reference(X)
    if N > 1:   # the threshold decision is never a rounding matter
        assert not ((std64 >= 5e-7) & (std64 <= 2e-6)).any()
    mean = torch.full((S,), float('nan'), device=DEV)
    std = torch.full((S,), float('nan'), device=DEV)
    ops.normalizer_fit(X.to(DEV), mean, std)
    mean, std = mean.cpu(), std.cpu()
    dm = (f64(mean) - f64(mean_ref.float())).abs() / ulp32(mean_ref.float())
    print(f'edge-ratio normalizer_fit mean S={S} N={N}: max {dm.max().item():.3g} ulp')
    assert (dm <= 1.0).all(), (dm.max().item(), int(dm.argmax()))
    if N == 1:
        assert torch.isnan(std).all()
        return
    one = std_ref == 1.0
    const = [c for c in range(S) if 3 <= c % 9 <= 7]
    assert all(one[c] for c in const)
    print(f'edge-ratio normalizer_fit S={S} N={N}: std of the constant / sub-threshold columns '
          f'{[f"{v:.4g}" for v in std[const][:5].tolist()]}')
    assert torch.equal(std[one], torch.ones(int(one.sum()))), std[one]
    ds = (f64(std[~one]) - f64(std_ref[~one])).abs() / ulp32(std_ref[~one])
    print(f'edge-ratio normalizer_fit std S={S} N={N}: max {ds.max().item() if ds.numel() else 0:.3g} ulp')
    assert (ds <= 2.0).all(), ds.max().item()


@pytest.mark.parametrize('n,S', [(37, 17), (4100, 256)])   # the second: past the 4096-block cap
def test_normalize(n, S):
    g = torch.Generator().manual_seed(n)
    mean = torch.randn(S, generator=g) * torch.tensor([1.0, 1e3, 1e-3])[torch.arange(S) % 3]
    std = torch.tensor([1.0, 4e-6, 1e-2, 0.3, 57.0])[torch.arange(S) % 5].clone()
    x = mean + std * torch.randn(n, S, generator=g) * 3
    x[0] = mean                                  # x == mean: exactly 0
    eps = 1e-6                                   # Normalizer's epsilon (src/normalization.py:7)
    y = ops.normalize(x.to(DEV), mean.to(DEV), std.to(DEV), eps).cpu()
    # The 2 ulp count one float32 subtraction and one division (a relative 2^-24 and half an ulp), so the
    # quotient's denominator is the float32 sum std + eps as the reference itself forms it. Against the
    # exact sum the rounding of std + eps adds another relative 2^-24: up to 2.5 ulp, printed only.
    den = (std + torch.tensor(eps)).double()
    ref = (x.double() - mean.double()) / den
    d = (f64(y) - ref).abs() / ulp32(ref)
    exact = (x.double() - mean.double()) / (std.double() + f32(eps))
    print(f'edge-ratio normalize n={n} S={S}: max {d.max().item():.3g} ulp '
          f'({((f64(y) - exact).abs() / ulp32(exact)).max().item():.3g} ulp against the exact std + eps)')
    assert torch.equal(y[0], torch.zeros(S))
    assert (d <= 2.0).all(), d.max().item()


# ---------------------------------------------------------------------------
# 6. Shield: drpo_shield_mix, drpo_shield_select (bit-equal to PyTorch CPU fp32)
# ---------------------------------------------------------------------------
def shield_actions(n, A, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, A, generator=g) * 2 - 1, torch.tanh(torch.randn(n, A, generator=g) * 2)


@pytest.mark.parametrize('A', [1, 6])
@pytest.mark.parametrize('n', [1, 65, 257])
@pytest.mark.parametrize('K', [2, 3, 11])
def test_shield_mix_bit_equal(K, n, A):
    a_perf, a_safe = shield_actions(n, A, 7 * K + n + A)
    got = ops.shield_mix(a_perf.to(DEV), a_safe.to(DEV), K).cpu()
    ratios = [(K - 1 - i) / (K - 1) for i in range(K)]                           # src/sampling.py:430-434
    ref = torch.stack([a_safe * r + a_perf * (1 - r) for r in ratios])
    assert torch.equal(got, ref)


def up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def down(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def rows_with_max(maxima, C, pos_seed):
    """[len(maxima)][C] float32 rows whose maximum is the given value, at a varying position"""
    q = torch.empty(len(maxima), C)
    for i, m in enumerate(maxima):
        q[i] = m - 0.5 - 0.25 * torch.arange(C)
        q[i, (i + pos_seed) % C] = m
    return q


@pytest.mark.parametrize('A', [1, 6])
@pytest.mark.parametrize('C', [1, 3])
def test_shield_select_threshold(C, A):
    thr = f32(0.3)
    edge = [thr, up(thr), down(thr), thr, -thr, 5.0, down(thr), up(thr)]
    g = torch.Generator().manual_seed(C + A)
    maxima = edge + (torch.randn(65 - len(edge), generator=g) + thr).tolist()
    n = len(maxima)
    q = rows_with_max(maxima, C, 1)
    a_perf, a_safe = shield_actions(n, A, 3)
    got = ops.shield_select(q.to(DEV), ops.SHIELD_THRESHOLD, thr, a_perf.to(DEV), a_safe.to(DEV)).cpu()
    ref = torch.empty(n, A)
    for i in range(n):                                      # src/smbpo.py:127-136: a_safe where max_C q > thr
        ref[i] = a_safe[i] if max(q[i].tolist()) > thr else a_perf[i]
    assert torch.equal(ref[0], a_perf[0]) and torch.equal(ref[1], a_safe[1]) and torch.equal(ref[2], a_perf[2])
    assert torch.equal(got, ref)
    none = ops.shield_select(q.to(DEV), ops.SHIELD_NONE, thr, a_perf.to(DEV), a_safe.to(DEV)).cpu()
    assert torch.equal(none, a_perf)


@pytest.mark.parametrize('A', [1, 6])
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('K,n', [(2, 1), (3, 65), (11, 257)])
def test_shield_select_linear(K, n, C, A):
    thr = f32(-0.125)
    g = torch.Generator().manual_seed(K * n + C)
    a_perf, a_safe = shield_actions(n, A, 5)
    mixes = ops.shield_mix(a_perf.to(DEV), a_safe.to(DEV), K)
    maxima = thr + torch.randn(K, n, generator=g)
    maxima[:, 0] = up(thr)                                   # no candidate passes: the safe action
    if n > 4:
        maxima[:, 1] = thr                                   # every one passes, exactly at the threshold (<=)
        maxima[:, 2] = up(thr)
        maxima[0, 2] = thr                                   # only k = 0 passes
        maxima[:, 3] = 1.0
        maxima[0, 3] = down(thr)                             # several pass; the last passing k is K - 2 ...
        maxima[K - 2, 3] = down(thr)
        maxima[:, 4] = down(thr)                             # ... and K - 1 here
    q = torch.stack([rows_with_max(maxima[k].tolist(), C, k) for k in range(K)])
    got = ops.shield_select(q.to(DEV), ops.SHIELD_LINEAR, thr, a_perf.to(DEV), a_safe.to(DEV), mixes).cpu()
    mixes = mixes.cpu()
    ref = torch.empty(n, A)
    for i in range(n):                                       # src/sampling.py:430-437: later k override earlier
        ref[i] = a_safe[i]
        for k in range(K):
            if max(q[k, i].tolist()) <= thr:
                ref[i] = mixes[k, i]
    assert torch.equal(ref[0], a_safe[0])
    if n > 4:
        assert torch.equal(ref[1], mixes[K - 1, 1]) and torch.equal(ref[2], mixes[0, 2])
        assert torch.equal(ref[3], mixes[K - 2, 3]) and torch.equal(ref[4], mixes[K - 1, 4])
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------------
# 5. Multiplier: drpo_multiplier_out, drpo_multiplier_head (libm)
# ---------------------------------------------------------------------------
THR, PLB, PUB, LAM_EPS = f32(0.1), -1.0, 100.0, 1.0


def multiplier_table(B, ub):
    """x, sqc, aqc of B rows: the 11 x 5 x 8 products walked with a stride coprime to their count"""
    xs = [0.0, 1e-3, -1e-3, ub / 2, -ub / 2, ub, -ub, 10 * ub, -10 * ub, 1e6, -1e6]
    sq = [-1.0, -0.0, 0.0, 1e-30, 1.0]
    pen = [PLB - 1, down(PLB), PLB, up(PLB), 0.37, down(PUB), PUB, PUB + 1]   # aqc - thr
    n = len(xs) * len(sq) * len(pen)
    j = (torch.arange(B) * 127 + 3) % n
    x = torch.tensor(xs)[j % len(xs)]
    sqc = torch.tensor(sq)[(j // len(xs)) % len(sq)]
    aqc = (torch.tensor(pen, dtype=torch.float64)[j // (len(xs) * len(sq))] + THR).float()
    return x, sqc, aqc


def lam64(x, ub):
    return ub / 2. * (1. + torch.tanh(x / ub * 2))            # src/ssac.py:109-110


@pytest.mark.parametrize('ub', [1.0, 25.0, 50.0])             # 50: MLPMultiplier's default
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
def test_multiplier(B, ub):
    L = _lib.lib()
    x, sqc, aqc = multiplier_table(B, ub)
    xd, sd, ad = dev(x), dev(sqc), dev(aqc)
    lam = torch.full((B,), float('nan'), device=DEV)
    _lib.check(L.drpo_multiplier_out(B, _lib.ptr(xd), ub, _lib.ptr(lam), _lib.stream()), 'multiplier_out')
    gx = torch.full((B,), float('nan'), device=DEV)
    loss = torch.zeros(1, device=DEV)
    _lib.check(L.drpo_multiplier_head(B, _lib.ptr(xd), _lib.ptr(sd), _lib.ptr(ad), THR, PLB, PUB, ub, LAM_EPS,
                                      _lib.ptr(gx), _lib.ptr(loss), _lib.stream()), 'multiplier_head')
    lsum = torch.zeros(1, device=DEV)
    _lib.check(L.drpo_multiplier_head(B, None, None, _lib.ptr(ad), THR, PLB, PUB, 0.0, 0.0, None, _lib.ptr(lsum),
                                      _lib.stream()), 'multiplier_head')
    # float64 autograd of src/ssac.py:540-563
    x64 = x.double().requires_grad_()
    s64, a64 = sqc.double(), aqc.double()
    penalty = torch.clamp(a64 - THR, min=PLB, max=PUB)
    lams = lam64(x64, ub)
    lams_safe, lams_unsafe = torch.mul(s64 <= 0, lams), torch.mul(s64 > 0, lams)
    target = (s64 > 0).double() * (ub - LAM_EPS)
    lam_loss = -0.5 * torch.mean(torch.mul(lams_safe, penalty)) + torch.nn.functional.mse_loss(lams_unsafe, target)
    lam_loss.backward()
    t = torch.tanh(x.double() / ub * 2)
    tag = f'B={B} ub={ub:g}'
    within(f'multiplier_out lam {tag}', lam, lams, ub / 2 * (1 + t.abs()), C_LIBM)
    safe = (s64 <= 0).double()
    lu, tu = lams_unsafe.detach().abs(), target.abs()
    # glam = (-0.5 safe pen + 2 (lu - tu) unsafe) / B; gx = glam * (1 - t^2), the difference's terms 1 + t^2
    t_glam = (0.5 * safe * penalty.abs() + 2 * (lu + tu)) / B
    within(f'multiplier_head gx {tag}', gx, x64.grad, t_glam * (1 + t * t), C_LIBM)
    # loss: sum of (-0.5 safe lam pen + (lu - tu)^2) / B; d = lu - tu carries eps (lu + tu), d^2 twice that times |d|
    t_loss = ((0.5 * safe * lams.detach() * penalty.abs() + (lu + tu) ** 2) / B).sum()
    within(f'multiplier_head loss {tag}', loss[0], lam_loss.detach(), t_loss, C_LIBM)
    within(f'multiplier_head penalty sum {tag}', lsum[0], penalty.sum(), (a64.abs() + abs(THR)).sum(), C_LIBM)


# ---------------------------------------------------------------------------
# 3. Constraint critic: drpo_cc_head, drpo_cc_dist (hardware transcendentals)
# ---------------------------------------------------------------------------
LMIN, LMAX, RATIO = -4.0, 4.0, 2.0
CC_LS = [-1e4, -100.0, -30.0, LMIN - 1, LMIN, 0.0, LMAX, LMAX + 1, 30.0, 100.0, 1e4]


def cc_log_std64(ls):
    log_std = LMAX - sp64(LMAX - ls)                           # src/ssac.py:75-77
    return LMIN + sp64(log_std - LMIN)


def cc_table(rows, C):
    g = torch.Generator().manual_seed(100 * rows + C)
    j = (torch.arange(rows * C) * 7 + rows) % len(CC_LS)
    ls = torch.tensor(CC_LS)[j].reshape(rows, C)
    mu = torch.randn(rows, C, generator=g) * 3
    want = {}                                                 # row -> arg-max the design fixes
    if rows >= 63:
        mu[5], ls[5], want[5] = 1.25, 0.5, 0                   # every value ties: the first wins
        if C >= 3:
            mu[6], ls[6] = 1.25, 0.5
            mu[6, 0], want[6] = 1.0, 1                         # columns 1.. tie above column 0
            mu[7], ls[7] = -0.75, -2.0
            ls[7, 2], want[7] = -1.5, 2                        # equal means: only the std term decides
            mu[8], ls[8] = 0.5, 1e4
            ls[8, C - 1], want[8] = -1e4, 0                    # both clamps in one row
    return mu, ls, want


@pytest.mark.parametrize('C', [1, 3, 5])
@pytest.mark.parametrize('rows', [1, 63, 64, 65])
def test_cc_head(rows, C):
    L = _lib.lib()
    mu, ls, want = cc_table(rows, C)
    mud, lsd = dev(mu), dev(ls)
    for dist in (1, 0):
        ub = torch.full((rows,), float('nan'), device=DEV)
        arg = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
        _lib.check(L.drpo_cc_head(_lib.ptr(mud), _lib.ptr(lsd), rows, C, dist, RATIO, LMIN, LMAX, _lib.ptr(ub),
                                  _lib.ptr(arg), _lib.stream()), 'cc_head')
        arg = arg.cpu().long()
        if not dist:
            assert torch.equal(ub.cpu(), mu.max(1).values)
            assert np.array_equal(arg.numpy(), np.argmax(mu.numpy(), axis=1))   # numpy: the first maximum
            continue
        log_std = cc_log_std64(ls.double())
        std = log_std.exp()
        v = mu.double() + RATIO * std                          # src/ssac.py:85, max: src/ssac.py:598
        terms = mu.double().abs() + RATIO * std
        best = torch.from_numpy(np.argmax(v.numpy(), axis=1))
        pick = lambda m, i: m.gather(1, i[:, None])[:, 0]
        tag = f'rows={rows} C={C}'
        # the value the kernel maximised is that of its own arg-max
        within(f'cc_head bound {tag}', ub, pick(v, arg), pick(terms, arg), C_HW, pick(log_std.abs(), arg))
        # and it is the float64 maximum to within both candidates' bounds
        bnd = C_HW * U32 * (terms + v.abs() * log_std.abs())
        gap = pick(v, best) - pick(v, arg)
        assert (gap <= pick(bnd, best) + pick(bnd, arg)).all()
        clear = torch.ones(rows, dtype=torch.bool)             # rows whose float64 winner leads by more than the bounds
        for c in range(C):
            other = torch.full((rows,), c)
            lead = pick(v, best) - v[:, c]
            clear &= (other == best) | (lead > pick(bnd, best) + bnd[:, c])
        assert torch.equal(arg[clear], best[clear])
        for r, a in want.items():
            assert int(arg[r]) == a, (r, int(arg[r]), a, v[r].tolist())


@pytest.mark.parametrize('C', [1, 3, 5])
@pytest.mark.parametrize('rows', [1, 63, 64, 65])
def test_cc_dist(rows, C):
    L = _lib.lib()
    mu, ls, _ = cc_table(rows, C)
    n = rows * C
    eps = torch.tensor([0.0, 1e-3, -1.0, 1.999, 2.0, 2.5, -2.0, -3.0, 7.0, -2.001, 0.5])[
        (torch.arange(n) * 5 + 1) % 11].reshape(rows, C)
    mud, lsd, ed = dev(mu), dev(ls), dev(eps)
    log_std = cc_log_std64(ls.double())
    std = log_std.exp()
    tag = f'rows={rows} C={C}'
    q = torch.full((rows, C), float('nan'), device=DEV)
    _lib.check(L.drpo_cc_dist(_lib.ptr(mud), _lib.ptr(lsd), n, 0, RATIO, LMIN, LMAX, None, 0, 0, None, _lib.ptr(q),
                              _lib.stream()), 'cc_dist')
    v = mu.double() + RATIO * std
    within(f'cc_dist mode 0 q {tag}', q, v, mu.double().abs() + RATIO * std, C_HW, log_std.abs())
    sd = torch.full((rows, C), float('nan'), device=DEV)
    _lib.check(L.drpo_cc_dist(_lib.ptr(mud), _lib.ptr(lsd), n, 1, RATIO, LMIN, LMAX, _lib.ptr(ed), 0, 0,
                              _lib.ptr(sd), _lib.ptr(q), _lib.stream()), 'cc_dist')
    noise = torch.clamp(eps.double(), -2., 2.)                 # src/ssac.py:88-89
    v = mu.double() + noise * std
    within(f'cc_dist mode 1 std {tag}', sd, std, std, C_HW, log_std.abs())
    within(f'cc_dist mode 1 q {tag}', q, v, mu.double().abs() + noise.abs() * std, C_HW, log_std.abs())


# ---------------------------------------------------------------------------
# 2 (a). Squashed-Gaussian head: drpo_policy_head (libm)
# ---------------------------------------------------------------------------
PI_MU = [0.0, 1e-4, -1e-4, 1.0, -1.0, 5.0, -5.0, 9.0, -9.0, 20.0, -20.0, 50.0, -50.0]
PI_PRE = [-100.0, -20.0, -1.0, 0.0, 1.0, 20.0, 100.0]
PI_EPS = [0.0, 1e-3, -1e-3, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0]
PI_SHAPES = [(rows, A) for A in (1, 6, 8) for rows in (1, 17, 33)]
LOG2, HALF_LOG_2PI = math.log(2.0), 0.5 * math.log(2.0 * math.pi)


def policy_table(rows, A):
    """raw [rows][2A] and eps [rows][A]: element j of the 13 * 7 * 9 = 819 (mu, pre, eps) triples is
    (j % 13, j % 7, j % 9) -- the three counts are pairwise coprime, so 819 consecutive j meet every
    triple once and any 117 every pair. The nine shapes take consecutive windows: 765 triples."""
    off = sum(r * a for r, a in PI_SHAPES[:PI_SHAPES.index((rows, A))])
    j = (off + torch.arange(rows * A)).reshape(rows, A)
    raw = torch.cat([torch.tensor(PI_MU)[j % 13], torch.tensor(PI_PRE)[j % 7]], 1)
    return raw.contiguous(), torch.tensor(PI_EPS)[j % 9].contiguous()


def policy_std64(pre):
    log_std = -6 + (4 - -6) * torch.sigmoid(pre)               # src/policy.py:93-96
    return log_std, log_std.exp() * 1.0


def squashed_logp64(u, mu, std):
    """Independent(TanhTransform(Normal(mu, std))).log_prob at the cached pre-image u, and the sum of
    the absolute terms; per row"""
    normal = -((u - mu) ** 2) / (2 * std ** 2) - std.log() - HALF_LOG_2PI
    sp = sp64(-2. * u)
    ladj = 2. * (LOG2 - u - sp)
    terms = ((u - mu) ** 2) / (2 * std ** 2) + std.log().abs() + HALF_LOG_2PI + 2. * (LOG2 + u.abs() + sp)
    return (normal - ladj).sum(-1), terms.sum(-1)


def policy_head(raw, A, mode, eps, outs):
    L = _lib.lib()
    rows = raw.shape[0]
    bufs = {k: torch.full((rows,) if k == 'logp' else (rows, A), float('nan'), device=DEV) for k in outs}
    p = lambda k: _lib.ptr(bufs.get(k))
    _lib.check(L.drpo_policy_head(_lib.ptr(raw), rows, A, mode, _lib.ptr(eps), 0, 0, 0, p('a'), p('logp'), p('u'),
                                  p('e'), p('amean'), _lib.stream()), 'policy_head')
    return {k: v.cpu() for k, v in bufs.items()}


@pytest.mark.parametrize('rows,A', PI_SHAPES)
def test_policy_head(rows, A):
    raw, eps = policy_table(rows, A)
    rawd, epsd = dev(raw), dev(eps)
    mu, pre, e = raw[:, :A].double(), raw[:, A:].double(), eps.double()
    log_std, std = policy_std64(pre)
    assert rows * A < 7 or (log_std.min() < -5.99 and log_std.max() > 3.99)       # both ends of the sigmoid
    tag = f'rows={rows} A={A}'
    for mode in (0, 1):
        o = policy_head(rawd, A, mode, epsd, ['a', 'logp', 'u', 'e', 'amean'])
        u_ref = mu + e * std                                   # Normal.sample / rsample
        within(f'policy_head mode {mode} u {tag}', o['u'], u_ref, mu.abs() + (e * std).abs(), C_LIBM, log_std.abs())
        assert torch.equal(o['e'], eps)
        u = f64(o['u'])                                        # the cached pre-image, as the reference's log_prob sees it
        within(f'policy_head mode {mode} a {tag}', o['a'], torch.tanh(u), torch.tanh(u).abs(), C_LIBM)
        within(f'policy_head mode {mode} amean {tag}', o['amean'], torch.tanh(mu), torch.tanh(mu).abs(), C_LIBM)
        lp, terms = squashed_logp64(u, mu, std)
        within(f'policy_head mode {mode} logp {tag}', o['logp'], lp, terms, C_LIBM, log_std.abs().max(-1).values)
    o = policy_head(rawd, A, 2, None, ['amean'])
    within(f'policy_head mode 2 amean {tag}', o['amean'], torch.tanh(mu), torch.tanh(mu).abs(), C_LIBM)
    o = policy_head(rawd, A, 3, None, ['u', 'e', 'amean'])     # mode 3: u <- loc, e <- scale
    assert torch.equal(o['u'], raw[:, :A])
    within(f'policy_head mode 3 scale {tag}', o['e'], std, std, C_LIBM, log_std.abs())
    within(f'policy_head mode 3 amean {tag}', o['amean'], torch.tanh(mu), torch.tanh(mu).abs(), C_LIBM)


# ---------------------------------------------------------------------------
# 4. Ensemble NLL and Gaussian head: drpo_ens_loss + drpo_ens_loss_reduce, drpo_ens_head (libm)
# ---------------------------------------------------------------------------
ENS_Z = 3
ENS_CASES = [(S, b) for S in (1, 15, 16, 31) for b in (1, 15, 16, 17, 33)] + [(255, 3)]
ENS_DIFF = [0.0, 1e-3, -0.5, 1.0, -3.0, 10.0, -30.0, 30.0]


def ens_inputs(S, b, per_member):
    """head outputs, states, targets and bounds; per_member: states and targets per member
    (non-zero member strides) or shared (zero strides)"""
    S1 = S + 1
    g = torch.Generator().manual_seed(1000 * S + b)
    lo = -10 + 8 * torch.rand(S1, generator=g)
    hi = -1 + 3 * torch.rand(S1, generator=g)
    n = ENS_Z * b * S1
    j = (torch.arange(n) * 11 + S).reshape(ENS_Z, b, S1)
    kinds = torch.stack([torch.full((S1,), -1e3), lo - 25, lo, (lo + hi) / 2, hi, hi + 25, torch.full((S1,), 1e3)])
    LVR = kinds[j % 7, torch.arange(S1).expand(ENS_Z, b, S1)]
    D = torch.randn(ENS_Z, b, S1, generator=g) * 2
    zs = ENS_Z if per_member else 1
    s = torch.randn(zs, b, S, generator=g) * 3
    m = D + torch.cat([s.expand(ENS_Z, b, S), torch.zeros(ENS_Z, b, 1)], -1)
    t = m + torch.tensor(ENS_DIFF)[(j // 7) % len(ENS_DIFF)]
    if not per_member:
        t = t[:1]           # shared targets: the members' diffs then differ through D
    return D.contiguous(), LVR.contiguous(), s.contiguous(), t.contiguous(), lo, hi


def ens_log_var64(raw, lo, hi):
    log_vars = hi - sp64(hi - raw)                             # src/dynamics.py:132-133
    return lo + sp64(log_vars - lo)


@pytest.mark.parametrize('S,b', ENS_CASES)
def test_ens_loss(S, b):
    L = _lib.lib()
    S1, Z = S + 1, ENS_Z
    case = ENS_CASES.index((S, b))
    per_member, scaled = case % 2 == 0, case % 3 != 0
    weight, gscale, g0 = 0.01, (0.37 if scaled else 1.0), 0.25
    D, LVR, s, t, lo, hi = ens_inputs(S, b, per_member)
    Dd, Ld, sd, td, lod, hid = dev(D), dev(LVR), dev(s), dev(t), dev(lo), dev(hi)
    gs = dev([gscale]) if scaled else None
    part = torch.full((max(1, L.drpo_ens_loss_workspace_size(b, S, Z) // 4),), float('nan'), device=DEV)
    mse = torch.full((Z,), float('nan'), device=DEV)
    loss = torch.full((1,), float('nan'), device=DEV)
    gmin, gmax = torch.full((S1,), g0, device=DEV), torch.full((S1,), g0, device=DEV)
    gD, gL = torch.full_like(Dd, float('nan')), torch.full_like(Dd, float('nan'))
    up_ = _abi.EnsUpstream()
    up_.D, up_.LVR, up_.s, up_.t = Dd.data_ptr(), Ld.data_ptr(), sd.data_ptr(), td.data_ptr()
    up_.s_zstride, up_.t_zstride = (b * S, b * S1) if per_member else (0, 0)
    up_.b, up_.S, up_.Z, up_.minlv, up_.maxlv, up_.part = b, S, Z, lod.data_ptr(), hid.data_ptr(), part.data_ptr()
    up_.gscale = gs.data_ptr() if scaled else None
    red = _abi.EnsReduce()
    red.mse, red.loss, red.gmin, red.gmax, red.weight = (mse.data_ptr(), loss.data_ptr(), gmin.data_ptr(),
                                                         gmax.data_ptr(), weight)
    deferred = _abi.EnsReduce()
    _lib.check(L.drpo_ens_loss(ctypes.byref(up_), ctypes.byref(red), _lib.ptr(gD), _lib.ptr(gL),
                               ctypes.byref(deferred), _lib.stream()), 'ens_loss')
    _lib.check(L.drpo_ens_loss_reduce(ctypes.byref(deferred), _lib.stream()), 'ens_loss_reduce')
    torch.cuda.synchronize()

    # float64 autograd of src/dynamics.py:143-153,236-253
    D64, L64 = D.double().requires_grad_(), LVR.double().requires_grad_()
    lo64, hi64 = lo.double().requires_grad_(), hi.double().requires_grad_()
    s64, t64 = s.double().expand(Z, b, S), t.double().expand(Z, b, S1)
    means = D64 + torch.cat([s64, torch.zeros(Z, b, 1, dtype=torch.float64)], -1)
    log_vars = ens_log_var64(L64, lo64, hi64)
    inv_vars = torch.exp(-log_vars)
    mse_ref = torch.mean((t64 - means) ** 2 * inv_vars, dim=(-2, -1)) + torch.mean(log_vars, dim=(-2, -1))
    loss_ref = torch.sum(mse_ref) + weight * (hi64.sum() - lo64.sum())
    (gscale * loss_ref).backward()

    # the error model's terms (module docstring), all detached float64
    with torch.no_grad():
        sp1 = sp64(hi64 - L64)
        l1 = hi64 - sp1
        sp2 = sp64(l1 - lo64)
        s1, s2 = torch.sigmoid(l1 - lo64), torch.sigmoid(hi64 - L64)
        # l = lo + sp2 is itself a sum that cancels (lo = -8.6, sp2 = 8.8 -> l = 0.2): its error, and so the
        # relative error of exp(-l), is 2^-24 times ITS absolute terms, not 2^-24 |l|; l1 = hi - sp1 enters
        # through the softplus' slope s1. a_l >= |l| takes the place of the exp argument.
        a_l = lo64.abs() + sp2 + s1 * (hi64.abs() + sp1)
        diff = t64 - means
        t_diff = t64.abs() + D64.abs() + torch.cat([s64, torch.zeros(Z, b, 1, dtype=torch.float64)], -1).abs()
        d2iv = diff ** 2 * inv_vars
        d2iv_t = d2iv + 2 * diff.abs() * t_diff * inv_vars       # |d^2 iv| with the difference's own terms
        el = d2iv + log_vars                                      # the element's loss term
        g = gscale / (b * S1)
        # tail sigmoids: exp arguments that scale a gradient (where the sigmoid is not yet 0 in float32)
        tail = lambda x: torch.where((x < 0) & (x > -104), x.abs(), torch.zeros_like(x))
        arg = torch.maximum(a_l, torch.maximum(tail(l1 - lo64), tail(hi64 - L64)))
        t_el = d2iv_t + a_l + d2iv * a_l
        t_dl = g * (1 + d2iv_t)
        dl = g * (1 - d2iv)
        cmn, cmx = dl * (1 - s1), dl * s1 * (1 - s2)
        t_cmn = t_dl * (1 + s1) + cmn.abs() * arg
        t_cmx = t_dl * s1 * (1 + s2) + cmx.abs() * arg
        gw = gscale * weight
    tag = f'S={S} b={b} zstride={"n" if per_member else 0} gscale={gscale:g}'
    within(f'ens_loss mse {tag}', mse, mse_ref.detach(), t_el.sum((-2, -1)) / (b * S1), C_LIBM)
    t_loss = t_el.sum() / (b * S1) + weight * (hi64.abs().sum() + lo64.abs().sum()).detach()
    within(f'ens_loss loss {tag}', loss[0], loss_ref.detach(), t_loss, C_LIBM)
    within(f'ens_loss gD {tag}', gD, D64.grad, 2 * g * inv_vars * (diff.abs() * (1 + a_l) + t_diff), C_LIBM)
    within(f'ens_loss gLVR {tag}', gL, L64.grad, t_dl * s1 * s2 + L64.grad.abs() * arg, C_LIBM)
    within(f'ens_loss gmin {tag}', gmin, g0 + lo64.grad, g0 + gw + t_cmn.sum((0, 1)), C_LIBM)
    within(f'ens_loss gmax {tag}', gmax, g0 + hi64.grad, g0 + gw + t_cmx.sum((0, 1)), C_LIBM)


@pytest.mark.parametrize('S,b', [(1, 1), (15, 17), (16, 33), (31, 16), (255, 3)])
def test_ens_head(S, b):
    L = _lib.lib()
    S1, Z = S + 1, ENS_Z
    per_member = S % 2 == 1 and b > 1
    D, LVR, s, _, lo, hi = ens_inputs(S, b, per_member)
    zsel = [2, 0, 2, 1]                                         # permutes and repeats members
    Zo = len(zsel)
    g = torch.Generator().manual_seed(S + b)
    eps = torch.tensor([0.0, 1.0, -1.0, 3.0, -4.0, 1e-3])[torch.randint(6, (Zo, b, S1), generator=g)]
    Dd, Ld, sd, lod, hid, ed = dev(D), dev(LVR), dev(s), dev(lo), dev(hi), dev(eps)
    zd = dev(zsel, torch.int32)
    mu, lv = torch.full((Zo, b, S1), float('nan'), device=DEV), torch.full((Zo, b, S1), float('nan'), device=DEV)
    s2, r = torch.full((Zo, b, S), float('nan'), device=DEV), torch.full((Zo, b), float('nan'), device=DEV)
    _lib.check(L.drpo_ens_head(_lib.ptr(Dd), _lib.ptr(Ld), _lib.ptr(sd), b * S if per_member else 0, b, S, Zo,
                               _lib.ptr(lod), _lib.ptr(hid), _lib.ptr(zd), _lib.ptr(ed), 0, 0, _lib.ptr(mu),
                               _lib.ptr(lv), _lib.ptr(s2), _lib.ptr(r), _lib.stream()), 'ens_head')
    D64, L64 = D.double()[zsel], LVR.double()[zsel]
    s64 = torch.cat([s.double().expand(Z, b, S)[zsel], torch.zeros(Zo, b, 1, dtype=torch.float64)], -1)
    lo64, hi64 = lo.double(), hi.double()
    means = D64 + s64                                           # src/dynamics.py:130-134
    log_vars = ens_log_var64(L64, lo64, hi64)
    stds = torch.exp(log_vars).sqrt()                           # src/dynamics.py:232-234
    samples = means + stds * eps.double()
    l1 = hi64 - sp64(hi64 - L64)
    s1 = torch.sigmoid(l1 - lo64)
    # l = lo + sp(l1 - lo); l1 = hi - sp(hi - raw) enters through the softplus' slope s1 (test_ens_loss: a_l)
    a_l = lo64.abs() + sp64(l1 - lo64) + s1 * (hi64.abs() + sp64(hi64 - L64))
    tag = f'S={S} b={b}'
    within(f'ens_head mu {tag}', mu, means, D64.abs() + s64.abs(), C_LIBM)
    within(f'ens_head lv {tag}', lv, log_vars, a_l, C_LIBM)
    t_x = D64.abs() + s64.abs() + (stds * eps.double()).abs()
    within(f'ens_head s2 {tag}', s2, samples[..., :-1], t_x[..., :-1], C_LIBM, torch.maximum(log_vars.abs(), a_l / 2)[..., :-1])
    within(f'ens_head r {tag}', r, samples[..., -1], t_x[..., -1], C_LIBM, torch.maximum(log_vars.abs(), a_l / 2)[..., -1])
