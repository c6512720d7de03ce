"""drpo_ens_spread (csrc/ensemble.hip), the reduction across ensemble members, against float64.

Inputs are built like ens_inputs of test_gpu_rowwise_edges.py: the raw log-variances cycle its
seven kinds (far below / at / between / at / far above the bounds, +-1e3), the diff-head outputs
cycle five column kinds (D_KINDS below), every third state column is 1e4 + 3z, and the column
weights are 1 / (0.1 + 5u) with the reward's 0. The comparison is gpu_helpers.within with
c = C_LIBM: bound = c 2^-24 (terms + |value| exp_arg) per element. With d the members' M
values of an element, f = max(1, M / 8) (a sequential float32 sum of M terms), a_l the absolute
terms of the soft clamp (test_ens_head's) and w the weights:

    mean            terms |s| + f mean_m|d|
    epistemic_std   terms max_m|d| + f mean_m|d| + value
    aleatoric_std   terms value, exp_arg max_m a_l / 2
    disagreement    terms max_pairs ||w (|d_m| + |d_m'|)||_2 + value
    epistemic       terms ||w (max_m|d| + f mean_m|d|)||_2 + value
    aleatoric       terms value, exp_arg the row's largest a_l / 2

The column 1e3 + 1e-2 z (spread 1e-5 of its offset) and the 1e4 state columns hold the kernel to
two passes over D alone: the variance through sums of squares, or through mu = D + s, has no
bits left there and misses epistemic_std by orders of magnitude.

Shapes: S + 1 on both sides of the kernel's 16-, 32-, 64- and 256-wide column groups (KP = S + 1
rounded up to a power of two in 16..256; S = 300 takes the kernel's second column chunk), and n
on both sides of its rows per block, 256 / KP (ROWS_PER_BLOCK). Measured error / bound per
output: profiles/ens_spread/README.md."""
import ctypes

import pytest
import torch

from drpo_amd import _abi, _lib
from gpu_helpers import C_LIBM, SPREAD_OUTPUTS as OUTPUTS, sp64, spread_statistics as statistics, within

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')

ROWS_PER_BLOCK = {1: 16, 12: 16, 15: 16, 16: 8, 51: 4, 255: 1, 300: 1}
SHAPES = sorted(ROWS_PER_BLOCK)
# (Z, zsel): repeats and unordered; the quadrotor tests' elites; every member of the largest list; M = 1
MEMBERS = [(3, [2, 0, 2, 1]), (7, [3, 0, 6, 2, 5]), (32, None), (5, [4])]
D_KINDS = 5


def rows_of(S):
    rp = ROWS_PER_BLOCK[S]
    return sorted({1, 5, 17, max(1, rp - 1), rp + 1})


def dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(x).to(dtype).contiguous().to(DEV)


def spread_inputs(S, n, Z):
    S1 = S + 1
    g = torch.Generator().manual_seed(100000 * Z + 1000 * S + n)
    lo = -10 + 8 * torch.rand(S1, generator=g)
    hi = -1 + 3 * torch.rand(S1, generator=g)
    j = (torch.arange(Z * n * S1) * 11 + S).reshape(Z, n, S1)
    kinds = torch.stack([torch.full((S1,), -1e3), lo - 25, lo, (lo + hi) / 2, hi, hi + 25, torch.full((S1,), 1e3)])
    LVR = kinds[j % 7, torch.arange(S1).expand(Z, n, S1)]
    z = torch.randn(Z, n, S1, generator=g)
    outlier = z.clone()
    outlier[Z // 2] += 50                                   # one member far from the rest
    cols = [2 * z, 1e3 + 1e-2 * z, (2 * z[:1]).expand(Z, n, S1), 1e-3 * z, outlier]
    kind = torch.arange(S1) % D_KINDS
    D = torch.stack(cols)[kind, :, :, torch.arange(S1)].permute(1, 2, 0)
    s = torch.randn(n, S, generator=g) * 3
    s[:, ::3] = 1e4 + 3 * torch.randn(n, len(range(0, S, 3)), generator=g)
    scale = 1 / (0.1 + 5 * torch.rand(S1, generator=g))
    scale[-1] = 0
    return D.contiguous().float(), LVR.contiguous().float(), s.contiguous().float(), lo, hi, scale.float(), kind


def spread(D, LVR, s, lo, hi, zsel, scale, outputs=OUTPUTS):
    """One drpo_ens_spread launch; the outputs named, prefilled with NaN, on the CPU."""
    Z, n, S1 = D.shape
    keep = [dev(D), dev(LVR), dev(s), dev(lo), dev(hi), dev(zsel, torch.int32), dev(scale)]
    bufs = {k: torch.full((n, S1) if k in OUTPUTS[:3] else (n,), float('nan'), device=DEV) for k in outputs}
    d = _abi.EnsSpread()
    d.D, d.LVR, d.s, d.minlv, d.maxlv, d.zsel, d.scale = (None if t is None else t.data_ptr() for t in keep)
    d.n, d.S, d.Z, d.M = n, S1 - 1, Z, Z if zsel is None else len(zsel)
    for k, v in bufs.items():
        setattr(d, k, v.data_ptr())
    _lib.check(_lib.lib().drpo_ens_spread(ctypes.byref(d), _lib.stream()), 'ens_spread')
    return {k: v.cpu() for k, v in bufs.items()}


def reference(D, LVR, s, lo, hi, zsel, scale):
    """float64 values of the six outputs and the (terms, exp_arg) of their bounds"""
    Z, n, S1 = D.shape
    sel = list(range(Z)) if zsel is None else list(zsel)
    d, raw = D.double()[sel], LVR.double()[sel]
    lo64, hi64 = lo.double(), hi.double()
    w = torch.ones(S1, dtype=torch.float64) if scale is None else scale.double()
    s0 = torch.cat([s.double(), torch.zeros(n, 1, dtype=torch.float64)], -1)
    l1 = hi64 - sp64(hi64 - raw)                                 # src/dynamics.py:132-133
    lv = lo64 + sp64(l1 - lo64)
    a_l = lo64.abs() + sp64(l1 - lo64) + torch.sigmoid(l1 - lo64) * (hi64.abs() + sp64(hi64 - raw))
    return statistics(d, lv, a_l / 2, s0, w, d.abs())


def bits(x):
    return x.view(torch.int32)


def same(a, b, names):
    for k in names:
        assert not torch.isnan(a[k]).any(), k
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize('Z,zsel', MEMBERS, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('S', SHAPES)
def test_against_float64(S, Z, zsel):
    for n in rows_of(S):
        D, LVR, s, lo, hi, scale, _ = spread_inputs(S, n, Z)
        for w in (scale, None) if n == 5 else (scale,):
            got = spread(D, LVR, s, lo, hi, zsel, w)
            ref, model = reference(D, LVR, s, lo, hi, zsel, w)
            tag = f'S={S} n={n} Z={Z} M={Z if zsel is None else len(zsel)} scale={"given" if w is not None else "NULL"}'
            for k in OUTPUTS:
                terms, exp_arg = model[k]
                within(f'ens_spread {k} {tag}', got[k], ref[k], terms, C_LIBM, exp_arg)


@pytest.mark.parametrize('S', [12, 16, 255, 300])
def test_one_member_and_identical_columns_are_exactly_zero(S):
    n = 9
    D, LVR, s, lo, hi, scale, kind = spread_inputs(S, n, 5)
    got = spread(D, LVR, s, lo, hi, [4], scale)
    zero = torch.zeros(n, dtype=torch.int32)
    assert torch.equal(bits(got['disagreement']), zero) and torch.equal(bits(got['epistemic']), zero)
    assert torch.equal(bits(got['epistemic_std']), torch.zeros(n, S + 1, dtype=torch.int32))
    assert torch.equal(bits(got['mean'][:, :-1]), bits(D[4, :, :-1] + s))
    # weights on the identical columns alone (kind 2): every pair's differences are exact zeros.
    # (The variance is not held to an exact 0 there: a float32 mean of equal values may round.)
    w = torch.where(kind == 2, scale + 1, torch.zeros_like(scale))
    assert int((w != 0).sum()) >= 2
    got = spread(D, LVR, s, lo, hi, [3, 0, 4, 2, 1], w)
    assert torch.equal(bits(got['disagreement']), zero)
    assert bool((got['epistemic_std'][:, kind == 0] > 0).all())
    got = spread(D, LVR, s, lo, hi, [3, 0, 4, 2, 1], scale)
    assert bool((got['disagreement'] > 0).all())


@pytest.mark.parametrize('S,Z,zsel', [(12, 7, [3, 0, 6, 2, 5]), (16, 3, [2, 0, 2, 1]), (51, 32, list(range(32))),
                                      (255, 7, [3, 0, 6, 2, 5]), (300, 32, list(range(32)))])
def test_member_order_does_not_move_the_disagreement(S, Z, zsel):
    """(a - b)^2 == (b - a)^2, a pair's sum runs over the columns in column order whichever lane
    takes it, and a maximum has no order."""
    n = 9
    D, LVR, s, lo, hi, scale, _ = spread_inputs(S, n, Z)
    first = spread(D, LVR, s, lo, hi, zsel, scale, ('disagreement',))
    g = torch.Generator().manual_seed(S)
    for perm in (zsel[::-1], [zsel[i] for i in torch.randperm(len(zsel), generator=g).tolist()]):
        assert perm != zsel
        same(spread(D, LVR, s, lo, hi, perm, scale, ('disagreement',)), first, ('disagreement',))


@pytest.mark.parametrize('S,n', [(12, 17), (51, 5), (300, 2)])
def test_null_outputs_and_null_zsel_change_no_bit(S, n):
    Z = 7
    D, LVR, s, lo, hi, scale, _ = spread_inputs(S, n, Z)
    full = spread(D, LVR, s, lo, hi, None, scale)
    same(spread(D, LVR, s, lo, hi, list(range(Z)), scale), full, OUTPUTS)     # zsel NULL is 0..Z-1
    for k in OUTPUTS:
        rest = tuple(o for o in OUTPUTS if o != k)
        same(spread(D, LVR, s, lo, hi, None, scale, rest), full, rest)
        same(spread(D, LVR, s, lo, hi, None, scale, (k,)), full, (k,))
    # without an aleatoric output LVR and the bounds may be NULL, without mean the states
    got = spread(D, None, None, None, None, None, scale, ('epistemic_std', 'disagreement', 'epistemic'))
    same(got, full, ('epistemic_std', 'disagreement', 'epistemic'))
