"""The squashed-Gaussian head fused into drpo_mlp_forward_multi (squash_head_tile, hardware
transcendentals) and its backward fused into drpo_mlp_backward_multi_actor (squash_upstream),
against float64 on the prescribed table of test_gpu_rowwise_edges.py.

The net is the smallest the descriptor checks admit: ONE identity-activation layer [2A -> 2A]
with the identity matrix and a zero bias. The fp32 MFMA products x * 1 and x * 0 and their sums
are exact, so the layer's output IS the table (asserted bit for bit on its save): +-50 in the
means and +-100 in the log-std pre-activations reach the head unscaled.

Error model: gpu_helpers.error_ratio (test_gpu_rowwise_edges.py states it), c = 32 for the fused
forward head, c = 8 for the backward (libm but for one hardware sigmoid). Two terms are added to
it, with their derivations where they are used: the terms of fast_tanh's own difference
1 - 2 / (e^2u + 1) for the actions, and the log-std as a factor of the TERMS of d/d std (its
1/std terms cancel only as far as std itself is accurate)."""
import ctypes

import pytest
import torch

from drpo_amd import _abi, _lib
from drpo_amd.mlp_desc import (ACT_ID, HEAD_MEAN, HEAD_RSAMPLE, HEAD_SAMPLE, UPSTREAM_SQUASH, UPSTREAM_SQUASH_SAFE,
                               Net, fill_bwd, fill_fwd, with_head)
from drpo_amd.params import packed_size
from gpu_helpers import C_HW, C_LIBM, f64, within
from test_gpu_rowwise_edges import PI_SHAPES, dev, policy_std64, policy_table, squashed_logp64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


def identity_net(n):
    """One identity-activation layer [n -> n], W = I, b = 0, with both packed mirrors"""
    L = _lib.lib()
    W, b = torch.eye(n, device=DEV), torch.zeros(n, device=DEV)
    ps = packed_size(n, n)
    Pk, PT = torch.zeros(ps, device=DEV), torch.zeros(ps, device=DEV)
    it = _abi.PackItem()
    it.W, it.P, it.PT, it.din, it.dout, it.nbatch = W.data_ptr(), Pk.data_ptr(), PT.data_ptr(), n, n, 1
    it.wstride, it.pstride, it.ptstride = n * n, ps, ps
    _lib.check(L.drpo_pack_weights(ctypes.byref(it), 1, _lib.stream()), 'pack')
    net = Net([(Pk, b, n, n, ACT_ID[None], PT)])
    net.keep = W
    return net


def dev_copy(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


# ---------------------------------------------------------------------------
# 2 (b). the fused head of drpo_mlp_forward_multi
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('rows,A', PI_SHAPES)
def test_fused_squash_head(rows, A):
    L = _lib.lib()
    raw, eps = policy_table(rows, A)
    rawd, epsd = dev(raw), dev(eps)
    mu, pre, e = raw[:, :A].double(), raw[:, A:].double(), eps.double()
    log_std, std = policy_std64(pre)
    tag = f'rows={rows} A={A}'
    tanh_terms = lambda x: 1 + (1 - torch.tanh(x))      # fast_tanh is 1 - 2 / (e^2x + 1): |1| + |2 / (e^2x + 1)|
    for mode in (HEAD_SAMPLE, HEAD_RSAMPLE, HEAD_MEAN):
        net = identity_net(2 * A)
        net.sy[0] = torch.full((rows, 2 * A), float('nan'), device=DEV)
        o = {k: torch.full((rows,) if k == 'logp' else (rows, A), float('nan'), device=DEV)
             for k in ('a', 'logp', 'u', 'e', 'amean')}
        d = fill_fwd([net], [(rawd, 2 * A), (None, 0), (None, 0)], rows)
        with_head(d, mode, A, epsd, 0, **o)
        arr = (_abi.MlpFwd * 1)(d)
        dcopy = dev_copy(arr)
        _lib.check(L.drpo_mlp_forward_multi(arr, dcopy.data_ptr(), 1, 0, 0, _lib.stream()), 'forward_multi')
        torch.cuda.synchronize()
        assert torch.equal(net.sy[0].cpu(), raw), 'the identity layer did not carry the table through'
        within(f'fused head mode {mode} amean {tag}', o['amean'], torch.tanh(mu), tanh_terms(mu), C_HW)
        if mode == HEAD_MEAN:
            assert all(bool(torch.isnan(o[k]).all()) for k in ('a', 'logp', 'u', 'e'))   # mean only: nothing else written
            continue
        u_ref = mu + e * std
        within(f'fused head mode {mode} u {tag}', o['u'], u_ref, mu.abs() + (e * std).abs(), C_HW, log_std.abs())
        assert torch.equal(o['e'].cpu(), eps)
        u = f64(o['u'])                                  # the cached pre-image (test_gpu_rowwise_edges.test_policy_head)
        within(f'fused head mode {mode} a {tag}', o['a'], torch.tanh(u), tanh_terms(u), C_HW)
        lp, terms = squashed_logp64(u, mu, std)
        within(f'fused head mode {mode} logp {tag}', o['logp'], lp, terms, C_HW, log_std.abs().max(-1).values)


# ---------------------------------------------------------------------------
# 2 (c). DRPO_UPSTREAM_SQUASH / _SQUASH_SAFE of drpo_mlp_backward_multi_actor
# ---------------------------------------------------------------------------
TARGET_ENTROPY = -2.0


def squash_case(rows, A, side):
    """the saved tensors of one policy: raw outputs, draws, the float32 pre-tanh sample u, dL/da"""
    rr, aa = PI_SHAPES[(PI_SHAPES.index((rows, A)) + 4 * side) % len(PI_SHAPES)]
    n = rr * aa
    raw_all, eps_all = policy_table(rr, aa)                   # the safe actor: another window of the table
    pick = torch.arange(rows * A) % n
    mu = raw_all[:, :aa].reshape(-1)[pick].reshape(rows, A)
    pre = raw_all[:, aa:].reshape(-1)[pick].reshape(rows, A)
    eps = eps_all.reshape(-1)[pick].reshape(rows, A).contiguous()
    raw = torch.cat([mu, pre], 1).contiguous()
    _, std = policy_std64(pre.double())
    u = (mu.double() + eps.double() * std).float()             # what a forward saved, rounded to float32
    g = torch.Generator().manual_seed(rows * A + side)
    dA = torch.randn(rows, A, generator=g)
    return raw, eps, u, dA


@pytest.mark.parametrize('log_alpha', [-3.0, 0.0])
@pytest.mark.parametrize('rows,A', [(17, 1), (33, 6), (33, 8)])
def test_squash_upstream(rows, A, log_alpha):
    L = _lib.lib()
    lp_scale = 0.5
    g = torch.Generator().manual_seed(rows + A)
    logp = torch.randn(rows, generator=g) * 30
    cases = [squash_case(rows, A, side) for side in (0, 1)]
    ntiles = (rows + 15) // 16
    keep, jobs, nets, dxs = [], [], [], []
    h = _abi.ActorHead()
    h.B, h.C, h.A = rows, 1, A
    for side, (raw, eps, u, dA) in enumerate(cases):
        net = identity_net(2 * A)
        net.sy[0] = dev(raw)
        net.dz[0] = torch.full((rows, 2 * A), float('nan'), device=DEV)
        dx = torch.full((rows, 2 * A), float('nan'), device=DEV)
        t = [dev(u), dev(eps), dev(dA)]
        h.u[side], h.e[side], h.dA[side] = (x.data_ptr() for x in t)
        jobs.append(fill_bwd([net], [None], rows, dx={0: (dx, 0, 2 * A, False)},
                             upstream=UPSTREAM_SQUASH_SAFE if side else UPSTREAM_SQUASH))
        keep.append(t)
        nets.append(net)
        dxs.append(dx)
    logpd, lad = dev(logp), dev([log_alpha])
    asum = torch.full((ntiles,), float('nan'), device=DEV)
    h.logp, h.log_alpha, h.lp_scale, h.target_entropy, h.alpha_sum = (logpd.data_ptr(), lad.data_ptr(), lp_scale,
                                                                      TARGET_ENTROPY, asum.data_ptr())
    arr = (_abi.MlpBwd * 2)(*jobs)
    dcopy = dev_copy(arr)
    _lib.check(L.drpo_mlp_backward_multi_actor(arr, dcopy.data_ptr(), 2, ctypes.byref(h), _lib.stream()),
               'backward_multi_actor')
    torch.cuda.synchronize()
    for side, (raw, eps, u32, dA) in enumerate(cases):
        glp = float(torch.tensor(log_alpha).exp()) * lp_scale if side == 0 else 0.0
        mu = raw[:, :A].double().requires_grad_()
        pre = raw[:, A:].double().requires_grad_()
        e, dA64 = eps.double(), dA.double()
        log_std, std = policy_std64(pre)
        u = mu + e * std                                       # rsample
        u = u + (u32.double() - u).detach()                    # at the float32 value the forward saved
        lp, _ = squashed_logp64(u, mu, std)
        loss = (dA64 * torch.tanh(u)).sum() + glp * lp.sum()
        loss.backward()
        with torch.no_grad():
            a, diff, var = torch.tanh(u), u - mu, std ** 2
            sg = torch.sigmoid(pre)
            sig = torch.sigmoid(2 * u)                         # softplus'(-2u) = 1 - sig ... its terms: at most 4
            t_du = dA64.abs() * (1 + a * a) + glp * (diff.abs() / var + 2 + 4 * (1 - sig))
            t_mu = t_du + glp * diff.abs() / var
            # d/d std = du e + glp (diff^2 / std^3 - 1 / std): -glp e diff / var (in du e) and glp diff^2 / std^3
            # cancel only as far as diff / std = e, and the backward's std = exp(log_std) carries the relative
            # error 2^-24 |log_std| of its argument: the log-std multiplies these TERMS, not the (small) value
            t_dsd = (e.abs() * t_du + glp * (diff ** 2 / (var * std) + 1 / std)) * (1 + log_std.abs())
            t_pre = t_dsd * std * 10 * sg * (1 + sg)           # (1 - sg): terms 1 + sg
        tag = f'{"safe" if side else "actor"} rows={rows} A={A} log_alpha={log_alpha:g}'
        got = nets[side].dz[0].cpu()
        within(f'squash_upstream d mu {tag}', got[:, :A], mu.grad, t_mu, C_LIBM)
        within(f'squash_upstream d pre {tag}', got[:, A:], pre.grad, t_pre, C_LIBM)
        # the identity layer's input gradient is its output gradient
        assert torch.equal(dxs[side].cpu(), got)
    tile = torch.arange(rows) // 16
    ref = torch.zeros(ntiles, dtype=torch.float64).index_add_(0, tile, logp.double() + TARGET_ENTROPY)
    terms = torch.zeros(ntiles, dtype=torch.float64).index_add_(0, tile, logp.double().abs() + abs(TARGET_ENTROPY))
    within(f'squash_upstream alpha_sum rows={rows} A={A}', asum, ref, terms, C_LIBM)
