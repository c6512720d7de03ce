"""The constraint bound formed inside drpo_mlp_forward_multi (drpo_mlp_fwd_t.ccb_out) against
the stand-alone drpo_cc_head on the same job's saved head outputs, and against a float64
evaluation of the bound: one trunk job at the paired-heads shape, trunk [S+A -> 256 -> 256],
heads [256 -> 256 -> C], C = 3, 33 rows (two full 16-row tiles and a one-row third).

drpo_cc_head evaluates the row formula's one definition (csrc/sac_rows.hpp cc_bound_row), the
forward kernel a written-out copy of it, on the same float32 head outputs: they must agree
bit for bit (as they did on the parent commit). Against float64 the error is that of the hardware exp / log / rcp
(~1e-6 relative per call; raw log-stds in [-3.1, 1.3], bounds up to 6.7): measured
1.521e-06 on this input before the formula was shared, and 0 without ccb_dist, a plain
maximum (profiles/sac_refactor/README.md); twice that is allowed.

A second job scales the log-std head until its raw outputs span both soft clamps at +-4 (about
[-57, 70]): the same bit-equality, and the float64 comparison under the per-element error model of
tests/test_gpu_rowwise_edges.py (hardware transcendentals, c = 32)."""
import ctypes

import pytest
import torch

from drpo_amd import _abi, _lib
from drpo_amd.mlp_desc import ACT_ID, Net, fill_fwd
from drpo_amd.params import packed_size
from gpu_helpers import C_HW, within

pytestmark = pytest.mark.gpu

S, A, C, ROWS = 17, 6, 3, 33
RATIO, LMIN, LMAX = 2.0, -4.0, 4.0          # ConstraintCritic's defaults (src/ssac.py:70-72)
CCB_F64_TOL = 2 * 1.521239e-06              # 2 x the error measured on the parent commit (hardware transcendentals)


def _net(gen, dims, acts, out_scale=1.0):
    """A Net of uniform(+-1/sqrt(din)) layers with packed forward mirrors and a save of its output."""
    L, dev = _lib.lib(), torch.device('cuda')
    layers, keep = [], []
    for l, act in enumerate(acts):
        din, dout = dims[l], dims[l + 1]
        k = (out_scale if l == len(acts) - 1 else 1.0) / din ** 0.5
        W = ((torch.rand(dout, din, generator=gen) * 2 - 1) * k).to(dev)
        b = ((torch.rand(dout, generator=gen) * 2 - 1) * k).to(dev)
        Pk = torch.zeros(packed_size(din, dout), device=dev)
        it = _abi.PackItem()
        it.W, it.P, it.din, it.dout, it.nbatch = W.data_ptr(), Pk.data_ptr(), din, dout, 1
        _lib.check(L.drpo_pack_weights(ctypes.byref(it), 1, _lib.stream()), 'pack')
        layers.append((Pk, b, din, dout, ACT_ID[act], None))
        keep.append(W)
    net = Net(layers)
    net.sy[-1] = torch.empty(ROWS, dims[-1], device=dev)
    net.keep = keep
    return net


def make_job(seed=1234, ls_scale=24.0):
    """The job's nets (head outputs saved) and inputs; ls_scale 24: raw log-stds of a few units."""
    gen = torch.Generator().manual_seed(seed)
    nets = [_net(gen, [S + A, 256, 256], ['relu', 'relu']), _net(gen, [256, 256, C], ['relu', None]),
            _net(gen, [256, 256, C], ['relu', None], out_scale=ls_scale)]
    s = (torch.randn(ROWS, S, generator=gen)).cuda()
    a = (torch.rand(ROWS, A, generator=gen) * 2 - 1).cuda()
    return nets, s, a


@pytest.fixture(scope='module')
def job():
    return make_job()


def log_std_f64(ls):
    sp = torch.nn.functional.softplus
    return LMIN + sp(LMAX - sp(LMAX - ls.double()) - LMIN)


def bound_f64(mu, ls, dist):
    mu = mu.double()
    if not dist:
        return mu.max(dim=1).values
    return (mu + RATIO * log_std_f64(ls).exp()).max(dim=1).values


def run_bounds(job, dist):
    """(in-kernel bound, drpo_cc_head's bound, float64 bound) of the job with ccb_dist = dist"""
    L = _lib.lib()
    nets, s, a = job
    out = torch.full((ROWS,), float('nan'), device='cuda')
    d = fill_fwd(nets, [(s, S), (a, A), (None, 0)], ROWS, trunk=True)
    d.ccb_out, d.ccb_dist, d.ccb_ratio, d.ccb_lmin, d.ccb_lmax = out.data_ptr(), int(dist), RATIO, LMIN, LMAX
    arr = (_abi.MlpFwd * 1)(d)
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    _lib.check(L.drpo_mlp_forward_multi(arr, dev.data_ptr(), 1, 0, 0, _lib.stream()), 'forward_multi')
    mu, ls = nets[1].sy[-1], nets[2].sy[-1]
    alone = torch.full((ROWS,), float('nan'), device='cuda')
    _lib.check(L.drpo_cc_head(mu.data_ptr(), ls.data_ptr(), ROWS, C, int(dist), RATIO, LMIN, LMAX, alone.data_ptr(),
                              None, _lib.stream()), 'cc_head')
    torch.cuda.synchronize()
    return out.cpu(), alone.cpu(), bound_f64(mu.cpu(), ls.cpu(), dist), ls.cpu(), mu.cpu()


@pytest.mark.parametrize('dist', [False, True])
def test_in_kernel_bound_matches_cc_head_and_float64(job, dist):
    fused, alone, ref, ls, _ = run_bounds(job, dist)
    err = (fused.double() - ref).abs().max().item()
    print(f'ccb dist={int(dist)}: bit-equal to drpo_cc_head: {torch.equal(fused, alone)}; max |fused - f64| = {err:.3e}; '
          f'|bound| <= {ref.abs().max().item():.3f}; raw log-std in [{ls.min().item():.2f}, {ls.max().item():.2f}]')
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, alone)
    assert err <= (CCB_F64_TOL if dist else 0.0)


def test_in_kernel_bound_with_both_clamps_acting():
    """raw log-stds far outside [-4, 4] on both sides: std saturates at exp(-4) and exp(4)"""
    fused, alone, ref, ls, mu = run_bounds(make_job(seed=4321, ls_scale=576.0), True)
    print(f'ccb wide: bit-equal to drpo_cc_head: {torch.equal(fused, alone)}; |bound| <= {ref.abs().max().item():.3f}; '
          f'raw log-std in [{ls.min().item():.2f}, {ls.max().item():.2f}]; below -4: {(ls < LMIN).float().mean().item():.2f}, '
          f'above 4: {(ls > LMAX).float().mean().item():.2f}')
    assert ls.min() < -40 and ls.max() > 40
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, alone)
    log_std = log_std_f64(ls)
    std = log_std.exp()
    v = mu.double() + RATIO * std
    # |max_c got_c - max_c ref_c| <= max_c |got_c - ref_c|: the largest element bound of the row
    terms = (mu.double().abs() + RATIO * std + v.abs() * log_std.abs()).max(dim=1).values
    within('ccb wide in-kernel bound', fused, ref, terms, C_HW)
