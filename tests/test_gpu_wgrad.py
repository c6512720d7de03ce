"""drpo_mlp_wgrad (csrc/wgrad.hip): grouped weight gradients gW += dZ^T Y, gb +=
colsum(dZ) for every layer of a group in one launch, against a float64 torch
reference of the same products (the autograd of nn.Linear / BatchedLinear,
src/dynamics.py:26-52, src/torch_util.py:190-211).

Covers every tile shape (64 / 16 wide on either side), widths that are not
multiples of 4 or 16, row counts that leave partial k-groups and partial row chunks,
ensemble batches (nbatch > 1), split-K over row chunks (the last-arriver combine),
the per-tile clip partials (sum of squares of the finished gradient), accumulation
into a non-zero gradient, bitwise determinism across launches and the workspace
being left zeroed. Tolerance (fp32 MFMA vs float64): |d| <= 1e-5 * sqrt(rows) *
max|ref| + 1e-5 * |ref|."""
import ctypes

import numpy as np
import pytest
import torch

import drpo_amd  # noqa: F401
from drpo_amd import _lib
from drpo_amd._abi import WgradItem

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


def make_items(shapes, rows, nbatch=1, seed=0, accumulate=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for dout, din in shapes:
        dz = torch.randn(nbatch, rows, dout, generator=g)
        y = torch.randn(nbatch, rows, din, generator=g)
        gW0 = torch.randn(nbatch, dout, din, generator=g) if accumulate else torch.zeros(nbatch, dout, din)
        gb0 = torch.randn(nbatch, dout, generator=g) if accumulate else torch.zeros(nbatch, dout)
        out.append(dict(dz=dz.to(DEV), y=y.to(DEV), gW=gW0.to(DEV), gb=gb0.to(DEV), gW0=gW0, gb0=gb0,
                        dout=dout, din=din))
    return out


def run(items, rows, nbatch, ws=None, sq=None):
    L = _lib.lib()
    arr = (WgradItem * len(items))()
    off = 0
    for k, d in enumerate(items):
        it = arr[k]
        it.dz, it.y, it.gW, it.gb = d['dz'].data_ptr(), d['y'].data_ptr(), d['gW'].data_ptr(), d['gb'].data_ptr()
        it.dout, it.din, it.rows, it.nbatch = d['dout'], d['din'], rows, nbatch
        it.zstride, it.ystride, it.gwstride, it.gbstride = rows * d['dout'], rows * d['din'], d['dout'] * d['din'], \
            d['dout']
        if sq is not None:
            it.sq, it.sq_off = sq.data_ptr(), off
            d['sq_off'] = off
            d['ntiles'] = L.drpo_mlp_wgrad_tiles(ctypes.byref(it))
            off += d['ntiles']
    need = L.drpo_mlp_wgrad_workspace_size(arr, len(items))
    if ws is None:
        ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=DEV)
    _lib.check(L.drpo_mlp_wgrad(arr, len(items), ws.data_ptr(), ws.numel(), _lib.stream()), 'wgrad')
    return ws


def reference(d):
    dz, y = d['dz'].double().cpu(), d['y'].double().cpu()
    gW = d['gW0'].double() + torch.einsum('zro,zri->zoi', dz, y)
    gb = d['gb0'].double() + dz.sum(1)
    return gW, gb


def check(d, rows):
    gW, gb = reference(d)
    scale = 1e-5 * np.sqrt(rows) * max(float(gW.abs().max()), 1.0)
    for got, ref, what in ((d['gW'], gW, 'gW'), (d['gb'], gb, 'gb')):
        err = (got.double().cpu() - ref).abs()
        tol = scale + 1e-5 * ref.abs()
        assert bool((err <= tol).all()), f'{what} {d["dout"]}x{d["din"]}: max err {float(err.max())}'
    return gW, gb


# (dout, din) per item: 64x64 tiles, 16-wide outputs (critic / head output layers),
# 16-wide inputs (S+A input layers), both narrow, widths not a multiple of 4 / 16
SHAPES = [(256, 256), (1, 256), (2, 256), (256, 14), (200, 200), (13, 200), (200, 14), (4, 4), (256, 53), (53, 256),
          (7, 13)]


@pytest.mark.parametrize('rows', [1, 37, 256, 1000, 4096])
def test_wgrad_shapes_and_rows(rows):
    items = make_items(SHAPES, rows, seed=rows)
    sq = torch.full((4096,), -1.0, device=DEV)
    run(items, rows, 1, sq=sq)
    torch.cuda.synchronize()
    for d in items:
        gW, gb = check(d, rows)
        # clip partials: sum of squares of the finished gradient, per tile (bias once per o-tile)
        parts = sq[d['sq_off']:d['sq_off'] + d['ntiles']].double().cpu()
        want = float((gW ** 2).sum() + (gb ** 2).sum())
        assert abs(float(parts.sum()) - want) <= 1e-4 * want + 1e-6, (d['dout'], d['din'], float(parts.sum()), want)


@pytest.mark.parametrize('rows,nbatch', [(256, 7), (256, 32), (100, 3), (2048, 2)])
def test_wgrad_ensemble_batches(rows, nbatch):
    shapes = [(200, 14), (200, 200), (200, 200), (13, 200), (200, 200), (13, 200)]
    items = make_items(shapes, rows, nbatch=nbatch, seed=nbatch)
    run(items, rows, nbatch)
    torch.cuda.synchronize()
    for d in items:
        check(d, rows)


def test_wgrad_accumulates_is_deterministic_and_leaves_workspace_zeroed():
    rows = 4096   # several row chunks per tile: the last-arriver combine
    items = make_items([(256, 256), (2, 256), (256, 14)], rows, seed=5, accumulate=True)
    base = [(d['gW'].clone(), d['gb'].clone()) for d in items]
    ws = run(items, rows, 1)
    torch.cuda.synchronize()
    for d in items:
        check(d, rows)
    first = [(d['gW'].clone(), d['gb'].clone()) for d in items]
    # the counters are back to zero (the slabs may hold data): a second launch on the same
    # workspace from the same start gives bitwise the same gradient
    for d, (w, b) in zip(items, base):
        d['gW'].copy_(w)
        d['gb'].copy_(b)
    run(items, rows, 1, ws=ws)
    torch.cuda.synchronize()
    for d, (w, b) in zip(items, first):
        assert torch.equal(d['gW'], w) and torch.equal(d['gb'], b)
    ntiles = 16 + 4 + 4     # arrival counters of the three items (first bytes of the workspace)
    assert int(ws[:4 * ntiles].view(torch.int32).abs().sum()) == 0


def test_wgrad_rejects_shared_gradient_and_small_workspace():
    rows = 64
    items = make_items([(16, 16)], rows)
    L = _lib.lib()
    arr = (WgradItem * 2)()
    for k in range(2):
        d = items[0]
        it = arr[k]
        it.dz, it.y, it.gW, it.gb = d['dz'].data_ptr(), d['y'].data_ptr(), d['gW'].data_ptr(), d['gb'].data_ptr()
        it.dout, it.din, it.rows, it.nbatch = 16, 16, rows, 1
        it.zstride, it.ystride, it.gwstride, it.gbstride = rows * 16, rows * 16, 256, 16
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    assert L.drpo_mlp_wgrad(arr, 2, ws.data_ptr(), ws.numel(), _lib.stream()) != 0
    big = make_items([(256, 256)], 4096)
    run(big, 4096, 1)          # sized workspace: fine
    arr1 = (WgradItem * 1)()
    d = big[0]
    it = arr1[0]
    it.dz, it.y, it.gW, it.gb = d['dz'].data_ptr(), d['y'].data_ptr(), d['gW'].data_ptr(), d['gb'].data_ptr()
    it.dout, it.din, it.rows, it.nbatch = 256, 256, 4096, 1
    it.zstride, it.ystride, it.gwstride, it.gbstride = 4096 * 256, 4096 * 256, 65536, 256
    assert L.drpo_mlp_wgrad(arr1, 1, ws.data_ptr(), 16, _lib.stream()) != 0


@pytest.mark.parametrize('rows', [37, 1792, 4096])
def test_wgrad_second_dz_term(rows):
    """drpo_wgrad_item_t.dz2 (the split-heads fit backward's trunk dZ = dz + dz2): the
    product is (dz + dz2)^T y and the bias colsum(dz + dz2), for 64-, 16- and odd-width
    tiles, ensemble batches and several row chunks."""
    L = _lib.lib()
    nb = 3
    shapes = [(200, 200), (200, 14), (13, 200)]
    items = make_items(shapes, rows, nbatch=nb, seed=rows + 7)
    g = torch.Generator().manual_seed(rows)
    arr = (WgradItem * len(items))()
    for k, d in enumerate(items):
        d['dz2'] = torch.randn(nb, rows, d['dout'], generator=g).to(DEV)
        it = arr[k]
        it.dz, it.y, it.gW, it.gb = d['dz'].data_ptr(), d['y'].data_ptr(), d['gW'].data_ptr(), d['gb'].data_ptr()
        it.dz2 = d['dz2'].data_ptr()
        it.dout, it.din, it.rows, it.nbatch = d['dout'], d['din'], rows, nb
        it.zstride, it.ystride, it.gwstride, it.gbstride = rows * d['dout'], rows * d['din'], d['dout'] * d['din'], \
            d['dout']
    need = L.drpo_mlp_wgrad_workspace_size(arr, len(items))
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=DEV)
    _lib.check(L.drpo_mlp_wgrad(arr, len(items), ws.data_ptr(), ws.numel(), _lib.stream()), 'wgrad')
    torch.cuda.synchronize()
    for d in items:
        dz = (d['dz'] + d['dz2']).double().cpu()
        y = d['y'].double().cpu()
        gW = torch.einsum('zro,zri->zoi', dz, y)
        gb = dz.sum(1)
        scale = 1e-5 * np.sqrt(rows) * max(float(gW.abs().max()), 1.0)
        for got, ref, what in ((d['gW'], gW, 'gW'), (d['gb'], gb, 'gb')):
            err = (got.double().cpu() - ref).abs()
            assert bool((err <= scale + 1e-5 * ref.abs()).all()), f'{what} {d["dout"]}x{d["din"]}: {float(err.max())}'


# ---- drpo_mlp_wgrad_adam: the Adam step and mirror refresh by the workgroup that finishes a tile ----
#
# One case = one layer (dout, din, nbatch) of a packed FlatGroup, the item being members
# [z0, z1) of it, driven twice from the same start: drpo_mlp_wgrad_adam, and drpo_mlp_wgrad +
# drpo_optim_step (zero_grad, the group's pack map with its host copy). Both run adam_step on
# gv + pv, so everything they leave is bitwise equal. The optimizer launch takes one segment
# over the whole group when the item is the whole matrix; for a member slice it takes the
# slice's weight and bias ranges, which is what the fused launch steps.
ADAM_LAYERS = [(200, 200, 3),    # 64x64 tiles, float4 finish
               (256, 53, 1),     # 64x64 tiles, scalar finish
               (200, 14, 3),     # 64x16
               (13, 200, 3),     # 16x64
               (7, 13, 1)]       # 16x16
# (layer, rows, members [z0, z1), start from a non-zero gradient); rows 37: one chunk with a
# partial k-group, rows 256: 4 row chunks per tile (the slab hand-off and the last arriver)
ADAM_CASES = [(ly, rows, (0, ly[2]), False) for ly in ADAM_LAYERS for rows in (37, 256)] + [
    ((200, 200, 3), 256, (1, 3), False),
    ((200, 200, 3), 37, (0, 3), True),
    ((13, 200, 3), 256, (0, 3), True)]


def adam_case(layer, rows, members, nonzero_grad, fused):
    from drpo_amd._abi import OptimSeg, WgradAdam
    from drpo_amd.optim import Adam
    from drpo_amd.params import FlatGroup
    dout, din, nb = layer
    z0, z1 = members
    nz = z1 - z0
    L = _lib.lib()
    g = FlatGroup('w')
    g.add('w.weight', (nb, dout, din))
    g.add('w.bias', (nb, dout))
    g.allocate(DEV)
    opt = Adam(g, lr=3e-3, weight_decay=1e-4)
    opt._ensure_state()
    gen = torch.Generator().manual_seed(1000 * dout + din + rows)
    for name in ('w.weight', 'w.bias'):    # the alignment padding between entries stays zero
        shape = g.entries[name][1]
        g.view(name).copy_(torch.randn(shape, generator=gen))
        g.view(name, opt.m).copy_(torch.randn(shape, generator=gen) * 0.01)
        g.view(name, opt.v).copy_(torch.rand(shape, generator=gen) * 0.01)
        if nonzero_grad:
            g.view(name, g.grad)[z0:z1].copy_(torch.randn((nz,) + shape[1:], generator=gen) * 0.1)
    dz = torch.randn(nz, rows, dout, generator=gen).to(DEV)
    y = torch.randn(nz, rows, din, generator=gen).to(DEV)
    g.enable_packing([('w.weight', din, dout, nb)], transposed=True)
    g.ensure_packed()
    start = dict(p=g.data.clone(), m=opt.m.clone(), v=opt.v.clone())
    arr = (WgradItem * 1)()
    it = arr[0]
    it.dz, it.y = dz.data_ptr(), y.data_ptr()
    it.gW, it.gb = g.view('w.weight', g.grad)[z0:].data_ptr(), g.view('w.bias', g.grad)[z0:].data_ptr()
    it.dout, it.din, it.rows, it.nbatch = dout, din, rows, nz
    it.zstride, it.ystride, it.gwstride, it.gbstride = rows * dout, rows * din, dout * din, dout
    need = L.drpo_mlp_wgrad_workspace_size(arr, 1)
    counters = (L.drpo_mlp_wgrad_tiles(ctypes.byref(it)) * 4 + 255) // 256 * 256
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=DEV)
    sc = opt.step_scalars()
    pm = g.pack_map()
    if fused:
        ad = WgradAdam()
        ad.g, ad.p, ad.m, ad.v = g.grad.data_ptr(), g.data.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr()
        ad.lr_over_bc1, ad.bc2_sqrt = sc
        ad.beta1, ad.beta2 = opt.betas
        ad.eps, ad.weight_decay = opt.eps, opt.weight_decay
        ad.map, ad.map_host = pm.data_ptr(), ctypes.addressof(pm.host)
        _lib.check(L.drpo_mlp_wgrad_adam(arr, 1, None, ctypes.byref(ad), ws.data_ptr(), ws.numel(), _lib.stream()),
                   'wgrad_adam')
    else:
        _lib.check(L.drpo_mlp_wgrad(arr, 1, ws.data_ptr(), ws.numel(), _lib.stream()), 'wgrad')
        if nz == nb:
            ranges = [(0, g.size)]
        else:
            ow, ob = g.offset('w.weight'), g.offset('w.bias')
            ranges = [(ow + z0 * dout * din, ow + z1 * dout * din), (ob + z0 * dout, ob + z1 * dout)]
        segs = [opt.segment(a, b, sc, zero_grad=True, pack_map=pm) for a, b in ranges]
        _lib.check(L.drpo_optim_step((OptimSeg * len(segs))(*segs), len(segs), _lib.stream()), 'optim_step')
    torch.cuda.synchronize()
    return g, opt, start, need, counters


@pytest.mark.parametrize('layer,rows,members,nonzero_grad', ADAM_CASES)
def test_wgrad_adam_matches_wgrad_then_optim_step(layer, rows, members, nonzero_grad):
    ga, oa, start, need, counters = adam_case(layer, rows, members, nonzero_grad, True)
    gb, ob, _, _, _ = adam_case(layer, rows, members, nonzero_grad, False)
    if rows == 256:   # row chunks: the slab hand-off and the last-arriver sum really ran
        assert need > counters, (need, counters)
    assert torch.equal(ga.data, gb.data), 'parameters'
    assert torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), 'Adam moments'
    assert torch.equal(ga.packed, gb.packed), 'forward mirror'
    assert torch.equal(ga.packedT, gb.packedT), 'transposed mirror'
    assert int((ga.grad != 0).sum()) == 0 and int((gb.grad != 0).sum()) == 0
    # the step happened, and only on the item's members
    dout, din, nb = layer
    z0, z1 = members
    W, W0 = ga.view('w.weight'), ga.view('w.weight', start['p'])
    assert not torch.equal(W[z0:z1], W0[z0:z1])
    assert torch.equal(W[:z0], W0[:z0]) and torch.equal(W[z1:], W0[z1:])
    # both mirrors == a fresh drpo_pack_weights of the result
    P, PT = ga.packed.clone(), ga.packedT.clone()
    ga.mark_dirty()
    ga.ensure_packed()
    torch.cuda.synchronize()
    assert torch.equal(P, ga.packed), 'forward mirror vs fresh pack'
    assert torch.equal(PT, ga.packedT), 'transposed mirror vs fresh pack'
