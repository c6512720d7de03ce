"""The riders on two launches, each against float64 or against the path the code promises to equal
bit for bit.

drpo_optim_step (csrc/optim.hip) besides Adam: a scalar parameter's gradient formed from device loss
partials (grad_from_sum, three kinds), the data-parallel mean folded into the step and into the clip
norm (grad_scale), the clip coefficient from any number of partials, and the flat fallback of a task
list that is full. mlp_wgrad_kernel (csrc/wgrad.hip) besides the weight gradients: its extra,
logically last workgroup, which adds loss partials (drpo_mlp_wgrad_sums), runs the NLL reduction
(drpo_mlp_wgrad_reduce) or runs it and steps the log-variance bounds (drpo_mlp_wgrad_adam with a
reduction: the production fit step).

The end-to-end goldens cannot see these: from a small state Adam moves a parameter by about
lr * sign(g), whatever the gradient's scale. So the gradient itself is probed: with m0 = v0 = 0 and no
weight decay, m' = (1 - beta1) g to one rounding, and m' / (1 - beta1) is the gradient the kernel formed.

References and error models: tests/optim_reference.py (its docstring has the derivations); measured
error / bound per comparison: profiles/launch_riders/README.md."""
import ctypes

import pytest
import torch

import drpo_amd  # noqa: F401
import test_gpu_optim as TO
import test_gpu_wgrad as TW
from drpo_amd import _lib
from drpo_amd._abi import EnsReduce, OptimSeg, SumDesc, WgradAdam, WgradItem
from drpo_amd.optim import Adam, fused_step, grad_sumsq
from drpo_amd.params import FlatGroup
from gpu_helpers import C_LIBM, f64, within
from optim_reference import (adam_ref, adam_terms, clip_coef_ref, ens_reduce_f32, ens_reduce_ref, f32,
                             lane_sum_roundings, scalar_grad_ref, sums_block_f32, sums_bound)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
NAN = float('nan')
GUARD = 64                               # NaNs behind every list a kernel walks: one element too far shows
BETAS32 = (f32(0.9), f32(0.999))         # the descriptor's c_float fields
EPS32 = f32(1e-8)
W1 = 1.0 - BETAS32[0]                    # 1.f - beta1, exact in float32


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    """bitwise equality (NaNs included)"""
    return torch.equal(bits(a), bits(b))


def item_array(items, rows, nbatch):
    arr = (WgradItem * len(items))()
    for it, d in zip(arr, items):
        it.dz, it.y, it.gW, it.gb = d['dz'].data_ptr(), d['y'].data_ptr(), d['gW'].data_ptr(), d['gb'].data_ptr()
        it.dout, it.din, it.rows, it.nbatch = d['dout'], d['din'], rows, nbatch
        it.zstride, it.ystride, it.gwstride, it.gbstride = rows * d['dout'], rows * d['din'], d['dout'] * d['din'], \
            d['dout']
    return arr


def small_item(nbatch, seed=0):
    """the smallest weight-gradient item, one row: units = nbatch, so the grid is nbatch + 1"""
    items = TW.make_items([(16, 16)], 1, nbatch=nbatch, seed=seed)
    arr = item_array(items, 1, nbatch)
    need = _lib.lib().drpo_mlp_wgrad_workspace_size(arr, 1)
    return items, arr, torch.zeros(max(need, 256), dtype=torch.uint8, device=DEV)


# ---------------------------------------------------------------------------
# 1. drpo_mlp_wgrad_sums: the sums block
# ---------------------------------------------------------------------------
def sum_values(n, seed):
    """mixed signs, magnitudes spread over 1e-3 .. 1e3"""
    g = torch.Generator().manual_seed(seed)
    mag = 10 ** (torch.rand(n, generator=g) * 6 - 3)
    return torch.where(torch.rand(n, generator=g) < 0.5, -mag, mag).float()


def sum_descs(ns, seed=0):
    vals = [sum_values(n, 1000 * seed + 7 * q + n) for q, n in enumerate(ns)]
    parts = [torch.cat([v, torch.full((GUARD,), NAN)]).to(DEV) for v in vals]
    outs = torch.full((len(ns),), NAN, device=DEV)
    arr = (SumDesc * len(ns))()
    for q, n in enumerate(ns):
        arr[q].part, arr[q].n, arr[q].out = parts[q].data_ptr(), n, outs[q:].data_ptr()
    return vals, parts, outs, arr


def launch_sums(items_arr, nitems, sums, nsums, ws):
    return _lib.lib().drpo_mlp_wgrad_sums(items_arr, nitems, sums, nsums, None if ws is None else ws.data_ptr(),
                                          0 if ws is None else ws.numel(), _lib.stream())


def check_sums(tag, vals, outs):
    """Each lane adds ceil(n / 256) values in order, block_tree_sum adds 8 levels:
    |err| <= (ceil(n / 256) + 8) 2^-24 sum |part|; nothing to round at n = 0 and n = 1. Then the same
    order in numpy float32 (optim_reference.sums_block_f32): the same bits."""
    got = outs.cpu()
    for q, v in enumerate(vals):
        ref, c, terms = sums_bound(v)
        if v.numel() == 0:
            assert same_bits(got[q], torch.zeros(())), (tag, q, got[q])
        elif v.numel() == 1:
            assert same_bits(got[q], v[0]), (tag, q, got[q], v[0])
        else:
            within(f'wgrad_sums {tag} sum {q} n={v.numel()}', got[q], torch.tensor(ref, dtype=torch.float64), terms, c)
        # and the documented order itself, bit for bit (the bound is a worst case, met to a hundredth)
        assert same_bits(got[q], torch.tensor(sums_block_f32(v))), (tag, q, got[q], sums_block_f32(v))


SUMS_NS = [(0,), (1,), (255,), (256,), (257,), (1000,), (257, 0), (1, 1000), (0, 256, 1000, 1), (255, 257, 1, 0)]


@pytest.mark.parametrize('ns', SUMS_NS, ids=lambda ns: '-'.join(map(str, ns)))
def test_wgrad_sums_counts(ns):
    items, arr, ws = small_item(1, seed=len(ns))
    vals, parts, outs, sums = sum_descs(ns, seed=sum(ns))
    _lib.check(launch_sums(arr, 1, sums, len(ns), ws), 'wgrad_sums')
    torch.cuda.synchronize()
    check_sums(f'ns={ns}', vals, outs)
    TW.check(items[0], 1)


def test_wgrad_sums_are_the_same_under_any_grid_and_without_items():
    """nbatch 1..8: grids of units + 1 = 2..9 workgroups, every residue mod 8 of xcd_block()'s remap;
    the extra workgroup is reached exactly once (an out written twice would still be right: the NaN
    prefill shows only a sum that was never stored, so the item's gradient, which accumulates, is
    what shows a unit run twice). No items, or only an item without rows: one workgroup, no workspace."""
    ns = (1000, 257, 0, 255)
    first = None
    for nb in range(1, 9):
        items, arr, ws = small_item(nb, seed=nb)
        for again in range(2):
            vals, parts, outs, sums = sum_descs(ns, seed=3)
            for d in items:
                d['gW'].zero_()
                d['gb'].zero_()
            _lib.check(launch_sums(arr, 1, sums, len(ns), ws), 'wgrad_sums')
            torch.cuda.synchronize()
            if first is None:
                check_sums('grid', vals, outs)
                first = outs.clone()
            assert same_bits(outs, first), (nb, again, outs, first)
            TW.check(items[0], 1)
    vals, parts, outs, sums = sum_descs(ns, seed=3)
    _lib.check(launch_sums(None, 0, sums, len(ns), None), 'wgrad_sums')
    torch.cuda.synchronize()
    assert same_bits(outs, first), (outs, first)
    items, _, _ = small_item(1)
    arr = item_array(items, 0, 1)          # rows = 0: planned away
    assert _lib.lib().drpo_mlp_wgrad_workspace_size(arr, 1) == 0
    vals, parts, outs, sums = sum_descs(ns, seed=3)
    _lib.check(launch_sums(arr, 1, sums, len(ns), None), 'wgrad_sums')
    torch.cuda.synchronize()
    assert same_bits(outs, first), (outs, first)
    assert int((items[0]['gW'] != 0).sum()) == 0 and int((items[0]['gb'] != 0).sum()) == 0


@pytest.mark.parametrize('brk', ['nsums = 5', 'null part', 'null out'])
def test_wgrad_sums_rejects_and_launches_nothing(brk):
    items, arr, ws = small_item(1)
    vals, parts, outs, sums = sum_descs((3, 257, 1, 5, 2))
    nsums = 5 if brk == 'nsums = 5' else 4
    if brk == 'null part':
        sums[1].part = None
    if brk == 'null out':
        sums[2].out = None
    assert launch_sums(arr, 1, sums, nsums, ws) != 0
    assert _lib.lib().drpo_last_error().decode().startswith('drpo_mlp_wgrad_sums'), brk
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs).all())
    assert int((items[0]['gW'] != 0).sum()) == 0


# ---------------------------------------------------------------------------
# 2. The NLL reduction block, alone and on a weight-gradient launch
# ---------------------------------------------------------------------------
# (Z, nbx, S1): one and several trips of the z, q and c loops (16-strided), both descriptor limits
RED_CASES = [(1, 1, 2), (3, 3, 16), (16, 16, 17), (17, 17, 16), (33, 40, 5), (7, 2, 256), (256, 1, 2)]
WEIGHT = f32(0.01)                     # the descriptor's c_float


def red_partials(Z, nbx, S1, seed, shift=0.0, mse_scale=2.0):
    """mse [Z][nbx], min / max [Z][nbx][S1] (mixed signs; shift: the bound gradients' common sign) and the
    bounds; the device workspace in the EnsPartials layout mse | min | max, NaNs behind it"""
    g = torch.Generator().manual_seed(seed)
    mse = torch.randn(Z, nbx, generator=g) * mse_scale
    mn = torch.randn(Z, nbx, S1, generator=g) * 0.05 + shift
    mx = torch.randn(Z, nbx, S1, generator=g) * 0.05 - shift
    minlv = -10 + 8 * torch.rand(S1, generator=g)
    maxlv = -1 + 3 * torch.rand(S1, generator=g)
    ws = torch.cat([mse.reshape(-1), mn.reshape(-1), mx.reshape(-1), torch.full((GUARD,), NAN)]).to(DEV)
    return mse, mn, mx, minlv, maxlv, ws


def red_desc(ws, Z, nbx, S1, minlv, maxlv, gscale, mse, loss, gmin, gmax):
    r = EnsReduce()
    r.part, r.nbx, r.Z, r.S1, r.weight = ws.data_ptr(), nbx, Z, S1, WEIGHT
    r.minlv, r.maxlv = minlv.data_ptr(), maxlv.data_ptr()
    r.gscale = None if gscale is None else gscale.data_ptr()
    r.mse = mse.data_ptr()
    r.loss = None if loss is None else loss.data_ptr()
    r.gmin = None if gmin is None else gmin.data_ptr()
    r.gmax = None if gmax is None else gmax.data_ptr()
    return r


@pytest.mark.parametrize('Z,nbx,S1', RED_CASES)
def test_reduce_block_alone_and_riding(Z, nbx, S1):
    """ens_loss_reduce_block through drpo_ens_loss_reduce and as the extra workgroup of
    drpo_mlp_wgrad_reduce (grids of 2 and 9): the same device function, so bitwise the same mse, loss,
    gmin, gmax; against float64 under optim_reference.ens_reduce_ref's counts, and bit for bit against the
    block's order restated in numpy float32 (ens_reduce_f32). Flavours: gscale NULL /
    0.37, gmin and gmax present (prefilled 0.25) / NULL, loss present / NULL; an output a flavour shares
    with an earlier one is bitwise the earlier one's."""
    L = _lib.lib()
    mse_p, mn_p, mx_p, minlv, maxlv, ws = red_partials(Z, nbx, S1, 100 * Z + nbx + S1)
    lo, hi = minlv.to(DEV), maxlv.to(DEV)
    gs37 = torch.tensor([0.37], device=DEV)
    tag = f'Z={Z} nbx={nbx} S1={S1}'
    seen = {}

    def compare(key, name, got, ref):
        if key in seen:
            assert same_bits(got, seen[key]), (tag, key)
            return
        seen[key] = got.clone()
        val, c, terms = ref
        within(f'reduce {name} {tag}', got.reshape(val.shape), val, terms, c)

    for gscale in (None, 0.37):
        ref = ens_reduce_ref(mse_p, mn_p, mx_p, minlv, maxlv, WEIGHT, None if gscale is None else f32(gscale), 0.25)
        for grads in (True, False):
            for has_loss in (True, False):
                outs = []
                for entry in ('alone', 1, 8):
                    mse = torch.full((Z,), NAN, device=DEV)
                    loss = torch.full((1,), NAN, device=DEV) if has_loss else None
                    gmin = torch.full((S1,), 0.25, device=DEV) if grads else None
                    gmax = torch.full((S1,), 0.25, device=DEV) if grads else None
                    red = red_desc(ws, Z, nbx, S1, lo, hi, gs37 if gscale else None, mse, loss, gmin, gmax)
                    if entry == 'alone':
                        _lib.check(L.drpo_ens_loss_reduce(ctypes.byref(red), _lib.stream()), 'ens_loss_reduce')
                    else:
                        items, arr, wws = small_item(entry, seed=Z + entry)
                        _lib.check(L.drpo_mlp_wgrad_reduce(arr, 1, ctypes.byref(red), wws.data_ptr(), wws.numel(),
                                                           _lib.stream()), 'wgrad_reduce')
                    torch.cuda.synchronize()
                    if entry != 'alone':
                        TW.check(items[0], 1)
                    outs.append((mse, loss, gmin, gmax))
                for other in outs[1:]:
                    for a, b in zip(outs[0], other):
                        assert (a is None and b is None) or same_bits(a, b), (tag, gscale, grads, has_loss)
                mse, loss, gmin, gmax = outs[0]
                compare('mse', 'mse', mse, ref['mse'])
                if has_loss:
                    compare('loss', 'loss', loss, ref['loss'])
                if grads:
                    compare(('gmin', gscale), f'gmin gscale={gscale}', gmin, ref['gmin'])
                    compare(('gmax', gscale), f'gmax gscale={gscale}', gmax, ref['gmax'])
    # the block's own order in numpy float32: the same bits (the loss up to the compiler's choice of an fma)
    emse, egmin, egmax, eloss = ens_reduce_f32(mse_p, mn_p, mx_p, minlv, maxlv, WEIGHT, 0.25)
    for key, want in (('mse', emse), (('gmin', None), egmin), (('gmax', None), egmax)):
        assert same_bits(seen[key].cpu(), torch.from_numpy(want)), (tag, key, seen[key], want)
    assert any(same_bits(seen['loss'].cpu()[0], torch.tensor(v)) for v in eloss), (tag, seen['loss'], eloss)


# ---------------------------------------------------------------------------
# 3. The fused fit step: drpo_mlp_wgrad_adam with a reduction
# ---------------------------------------------------------------------------
FIT_ENTRIES = ('w.weight', 'w.bias', 'min_log_var', 'max_log_var')
# (layer (dout, din, nbatch), S1, rows); rows 37: one row chunk, 256: the slab hand-off
FIT_CASES = [((200, 14, 3), 14, 37), ((200, 14, 3), 14, 256), ((13, 200, 3), 17, 256)]


def fit_case(layer, S1, rows, nonzero, fused):
    """One FlatGroup (weight, bias and the two log-variance bounds; random non-zero Adam state), the
    layer's weight-gradient item and synthetic NLL partials whose reduction reads and writes the bounds
    inside the group. fused: drpo_mlp_wgrad_adam with the reduction; else drpo_mlp_wgrad_reduce, then
    one drpo_optim_step segment over the whole group."""
    dout, din, nb = layer
    L = _lib.lib()
    g = FlatGroup('w')
    g.add('w.weight', (nb, dout, din))
    g.add('w.bias', (nb, dout))
    g.add('min_log_var', (S1,))
    g.add('max_log_var', (S1,))
    g.allocate(DEV)
    opt = Adam(g, lr=3e-3, weight_decay=1e-4)
    opt._ensure_state()
    gen = torch.Generator().manual_seed(1000 * dout + din + rows)
    for name in FIT_ENTRIES:           # the alignment padding between entries stays zero
        shape = g.entries[name][1]
        g.view(name).copy_(torch.randn(shape, generator=gen))
        g.view(name, opt.m).copy_(torch.randn(shape, generator=gen) * 0.01)
        g.view(name, opt.v).copy_(torch.rand(shape, generator=gen) * 0.01)
        if nonzero:
            g.view(name, g.grad).copy_(torch.randn(shape, generator=gen) * 0.1)
    dz = torch.randn(nb, rows, dout, generator=gen).to(DEV)
    y = torch.randn(nb, rows, din, generator=gen).to(DEV)
    g.enable_packing([('w.weight', din, dout, nb)], transposed=True)
    g.ensure_packed()
    start = dict(p=g.data.clone(), g=g.grad.clone(), m=opt.m.clone(), v=opt.v.clone())
    arr = item_array([dict(dz=dz, y=y, gW=g.view('w.weight', g.grad), gb=g.view('w.bias', g.grad), dout=dout,
                           din=din)], rows, nb)
    need = L.drpo_mlp_wgrad_workspace_size(arr, 1)
    wws = torch.zeros(max(need, 256), dtype=torch.uint8, device=DEV)
    # the bound gradients get a common sign (min up, max down), so the step moves
    # sum(max) - sum(min) one way: the loss must have been formed from the values before it
    Z, nbx = nb, (rows + 15) // 16
    parts = red_partials(Z, nbx, S1, rows + S1, shift=0.1, mse_scale=0.1)
    gscale = torch.tensor([0.37], device=DEV) if nonzero else None
    mse = torch.full((Z,), NAN, device=DEV)
    loss = torch.full((1,), NAN, device=DEV)
    red = red_desc(parts[5], Z, nbx, S1, g.view('min_log_var'), g.view('max_log_var'), gscale, mse, loss,
                   g.view('min_log_var', g.grad), g.view('max_log_var', g.grad))
    sc = opt.step_scalars()
    pm = g.pack_map()
    if fused:
        ad = WgradAdam()
        ad.g, ad.p, ad.m, ad.v = g.grad.data_ptr(), g.data.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr()
        ad.lr_over_bc1, ad.bc2_sqrt = sc
        ad.beta1, ad.beta2 = opt.betas
        ad.eps, ad.weight_decay = opt.eps, opt.weight_decay
        ad.map, ad.map_host = pm.data_ptr(), ctypes.addressof(pm.host)
        _lib.check(L.drpo_mlp_wgrad_adam(arr, 1, ctypes.byref(red), ctypes.byref(ad), wws.data_ptr(), wws.numel(),
                                         _lib.stream()), 'wgrad_adam')
    else:
        _lib.check(L.drpo_mlp_wgrad_reduce(arr, 1, ctypes.byref(red), wws.data_ptr(), wws.numel(), _lib.stream()),
                   'wgrad_reduce')
        fused_step([opt.segment(0, g.size, sc, zero_grad=True, pack_map=pm)])
    torch.cuda.synchronize()
    return g, opt, start, sc, parts, mse, loss, (0.37 if nonzero else None)


@pytest.mark.parametrize('nonzero', [False, True], ids=['zero-grad', 'nonzero-grad'])
@pytest.mark.parametrize('layer,S1,rows', FIT_CASES)
def test_fused_fit_step_matches_reduce_then_optim_step(layer, S1, rows, nonzero):
    ga, oa, start, sc, parts, mse_a, loss_a, gscale = fit_case(layer, S1, rows, nonzero, True)
    gb, ob, _, _, _, mse_b, loss_b, _ = fit_case(layer, S1, rows, nonzero, False)
    # both paths run adam_step on g0 + (a -/+ gw): bitwise
    assert torch.equal(ga.data, gb.data), 'parameters'
    assert torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), 'Adam moments'
    assert torch.equal(ga.packed, gb.packed) and torch.equal(ga.packedT, gb.packedT), 'mirrors'
    assert int((ga.grad != 0).sum()) == 0 and int((gb.grad != 0).sum()) == 0
    assert same_bits(mse_a, mse_b) and same_bits(loss_a, loss_b)
    mse_p, mn_p, mx_p, _, _, _ = parts
    v0 = lambda name, key: f64(ga.view(name, start[key]))
    tag = f'{layer} S1={S1} rows={rows} nonzero={nonzero}'
    ref = ens_reduce_ref(mse_p, mn_p, mx_p, v0('min_log_var', 'p'), v0('max_log_var', 'p'), WEIGHT,
                         None if gscale is None else f32(gscale), (v0('min_log_var', 'g'), v0('max_log_var', 'g')))
    # the loss is that of the bounds BEFORE the step, which moved them by far more than the bound
    val, c, terms = ref['loss']
    within(f'fit loss {tag}', loss_a[0], val, terms, c)
    moved = WEIGHT * ((f64(ga.view('max_log_var')) - v0('max_log_var', 'p')).sum()
                      - (f64(ga.view('min_log_var')) - v0('min_log_var', 'p')).sum())
    assert abs(float(moved)) > 20 * c * 2.0 ** -24 * float(terms), (float(moved), float(terms))
    within(f'fit mse {tag}', mse_a, ref['mse'][0], ref['mse'][2], ref['mse'][1])
    # the bounds' new values against float64 Adam on the float64 bound gradient
    a, bc2 = f32(sc[0]), f32(sc[1])
    wd = f32(1e-4)
    for name, key in (('min_log_var', 'gmin'), ('max_log_var', 'gmax')):
        gref, c_g, t_g = ref[key]
        p, m, v = adam_ref(v0(name, 'p'), gref, v0(name, 'm'), v0(name, 'v'), a, bc2, BETAS32, EPS32, wd)
        _, T_m, _ = adam_terms(v0(name, 'p'), gref, v0(name, 'm'), v0(name, 'v'), t_g * c_g / C_LIBM, a, bc2,
                               BETAS32, EPS32, wd)
        within(f'fit {name} m {tag}', ga.view(name, oa.m), m, T_m, C_LIBM)
        for got, want, what in ((ga.view(name), p, 'p'), (ga.view(name, oa.v), v, 'v')):
            err = (f64(got) - want).abs()
            tol = 2e-6 * want.abs() + 1e-7
            print(f'edge-ratio fit {name} {what} {tag}: max err/tol {(err / tol).max().item():.3g}')
            assert bool((err <= tol).all()), f'{name} {what}: max err {float(err.max())}'
        assert not torch.equal(ga.view(name), ga.view(name, start['p']))


# ---------------------------------------------------------------------------
# 4. Scalar gradients from a device sum: grad_from_sum
# ---------------------------------------------------------------------------
KIND_P = {0: [-20.0, -5.0, 0.0, 1.5, 10.0], 1: [-30.0, -1.0, 0.0, 2.0, 30.0], 2: [0.3] * 5}
GS_N = [0, 1, 16, 63, 64, 65, 200]
LR = 3e-3


def small_group(seed, wd=1e-4, state=True):
    """a few thousand elements: two packed matrices (members, din % 4 != 0; one float4-able) and biases"""
    layers = [('a.weight', 14, 13, 3), ('b.weight', 16, 8, 1)]
    g = FlatGroup('s')
    for name, din, dout, nb in layers:
        g.add(name, (nb, dout, din) if nb > 1 else (dout, din))
        g.add(name.replace('weight', 'bias'), (nb, dout) if nb > 1 else (dout,))
    g.allocate(DEV)
    gen = torch.Generator().manual_seed(seed)
    g.data.copy_(torch.randn(g.size, generator=gen))
    g.grad.copy_(torch.randn(g.size, generator=gen) * 0.1)
    g.enable_packing(layers, transposed=True)
    g.ensure_packed()
    opt = Adam(g, lr=LR, weight_decay=wd)
    opt._ensure_state()
    if state:
        opt.m.copy_(torch.randn(g.size, generator=gen) * 0.01)
        opt.v.copy_(torch.rand(g.size, generator=gen) * 0.01)
    return g, opt


def matrix_segment(seed):
    g, opt = small_group(seed)
    part = grad_sumsq(g.grad)
    return g, opt, opt.segment(0, g.size, opt.step_scalars(), clip=(part, 0.5), zero_grad=True,
                               pack_map=g.pack_map()), part


class Scalar:
    """A one-element optimizer whose gradient the step forms from device partials."""

    def __init__(self, kind, p, partials, n, rows, m0, v0):
        self.kind, self.n, self.rows = kind, n, rows
        self.t = torch.tensor([p], device=DEV)
        self.p0 = float(self.t.item())
        self.opt = Adam(None, lr=LR, tensor=self.t)
        self.opt._ensure_state()
        self.opt.m.fill_(m0)
        self.opt.v.fill_(v0)
        self.m0, self.v0 = float(self.opt.m.item()), float(self.opt.v.item())
        self.partials, self.grad = partials, torch.full((1,), 7.0, device=DEV)
        self.sc = self.opt.step_scalars()
        self.seg = self.opt.segment(0, 1, self.sc, grad=self.grad, grad_from_sum=(partials, rows, n),
                                    grad_from_sum_kind=kind)

    def result(self):
        return torch.stack([self.t[0], self.opt.m[0], self.opt.v[0]]).cpu()


def scalar_partials(n, seed):
    """max(n, 1) mixed-sign values (the kernel treats n = 0 as 1), NaNs behind them"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(max(n, 1), generator=g) * 3
    return vals, torch.cat([vals, torch.full((GUARD,), NAN)]).to(DEV)


@pytest.mark.parametrize('n', GS_N)
def test_scalar_gradient_from_device_partials(n):
    """The three kinds as three segments of one launch next to a clipped matrix segment (the actor
    launch of sac_step.py), and each alone: bitwise the same. Probe (m0 = v0 = 0): m' / (1 - beta1) is the
    gradient the kernel formed, -c(p) sum / rows, within (ceil(n / 64) + 6 + C_LIBM) 2^-24 c(p) sum|part| /
    rows: the lane loop, wave_sum's 6 levels, and C_LIBM for the expf, the divide and the products. Full
    step (random m0, v0): m, v, p within optim_reference.adam_terms at C_LIBM."""
    n_eff = max(n, 1)
    c_sum = lane_sum_roundings(n_eff, 64, 6) + C_LIBM
    for rows in (256, 512):
        for i in range(5):
            for mode in ('probe', 'full'):
                vals, partials = scalar_partials(n, 1000 * n + rows + i)
                before = partials.clone()
                gen = torch.Generator().manual_seed(i + rows)
                st = lambda: (0.0, 0.0) if mode == 'probe' else (
                    float(torch.randn((), generator=gen)) * 0.01, float(torch.rand((), generator=gen)) * 0.01 + 1e-5)
                states = [st() for _ in range(3)]
                make = lambda: [Scalar(k, KIND_P[k][i], partials, n, rows, *states[k]) for k in range(3)]
                company = make()
                gm, om, seg_m, part_m = matrix_segment(i)
                fused_step([seg_m] + [s.seg for s in company])
                alone = make()
                for s in alone:
                    fused_step([s.seg])
                ga_, oa_, seg_a, part_a = matrix_segment(i)
                fused_step([seg_a])
                torch.cuda.synchronize()
                assert torch.equal(gm.data, ga_.data) and torch.equal(om.m, oa_.m) and torch.equal(om.v, oa_.v)
                assert torch.equal(gm.packed, ga_.packed) and torch.equal(gm.packedT, ga_.packedT)
                assert same_bits(partials, before), 'the partials are read, never written'
                for s, a in zip(company, alone):
                    tag = f'kind={s.kind} p={s.p0:g} n={n} rows={rows} {mode}'
                    p, m, v = s.result().double()
                    assert same_bits(s.result(), a.result()), tag
                    assert float(s.grad.item()) == 7.0 and float(a.grad.item()) == 7.0, 'grad= is left alone'
                    gref, terms = scalar_grad_ref(s.kind, s.p0, vals[:n_eff], rows)
                    if mode == 'probe':
                        within(f'grad_from_sum gradient {tag}', m / W1, torch.tensor(gref, dtype=torch.float64), terms,
                               c_sum)
                    lr1, bc2 = f32(s.sc[0]), f32(s.sc[1])
                    rp, rm, rv = adam_ref(*(torch.tensor(x, dtype=torch.float64) for x in (s.p0, gref, s.m0, s.v0)),
                                          lr1, bc2, BETAS32, EPS32, 0.0)
                    T_p, T_m, T_v = adam_terms(s.p0, gref, s.m0, s.v0, terms * c_sum / C_LIBM, lr1, bc2, BETAS32,
                                               EPS32, 0.0)
                    within(f'grad_from_sum m {tag}', m, rm, T_m, C_LIBM)
                    within(f'grad_from_sum v {tag}', v, rv, T_v, C_LIBM)
                    within(f'grad_from_sum p {tag}', p, rp, T_p, C_LIBM)


# ---------------------------------------------------------------------------
# 5. grad_scale: the data-parallel mean inside the step
# ---------------------------------------------------------------------------
def scale_run(block, clip, scale, gmul=1.0):
    """test_gpu_optim's group and state, one segment over all of it; gmul: the gradient pre-multiplied"""
    g = TO.make_group('g', 1)
    if gmul != 1.0:
        g.grad.mul_(gmul)
    opt = Adam(g, lr=3e-3, weight_decay=1e-4)
    opt._ensure_state()
    gen = torch.Generator(device='cpu').manual_seed(3)
    opt.m.copy_(torch.randn(g.size, generator=gen) * 0.01)
    opt.v.copy_(torch.rand(g.size, generator=gen) * 0.01)
    g0 = dict(p=g.data.clone(), g=g.grad.clone(), m=opt.m.clone(), v=opt.v.clone())
    pm = g.pack_map()
    if not block:
        pm = pm.clone()         # a device map without the host copy: the flat split
    part = grad_sumsq(g.grad) if clip else None
    sc = opt.step_scalars()
    fused_step([opt.segment(0, g.size, sc, clip=(part, 0.5) if clip else None, zero_grad=True, pack_map=pm,
                            grad_scale=scale)])
    torch.cuda.synchronize()
    return g, opt, g0, sc


def assert_same_step(a, b):
    (ga, oa, _, _), (gb, ob, _, _) = a, b
    assert torch.equal(ga.data, gb.data), 'parameters'
    assert torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), 'Adam moments'
    assert torch.equal(ga.packed, gb.packed) and torch.equal(ga.packedT, gb.packedT), 'mirrors'
    assert int((ga.grad != 0).sum()) == 0 and int((gb.grad != 0).sum()) == 0


@pytest.mark.parametrize('clip', [False, True], ids=['noclip', 'clip'])
@pytest.mark.parametrize('block', [True, False], ids=['blocks', 'flat'])
def test_grad_scale_half_is_the_halved_gradient(block, clip):
    """sum (g/2)^2 = sum g^2 / 4 and sqrt(s / 4) = sqrt(s) / 2 are exact, so scale = 0.5 is bitwise the
    step of the pre-halved gradient with its own clip partials ("exact for power-of-2 ranks")"""
    assert_same_step(scale_run(block, clip, 0.5), scale_run(block, clip, 1.0, gmul=0.5))


@pytest.mark.parametrize('clip', [False, True], ids=['noclip', 'clip'])
@pytest.mark.parametrize('block', [True, False], ids=['blocks', 'flat'])
def test_grad_scale_zero_is_one(block, clip):
    """a zeroed descriptor (the ABI default) means no scaling"""
    one = scale_run(block, clip, 1.0)
    assert_same_step(scale_run(block, clip, 0.0), one)
    assert not torch.equal(one[0].data, one[2]['p'])


@pytest.mark.parametrize('block', [True, False], ids=['blocks', 'flat'])
def test_grad_scale_third_against_float64(block):
    g, opt, g0, sc = scale_run(block, True, 1 / 3)
    p0, gr, m0, v0 = (f64(g0[k]) for k in 'pgmv')
    s = f32(1 / 3)
    coef = clip_coef_ref(float((gr * gr).sum()), 0.5, s)
    assert coef < 0.9, coef       # the clip is active: its norm carries the scale
    p, m, v = adam_ref(p0, gr, m0, v0, sc[0], sc[1], (0.9, 0.999), 1e-8, 1e-4, coef=coef, scale=s)
    for got, ref, what in ((g.data, p, 'p'), (opt.m, m, 'm'), (opt.v, v, 'v')):
        err = (f64(got) - ref).abs()
        tol = 2e-6 * ref.abs() + 1e-7
        print(f'edge-ratio grad_scale 1/3 {what} block={block}: max err/tol {(err / tol).max().item():.3g}')
        assert bool((err <= tol).all()), f'{what}: max err {float(err.max())}'


@pytest.mark.parametrize('scale', [1.0, 1 / 3], ids=['scale1', 'scale3rd'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 130])
def test_clip_coefficient_from_n_partials(n, scale):
    """The clip coefficient min(1, max / (sqrt(sum partial) * scale + 1e-6)) from n partials (64 strided
    lanes, wave_sum), probed through m' = (1 - beta1) (g * scale) * coef (m0 = 0, no weight decay). The sum
    has ceil(n / 64) + 6 roundings, all of one sign, so relative ones, which the square root halves; sqrt,
    the product with the scale, the + 1e-6 and the divide add 4: (ceil(n / 64) + 6 + 4) 2^-24 relative.
    The probe's own three products fit in the half the square root gave back."""
    g, opt = small_group(n, wd=0.0, state=False)
    gen = torch.Generator().manual_seed(n)
    w = torch.rand(n, generator=gen, dtype=torch.float64) ** 3
    if n > 1:
        w[torch.randperm(n, generator=gen)[:n // 3]] = 0.0      # some empty partials
    total = float(f64(g.grad).pow(2).sum())
    part = (w / w.sum() * total).float()
    before, part_dev = g.grad.clone(), part.to(DEV)
    fused_step([opt.segment(0, g.size, opt.step_scalars(), clip=(part_dev, 0.5), pack_map=g.pack_map(),
                            grad_scale=scale)])
    torch.cuda.synchronize()
    s = f32(scale)
    coef = clip_coef_ref(float(part.double().sum()), 0.5, s)
    assert coef < 0.9, coef
    ref = W1 * f64(before) * s * coef
    assert torch.equal(g.grad, before)
    within(f'clip coefficient n={n} scale={scale:.3g}', opt.m, ref, ref.abs(), lane_sum_roundings(n, 64, 6) + 4)


# ---------------------------------------------------------------------------
# 6. A full task list: the flat fallback
# ---------------------------------------------------------------------------
# 16 matrices (the pack map's limit), a vector before, between and after them: 33 tasks as 4x4-block
# work, more than the 32 of the list, so plan_segment hands the last matrix to the flat split
FULL_LAYERS = [(f'w{i}.weight', din, dout, nb) for i, (dout, din, nb) in enumerate(
    [(13, 14, 1), (1, 7, 1), (8, 8, 2), (5, 3, 1), (16, 4, 1), (4, 16, 3), (1, 1, 1), (7, 9, 1), (12, 20, 1),
     (20, 12, 1), (3, 5, 2), (9, 6, 1), (6, 10, 1), (2, 18, 1), (17, 2, 1), (10, 11, 2)])]


def make_full_group(name, seed, transposed=True, grads=True):
    g = FlatGroup(name)
    g.add('lead', (5,))
    for wname, din, dout, nb in FULL_LAYERS:
        g.add(wname, (nb, dout, din) if nb > 1 else (dout, din))
        g.add(wname.replace('weight', 'bias'), (nb, dout) if nb > 1 else (dout,))
    g.allocate(DEV)
    gen = torch.Generator(device='cpu').manual_seed(seed)
    g.data.copy_(torch.randn(g.size, generator=gen))
    if grads:
        g.grad.copy_(torch.randn(g.size, generator=gen) * 0.1)
    else:
        g.grad = None
    g.enable_packing(FULL_LAYERS, transposed=transposed)
    g.ensure_packed()
    return g


def full_segment(seed, block=True):
    g = make_full_group('g', seed)
    t = make_full_group('t', seed + 1, transposed=False, grads=False)
    opt = Adam(g, lr=3e-3, weight_decay=1e-4)
    opt._ensure_state()
    gen = torch.Generator(device='cpu').manual_seed(3)
    opt.m.copy_(torch.randn(g.size, generator=gen) * 0.01)
    opt.v.copy_(torch.rand(g.size, generator=gen) * 0.01)
    g0 = dict(p=g.data.clone(), g=g.grad.clone(), m=opt.m.clone(), v=opt.v.clone(), t=t.data.clone())
    pm = g.pack_map(t)
    if not block:
        pm = pm.clone()
    part = grad_sumsq(g.grad)
    sc = opt.step_scalars()
    seg = opt.segment(0, g.size, sc, clip=(part, 0.5), zero_grad=True, ema=(t.data, 0.01), pack_map=pm)
    return g, t, opt, g0, sc, seg, (pm, part)


def test_full_task_list_falls_back_to_flat_ranges():
    runs = []
    for block in (True, False):
        g, t, opt, g0, sc, seg, keep = full_segment(1, block)
        fused_step([seg])
        torch.cuda.synchronize()
        runs.append((g, t, opt))
    (gb, tb, ob), (gf, tf, of) = runs
    assert torch.equal(gb.data, gf.data) and not torch.equal(gb.data, g0['p'])
    assert torch.equal(ob.m, of.m) and torch.equal(ob.v, of.v)
    assert torch.equal(tb.data, tf.data)
    assert int((gb.grad != 0).sum()) == 0
    for grp in (gb, tb):      # mirrors == a fresh pack of the updated weights
        P, PT = grp.packed.clone(), None if grp.packedT is None else grp.packedT.clone()
        grp.mark_dirty()
        grp._pk_ver = None
        grp.ensure_packed()
        torch.cuda.synchronize()
        assert torch.equal(P, grp.packed), f'{grp.name}: forward mirror'
        if PT is not None:
            assert torch.equal(PT, grp.packedT), f'{grp.name}: transposed mirror'
    p, m, v, t = TO.reference(g0, sc, True, (0, gb.size), True)
    for got, ref, what in ((gb.data, p, 'p'), (ob.m, m, 'm'), (ob.v, v, 'v'), (tb.data, t, 't')):
        err = (got.double().cpu() - ref).abs()
        tol = 2e-6 * ref.abs() + 1e-7
        print(f'edge-ratio full task list {what}: max err/tol {(err / tol).max().item():.3g}')
        assert bool((err <= tol).all()), f'{what}: max err {float(err.max())}'


def test_three_full_segments_are_refused_and_nothing_is_launched():
    segs = [full_segment(10 * k) for k in range(3)]
    arr = (OptimSeg * 3)(*[s[5] for s in segs])
    torch.cuda.synchronize()
    assert _lib.lib().drpo_optim_step(arr, 3, _lib.stream()) != 0
    msg = _lib.lib().drpo_last_error().decode()
    assert msg.startswith('drpo_optim_step: more than 32 tasks'), msg
    torch.cuda.synchronize()
    for g, t, opt, g0, sc, seg, keep in segs:
        assert torch.equal(g.data, g0['p']) and torch.equal(g.grad, g0['g'])
        assert torch.equal(opt.m, g0['m']) and torch.equal(opt.v, g0['v']) and torch.equal(t.data, g0['t'])


def fresh_pack_matches(grp):
    P, PT = grp.packed.clone(), grp.packedT.clone()
    grp.mark_dirty()
    grp._pk_ver = None
    grp.ensure_packed()
    torch.cuda.synchronize()
    return torch.equal(P, grp.packed) and torch.equal(PT, grp.packedT)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_flat_range_that_begins_before_a_matrix(lead):
    """What the full task list first showed (profiles/launch_riders/README.md): a flat range need not begin
    at a multiple of 4, so a thread's 4 elements can begin in the vector before a matrix; the elements
    inside the matrix still reach the mirrors. Here the range is a segment of the flat split beginning
    `lead` elements before b.weight."""
    runs = []
    for block in (True, False):
        g, opt = small_group(5)
        s0 = g.offset('b.weight') - lead
        pm = g.pack_map() if block else g.pack_map().clone()
        start = g.data.clone()
        fused_step([opt.segment(s0, g.size, opt.step_scalars(), zero_grad=True, pack_map=pm)])
        torch.cuda.synchronize()
        assert torch.equal(g.data[:s0], start[:s0]) and not torch.equal(g.view('b.weight'), g.view('b.weight', start))
        assert fresh_pack_matches(g), f'mirrors, block={block}'
        runs.append((g, opt))
    assert torch.equal(runs[0][0].data, runs[1][0].data) and torch.equal(runs[0][1].m, runs[1][1].m)


def test_flat_range_that_crosses_from_one_matrix_into_the_next():
    """two matrices with nothing between them (the first fills its 64-float slot), a segment of the flat
    split that begins one element into the first: a thread's 4 elements leave it and enter the second"""
    layers = [('x.weight', 8, 8, 1), ('y.weight', 12, 5, 1)]
    g = FlatGroup('adj')
    for name, din, dout, nb in layers:
        g.add(name, (dout, din))
    g.allocate(DEV)
    assert g.offset('y.weight') == 64
    gen = torch.Generator().manual_seed(0)
    g.data.copy_(torch.randn(g.size, generator=gen))
    g.grad.copy_(torch.randn(g.size, generator=gen) * 0.1)
    g.enable_packing(layers, transposed=True)
    g.ensure_packed()
    opt = Adam(g, lr=LR)
    start = g.data.clone()
    fused_step([opt.segment(1, g.size, opt.step_scalars(), pack_map=g.pack_map().clone())])
    torch.cuda.synchronize()
    assert torch.equal(g.data[:1], start[:1]) and not torch.equal(g.view('y.weight'), g.view('y.weight', start))
    assert fresh_pack_matches(g)
