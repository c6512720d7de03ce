"""Launch descriptors of the MLP kernels (csrc/mlp.hip, csrc/wgrad.hip), built from flat
parameter groups: a Net is one MLP as the kernels see it, fill_fwd / fill_bwd /
wgrad_items turn Nets and tensors into drpo_mlp_fwd_t / drpo_mlp_bwd_t /
drpo_wgrad_item_t, the with_* helpers attach the multi-job launch's fused pieces
(policy heads, chains), and the FLOP counters + LaunchProfiler time the launches. Used
by the SAC engine (sac_step.py), the ensemble engine (ensemble_engine.py) and the
stand-alone forwards of ops.py."""
import ctypes
from collections import namedtuple

import torch

from . import _lib
from ._abi import MlpBwd, MlpFwd, MlpNet, WgradItem

# the ids below mirror include/drpo_hip.h (DRPO_ACT_*, DRPO_UPSTREAM_*, DRPO_HEAD_*): they are
# read at import, before the library loads, and tests/test_path_queries.py pins each to
# drpo_abi_const
ACT_ID = {None: 0, 'identity': 0, 'relu': 1, 'swish': 2, 'tanh': 3}

# one layer as the kernels see it: packed forward mirror, bias, widths, activation id,
# packed transposed mirror (None for a group that is never trained)
Layer = namedtuple('Layer', 'P b din dout act PT')


def spec_layers(group, prefix, spec, buf=None):
    """[Layer] for an MLPSpec stored under prefix in a flat group:
    P / PT are the layer's packed forward / transposed weight mirrors (group.pview),
    b the bias view (of ``buf`` if given, else the group data)."""
    out = []
    n = spec.n_layers
    for i in range(n):
        act = spec.act if i < n - 1 else spec.out_act
        key = f'{prefix}{2 * i}.weight'
        b = group.view(f'{prefix}{2 * i}.bias', buf)
        PT = group.pview(key, True)
        out.append(Layer(group.pview(key)[0], b, spec.dims[i], spec.dims[i + 1], ACT_ID[act],
                         None if PT is None else PT[0]))
    return out


class Net:
    """One MLP as seen by the kernels: layers + (optional) per-layer save buffers."""

    def __init__(self, layers, grad_layers=None):
        self.layers = [Layer(*x) for x in layers]
        self.grad_layers = grad_layers    # [(gW, gb)] or None
        self.sy = [None] * len(layers)
        self.sz = [None] * len(layers)
        self.dz = [None] * len(layers)
        self.dz2 = [None] * len(layers)   # split-heads trunk: the second head's dZ share

    @property
    def dout(self):
        return self.layers[-1].dout

    @property
    def din(self):
        return self.layers[0].din

    def desc(self):
        """This net as a drpo_mlp_net_t: what the path queries of include/drpo_hip.h take."""
        d = MlpNet()
        fill_net(d, self)
        return d


def _p(t):
    return 0 if t is None else t.data_ptr()


def fill_net(dst, net, wstride=None):
    """drpo_mlp_net_t of a Net (layers, save buffers, per-member strides)."""
    dst.nl = len(net.layers)
    for l, (L, lay) in enumerate(zip(dst.L, net.layers)):   # (a net of more than 3 layers: the library refuses nl)
        L.W, L.b, L.din, L.dout, L.act = lay.P.data_ptr(), lay.b.data_ptr(), lay.din, lay.dout, lay.act
        L.sy, L.sz = _p(net.sy[l]), _p(net.sz[l])
        L.wstride, L.bstride = (0, 0) if wstride is None else wstride[l]


def fill_fwd(nets, srcs, rows, trunk=False, save_x=None, norm=None, nbatch=1, wstride=None, sstride=None,
             split_heads=False, pair=False):
    """pair: the two nets run by one workgroup (multi-job launches; drpo_mlp_fwd_t.pair)."""
    d = MlpFwd()
    for k, (t, cols) in enumerate(srcs):
        d.src[k] = _p(t)
        d.cols[k] = cols
        d.ld[k] = t.shape[-1] if t is not None and t.dim() > 1 else 1
        d.sstride[k] = 0 if sstride is None else sstride[k]
    d.nmean, d.nstd = (norm[0].data_ptr(), norm[1].data_ptr()) if norm is not None else (0, 0)
    d.save_x = _p(save_x)
    for j, net in enumerate(nets):
        fill_net(d.net[j], net, None if wstride is None else wstride[j])
    d.nnets, d.trunk, d.rows, d.nbatch = len(nets), int(trunk), rows, nbatch
    d.split_heads = int(split_heads)
    d.pair = int(pair)
    return d


def pairable(a, b):
    """Two nets one pair job can run: what drpo_mlp_forward_multi admits with pair = 1."""
    return bool(_lib.lib().drpo_mlp_pair_ok(ctypes.byref(a.desc()), ctypes.byref(b.desc())))


def with_pre(d, policy, mode, A, eps, site, logp=None):
    """Chain (drpo_mlp_fwd_t.pre): the policy runs first in the same workgroup on the
    src[0] columns; its sampled action (mode 1 sample / 2 rsample) is the job's src[1]
    block, straight from LDS."""
    fill_net(d.pre, policy)
    h = d.pre_head
    h.mode, h.A, h.eps, h.site, h.logp = mode, A, _p(eps), site, _p(logp)
    return d


def with_post(d, net, post_x=None):
    """Post chain (drpo_mlp_fwd_t.post): `net` (the MLPMultiplier) runs after the job's
    constraint bound (ccb_out), in the same workgroup, on [src[0] columns, bound]; its
    layers save as any net's, post_x saves the assembled input (the multiplier update's
    weight-gradient Y)."""
    fill_net(d.post, net)
    d.post_x = _p(post_x)
    return d


# drpo_mlp_bwd_t.upstream (include/drpo_hip.h DRPO_UPSTREAM_*)
UPSTREAM_GOUT, UPSTREAM_CRITIC, UPSTREAM_CERT, UPSTREAM_ENS = 0, 1, 2, 3
UPSTREAM_ACTOR_CC, UPSTREAM_SAFE_CC, UPSTREAM_NEG_MEAN, UPSTREAM_SQUASH, UPSTREAM_SQUASH_SAFE = 4, 5, 6, 7, 8


def fill_bwd(nets, gouts, rows, trunk=False, dx=None, nbatch=1, wstride=None, split_heads=False, upstream=0):
    """nets[0] trunk when trunk=True (gouts[0] ignored); dx: {net_index: (tensor, col0, cols, accumulate)};
    split_heads: one workgroup per head, the second head's trunk dZ share into nets[0].dz2;
    upstream: output gradients from the gout arrays, or formed in-kernel from the
    launch's critic head (UPSTREAM_CRITIC / UPSTREAM_CERT)."""
    d = MlpBwd()
    d.upstream = upstream
    for j, net in enumerate(nets):
        d.net[j].nl = len(net.layers)
        for l, (W, b, din, dout, act, WT) in enumerate(net.layers):
            L = d.net[j].L[l]
            assert WT is not None, 'backward needs the transposed weight mirror (trained group)'
            L.W, L.din, L.dout, L.act = WT.data_ptr(), din, dout, act
            L.sy, L.sz, L.dz = _p(net.sy[l]), _p(net.sz[l]), _p(net.dz[l])
            L.dz2 = _p(net.dz2[l]) if getattr(net, 'dz2', None) else 0
            L.wstride = 0 if wstride is None else wstride[j][l][0]
        d.net[j].gout = _p(gouts[j])
        if dx and j in dx:
            t, c0, nc, accum = dx[j]
            d.net[j].dx, d.net[j].dx_col0, d.net[j].dx_cols, d.net[j].dx_accumulate = t.data_ptr(), c0, nc, int(accum)
    d.nnets, d.trunk, d.rows, d.nbatch = len(nets), int(trunk), rows, nbatch
    d.split_heads = int(split_heads)
    return d


HEAD_SAMPLE, HEAD_RSAMPLE, HEAD_MEAN = 1, 2, 3


def with_head(d, mode, A, eps, site, a=None, logp=None, u=None, e=None, amean=None, second=False):
    """Attach a fused squashed-Gaussian head (drpo_policy_head_t) to a forward descriptor
    (second: the head of a pair job's net 1, drpo_mlp_fwd_t.head2)."""
    h = d.head2 if second else d.head
    h.mode, h.A, h.eps, h.site = mode, A, _p(eps), site
    h.a, h.logp, h.u, h.e, h.amean = _p(a), _p(logp), _p(u), _p(e), _p(amean)
    return d


def wgrad_items(entries, rows, sq=None):
    """entries: [(net, inputs_per_layer[, segment])] -> (ctypes array of WgradItem, count,
    {segment: partial slots used}). With sq = {segment: device tensor}, every item of a
    segment writes the sums of squares of its finished gradient tiles into consecutive
    slots of that segment's tensor (the clip partials of drpo_optim_step)."""
    L = _lib.lib()
    items, used = [], {}
    units = [(ent[0], ent[1], ent[2] if len(ent) > 2 else None, l) for ent in entries for l in range(len(ent[0].layers))]
    for net, ins, seg, l in units:
        W, b, din, dout, act, WT = net.layers[l]
        gW, gb = net.grad_layers[l]
        it = WgradItem()
        it.dz, it.y, it.gW, it.gb = net.dz[l].data_ptr(), ins[l].data_ptr(), gW.data_ptr(), gb.data_ptr()
        it.dout, it.din, it.rows, it.nbatch = dout, din, rows, 1
        if sq is not None and seg is not None:
            it.sq, it.sq_off = sq[seg].data_ptr(), used.get(seg, 0)
            used[seg] = it.sq_off + L.drpo_mlp_wgrad_tiles(ctypes.byref(it))
            assert used[seg] <= sq[seg].numel(), 'clip partial buffer too small'
        items.append(it)
    arr = (WgradItem * len(items))(*items)
    return arr, len(items), used


def wgrad_workspace(cache, key, arr, n, dev):
    """Zero-initialised workspace of one drpo_mlp_wgrad call site (the launches keep it
    zeroed), cached by key and grown when the plan needs more."""
    need = int(_lib.lib().drpo_mlp_wgrad_workspace_size(arr, n))
    t = cache.get(key)
    if t is None or t.numel() < need:
        t = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)
        cache[key] = t
    return t


def fwd_flops(d):
    """Algorithmic FLOPs of one drpo_mlp_forward launch (2 * rows * sum din*dout), the
    chained policy and the post-chain multiplier of a multi-job launch included."""
    macs = 0
    for n in [d.net[j] for j in range(d.nnets)] + [d.pre, d.post]:
        for l in range(n.nl):
            macs += n.L[l].din * n.L[l].dout
    return 2 * d.rows * d.nbatch * macs


def bwd_flops(d):
    """Backward-data products (dY = dZ W) of one drpo_mlp_backward launch; layer 0's
    product runs only for trunk-mode heads (it feeds the trunk) or when the input
    gradient is requested."""
    macs = 0
    for j in range(d.nnets):
        n = d.net[j]
        for l in range(n.nl):
            if l > 0 or n.dx or (d.trunk and j > 0):
                macs += n.L[l].din * n.L[l].dout
    return 2 * d.rows * d.nbatch * macs


def wgrad_flops(arr, n):
    # (arr, n[, used]) descriptors
    return sum(2 * arr[i].rows * arr[i].nbatch * arr[i].dout * (arr[i].din + 1) for i in range(n))


class LaunchProfiler:
    """HIP events around every MLP launch of the engine (stream-ordered on the launch
    stream), with each launch's algorithmic FLOPs; summarise() after a synchronize."""

    def __init__(self):
        self.recs = []

    def begin(self, kind, key, flops):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        return (kind, key, flops, e0, e1)

    def end(self, rec):
        rec[4].record()
        self.recs.append(rec)

    def summarise(self):
        out = {}
        for kind, key, flops, e0, e1 in self.recs:
            ms = e0.elapsed_time(e1)
            for k in (kind, f'{kind}:{key}'):
                o = out.setdefault(k, {'launches': 0, 'ms': 0.0, 'flop': 0.0})
                o['launches'] += 1
                o['ms'] += ms
                o['flop'] += flops
        for o in out.values():
            o['avg_ms'] = o['ms'] / o['launches']
            o['tflops'] = o['flop'] / (o['ms'] * 1e-3) / 1e12 if o['ms'] > 0 else 0.0
        self.recs = []
        return out
