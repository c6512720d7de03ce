"""Dynamics-ensemble engine: BatchedGaussianEnsemble's forward / sample / loss / fit
(src/dynamics.py:112-253) as HIP launches over the model's flat HBM group.

Every pass is one fused MLP launch over all members (grid.z = member; weights are
the [E, out, in] BatchedLinear layout, so member z reads W + z*out*in) around
small row-wise kernels (csrc/ensemble.hip):

  forward     drpo_mlp_forward (trunk + diff head + log-var head in one launch)
              -> drpo_ens_head (residual mean, soft log-var clamp [, sample])
  spread      forward of every member on shared rows (member stride 0) -> drpo_ens_spread
              (the statistics across members; no per-member output)
  holdout     drpo_ens_gather_steps -> forward with member stride 0 (the reference's
              .repeat(E, 1) without the copy) -> drpo_ens_loss (no grads)
  fit         drpo_ens_gather_steps once per chunk of steps (every step's minibatch in one
              launch), then per step FitPlan.compute and FitPlan.apply

FitPlan.compute -- forward, NLL and backward-data, leaving the NLL's block partials and
their reduction as data (drpo_ens_reduce_t). The first variant whose condition holds:
  1. drpo_ens_fit_fb, all three in one launch: the shapes that entry point admits (the
     reference default: two trunk layers, one hidden layer per head, width 200 | 256,
     S+A <= 64, S+1 <= 16), a split-heads grid, and the switches fit_fb_enabled and
     split_bwd on.
  2. drpo_mlp_forward + drpo_mlp_backward_ens, the NLL gradients formed inside the
     backward launch: the shapes that entry point admits (heads [H -> 200|256 -> S+1 <= 64]).
  (Which shapes: drpo_ens_fit_paths, the library's own conditions.)
     One workgroup per (row tile, head) at split-heads grids with split_bwd on, else
     one per row tile with the heads paired.
  3. drpo_mlp_forward + drpo_ens_loss (deferred reduction) + drpo_mlp_backward: any other
     model, e.g. head_hidden_layers = 2.
FitPlan.apply -- weight gradients of all 6 layers x members, the NLL reduction, Adam:
  1. 'fused': drpo_mlp_wgrad_adam, one launch (Adam and the mirror refresh by the
     workgroup that finishes a tile, the reduction and the bounds' Adam step by one extra
     workgroup): compute variant 1 or 2, one process, switch fused_adam on.
  2. 'fused-shard': the same launch for the rank's members of a member-sharded fit, while
     a side stream runs drpo_ens_loss_reduce, the all-reduce of the shared log-var bounds'
     gradients (the step's one collective) and their drpo_optim_step; the next step's
     backward waits for it (after its forward has been launched).
  3. 'separate': drpo_mlp_wgrad_reduce (the reduction as its last workgroup), the
     gradients' all-reduce under batch data parallelism, drpo_optim_step over the group:
     compute variant 3, batch data parallelism, or fused_adam off.

The per-step ``loss.item()`` of the reference is deferred: losses land in a device
array that is read once at the end of fit (same returned list of floats).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .optim import OPT_MAXSEG, fused_step
from .rng import DeviceNoise
from .mlp_desc import ACT_ID, UPSTREAM_ENS, UPSTREAM_GOUT, Layer, Net, fill_bwd, fill_fwd, wgrad_workspace
from ._abi import EnsReduce, EnsSpread, EnsUpstream, WgradItem


# Forward: one workgroup per (row tile, head) when the plain grid (16-row tiles x
# members) would leave most of the 256 CUs idle. The trunk is recomputed per head
# (1.33x the forward FLOPs) but each workgroup's serial chain shortens from 5 to 3
# dense layers: fit forward 28.8 -> 20.1 us at E=7, b=256 (csrc/mlp.hip, split_heads).
# Backward: the same split -- one workgroup per (row tile, head), each forming the NLL
# gradient of its head in-kernel (drpo_mlp_backward_ens) and backing its share through
# the trunk -- leaves the trunk dZ as two terms (dz + dz2). The weight-gradient launch
# takes both terms as ONE item (drpo_wgrad_item_t.dz2: the product (dz + dz2)^T y reads
# the trunk activations once; round 2's two-item form re-read them and was rejected).
SPLIT_HEADS_MAX_TILES = 256


def split_heads(n, Z):
    return (n + 15) // 16 * Z <= SPLIT_HEADS_MAX_TILES


def _addr(t):
    return 0 if t is None else t.data_ptr()


class EnsembleEngine:
    def __init__(self, model):
        self.m = model
        # single-process fit: Adam (+ mirror refresh) fused into the weight-gradient launch
        # (drpo_mlp_wgrad_adam; bitwise the same step as drpo_optim_step). The three switches
        # below are the production dispatch; the bitwise / parity tests turn them off to run
        # the launches each fusion replaced as their reference
        # (tests/test_gpu_configs.py::test_fit_fused_adam_matches_separate_step,
        # ::test_fit_fb_matches_two_launches).
        self.fused_adam = True
        self.split_bwd = True     # one backward workgroup per (row tile, head); False: paired heads
        self.fit_fb_enabled = True   # forward + NLL + backward-data as one launch (drpo_ens_fit_fb)
        self.ws = {}
        self.wg_ws = {}
        self._zsel = {}
        self.noise = None
        self.dev = model.group.data.device
        from .distributed import GradReducer
        self.dp = GradReducer()

    # ------------------------------------------------------------------ helpers
    def buf(self, name, *shape, dtype=torch.float32):
        t = self.ws.get(name)
        if t is None or t.numel() < int(np.prod(shape)) or t.dtype != dtype:
            t = torch.empty(int(np.prod(shape)), dtype=dtype, device=self.dev)
            self.ws[name] = t
        return t[:int(np.prod(shape))].view(*shape)

    def _noise(self, noise):
        if noise is not None:
            return noise
        if self.noise is None:
            self.noise = DeviceNoise(torch.initial_seed() ^ 0x5EED0DE1)
        return self.noise

    def _specs(self):
        m = self.m
        return (('trunk.', m.trunk_spec), ('diff_head.', m.diff_spec), ('log_var_head.', m.logvar_spec))

    def _nets(self, member=None, grads=False, z0=0):
        """Kernel views of the trunk and both heads: one member (``member``) or the
        members from ``z0`` on (member stride; z0 > 0 for an ensemble shard)."""
        g = self.m.group
        nets, strides = [], []
        for prefix, spec in self._specs():
            lay, gl, st = [], [], []
            for i in range(spec.n_layers):
                key = f'{prefix}{2 * i}.weight'
                W, WT, b = g.pview(key), g.pview(key, True), g.view(f'{prefix}{2 * i}.bias')
                din, dout = spec.dims[i], spec.dims[i + 1]
                act = spec.act if i < spec.n_layers - 1 else spec.out_act
                if member is not None:
                    W, WT, b = W[member], WT[member], b[member]
                    st.append((0, 0))
                else:          # packed-mirror stride per member, bias stride
                    st.append((W.shape[1], dout))
                    W, WT, b = W[z0], WT[z0], b[z0]
                lay.append(Layer(W, b, din, dout, ACT_ID[act], WT))
                if grads:
                    gl.append((g.view(f'{prefix}{2 * i}.weight', g.grad)[z0],
                               g.view(f'{prefix}{2 * i}.bias', g.grad)[z0]))
            nets.append(Net(lay, gl if grads else None))
            strides.append(st)
        return nets, strides

    # ------------------------------------------------------------------ forward
    def _forward_desc(self, s, a, n, Z, s_zs, a_zs, member=None, tag='f', save=False, z0=0):
        """Descriptor of one fused ensemble forward (raw head outputs D, LVR [Z*n, S+1]);
        with save=True the activations needed for the backward pass are kept."""
        m = self.m
        S, A = m.state_dim, m.action_dim
        S1 = S + 1
        m.group.ensure_packed()
        nets, strides = self._nets(member, grads=save, z0=z0)
        rows = Z * n
        split = split_heads(n, Z)
        if save:
            for j, net in enumerate(nets):
                for l, (_, _, din, dout, act, _) in enumerate(net.layers):
                    net.sy[l] = self.buf(f'{tag}.sy{j}{l}', rows, dout)
                    net.sz[l] = self.buf(f'{tag}.sz{j}{l}', rows, dout) if act == ACT_ID['swish'] else None
                    net.dz[l] = self.buf(f'{tag}.dz{j}{l}', rows, dout)
                    if j == 0 and self.split_bwd and split:
                        net.dz2[l] = self.buf(f'{tag}.dzb{l}', rows, dout)
            save_x = self.buf(f'{tag}.x', rows, S + A)
        else:
            save_x = None
            nets[1].sy[-1] = self.buf(f'{tag}.D', rows, S1)
            nets[2].sy[-1] = self.buf(f'{tag}.L', rows, S1)
        norm = m.state_normalizer
        d = fill_fwd(nets, [(s, S), (a, A)], n, trunk=True, save_x=save_x, norm=(norm.mean, norm.std), nbatch=Z,
                     wstride=strides, sstride=[s_zs, a_zs, 0], split_heads=split)
        return d, nets, strides, save_x

    def _forward(self, s, a, n, Z, s_zs, a_zs, member=None, tag='f', save=False, z0=0):
        d, nets, strides, save_x = self._forward_desc(s, a, n, Z, s_zs, a_zs, member, tag, save, z0)
        _lib.check(_lib.lib().drpo_mlp_forward(ctypes.byref(d), _lib.stream()), 'ensemble forward')
        return nets, strides, save_x

    def _head(self, D, LVR, s, s_zs, n, Zo, zsel=None, eps=None, noise=None, outputs=('mu', 'lv'), out=None):
        m, L = self.m, _lib.lib()
        S = m.state_dim
        if out is not None:
            outputs = ()
        out = {} if out is None else out
        if 'mu' in outputs:
            out['mu'] = torch.empty(Zo, n, S + 1, device=self.dev)
            out['lv'] = torch.empty(Zo, n, S + 1, device=self.dev)
        if 's2' in outputs:
            out['s2'] = torch.empty(Zo, n, S, device=self.dev)
            out['r'] = torch.empty(Zo, n, device=self.dev)
        seed, ctr = (0, 0)
        if 's2' in out and eps is None:
            nz = self._noise(noise)
            seed, ctr = nz.seed, nz.next()
        zs = None
        if zsel is not None:
            zs = torch.tensor(list(zsel), dtype=torch.int32, device=self.dev)
        _lib.check(L.drpo_ens_head(_lib.ptr(D), _lib.ptr(LVR), _lib.ptr(s), s_zs, n, S, Zo, _lib.ptr(m.min_log_var),
                                   _lib.ptr(m.max_log_var), _lib.ptr(zs), _lib.ptr(eps), seed, ctr,
                                   _lib.ptr(out.get('mu')), _lib.ptr(out.get('lv')), _lib.ptr(out.get('s2')),
                                   _lib.ptr(out.get('r')), _lib.stream()), 'ens_head')
        return out

    def _prep(self, *xs):
        _lib.require_device(self.m.group.data, *xs)
        return [x.contiguous().float() for x in xs]

    def forward1(self, s, a, index):
        s, a = self._prep(s, a)
        n = s.shape[0]
        nets, _, _ = self._forward(s, a, n, 1, 0, 0, member=int(index))
        o = self._head(nets[1].sy[-1], nets[2].sy[-1], s, 0, n, 1)
        return o['mu'][0], o['lv'][0]

    def forward_all(self, s, a):
        """s [E|1, n, S], a [E|1, n, A] (leading 1 = shared rows, stride 0)."""
        s, a = self._prep(s, a)
        E = self.m.ensemble_size
        n = s.shape[-2]
        s_zs = 0 if s.dim() == 2 or s.shape[0] == 1 else n * s.shape[-1]
        a_zs = 0 if a.dim() == 2 or a.shape[0] == 1 else n * a.shape[-1]
        if s.dim() == 3:
            assert s.shape[0] in (1, E) and a.shape[0] in (1, E)
        nets, _, _ = self._forward(s, a, n, E, s_zs, a_zs)
        o = self._head(nets[1].sy[-1], nets[2].sy[-1], s, s_zs, n, E)
        return o['mu'], o['lv']

    def sample(self, s, a, index, noise, eps=None, out=None, tag='f'):
        """sample (src/dynamics.py:198-203) for member ``index``. eps: recorded draws
        (device tensor) or None (tape / Philox); out: optional {'s2', 'r'} buffers."""
        s, a = self._prep(s, a)
        n, S = s.shape
        if eps is None and noise is not None and noise.parity:
            eps = torch.from_numpy(noise.randn_like((n, S + 1))).to(self.dev)
        nets, _, _ = self._forward(s, a, n, 1, 0, 0, member=int(index), tag=tag)
        o = self._head(nets[1].sy[-1], nets[2].sy[-1], s, 0, n, 1, eps=eps, noise=noise, outputs=('s2',), out=out)
        return o['s2'].reshape(n, S), o['r'].reshape(n)

    def elite_samples(self, s, a, elites, noise):
        s, a = self._prep(s, a)
        n, S = s.shape
        E = self.m.ensemble_size
        eps = None
        if noise is not None and noise.parity:
            eps = torch.from_numpy(noise.randn_like((len(elites), n, S + 1))).to(self.dev)
        nets, _, _ = self._forward(s, a, n, E, 0, 0)
        o = self._head(nets[1].sy[-1], nets[2].sy[-1], s, 0, n, len(elites), zsel=elites, eps=eps, noise=noise,
                       outputs=('s2',))
        return o['s2'], o['r']

    # rows per forward + reduction of spread(): bounds the [E, rows, S+1] head-output workspace
    spread_chunk_rows = 65536

    def spread(self, s, a, members, scale, outputs=None):
        """BatchedGaussianEnsemble.disagreement: per chunk of rows one all-member forward on
        shared rows (as elite_samples) and drpo_ens_spread over its raw head outputs. Rows are
        independent, so the chunk size does not change a bit of the result. scale None: the
        model's normalised state units. What the reduction alone needs (outputs, member list,
        weights) is made after the first forward is under way, not in front of it.
        outputs: the names of EnsembleSpread.TENSORS to compute (None: all); the others stay None."""
        from .ops import EnsembleSpread
        outputs = EnsembleSpread.TENSORS if outputs is None else tuple(outputs)
        if not outputs or set(outputs) - set(EnsembleSpread.TENSORS):
            raise ValueError(f'spread: outputs {outputs!r} (one or more of {EnsembleSpread.TENSORS})')
        m = self.m
        S, A, E = m.state_dim, m.action_dim, m.ensemble_size
        s, a = self._prep(s.reshape(-1, S), a.reshape(-1, A))
        n, S1 = len(s), S + 1
        if n == 0:
            empty = {k: s.new_empty(*((0, S1) if i < 3 else (0,))) if k in outputs else None
                     for i, k in enumerate(EnsembleSpread.TENSORS)}
            return EnsembleSpread(list(members), **empty)
        out = EnsembleSpread(list(members), *[None] * 6)
        d = EnsSpread()
        d.S, d.Z, d.M = S, E, len(out.members)
        d.minlv, d.maxlv = m.min_log_var.data_ptr(), m.max_log_var.data_ptr()
        chunk = max(1, int(self.spread_chunk_rows))
        for r0 in range(0, n, chunk):
            c = min(chunk, n - r0)
            nets, _, _ = self._forward(s[r0:r0 + c], a[r0:r0 + c], c, E, 0, 0)
            if r0 == 0:
                for i, k in enumerate(EnsembleSpread.TENSORS):
                    if k in outputs:
                        setattr(out, k, torch.empty(*((n, S1) if i < 3 else (n,)), device=self.dev))
                zsel = self._zsel.get(tuple(out.members))       # device copies of the member lists seen
                if zsel is None:
                    zsel = self._zsel[tuple(out.members)] = torch.tensor(out.members, dtype=torch.int32,
                                                                         device=self.dev)
                if scale is None:
                    norm = m.state_normalizer
                    scale = torch.nn.functional.pad(1.0 / (norm.std + norm.epsilon), (0, 1))
                scale = scale.to(self.dev).contiguous().float()
                d.zsel, d.scale = zsel.data_ptr(), scale.data_ptr()
            d.D, d.LVR, d.s, d.n = nets[1].sy[-1].data_ptr(), nets[2].sy[-1].data_ptr(), s[r0:].data_ptr(), c
            for k in outputs:
                setattr(d, k, getattr(out, k)[r0:].data_ptr())
            _lib.check(_lib.lib().drpo_ens_spread(ctypes.byref(d), _lib.stream()), 'ens_spread')
        return out

    # ------------------------------------------------------------------ loss / grads
    def _loss_ws(self, tag, b, Z):
        """Partial-sum workspace of drpo_ens_loss."""
        nb = int(_lib.lib().drpo_ens_loss_workspace_size(b, self.m.state_dim, Z))
        key = f'{tag}.lossws'
        t = self.ws.get(key)
        if t is None or t.numel() < nb:
            t = torch.zeros(nb, dtype=torch.uint8, device=self.dev)
            self.ws[key] = t
        return t

    def _loss_descs(self, nets, s, s_zs, t, t_zs, b, Z, grads, gscale=None, loss_out=None, tag='f', bound=True):
        """The NLL's two descriptors over a forward's head outputs: (up, red_in, mse, gD, gL).
        up: what drpo_ens_loss, drpo_mlp_backward_ens and drpo_ens_fit_fb read; red_in: where
        the reduction puts the per-member NLL, the loss and (grads) the bounds' gradients."""
        m = self.m
        S = m.state_dim
        g = m.group
        mse = self.buf(f'{tag}.mse', Z)
        gD = gL = None
        up, red_in = EnsUpstream(), EnsReduce()
        up.D, up.LVR = nets[1].sy[-1].data_ptr(), nets[2].sy[-1].data_ptr()
        up.s, up.s_zstride, up.t, up.t_zstride = s.data_ptr(), s_zs, t.data_ptr(), t_zs
        up.b, up.S, up.Z = b, S, Z
        up.minlv, up.maxlv = m.min_log_var.data_ptr(), m.max_log_var.data_ptr()
        up.gscale = _addr(gscale)
        up.part = self._loss_ws(tag, b, Z).data_ptr()
        red_in.weight = float(m.log_var_bound_weight) if bound else 0.0
        red_in.mse, red_in.loss = mse.data_ptr(), _addr(loss_out)
        if grads:
            gD, gL = self.buf(f'{tag}.gD', Z * b, S + 1), self.buf(f'{tag}.gL', Z * b, S + 1)
            red_in.gmin = g.view('min_log_var', g.grad).data_ptr()
            red_in.gmax = g.view('max_log_var', g.grad).data_ptr()
        return up, red_in, mse, gD, gL

    def _loss(self, nets, s, s_zs, t, t_zs, b, Z, grads, gscale=None, loss_out=None, tag='f', bound=True):
        up, red_in, mse, gD, gL = self._loss_descs(nets, s, s_zs, t, t_zs, b, Z, grads, gscale, loss_out, tag, bound)
        _lib.check(_lib.lib().drpo_ens_loss(ctypes.byref(up), ctypes.byref(red_in), _lib.ptr(gD), _lib.ptr(gL), None,
                                            _lib.stream()), 'ens_loss')
        return mse, gD, gL

    def _backward_descs(self, nets, strides, save_x, gD, gL, b, Z):
        """Backward-data descriptor and the weight-gradient items: (desc, [(items, n)]).
        Split heads (EnsembleEngine.split_bwd) leave the trunk dZ as two terms, which the trunk
        layers' items carry as dz + dz2."""
        split = nets[0].dz2[0] is not None
        d = fill_bwd(nets, [None, gD, gL], b, trunk=True, nbatch=Z, wstride=strides, split_heads=split)
        items = []
        trunk_out = nets[0].sy[-1]
        for j, net in enumerate(nets):
            ins = [save_x if j == 0 else trunk_out] + [net.sy[l] for l in range(len(net.layers) - 1)]
            for l, (W, bb, din, dout, act, _) in enumerate(net.layers):
                gW, gb = net.grad_layers[l]
                it = WgradItem()
                it.dz, it.y, it.gW, it.gb = net.dz[l].data_ptr(), ins[l].data_ptr(), gW.data_ptr(), gb.data_ptr()
                it.dz2 = 0 if net.dz2[l] is None else net.dz2[l].data_ptr()
                it.dout, it.din, it.rows, it.nbatch = dout, din, b, Z
                it.zstride, it.ystride, it.gwstride, it.gbstride = b * dout, b * din, dout * din, dout
                items.append(it)
        return d, [((WgradItem * len(items))(*items), len(items))]

    def _wgrad_ws(self, key, arr, n):
        """Per-call-site weight-gradient workspace (sized once per descriptor array)."""
        c = self.wg_ws.get(key)
        if c is not None and c[0] is arr:
            return c[1]
        ws = wgrad_workspace(self.ws, f'{key}.wgws', arr, n, self.dev)
        self.wg_ws[key] = (arr, ws)
        return ws

    def _wgrad(self, key, launches, red=None, stream=None):
        L = _lib.lib()
        stream = _lib.stream() if stream is None else stream
        for k, (arr, n) in enumerate(launches):
            ws = self._wgrad_ws(f'{key}{k}', arr, n)
            if k == 0 and red is not None:
                _lib.check(L.drpo_mlp_wgrad_reduce(arr, n, ctypes.byref(red), ws.data_ptr(), ws.numel(), stream),
                           'ensemble wgrad')
            else:
                _lib.check(L.drpo_mlp_wgrad(arr, n, ws.data_ptr(), ws.numel(), stream), 'ensemble wgrad')

    def _backward(self, nets, strides, save_x, gD, gL, b, Z):
        L = _lib.lib()
        d, launches = self._backward_descs(nets, strides, save_x, gD, gL, b, Z)
        _lib.check(L.drpo_mlp_backward(ctypes.byref(d), _lib.stream()), 'ensemble backward')
        self._wgrad('cl', launches)

    def compute_loss_value(self, s, a, t, with_grads=False, gscale=None):
        """compute_loss on explicit rows (truncated to a multiple of E); returns a 0-d device
        loss, optionally accumulating the gradients into the group's grad."""
        s, a, t = self._prep(s, a, t)
        E = self.m.ensemble_size
        n = len(t) - len(t) % E
        b = n // E
        assert b >= 1, f'compute_loss needs at least {E} rows'
        S, A = self.m.state_dim, self.m.action_dim
        s, a, t = s[:n], a[:n], t[:n]
        loss = torch.empty((), device=self.dev)
        nets, strides, save_x = self._forward(s, a, b, E, b * S, b * A, tag='cl', save=True)
        mse, gD, gL = self._loss(nets, s, b * S, t, b * (S + 1), b, E, with_grads, gscale=gscale, loss_out=loss,
                                 tag='cl')
        if with_grads:
            self._backward(nets, strides, save_x, gD, gL, b, E)
        return loss

    # ------------------------------------------------------------------ fit
    def _gather(self, rb, rows, out, steps=1, idx=None, ctr=0, seed=0, device_ptr=False):
        """Replay rows -> out = (states, actions, targets [s', r]) for `steps` minibatches of
        `rows` rows in one launch: chronological indices idx (a tensor or an address, step k's
        at idx[k*rows ..]) or, without, Philox randint with counters ctr + k. device_ptr: read
        the buffer's fill pointer on the device when it keeps no host copy (a fit inside a
        captured or asynchronous collection); otherwise the host value."""
        m = self.m
        ptr_dev = rb._pointer if device_ptr and rb._host_ptr is None else None
        ptr_host = rb.pointer if not device_ptr else (rb._host_ptr or 0)
        idx = _lib.ptr(idx) if torch.is_tensor(idx) else idx
        _lib.check(_lib.lib().drpo_ens_gather_steps(
            _lib.ptr(rb._states), _lib.ptr(rb._actions), _lib.ptr(rb._next_states), _lib.ptr(rb._rewards), ptr_host,
            _lib.ptr(ptr_dev), rb.capacity, rows, steps, idx, seed, ctr, m.state_dim, m.action_dim, _lib.ptr(out[0]),
            _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream()), 'ens_gather')

    def _side_stream(self):
        """The member-sharded fit's side stream and its two fence-free library events
        (csrc/core.hip), created once per engine: (torch stream, ev_bwd, ev_done)."""
        if getattr(self, '_side', None) is None:
            evs = []
            for _ in range(2):
                e = ctypes.c_void_p()
                _lib.check(_lib.lib().drpo_event_create(ctypes.byref(e)), 'event_create')
                evs.append(e)
            self._side = (torch.cuda.Stream(device=self.dev), evs[0], evs[1])
        return self._side

    def fit_plan(self, steps=1, sh=None):
        """The FitPlan of a fit(steps=) call over the members of shard ``sh`` (None: all), with
        its gathered-minibatch workspace: .fused / .fb / .path say which launches it runs."""
        m = self.m
        S, A = m.state_dim, m.action_dim
        rows = (sh.count if sh is not None else m.ensemble_size) * m.batch_size
        # The minibatches of a chunk of steps are gathered in ONE launch (the replay is
        # not written during the fit); the step's descriptors are pointed at its slice.
        # Chunks of <= 64 MB of gathered rows.
        chunk = max(1, min(steps, (64 << 20) // (4 * (2 * S + A + 1) * max(rows, 1))))
        mb = (self.buf('fit.s_all', chunk * rows, S), self.buf('fit.a_all', chunk * rows, A),
              self.buf('fit.t_all', chunk * rows, S + 1))
        return FitPlan(self, sh, mb, torch.empty(max(steps, 1), device=self.dev), chunk)

    def fit(self, buffer, steps, noise=None):
        """fit(steps=) (src/dynamics.py:155-183). Under data parallelism the members are
        sharded over the ranks (distributed.MemberShard) unless dp_mode='batch', in which
        case every rank fits all members on its own draw and the gradients are averaged."""
        from .distributed import member_sharding
        m = self.m
        nz = self._noise(noise)
        rb = getattr(buffer, '_module', buffer)
        _lib.require_device(m.group.data, rb._states)
        n = len(rb)
        S, A = m.state_dim, m.action_dim
        S1 = S + 1
        sh = member_sharding(m)
        # Normalizer over the chronological states (physical rows [0, n) hold the same set)
        m.state_normalizer.fit(rb._states[:n])
        if sh is not None:       # one normalizer for the whole ensemble (rank 0's replay)
            sh.broadcast_(m.state_normalizer.mean, m.state_normalizer.std)
        elif self.dp.active:     # batch DP: replicas must normalise alike too
            self.dp.broadcast_(m.state_normalizer.mean, m.state_normalizer.std)
        E, b = m.ensemble_size, m.batch_size
        z0, Z = (sh.z0, sh.count) if sh is not None else (0, E)
        rows = Z * b
        m.group.grad.zero_()
        plan = self.fit_plan(steps, sh)
        mb, losses, chunk = plan.mb, plan.losses, plan.chunk
        self.fit_fb, self.fit_path = plan.fb, plan.path    # (tests, probes)
        # parity mode: the reference's randint over all E*b rows, this shard's slice
        idx_all = None
        if nz.parity and steps > 0:
            draws = [np.asarray(nz.randint(n, E * b))[z0 * b:z0 * b + rows] for _ in range(steps)]
            idx_all = torch.from_numpy(np.ascontiguousarray(np.stack(draws), dtype=np.int64)).to(self.dev)
        for i in range(steps):
            k = i % chunk
            if k == 0:
                nc = min(chunk, steps - i)
                if idx_all is not None:
                    idx, ctr = ctypes.c_void_p(idx_all.data_ptr() + 8 * rows * i), 0
                else:   # the counters the per-step draws would take: ctr, ctr + 1, ...
                    idx, ctr = None, nz.next()
                    for _ in range(nc - 1):
                        nz.next()
                self._gather(rb, rows, mb, steps=nc, idx=idx, ctr=ctr, seed=nz.seed, device_ptr=True)
            plan.compute(i, k)
            plan.apply(i)
        plan.finish()
        # holdout: the same rows for every member (src/dynamics.py:175-183)
        hb = m.holdout_size
        assert hb == b, 'reference asserts holdout_size == batch_size (src/dynamics.py:177)'
        ho = (self.buf('ho.s', hb, S), self.buf('ho.a', hb, A), self.buf('ho.t', hb, S1))
        idx = torch.from_numpy(np.ascontiguousarray(nz.randint(n, hb))).to(self.dev) if nz.parity else None
        self._gather(rb, hb, ho, idx=idx, ctr=0 if nz.parity else nz.next(), seed=nz.seed, device_ptr=True)
        if sh is not None:
            sh.broadcast_(*ho)
        nets, _, _ = self._forward(ho[0], ho[1], hb, Z, 0, 0, tag='ho', z0=z0)
        mse, _, _ = self._loss(nets, ho[0], 0, ho[2], 0, hb, Z, False, tag='ho')
        if sh is None:
            self.dp.mean_(mse)       # identical elites on every rank
        else:
            mse = sh.merge_members(mse, torch.zeros(E, device=self.dev))
            sh.sum_(losses)          # per-step loss = sum of the shards' member terms
            self._gather_members(sh)
        mse_h = mse.tolist()
        m.holdout_losses = mse_h
        m._elite_inds = [int(i) for i in np.argsort(np.asarray(mse_h, np.float32), kind='stable')[:m.num_elites]]
        return [float(x) for x in losses[:steps].tolist()]

    def _shard_ranges(self, z0, Z):
        """Flat-group element ranges of members [z0, z0+Z) of every layer, plus the
        shared log-var bounds (the Adam segments of a member shard)."""
        g, out = self.m.group, []
        for prefix, spec in self._specs():
            for i in range(spec.n_layers):
                for key in (f'{prefix}{2 * i}.weight', f'{prefix}{2 * i}.bias'):
                    off, shape = g.entries[key]
                    per = int(np.prod(shape[1:]))
                    out.append((off + z0 * per, off + (z0 + Z) * per))
        S1 = self.m.state_dim + 1
        out.append((g.offset('min_log_var'), g.offset('max_log_var') + S1))
        return out

    def _gather_members(self, sh):
        """Every member's weights on every rank after a sharded fit."""
        g = self.m.group
        for prefix, spec in self._specs():
            for i in range(spec.n_layers):
                for key in (f'{prefix}{2 * i}.weight', f'{prefix}{2 * i}.bias'):
                    sh.gather_members_(g.view(key))
        g.mark_dirty()

    def fit_epochs(self, buffer, epochs, max_grad_norm=None, post_epoch_callback=None, post_step_callback=None,
                   progress_bar=False, verbose=False):
        """fit(epochs=) == epochal_training over E*epochs epochs of randperm minibatches of
        E*batch_size rows (src/dynamics.py:185-190, src/train.py:58-100). randperm uses the
        CPU generator like the reference; the minibatch rows are gathered on the device."""
        from .optim import grad_sumsq
        m = self.m
        rb = getattr(buffer, '_module', buffer)
        _lib.require_device(m.group.data, rb._states)
        n = len(rb)
        S, A = m.state_dim, m.action_dim
        m.state_normalizer.fit(rb._states[:n])
        # the same data-parallel contract as fit(steps=): one normalizer (rank 0's) on
        # every replica, gradients sum-reduced with the 1/G in the optimizer
        self.dp.broadcast_(m.state_normalizer.mean, m.state_normalizer.std)
        E, tb = m.ensemble_size, m.total_batch_size
        n_batches = -(-n // tb)
        losses = []
        for epoch in range(E * epochs):
            perm = torch.randperm(n).to(self.dev)
            ep = torch.empty(n_batches, device=self.dev)
            for bi in range(n_batches):
                idx = perm[bi * tb:min(n, (bi + 1) * tb)]
                cnt = len(idx)
                xs, xa, xt = self.buf('ep.s', cnt, S), self.buf('ep.a', cnt, A), self.buf('ep.t', cnt, S + 1)
                self._gather(rb, cnt, (xs, xa, xt), idx=idx)
                m.group.grad.zero_()
                ep_i = ep[bi:bi + 1].view(())
                loss = self.compute_loss_value(xs, xa, xt, with_grads=True)
                ep_i.copy_(loss)
                self.dp.sum_(m.group.grad)
                # Adam (clipped on the reduced gradient's norm when asked) with the DP 1/G
                # applied to the gradient and its norm inside the step
                clip = None
                if max_grad_norm is not None:
                    clip = (grad_sumsq(m.group.grad), max_grad_norm)
                sc = m.optimizer.step_scalars()
                fused_step([m.optimizer.segment(0, m.group.size, sc, clip=clip, pack_map=m.group.pack_map(),
                                                grad_scale=self.dp.scale)])
                if post_step_callback is not None:
                    post_step_callback(epoch, bi, n_batches)
            losses.append(float(np.mean(ep.tolist())))
            if post_epoch_callback is not None:
                post_epoch_callback(epoch)
        return losses


class FitPlan:
    """One fit(steps=) call's step, built once: the descriptors point at fixed workspaces, and
    per step only the minibatch slice (fd.src, up.s, up.t), the loss slot (red_in.loss) and
    Adam's bias-corrected step sizes change. compute(i, k) and apply(i) issue step i's
    launches in order; which of their three variants run is decided here (the header of
    this file says when)."""

    def __init__(self, eng, sh, mb, losses, chunk):
        from ._abi import OptimSeg, WgradAdam
        m, g = eng.m, eng.m.group
        S, A, b = m.state_dim, m.action_dim, m.batch_size
        z0, Z = (sh.z0, sh.count) if sh is not None else (0, m.ensemble_size)
        self.eng, self.sh, self.mb, self.rows = eng, sh, mb, Z * b
        self.losses, self.chunk = losses, chunk
        self.loss_base = losses.data_ptr()
        self.fd, nets, strides, save_x = eng._forward_desc(mb[0], mb[1], b, Z, b * S, b * A, tag='fit', save=True,
                                                           z0=z0)
        self.up, self.red_in, _, gD, gL = eng._loss_descs(nets, mb[0], b * S, mb[2], b * (S + 1), b, Z, True,
                                                          tag='fit', bound=sh is None or sh.rank == 0)
        self.red = EnsReduce()
        self.gD, self.gL = _lib.ptr(gD), _lib.ptr(gL)
        self.bd, wl = eng._backward_descs(nets, strides, save_x, gD, gL, b, Z)
        self.refs = [ctypes.byref(x) for x in (self.fd, self.bd, self.up, self.red_in, self.red)]
        self.L, self.stream = _lib.lib(), _lib.stream()
        # compute: the NLL in the backward launch needs the shapes drpo_mlp_backward_ens takes
        # (bit 0), the one-launch step also a split-heads grid and the shapes of drpo_ens_fit_fb
        # (bit 1)
        paths = self.L.drpo_ens_fit_paths(*self.refs[:3])
        self.fused = bool(paths & 1)
        self.bd.upstream = UPSTREAM_ENS if self.fused else UPSTREAM_GOUT
        self.fb = eng.fit_fb_enabled and self.fused and bool(self.bd.split_heads) and bool(paths & 2)
        # apply: Adam in the weight-gradient launch needs the fused NLL, no clip and no exchange
        # of the member gradients (a member shard and batch DP exclude each other:
        # member_sharding() is None under dp_mode='batch')
        assert sh is None or getattr(m, 'dp_mode', 'auto') != 'batch'
        fuse = eng.fused_adam and self.fused and len(wl) == 1 and not (sh is None and eng.dp.active)
        self.path = 'separate' if not fuse else ('fused' if sh is None else 'fused-shard')
        self.wl = wl
        if fuse:
            opt = m.optimizer
            opt._ensure_state()
            pm = g.pack_map()
            ad = self.ad = WgradAdam()
            ad.g, ad.p, ad.m, ad.v = g.grad.data_ptr(), g.data.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr()
            ad.beta1, ad.beta2 = opt.betas
            ad.eps, ad.weight_decay = opt.eps, opt.weight_decay
            ad.map, ad.map_host = pm.data_ptr(), ctypes.addressof(pm.host)
            self.wws = eng._wgrad_ws('fit0', *wl[0])
        if sh is None:   # batch DP: the gradient is sum-reduced, the optimizer applies 1/G
            segs = [m.optimizer.segment(0, g.size, (0.0, 1.0), zero_grad=True, pack_map=g.pack_map(),
                                        grad_scale=eng.dp.scale)]
        else:            # the shard's members and the shared log-var bounds
            lo, hi = g.offset('min_log_var'), g.offset('max_log_var') + S + 1
            self.bounds_grad = g.grad[lo:hi]
            pmap = g.pack_map()
            segs = [m.optimizer.segment(a, c, (0.0, 1.0), zero_grad=True, pack_map=pmap)
                    for a, c in eng._shard_ranges(z0, Z)]
            if fuse:
                self.bseg = (OptimSeg * 1)(m.optimizer.segment(lo, hi, (0.0, 1.0), zero_grad=True))
                self.side, self.ev_bwd, self.ev_done = eng._side_stream()
                self.side_s = ctypes.c_void_p(self.side.cuda_stream)
        chunks = [segs[k:k + OPT_MAXSEG] for k in range(0, len(segs), OPT_MAXSEG)]
        self.seg_arr = [(OptimSeg * len(c))(*c) for c in chunks]
        self.pending = False    # fused-shard: the previous step's bounds update is in flight

    def compute(self, i, k):
        """Step i on minibatch k of the gathered chunk: forward, NLL and backward-data, with
        the NLL partials and self.red (their reduction, as data) left for apply()."""
        L, stream = self.L, self.stream
        fd, bd, up, red_in, red = self.refs
        S, A = self.up.S, self.eng.m.action_dim
        cs, ca, ct = self.mb
        self.fd.src[0], self.fd.src[1] = cs.data_ptr() + 4 * k * self.rows * S, ca.data_ptr() + 4 * k * self.rows * A
        self.up.s, self.up.t = self.fd.src[0], ct.data_ptr() + 4 * k * self.rows * (S + 1)
        self.red_in.loss = self.loss_base + 4 * i
        if not self.fb:
            _lib.check(L.drpo_mlp_forward(fd, stream), 'ensemble forward')
        if self.pending:     # the previous step's bounds are stepped (the backward reads them)
            _lib.check(L.drpo_stream_wait_event(stream, self.ev_done), 'stream_wait_event')
        if self.fb:
            _lib.check(L.drpo_ens_fit_fb(fd, bd, up, red_in, red, stream), 'ensemble fit fwd+bwd')
        elif self.fused:
            _lib.check(L.drpo_mlp_backward_ens(bd, up, red_in, red, stream), 'ensemble backward')
        else:
            _lib.check(L.drpo_ens_loss(up, red_in, self.gD, self.gL, red, stream), 'ens_loss')
            _lib.check(L.drpo_mlp_backward(bd, stream), 'ensemble backward')

    def apply(self, i):
        """Step i's weight gradients, the NLL reduction and the Adam step."""
        L, stream = self.L, self.stream
        eng, m, sh = self.eng, self.eng.m, self.sh
        lr_bc1, bc2 = m.optimizer.step_scalars()
        if self.path == 'separate':
            # the loss reduction rides as the last workgroup of the wgrad launch
            eng._wgrad('fit', self.wl, self.red, stream)
            if sh is None:
                eng.dp.sum_(m.group.grad)
            else:
                sh.sum_(self.bounds_grad)      # shared log-var bounds: the sum over all members
            # Adam + grad zeroing + packed-mirror refresh in one launch
            for arr in self.seg_arr:
                for k in range(len(arr)):
                    arr[k].lr_over_bc1, arr[k].bc2_sqrt = lr_bc1, bc2
                _lib.check(L.drpo_optim_step(arr, len(arr), stream), 'optim_step')
            return
        (warr, wn), wws, ad = self.wl[0], self.wws, self.ad
        ad.lr_over_bc1, ad.bc2_sqrt = lr_bc1, bc2
        if self.path == 'fused':
            # weight gradients + the NLL reduction + Adam + mirror refresh: one launch
            _lib.check(L.drpo_mlp_wgrad_adam(warr, wn, self.refs[4], ctypes.byref(ad), wws.data_ptr(),
                                             wws.numel(), stream), 'ensemble wgrad + adam')
            return
        # Member shard: only the shared log-var bounds' 2(S+1) gradients leave
        # the step. Their reduction runs as its own one-block launch on the side stream as soon
        # as the backward has written the NLL partials; the side stream then sum-all-reduces
        # them (the step's ONE collective) and steps the bounds, overlapped with the members'
        # fused weight-gradient + Adam launch on the main stream.
        side_s = self.side_s
        _lib.check(L.drpo_event_record(self.ev_bwd, stream), 'event_record')
        _lib.check(L.drpo_stream_wait_event(side_s, self.ev_bwd), 'stream_wait_event')
        _lib.check(L.drpo_ens_loss_reduce(ctypes.byref(self.red), side_s), 'ens_loss_reduce')
        with torch.cuda.stream(self.side):      # the collective on the side stream
            sh.sum_(self.bounds_grad)
        self.bseg[0].lr_over_bc1, self.bseg[0].bc2_sqrt = lr_bc1, bc2
        _lib.check(L.drpo_optim_step(self.bseg, 1, side_s), 'optim_step (log-var bounds)')
        _lib.check(L.drpo_event_record(self.ev_done, side_s), 'event_record')
        self.pending = True
        _lib.check(L.drpo_mlp_wgrad_adam(warr, wn, None, ctypes.byref(ad), wws.data_ptr(), wws.numel(), stream),
                   'ensemble wgrad + adam (member shard)')

    def finish(self):
        """The main stream waits for the last step's bounds update (member shard)."""
        if self.pending:
            _lib.check(self.L.drpo_stream_wait_event(self.stream, self.ev_done), 'stream_wait_event')
            self.pending = False


class EnsembleLoss(torch.autograd.Function):
    """compute_loss as a differentiable 0-d tensor for external training loops
    (src/train.py:58-69 epochal_training: loss.backward(); optimizer.step()).
    backward() re-runs the fused forward with gradients (scaled by the incoming
    grad) and accumulates into the flat group's grad (= every parameter's .grad)."""

    @staticmethod
    def forward(ctx, anchor, engine, s, a, t):
        ctx.engine, ctx.rows = engine, (s, a, t)
        return engine.compute_loss_value(s, a, t, with_grads=False)

    @staticmethod
    def backward(ctx, g):
        s, a, t = ctx.rows
        ctx.engine.compute_loss_value(s, a, t, with_grads=True, gscale=g.detach().contiguous().float())
        return None, None, None, None, None
