"""The MLP kernels at every width class they admit (1..256), against float64.

drpo_pack_weights, drpo_mlp_forward, drpo_mlp_backward (DRPO_UPSTREAM_GOUT) and the generic
jobs of drpo_mlp_forward_multi / drpo_mlp_backward_multi, over a lattice of nets chosen so
that every code path the kernels pick by width runs: tile_dense's unrolled k-step cores
(1, 4, 13, 16 steps, each also at a K other than 200 / 256) and its runtime K loop (2..15
steps), waves owning one and two column blocks, the split-K narrow layers (dout <= 16)
at every k-step count, wide layers whose width is no multiple of 4 (strided save
fallback), the deferred 16-byte saves of the multi launch, and all four activations on
wide and narrow layers, forward and backward. test_lattice_covers_every_width_class (host
only) states the classes and fails when a lattice row that carries one is removed.

Reference: y = act(x W^T + b) and its backward restated in torch float64. The backward is
fed float32 roundings of the float64 forward's saves (ReLU saves hold exact zeros), and
the reference uses the same tensors, so no mask can flip.

Tolerance, per compared tensor: scale = max|ref64|, e32 = the max error of the same
computation by torch on the CPU in float32 against ref64;
    max|got - ref64| <= max(4 * e32, 32 * 2^-24 * scale)
(4x: MFMA k-chunk accumulation order against the CPU's blocked sums; the floor: hardware
exp / rcp of fast_sigmoid and tanhf where e32 happens to be tiny), and every element within
the project's fp32 convention 1e-4 + 1e-4 |ref| (test_gpu_nets.py), the hard ceiling.

Measured on an MI355X, max over all cases of max|got - ref64| / scale and the largest
share of its bound any tensor used (a run with -s prints both per tensor and per op):
    drpo_pack_weights        bit-exact
    drpo_mlp_forward         2.5e-06 (a one-row, one-output tensor; 8.8e-07 otherwise), 0.46 of the bound
    drpo_mlp_forward_multi   5.6e-07, 0.29        drpo_mlp_backward_multi  6.3e-07, 0.33
    drpo_mlp_backward        6.6e-07, 0.35
The 4x margin was not needed. The multi launches' generic jobs, and the split-heads
backward's head dZ, were bit-equal to the single / unsplit launches (printed, not asserted).
"""
import ctypes
import math

import pytest
import torch

from drpo_amd import _abi, _lib
from drpo_amd.mlp_desc import ACT_ID, Net, fill_bwd, fill_fwd

gpu = pytest.mark.gpu

MEASURED = {}    # op -> [max err / scale, max err / bound] of this run (printed at its end)

# (dims, activations): the issue's lattice, with two changes so that the forward products
# alone reach every unrolled core at a K other than 200 / 256 (1 -> 17 -> 255 -> 33: 16
# k-steps at K = 255; 208 -> 250 -> 13: 13 k-steps at K = 208) and swish runs on a narrow
# layer (72 -> 16)
LATTICE = [
    ([14, 256, 256, 1], ['relu', 'relu', None]),          # the project's own shape (control)
    ([23, 64, 64, 4], ['relu', 'relu', None]),
    ([64, 128, 128, 2], ['swish', 'swish', None]),
    ([17, 136, 72, 16], ['tanh', 'relu', 'swish']),
    ([1, 17, 255, 33], ['relu', 'tanh', None]),
    ([53, 200, 208, 7], ['swish', 'swish', None]),
    ([100, 240, 129, 33], ['relu', 'swish', 'tanh']),
    ([256, 32, 16, 256], ['relu', 'relu', None]),
    ([208, 250, 13], ['tanh', None]),
    ([40, 48], [None]),
    ([48, 16, 1], ['tanh', None]),
]
ROWS = [1, 16, 17, 49]    # a one-row tile, a full tile, full + one row, three full + one row


def lattice_layers(lattice):
    """[(kind, K, N, act)] of every product the lattice runs: forward layers (K = din, N =
    dout; narrow = N <= 16, the split-K path) and the backward-data products dY = dZ W
    (K = dout, N = din; always tile_dense)."""
    out = []
    for dims, acts in lattice:
        for l, act in enumerate(acts):
            din, dout = dims[l], dims[l + 1]
            out.append(('narrow' if dout <= 16 else 'wide', din, dout, act))
            out.append(('bwd', dout, din, act))
    return out


def coverage_gaps(lattice):
    """The width classes of the header that no layer of `lattice` reaches."""
    layers = lattice_layers(lattice)
    ks = lambda K: (K + 15) // 16
    gaps = []
    for kind in ('wide', 'bwd'):     # tile_dense: forward wide layers, and backward products
        kn = [(K, N) for k, K, N, _ in layers if k == kind]
        classes = {'1': any(ks(K) == 1 for K, _ in kn), '4': any(ks(K) == 4 for K, _ in kn),
                   '13, K != 200': any(ks(K) == 13 and K != 200 for K, _ in kn),
                   '13, K == 200': any(K == 200 for K, _ in kn),
                   '16, K != 256': any(ks(K) == 16 and K != 256 for K, _ in kn),
                   '16, K == 256': any(K == 256 for K, _ in kn)}
        gaps += [f'{kind}: unrolled k-steps {c}' for c, hit in classes.items() if not hit]
        runtime = {ks(K) for K, _ in kn} - {1, 4, 13, 16}
        if len(runtime) < 5 or 8 not in runtime:
            gaps.append(f'{kind}: runtime K loop step counts {sorted(runtime)} (five, with 8)')
        # a wave owning two column blocks together with the runtime K loop
        if not any((N + 15) // 16 > 8 and ks(K) not in (1, 4, 13, 16) for K, N in kn):
            gaps.append(f'{kind}: two blocks per wave with the runtime K loop')
    narrow = [(K, N) for k, K, N, _ in layers if k == 'narrow']
    for what, hit in (('N == 1', any(N == 1 for _, N in narrow)), ('N in 2..15', any(2 <= N <= 15 for _, N in narrow)),
                      ('N == 16', any(N == 16 for _, N in narrow))):
        if not hit:
            gaps.append(f'narrow: {what}')
    if len({ks(K) for K, _ in narrow}) < 5:
        gaps.append('narrow: five k-step counts')
    wide = [(K, N) for k, K, N, _ in layers if k == 'wide']
    blocks = {(N + 15) // 16 for _, N in wide}
    for want in ({2}, {4}, {8}, {9, 10, 11, 12}, {13}, {15, 16}):
        if not blocks & want:
            gaps.append(f'wide: column blocks {sorted(want)}')
    if not any(N % 4 for _, N in wide):
        gaps.append('wide: N % 4 != 0')
    if not any((K, N) == (256, 256) for K, N in wide):
        gaps.append('wide: 16 k-steps x 16 column blocks (the control, 256 -> 256)')
    if {len(acts) for _, acts in lattice} != {1, 2, 3}:
        gaps.append('nets of 1, 2 and 3 layers')
    for act in ('relu', 'swish', 'tanh', None):     # every layer runs forward and backward
        for kind in ('wide', 'narrow'):
            if not any(k == kind and a == act for k, _, _, a in layers):
                gaps.append(f'{kind}: activation {act}')
    return gaps


def test_lattice_covers_every_width_class():
    assert coverage_gaps(LATTICE) == []
    for i in range(len(LATTICE)):    # every row carries a class of its own
        assert coverage_gaps(LATTICE[:i] + LATTICE[i + 1:]), f'row {i} {LATTICE[i][0]} carries no class'


# ------------------------------------------------------------------------------ reference
def act_f(act, z):
    if act == 'relu':
        return z.clamp_min(0)
    if act == 'swish':
        return z * torch.sigmoid(z)
    if act == 'tanh':
        return torch.tanh(z)
    return z


def act_grad_f(act, y, z):
    """dy/dz from the saves the kernel reads: y for relu / tanh, z for swish (csrc/mlp.hip act_grad)"""
    if act == 'relu':
        return (y > 0).to(y.dtype)
    if act == 'tanh':
        return 1 - y * y
    if act == 'swish':
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    return torch.ones_like(y)


class TNet:
    """A net's weights ([nbatch][dout][din] uniform(+-1/sqrt(din)), fp32, on the CPU) and their
    packed mirrors on the device (member stride drpo_packed_size + gap)."""

    def __init__(self, dims, acts, gen, nbatch=1, gap=0):
        L = _lib.lib()
        self.dims, self.acts, self.nbatch = list(dims), list(acts), nbatch
        self.W, self.b, self.P, self.PT, self.bd, self.strides = [], [], [], [], [], []
        items = []
        for l in range(len(acts)):
            din, dout = dims[l], dims[l + 1]
            k = 1.0 / din ** 0.5
            W = (torch.rand(nbatch, dout, din, generator=gen) * 2 - 1) * k
            b = (torch.rand(nbatch, dout, generator=gen) * 2 - 1) * k
            ps = int(L.drpo_packed_size(din, dout)) + gap
            Wd = W.cuda()
            P = torch.zeros(nbatch, ps, device='cuda')
            PT = torch.zeros(nbatch, ps, device='cuda')
            it = _abi.PackItem()
            it.W, it.P, it.PT, it.din, it.dout, it.nbatch = Wd.data_ptr(), P.data_ptr(), PT.data_ptr(), din, dout, nbatch
            it.wstride, it.pstride, it.ptstride = dout * din, ps, ps
            items.append((it, Wd))
            self.W.append(W)
            self.b.append(b)
            self.P.append(P)
            self.PT.append(PT)
            self.bd.append(b.cuda())
            self.strides.append((ps, dout))
        arr = (_abi.PackItem * len(items))(*[it for it, _ in items])
        _lib.check(L.drpo_pack_weights(arr, len(items), _lib.stream()), 'pack')
        torch.cuda.synchronize()

    def net(self):
        return Net([(self.P[l], self.bd[l], self.dims[l], self.dims[l + 1], ACT_ID[a], self.PT[l])
                    for l, a in enumerate(self.acts)])

    def forward(self, x, dtype):
        """x [nbatch][rows][din] -> ([y_l], [z_l]) in dtype"""
        ys, zs, y = [], [], x.to(dtype)
        for W, b, a in zip(self.W, self.b, self.acts):
            z = torch.bmm(y, W.to(dtype).transpose(1, 2)) + b.to(dtype)[:, None, :]
            y = act_f(a, z)
            ys.append(y)
            zs.append(z)
        return ys, zs

    def backward(self, g, sy, sz, dtype):
        """g [nbatch][rows][dout], saves in fp32 -> ([dz_l], input gradient) in dtype"""
        dzs, g = [None] * len(self.acts), g.to(dtype)
        for l in reversed(range(len(self.acts))):
            dz = g * act_grad_f(self.acts[l], sy[l].to(dtype), sz[l].to(dtype))
            dzs[l] = dz
            g = torch.bmm(dz, self.W[l].to(dtype))
        return dzs, g


def nanbuf(n, off=0):
    """(base, view): n floats at float offset `off` of a NaN-filled buffer with a guard after"""
    base = torch.full((off + n + 260,), float('nan'), device='cuda')
    return base, base[off:off + n]


def guards_ok(base, view):
    off = view.storage_offset()
    return bool(torch.isnan(base[:off]).all() and torch.isnan(base[off + view.numel():]).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(op, what, got, ref64, ref32):
    """The header's bound for one tensor; prints the figures before it asserts."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    assert torch.isfinite(got).all(), f'{op} {what}: not finite'
    scale = float(ref64.abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    err = float((got - ref64).abs().max())
    bound = max(4 * e32, 32 * 2.0 ** -24 * scale)
    m = MEASURED.setdefault(op, [0.0, 0.0])
    if scale > 0:
        m[0] = max(m[0], err / scale)
        m[1] = max(m[1], err / bound)
    print(f'{op} {what}: err {err:.3e} scale {scale:.3e} e32 {e32:.3e} bound {bound:.3e}')
    assert err <= bound, f'{op} {what}: max err {err:.3e} > {bound:.3e} (scale {scale:.3e}, e32 {e32:.3e})'
    assert bool(((got - ref64).abs() <= 1e-4 + 1e-4 * ref64.abs()).all()), f'{op} {what}: past the fp32 ceiling'


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for op, (rel, frac) in sorted(MEASURED.items()):
        print(f'\nMEASURED {op}: max err / scale = {rel:.3e}, max err / bound = {frac:.3f}')


# ------------------------------------------------------------------------------ packer
def packed_ref(W, transposed=False):
    """csrc/pack_layout.hpp's index formula: P[(cb*NKS + s)*256 + 4*l + i] = W[16cb + (l&15)][16s + 4(l>>4) + i]
    (zero outside the matrix); the transposed mirror is the same formula on W^T."""
    if transposed:
        W = W.t()
    dout, din = W.shape
    ncb, nks = (dout + 15) // 16, (din + 15) // 16
    Wp = torch.zeros(16 * ncb, 16 * nks)
    Wp[:dout, :din] = W
    # [cb][l15][s][g][i] -> [cb][s][g][l15][i]: l = 16 g + l15
    return Wp.view(ncb, 16, nks, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()


LAYERS = sorted({(dims[l], dims[l + 1]) for dims, acts in LATTICE for l in range(len(acts))})


@gpu
def test_packed_size_is_the_formula():
    L = _lib.lib()
    for din, dout in LAYERS + [(1, 1), (256, 256), (16, 17), (17, 16)]:
        assert L.drpo_packed_size(din, dout) == math.ceil(din / 16) * math.ceil(dout / 16) * 256


@gpu
@pytest.mark.parametrize('nbatch,gap', [(1, 0), (3, 64)])
def test_pack_weights_bit_for_bit(nbatch, gap):
    """Every lattice layer, 16 items per launch: P and PT against the index formula, zero
    padding included; with nbatch = 3 the member strides exceed drpo_packed_size and the
    gap floats keep their NaN sentinel. Two launches give the same bits."""
    L = _lib.lib()
    gen = torch.Generator().manual_seed(7)
    assert len(LAYERS) > 16
    for first in range(0, len(LAYERS), 16):
        chunk = LAYERS[first:first + 16]
        keep, items = [], []
        for din, dout in chunk:
            W = torch.randn(nbatch, dout, din, generator=gen)
            ps = int(L.drpo_packed_size(din, dout))
            bufs = [nanbuf(nbatch * (ps + gap)) for _ in range(4)]    # P, PT of two launches
            Wd = W.cuda()
            keep.append((W, Wd, ps, bufs))
        outs = []
        for rep in range(2):
            arr = (_abi.PackItem * len(chunk))()
            for k, ((din, dout), (W, Wd, ps, bufs)) in enumerate(zip(chunk, keep)):
                it = arr[k]
                it.W, it.P, it.PT = Wd.data_ptr(), bufs[2 * rep][1].data_ptr(), bufs[2 * rep + 1][1].data_ptr()
                it.din, it.dout, it.nbatch = din, dout, nbatch
                it.wstride, it.pstride, it.ptstride = dout * din, ps + gap, ps + gap
            _lib.check(L.drpo_pack_weights(arr, len(chunk), _lib.stream()), 'pack')
        torch.cuda.synchronize()
        for (din, dout), (W, Wd, ps, bufs) in zip(chunk, keep):
            for tr in (0, 1):
                (base, got), (base2, got2) = bufs[tr], bufs[2 + tr]
                assert same_bits(got, got2), (din, dout, tr, 'two launches differ')
                assert guards_ok(base, got)
                g = got.cpu().view(nbatch, ps + gap)
                for z in range(nbatch):
                    assert same_bits(g[z, :ps], packed_ref(W[z], bool(tr))), (din, dout, z, 'PT' if tr else 'P')
                    assert bool(torch.isnan(g[z, ps:]).all()), (din, dout, z, 'gap written')


# ------------------------------------------------------------------------------ forward
class FwdRun:
    """One forward launch: descriptors, save buffers (NaN guards), results."""

    def __init__(self, tnets, rows, nbatch=1, saves='yz', sy_off=0):
        self.tnets, self.rows, self.nbatch = tnets, rows, nbatch
        self.nets, self.bases = [], []
        for t in tnets:
            n = t.net()
            for l in range(len(t.acts)):
                cnt = nbatch * rows * t.dims[l + 1]
                if 'y' in saves:
                    base, n.sy[l] = nanbuf(cnt, sy_off)
                    self.bases.append((base, n.sy[l]))
                if 'z' in saves:
                    base, n.sz[l] = nanbuf(cnt)
                    self.bases.append((base, n.sz[l]))
            self.nets.append(n)

    def desc(self, srcs, lds=None, trunk=False, split=False, norm=None, sstride=None, save_x=True):
        din0 = sum(c for _, c in srcs)
        self.save_x = None
        if save_x:
            base, self.save_x = nanbuf(self.nbatch * self.rows * din0)
            self.bases.append((base, self.save_x))
        ws = [t.strides for t in self.tnets] if self.nbatch > 1 else None
        d = fill_fwd(self.nets, srcs, self.rows, trunk=trunk, save_x=self.save_x, norm=norm, nbatch=self.nbatch,
                     wstride=ws, sstride=sstride, split_heads=split)
        for k, ld in enumerate(lds or []):
            d.ld[k] = ld
        return d

    def all_saves(self):
        out = [self.save_x] if self.save_x is not None else []
        for n in self.nets:
            out += [t for t in n.sy + n.sz if t is not None]
        return out

    def guards(self):
        return all(guards_ok(b, v) for b, v in self.bases)


def fwd_launch(d):
    _lib.check(_lib.lib().drpo_mlp_forward(ctypes.byref(d), _lib.stream()), 'forward')


def fwd_twice(make):
    """Runs make() -> (FwdRun, descriptor, keep-alive) twice on fresh buffers: the same bits."""
    a = make()
    fwd_launch(a[1])
    b = make()
    fwd_launch(b[1])
    torch.cuda.synchronize()
    for x, y in zip(a[0].all_saves(), b[0].all_saves()):
        assert same_bits(x, y), 'two launches differ'
    assert a[0].guards(), 'a save wrote outside its rows'
    return a[0]


def check_net_saves(op, tag, tnet, net, x64, rows, nbatch):
    """Every layer's sy / sz of one net against the float64 forward from x64 ([nbatch][rows][din])."""
    y64, z64 = tnet.forward(x64, torch.float64)
    y32, z32 = tnet.forward(x64.float(), torch.float32)
    for l in range(len(tnet.acts)):
        if net.sy[l] is not None:
            check(op, f'{tag} sy{l}', net.sy[l], y64[l], y32[l])
        if net.sz[l] is not None:
            check(op, f'{tag} sz{l}', net.sz[l], z64[l], z32[l])
    return y64[-1]


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('li', range(len(LATTICE)))
def test_forward_lattice(li, rows):
    """Every lattice net x row count: the final output (the last layer's sy), every layer's
    sy and sz, save_x; NaN guards after the saved rows; two launches bit-equal."""
    dims, acts = LATTICE[li]
    gen = torch.Generator().manual_seed(100 * li + rows)
    t = TNet(dims, acts, gen)
    x = torch.randn(1, rows, dims[0], generator=gen)
    xd = x.cuda()

    def make():
        r = FwdRun([t], rows)
        return r, r.desc([(xd[0], dims[0]), (None, 0), (None, 0)]), xd
    r = fwd_twice(make)
    assert same_bits(r.save_x.cpu(), x.reshape(-1))
    check_net_saves('forward', f'{dims} rows {rows}', t, r.nets[0], x.double(), rows, 1)


@gpu
def test_forward_unaligned_save_pointer():
    """sy one float past a 16-byte boundary (the strided save fallback), wide N % 4 == 0 layers"""
    dims, acts = LATTICE[2]
    gen = torch.Generator().manual_seed(11)
    t = TNet(dims, acts, gen)
    x = torch.randn(1, 17, dims[0], generator=gen)
    xd = x.cuda()

    def make():
        r = FwdRun([t], 17, sy_off=1)
        assert r.nets[0].sy[0].data_ptr() % 16 == 4
        return r, r.desc([(xd[0], dims[0]), (None, 0), (None, 0)]), xd
    r = fwd_twice(make)
    check_net_saves('forward', 'unaligned sy', t, r.nets[0], x.double(), 17, 1)


@gpu
@pytest.mark.parametrize('rows', [17])
def test_forward_three_strided_sources_with_normaliser(rows):
    """Three concatenated sources that are column views of wider tensors (ld > cols), the
    first normalised by nmean / nstd: 9 + 11 + 3 = 23 input columns."""
    dims, acts = LATTICE[1]
    gen = torch.Generator().manual_seed(12)
    t = TNet(dims, acts, gen)
    wide = [torch.randn(rows, w, generator=gen) for w in (20, 11 + 6, 40)]
    cols, c0 = [9, 11, 3], [5, 6, 37]
    mean, std = torch.randn(9, generator=gen), torch.rand(9, generator=gen) + 0.5
    wd, md, sd = [w.cuda() for w in wide], mean.cuda(), std.cuda()
    views = [wd[k][:, c0[k]:c0[k] + cols[k]] for k in range(3)]

    def make():
        r = FwdRun([t], rows)
        d = r.desc([(views[k], cols[k]) for k in range(3)], lds=[w.shape[1] for w in wide], norm=(md, sd))
        return r, d, (wd, md, sd)
    r = fwd_twice(make)

    def assemble(dt):
        s = [wide[k][:, c0[k]:c0[k] + cols[k]].to(dt) for k in range(3)]
        return torch.cat([(s[0] - mean.to(dt)) / (std.to(dt) + 1e-6), s[1], s[2]], 1)[None]
    x64 = assemble(torch.float64)
    check('forward', 'strided sources save_x', r.save_x, x64, assemble(torch.float32))
    # the layers against the float64 net on the kernel's own (float32) assembled input: the
    # normaliser's rounding is checked above and not amplified into the layer bound
    check_net_saves('forward', 'strided sources', t, r.nets[0], r.save_x.cpu().double().view(1, rows, 23), rows, 1)


@gpu
@pytest.mark.parametrize('shared', [True, False])
def test_forward_ensemble_members(shared):
    """nbatch = 3 with per-member wstride (past drpo_packed_size) / bstride, the input shared
    (sstride = 0) or per member"""
    dims, acts = LATTICE[5]
    rows = 17
    gen = torch.Generator().manual_seed(13)
    t = TNet(dims, acts, gen, nbatch=3, gap=64)
    x = torch.randn(1 if shared else 3, rows, dims[0], generator=gen)
    xd = x.cuda()

    def make():
        r = FwdRun([t], rows, nbatch=3)
        d = r.desc([(xd, dims[0]), (None, 0), (None, 0)], sstride=[0 if shared else rows * dims[0], 0, 0])
        return r, d, xd
    r = fwd_twice(make)
    x3 = x.expand(3, rows, dims[0]).double()
    assert same_bits(r.save_x.cpu(), x3.float().reshape(-1))
    check_net_saves('forward', f'nbatch 3 shared {shared}', t, r.nets[0], x3, rows, 3)


@gpu
@pytest.mark.parametrize('nn', [2, 3])
def test_forward_independent_nets_on_one_input(nn):
    """two / three nets of different shapes on one input (grid.y)"""
    rows, din = 49, 23
    gen = torch.Generator().manual_seed(14 + nn)
    shapes = [LATTICE[1], ([din] + LATTICE[3][0][1:], LATTICE[3][1]), ([din] + LATTICE[6][0][1:], LATTICE[6][1])][:nn]
    ts = [TNet(d, a, gen) for d, a in shapes]
    x = torch.randn(1, rows, din, generator=gen)
    xd = x.cuda()

    def make():
        r = FwdRun(ts, rows)
        return r, r.desc([(xd[0], din), (None, 0), (None, 0)]), xd
    r = fwd_twice(make)
    for j, t in enumerate(ts):
        check_net_saves('forward', f'{nn} nets, net {j}', t, r.nets[j], x.double(), rows, 1)


TRUNK = ([17, 136, 72], ['tanh', 'relu'])
HEADS = [([72, 64, 4], ['relu', None]), ([72, 129, 33], ['swish', 'tanh'])]


def trunk_nets(gen, nheads, nbatch=1):
    return [TNet(*TRUNK, gen, nbatch=nbatch)] + [TNet(*h, gen, nbatch=nbatch) for h in HEADS[:nheads]]


@gpu
@pytest.mark.parametrize('nheads', [1, 2])
def test_forward_trunk_and_heads_split_equals_unsplit(nheads):
    """A 72-wide trunk with one / two heads against float64; split_heads = 1 (one workgroup
    per head, each recomputing the trunk) equals the unsplit launch bit for bit on the
    heads and on the trunk saves."""
    rows = 33
    gen = torch.Generator().manual_seed(20 + nheads)
    ts = trunk_nets(gen, nheads)
    x = torch.randn(1, rows, 17, generator=gen)
    xd = x.cuda()
    runs = {}
    for split in (False, True):
        def make():
            r = FwdRun(ts, rows)
            return r, r.desc([(xd[0], 17), (None, 0), (None, 0)], trunk=True, split=split), xd
        runs[split] = fwd_twice(make)
    r = runs[False]
    t64 = check_net_saves('forward', 'trunk', ts[0], r.nets[0], x.double(), rows, 1)
    for h in range(nheads):
        # heads against float64 from the float64 trunk output: the trunk's error is theirs too
        check_net_saves('forward', f'head {h}', ts[1 + h], r.nets[1 + h], t64, rows, 1)
    for a, b in zip(runs[False].all_saves(), runs[True].all_saves()):
        assert same_bits(a, b), 'split_heads differs from the unsplit launch'


# ------------------------------------------------------------------------------ backward
class BwdCase:
    """A net's float64 forward on random inputs, rounded to the fp32 saves the kernel reads,
    a random output gradient, and dz buffers."""

    def __init__(self, t, rows, gen, x64=None):
        self.t, self.rows = t, rows
        nb = t.nbatch
        if x64 is None:
            x64 = torch.randn(nb, rows, t.dims[0], generator=gen).double()
        y64, z64 = t.forward(x64, torch.float64)
        self.out64 = y64[-1]
        self.sy, self.sz = [y.float() for y in y64], [z.float() for z in z64]
        self.g = torch.randn(nb, rows, t.dims[-1], generator=gen)
        self.gd = self.g.cuda()

    def net(self, dz2=False):
        n = self.t.net()
        n.sy, n.sz = [y.cuda() for y in self.sy], [z.cuda() for z in self.sz]
        self.bases = []
        for l in range(len(self.t.acts)):
            base, n.dz[l] = nanbuf(self.t.nbatch * self.rows * self.t.dims[l + 1])
            self.bases.append((base, n.dz[l]))
            if dz2:
                base, n.dz2[l] = nanbuf(self.t.nbatch * self.rows * self.t.dims[l + 1])
                self.bases.append((base, n.dz2[l]))
        return n

    def ref(self, g, dtype):
        return self.t.backward(g, self.sy, self.sz, dtype)


def bwd_launch(d):
    _lib.check(_lib.lib().drpo_mlp_backward(ctypes.byref(d), _lib.stream()), 'backward')


def check_dz(op, tag, case, net, g):
    d64, gx64 = case.ref(g.double(), torch.float64)
    d32, gx32 = case.ref(g.float(), torch.float32)
    for l in range(len(case.t.acts)):
        check(op, f'{tag} dz{l}', net.dz[l], d64[l], d32[l])
    return gx64, gx32


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('li', range(len(LATTICE)))
def test_backward_lattice(li, rows):
    """Every lattice net x row count: every layer's dz, and dx for a column window
    [col0, col0 + cols) inside the input (all of it when din = 1) accumulated into a non-zero
    buffer with NaN guards around it; two launches bit-equal."""
    dims, acts = LATTICE[li]
    gen = torch.Generator().manual_seed(200 * li + rows)
    t = TNet(dims, acts, gen)
    case = BwdCase(t, rows, gen)
    din = dims[0]
    col0, cols = (0, 1) if din == 1 else (max(1, din // 3), max(1, din // 2))
    assert col0 + cols <= din and (din == 1 or (col0 > 0 and cols < din))
    dx0 = torch.randn(rows, cols, generator=gen)
    outs = []
    for rep in range(2):
        net = case.net()
        base, dx = nanbuf(rows * cols)
        dx.copy_(dx0.reshape(-1))
        d = fill_bwd([net], [case.gd], rows, dx={0: (dx, col0, cols, True)})
        bwd_launch(d)
        outs.append((net, base, dx, case.bases))
    torch.cuda.synchronize()
    (net, base, dx, bases), (net2, _, dx2, _) = outs
    assert same_bits(dx, dx2) and all(same_bits(a, b) for a, b in zip(net.dz, net2.dz)), 'two launches differ'
    assert guards_ok(base, dx) and all(guards_ok(b, v) for b, v in bases)
    gx64, gx32 = check_dz('backward', f'{dims} rows {rows}', case, net, case.g)
    check('backward', f'{dims} rows {rows} dx', dx, dx0.double() + gx64[0][:, col0:col0 + cols],
          dx0 + gx32[0][:, col0:col0 + cols])


@gpu
def test_backward_job_without_dx_writes_none():
    """Two nets on grid.y, only the second asks for its input gradient (overwriting): the
    first stops after dz0, and the second's dx is written inside its guards only."""
    rows = 17
    gen = torch.Generator().manual_seed(31)
    ts = [TNet(*LATTICE[1], gen), TNet(*LATTICE[3], gen)]
    cases = [BwdCase(t, rows, gen) for t in ts]
    nets = [c.net() for c in cases]
    base, dx = nanbuf(rows * 17)
    d = fill_bwd(nets, [c.gd for c in cases], rows, dx={1: (dx, 0, 17, False)})
    assert d.net[0].dx is None and d.net[1].dx
    bwd_launch(d)
    torch.cuda.synchronize()
    assert guards_ok(base, dx) and all(guards_ok(b, v) for c in cases for b, v in c.bases)
    check_dz('backward', 'no-dx net', cases[0], nets[0], cases[0].g)
    gx64, gx32 = check_dz('backward', 'dx net', cases[1], nets[1], cases[1].g)
    check('backward', 'dx (overwrite)', dx, gx64[0], gx32[0])


@gpu
def test_backward_ensemble_members():
    """nbatch = 3, member strides past drpo_packed_size"""
    dims, acts = LATTICE[5]
    rows = 17
    gen = torch.Generator().manual_seed(32)
    t = TNet(dims, acts, gen, nbatch=3, gap=64)
    case = BwdCase(t, rows, gen)
    net = case.net()
    base, dx = nanbuf(3 * rows * dims[0])
    d = fill_bwd([net], [case.gd], rows, dx={0: (dx, 0, dims[0], False)}, nbatch=3, wstride=[t.strides])
    bwd_launch(d)
    torch.cuda.synchronize()
    assert guards_ok(base, dx) and all(guards_ok(b, v) for b, v in case.bases)
    gx64, gx32 = check_dz('backward', 'nbatch 3', case, net, case.g)
    check('backward', 'nbatch 3 dx', dx, gx64, gx32)


@gpu
def test_backward_trunk_two_heads_and_split():
    """A 72-wide trunk with two heads (the generic one-head-at-a-time path): the trunk's output
    gradient is the sum of the heads' input gradients; every dz and the trunk's dx against
    float64. split_heads: dz + dz2 of every trunk layer equals the unsplit dz within the bound
    (the reference: the float64 dz)."""
    rows = 33
    gen = torch.Generator().manual_seed(33)
    ts = trunk_nets(gen, 2)
    trunk = BwdCase(ts[0], rows, gen)
    heads = [BwdCase(t, rows, gen, x64=trunk.out64) for t in ts[1:]]
    hg64 = [h.ref(h.g.double(), torch.float64)[1] for h in heads]
    hg32 = [h.ref(h.g.float(), torch.float32)[1] for h in heads]
    g64, g32 = hg64[0] + hg64[1], hg32[0] + hg32[1]
    t64, tx64 = trunk.ref(g64, torch.float64)
    t32, tx32 = trunk.ref(g32, torch.float32)

    nets = [trunk.net()] + [h.net() for h in heads]
    base, dx = nanbuf(rows * 17)
    d = fill_bwd(nets, [None] + [h.gd for h in heads], rows, trunk=True, dx={0: (dx, 0, 17, False)})
    bwd_launch(d)
    torch.cuda.synchronize()
    assert guards_ok(base, dx)
    for j, h in enumerate(heads):
        check_dz('backward', f'trunk job head {j}', h, nets[1 + j], h.g)
    for l in range(2):
        check('backward', f'trunk dz{l}', nets[0].dz[l], t64[l], t32[l])
    check('backward', 'trunk dx', dx, tx64, tx32)

    snets = [trunk.net(dz2=True)] + [h.net() for h in heads]
    d = fill_bwd(snets, [None] + [h.gd for h in heads], rows, trunk=True, split_heads=True)
    bwd_launch(d)
    torch.cuda.synchronize()
    assert all(guards_ok(b, v) for b, v in trunk.bases)
    for j, h in enumerate(heads):
        check_dz('backward', f'split job head {j}', h, snets[1 + j], h.g)
        print(f'split head {j} dz bit-equal to the unsplit launch:',
              all(same_bits(a, b) for a, b in zip(snets[1 + j].dz, nets[1 + j].dz)))
    for l in range(2):
        check('backward', f'split trunk dz{l} + dz2', snets[0].dz[l] + snets[0].dz2[l], t64[l], t32[l])


# ------------------------------------------------------------------------------ multi-job launches
MULTI = [(2, 17, 'y', 0), (3, 1, 'yz', 0), (6, 49, 'y', 1), (8, 16, 'y', 0)]   # (lattice row, rows, saves, sy offset)


def _dev_copy(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


@gpu
def test_forward_multi_generic_jobs():
    """Four generic jobs of different lattice shapes and row counts in one
    drpo_mlp_forward_multi launch (no pair / head / pre / post / ccb): sy-only saves (the
    deferred 16-byte save where the width allows, the strided fallback for widths that are
    no multiple of 4 and for a pointer one float off), sy + sz saves, save_x; against float64,
    twice for bits. Whether they are bit-equal to the single launches is printed."""
    L = _lib.lib()
    gen = torch.Generator().manual_seed(41)
    ts = [TNet(*LATTICE[li], gen) for li, _, _, _ in MULTI]
    xs = [torch.randn(1, rows, t.dims[0], generator=gen) for t, (_, rows, _, _) in zip(ts, MULTI)]
    xd = [x.cuda() for x in xs]

    def runs():
        rs = [FwdRun([t], rows, saves=sv, sy_off=off) for t, (_, rows, sv, off) in zip(ts, MULTI)]
        return rs, [r.desc([(x[0], t.dims[0]), (None, 0), (None, 0)]) for r, x, t in zip(rs, xd, ts)]
    both = []
    for rep in range(2):
        rs, ds = runs()
        arr = (_abi.MlpFwd * len(ds))(*ds)
        dev = _dev_copy(arr)
        _lib.check(L.drpo_mlp_forward_multi(arr, dev.data_ptr(), len(ds), 0, 0, _lib.stream()), 'forward_multi')
        both.append((rs, dev))
    singles, ds = runs()
    for d in ds:
        fwd_launch(d)
    torch.cuda.synchronize()
    for j, (r, r2, s, t, x) in enumerate(zip(both[0][0], both[1][0], singles, ts, xs)):
        assert all(same_bits(a, b) for a, b in zip(r.all_saves(), r2.all_saves())), 'two launches differ'
        assert r.guards()
        assert same_bits(r.save_x.cpu(), x.reshape(-1))
        check_net_saves('forward_multi', f'job {j} {t.dims} rows {r.rows}', t, r.nets[0], x.double(), r.rows, 1)
        print(f'forward_multi job {j}: bit-equal to drpo_mlp_forward:',
              all(same_bits(a, b) for a, b in zip(r.all_saves(), s.all_saves())))


@gpu
def test_backward_multi_generic_jobs():
    """The same four shapes as generic DRPO_UPSTREAM_GOUT jobs of one drpo_mlp_backward_multi
    launch: every dz and the whole input gradient against float64, twice for bits."""
    L = _lib.lib()
    gen = torch.Generator().manual_seed(42)
    ts = [TNet(*LATTICE[li], gen) for li, _, _, _ in MULTI]
    cases = [BwdCase(t, rows, gen) for t, (_, rows, _, _) in zip(ts, MULTI)]

    def jobs():
        out = []
        for c in cases:
            net = c.net()
            base, dx = nanbuf(c.rows * c.t.dims[0])
            d = fill_bwd([net], [c.gd], c.rows, dx={0: (dx, 0, c.t.dims[0], False)})
            out.append((net, base, dx, c.bases, d))
        return out
    both = []
    for rep in range(2):
        js = jobs()
        arr = (_abi.MlpBwd * len(js))(*[j[4] for j in js])
        dev = _dev_copy(arr)
        _lib.check(L.drpo_mlp_backward_multi(arr, dev.data_ptr(), len(js), _lib.stream()), 'backward_multi')
        both.append((js, dev))
    singles = jobs()
    for j in singles:
        bwd_launch(j[4])
    torch.cuda.synchronize()
    for k, (a, b, s, c) in enumerate(zip(both[0][0], both[1][0], singles, cases)):
        assert same_bits(a[2], b[2]) and all(same_bits(x, y) for x, y in zip(a[0].dz, b[0].dz)), 'two launches differ'
        assert guards_ok(a[1], a[2]) and all(guards_ok(bb, v) for bb, v in a[3])
        gx64, gx32 = check_dz('backward_multi', f'job {k} {c.t.dims} rows {c.rows}', c, a[0], c.g)
        check('backward_multi', f'job {k} dx', a[2], gx64, gx32)
        print(f'backward_multi job {k}: bit-equal to drpo_mlp_backward:',
              same_bits(a[2], s[2]) and all(same_bits(x, y) for x, y in zip(a[0].dz, s[0].dz)))
