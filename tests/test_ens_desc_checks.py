"""Host-side checks of the model fit's two NLL descriptors, drpo_ens_upstream_t and
drpo_ens_reduce_t (csrc/ens_nll.hpp: ens_upstream_check, ens_reduce_check), no GPU: every
call here is refused before any launch, and the message names the entry point that refused.
Pointers are dummies the host never dereferences."""
import ctypes

import pytest

from drpo_amd import _abi, _lib
from drpo_amd.mlp_desc import ACT_ID

P = 0x1000          # a non-null pointer value (never dereferenced)
EINVAL = 1
SWISH, NONE = ACT_ID['swish'], ACT_ID[None]


def _err():
    return _lib.lib().drpo_last_error().decode()


def _up(S=12, Z=7, b=256):
    u = _abi.EnsUpstream()
    u.D = u.LVR = u.s = u.t = u.minlv = u.maxlv = u.part = P
    u.s_zstride, u.t_zstride, u.b, u.S, u.Z = b * S, b * (S + 1), b, S, Z
    return u


def _red(S1=13, Z=7, nbx=16):
    r = _abi.EnsReduce()
    r.part = r.minlv = r.maxlv = r.mse = r.loss = r.gmin = r.gmax = P
    r.nbx, r.Z, r.S1, r.weight = nbx, Z, S1, 0.01
    return r


def _fit_descs(S=12, A=2, H=200, Z=7, b=256):
    """The descriptors drpo_ens_fit_fb takes for trunk [S+A -> H -> H], heads [H -> H -> S+1]."""
    f, bd = _abi.MlpFwd(), _abi.MlpBwd()
    f.src[0] = f.src[1] = P
    f.cols[0], f.cols[1], f.ld[0], f.ld[1] = S, A, S, A
    nets = [([S + A, H, H], [SWISH, SWISH])] + [([H, H, S + 1], [SWISH, NONE])] * 2
    for j, (dims, acts) in enumerate(nets):
        f.net[j].nl = bd.net[j].nl = 2
        for l in range(2):
            fl, bl = f.net[j].L[l], bd.net[j].L[l]
            fl.W, fl.b, fl.din, fl.dout, fl.act = P, P, dims[l], dims[l + 1], acts[l]
            bl.W, bl.din, bl.dout, bl.act, bl.dz = P, dims[l], dims[l + 1], acts[l], P
    for l in range(2):
        bd.net[0].L[l].dz2 = P
    f.nnets = bd.nnets = 3
    f.trunk = bd.trunk = f.split_heads = bd.split_heads = 1
    f.rows = bd.rows = b
    f.nbatch = bd.nbatch = Z
    bd.upstream = 3
    return f, bd


# what each case breaks, in an upstream and in a reduction (whose rows are counted in blocks)
CASES = {
    'null part': (dict(part=0), dict(part=0)),
    'Z = 0': (dict(Z=0), dict(Z=0)),
    'Z = 257': (dict(Z=257), dict(Z=257)),
    'S + 1 = 257': (dict(S=256), dict(S1=257)),
    'b = 0': (dict(b=0), dict(nbx=0)),
}


def _call(entry, up, red):
    L, out = _lib.lib(), _abi.EnsReduce()
    r = ctypes.byref
    if entry == 'drpo_ens_loss':
        return L.drpo_ens_loss(r(up), r(red), P, P, r(out), None)
    if entry == 'drpo_ens_loss_reduce':
        return L.drpo_ens_loss_reduce(r(red), None)
    if entry == 'drpo_mlp_backward_ens':
        _, bd = _fit_descs()
        return L.drpo_mlp_backward_ens(r(bd), r(up), r(red), r(out), None)
    if entry == 'drpo_ens_fit_fb':
        f, bd = _fit_descs()
        return L.drpo_ens_fit_fb(r(f), r(bd), r(up), r(red), r(out), None)
    if entry == 'drpo_mlp_wgrad_reduce':
        return L.drpo_mlp_wgrad_reduce(None, 0, r(red), None, 0, None)
    assert entry == 'drpo_mlp_wgrad_adam'
    return L.drpo_mlp_wgrad_adam(None, 0, r(red), r(_abi.WgradAdam()), None, 0, None)


TAKES_UPSTREAM = ('drpo_ens_loss', 'drpo_mlp_backward_ens', 'drpo_ens_fit_fb')
TAKES_REDUCTION = ('drpo_ens_loss_reduce', 'drpo_mlp_wgrad_reduce', 'drpo_mlp_wgrad_adam')


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('entry', TAKES_UPSTREAM + TAKES_REDUCTION)
def test_shared_reduction_cases_are_refused(entry, case):
    up, red = _up(), _red()
    brk_up, brk_red = CASES[case]
    upstream = entry in TAKES_UPSTREAM
    for k, v in (brk_up if upstream else brk_red).items():
        setattr(up if upstream else red, k, v)
    assert _call(entry, up, red) == EINVAL
    msg = _err()
    assert msg.startswith(entry + ': bad ' + ('upstream' if upstream else 'reduction')), msg


@pytest.mark.parametrize('entry', TAKES_UPSTREAM)
def test_a_launch_refuses_a_reduction_without_mse(entry):
    """The reduction a launch hands on (ens_reduce_from: red_in + the launch's layout) is held
    to the check of the entry points that will run it."""
    red = _red()
    red.mse = 0
    assert _call(entry, _up(), red) == EINVAL
    assert _err().startswith(entry + ': bad reduction'), _err()


@pytest.mark.parametrize('kw,what', [(dict(S=16), 'S + 1 = 17'), (dict(H=128), 'H = 128')])
def test_fit_fb_refuses_shapes_outside_its_kernel(kw, what):
    L = _lib.lib()
    f, bd = _fit_descs(**kw)
    up, red, out = _up(S=kw.get('S', 12)), _red(), _abi.EnsReduce()
    assert L.drpo_ens_fit_fb(ctypes.byref(f), ctypes.byref(bd), ctypes.byref(up), ctypes.byref(red),
                             ctypes.byref(out), None) == EINVAL
    assert _err().startswith('drpo_ens_fit_fb: needs the ensemble trunk'), (what, _err())


def _full_list_segment():
    """A segment over 16 matrices with a vector before, between and after them: 33 tasks as
    4x4-block work, 31 once plan_segment (csrc/optim.hip) has turned the last matrix into a flat
    range."""
    mp = _abi.PackMap()
    mp.nlayers, off = 16, 64
    for l in range(16):
        mp.off[l], mp.din[l], mp.dout[l], mp.nbatch[l], mp.poff[l] = off, 4, 4, 1, 256 * l
        off += 64
    mp.P = mp.PT = P
    sg = _abi.OptimSeg()
    sg.p = sg.g = sg.m = sg.v = sg.map = P
    sg.start, sg.end, sg.adam, sg.bc2_sqrt, sg.grad_scale = 0, off, 1, 1.0, 1.0
    sg.map_host = ctypes.addressof(mp)
    return sg, mp


def test_optim_step_refuses_what_its_task_list_cannot_hold():
    """Two full segments still fit (31 tasks, then one flat task); the third does not: refused
    before any launch, by name."""
    segs = [_full_list_segment() for _ in range(3)]
    arr = (_abi.OptimSeg * 3)(*[s for s, _ in segs])
    assert _lib.lib().drpo_optim_step(arr, 3, None) == EINVAL
    assert _err().startswith('drpo_optim_step: more than 32 tasks'), _err()
    assert _lib.lib().drpo_optim_step(arr, 9, None) == EINVAL
    assert _err().startswith('drpo_optim_step: at most 8 segments'), _err()


@pytest.mark.parametrize('brk,what', [(dict(nsums=5), '0..4 sums'), (dict(part=0), 'sum 1'), (dict(out=0), 'sum 1'),
                                      (dict(n=-1), 'sum 1')])
def test_wgrad_sums_refuses_bad_sums(brk, what):
    sums = (_abi.SumDesc * 5)()
    for s in sums:
        s.part, s.n, s.out = P, 3, P
    nsums = brk.pop('nsums', 2)
    for k, v in brk.items():
        setattr(sums[1], k, v)
    assert _lib.lib().drpo_mlp_wgrad_sums(None, 0, sums, nsums, None, 0, None) == EINVAL
    assert _err().startswith('drpo_mlp_wgrad_sums: ' + what), _err()


def test_loss_refuses_gD_without_gLVR():
    L = _lib.lib()
    up, red, out = _up(), _red(), _abi.EnsReduce()
    assert L.drpo_ens_loss(ctypes.byref(up), ctypes.byref(red), P, None, ctypes.byref(out), None) == EINVAL
    assert _err().startswith('drpo_ens_loss: gradient outputs'), _err()
    red.gmin = red.gmax = 0      # and the bounds' gradients with the head outputs'
    assert L.drpo_ens_loss(ctypes.byref(up), ctypes.byref(red), P, P, ctypes.byref(out), None) == EINVAL
    assert _err().startswith('drpo_ens_loss: gradient outputs'), _err()
