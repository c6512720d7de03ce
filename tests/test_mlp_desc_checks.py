"""Host-side descriptor checks of the MLP launches (csrc/mlp.hip), no GPU: every call here
is either rejected before any launch or has rows == 0 and returns DRPO_OK before any
launch. Pointers are dummies the host never dereferences."""
import ctypes

import pytest

from drpo_amd import _abi, _lib, mlp_desc
from drpo_amd.mlp_desc import ACT_ID

P = 0x1000          # a non-null pointer value (never dereferenced)
OK, EINVAL = 0, 1
MAXL = 3
RELU, NONE, TANH = ACT_ID['relu'], ACT_ID[None], ACT_ID['tanh']


def _err():
    return _lib.lib().drpo_last_error().decode()


def _fwd_net(dst, dims, acts):
    dst.nl = len(dims) - 1
    for l in range(min(dst.nl, MAXL)):
        L = dst.L[l]
        L.W, L.b, L.din, L.dout, L.act = P, P, dims[l], dims[l + 1], acts[l]


def _fwd_job(nets, din, rows=0, trunk=0, pair=0):
    d = _abi.MlpFwd()
    d.src[0], d.cols[0], d.ld[0] = P, din, din
    for j, (dims, acts) in enumerate(nets):
        _fwd_net(d.net[j], dims, acts)
    d.nnets, d.trunk, d.rows, d.nbatch, d.pair = len(nets), trunk, rows, 1, pair
    return d


def _bwd_net(dst, dims, acts, gout=P, nl=None, sy=0):
    dst.nl = len(dims) - 1 if nl is None else nl
    for l in range(len(dims) - 1):
        L = dst.L[l]
        L.W, L.din, L.dout, L.act, L.sy = P, dims[l], dims[l + 1], acts[l], sy
    dst.gout = gout


def _bwd_job(nets, rows=0, trunk=0, upstream=0, **kw):
    d = _abi.MlpBwd()
    for j, (dims, acts) in enumerate(nets):
        _bwd_net(d.net[j], dims, acts, **kw)
    d.nnets, d.trunk, d.rows, d.nbatch, d.upstream = len(nets), trunk, rows, 1, upstream
    return d


def _multi(fn, jobs, *extra):
    arr = (type(jobs[0]) * len(jobs))(*jobs)
    return fn(arr, P, len(jobs), *extra, None)


Q = ([20, 256, 256, 1], [RELU, RELU, NONE])                      # a critic
TRUNK, HEAD = ([20, 256, 256], [RELU, RELU]), ([256, 256, 3], [RELU, NONE])   # the constraint critic, C = 3
PI = ([17, 256, 256, 6], [RELU, RELU, NONE])                      # a policy, A = 3


def test_backward_rejects_a_trunk_with_too_many_layers():
    L = _lib.lib()
    d = _bwd_job([TRUNK, HEAD, HEAD], trunk=1)
    assert L.drpo_mlp_backward(ctypes.byref(d), None) == OK
    d.net[0].nl = MAXL + 1
    assert L.drpo_mlp_backward(ctypes.byref(d), None) == EINVAL
    assert 'drpo_mlp_backward: job 0: net 0 has 4 layers' in _err()


@pytest.mark.parametrize('upstream', [mlp_desc.UPSTREAM_CRITIC, mlp_desc.UPSTREAM_ENS, mlp_desc.UPSTREAM_SQUASH])
def test_backward_rejects_an_in_kernel_upstream(upstream):
    L = _lib.lib()
    d = _bwd_job([Q], upstream=upstream)
    assert L.drpo_mlp_backward(ctypes.byref(d), None) == EINVAL
    assert f'drpo_mlp_backward: upstream {upstream}' in _err()


def test_backward_requires_gout_only_where_it_is_read():
    L = _lib.lib()
    d = _bwd_job([TRUNK, HEAD, HEAD], trunk=1)
    d.net[0].gout = 0                     # the trunk's gradient comes from its heads
    assert L.drpo_mlp_backward(ctypes.byref(d), None) == OK
    d.net[2].gout = 0
    assert L.drpo_mlp_backward(ctypes.byref(d), None) == EINVAL
    assert 'drpo_mlp_backward: job 0: net 2 needs gout' in _err()


@pytest.mark.parametrize('field', ['pair', 'head.mode', 'head2.mode', 'pre.nl', 'post.nl', 'post_x', 'ccb_out'])
def test_forward_rejects_what_only_the_multi_launch_runs(field):
    L = _lib.lib()
    d = _fwd_job([Q, Q], 20)
    assert L.drpo_mlp_forward(ctypes.byref(d), None) == OK
    obj, _, name = field.rpartition('.')
    setattr(getattr(d, obj) if obj else d, name, P if field in ('post_x', 'ccb_out') else 1)
    assert L.drpo_mlp_forward(ctypes.byref(d), None) == EINVAL
    assert 'drpo_mlp_forward: head, head2, pair, pre, post, post_x and ccb_out need drpo_mlp_forward_multi' in _err()


def _critic_head():
    h = _abi.CriticHead()
    h.B, h.C = 0, 3
    h.loss_part = h.log_alpha = h.q0 = h.q1 = h.mu = P
    return h


def _actor_head():
    h = _abi.ActorHead()
    h.B, h.C, h.A = 0, 3, 3
    h.u[0] = h.e[0] = h.dA[0] = h.u[1] = h.e[1] = h.dA[1] = P
    return h


def test_multi_head_accepts_upstream_jobs_without_gout():
    L = _lib.lib()
    jobs = [_bwd_job([TRUNK, HEAD], trunk=1, upstream=mlp_desc.UPSTREAM_CERT, gout=0),
            _bwd_job([Q, Q], upstream=mlp_desc.UPSTREAM_CRITIC, gout=0)]
    h = _critic_head()
    assert _multi(L.drpo_mlp_backward_multi_head, jobs, ctypes.byref(h)) == OK, _err()


def test_multi_actor_accepts_upstream_jobs_without_gout():
    L = _lib.lib()
    h = _actor_head()
    jobs = [_bwd_job([TRUNK, HEAD], trunk=1, upstream=mlp_desc.UPSTREAM_ACTOR_CC, gout=0, sy=P),
            _bwd_job([TRUNK, HEAD], trunk=1, upstream=mlp_desc.UPSTREAM_SAFE_CC, gout=0, sy=P),
            _bwd_job([Q], upstream=mlp_desc.UPSTREAM_NEG_MEAN, gout=0)]
    assert _multi(L.drpo_mlp_backward_multi_actor, jobs, ctypes.byref(h)) == OK, _err()
    jobs = [_bwd_job([PI], upstream=mlp_desc.UPSTREAM_SQUASH, gout=0, sy=P),
            _bwd_job([PI], upstream=mlp_desc.UPSTREAM_SQUASH_SAFE, gout=0, sy=P)]
    assert _multi(L.drpo_mlp_backward_multi_actor, jobs, ctypes.byref(h)) == OK, _err()


def test_multi_still_rejects_a_gout_job_without_gout():
    L = _lib.lib()
    h = _actor_head()
    jobs = [_bwd_job([Q], upstream=mlp_desc.UPSTREAM_NEG_MEAN, gout=0), _bwd_job([Q], gout=0)]
    assert _multi(L.drpo_mlp_backward_multi_actor, jobs, ctypes.byref(h)) == EINVAL
    assert 'drpo_mlp_backward_multi: job 1: net 0 needs gout' in _err()
    assert _multi(L.drpo_mlp_backward_multi, jobs[1:]) == EINVAL
    assert 'drpo_mlp_backward_multi: job 0: net 0 needs gout' in _err()
    jobs[1].net[0].gout = P
    assert _multi(L.drpo_mlp_backward_multi_actor, jobs, ctypes.byref(h)) == OK, _err()


class _T:
    """stands in for a weight tensor in a Net's layer tuples"""

    def data_ptr(self):
        return P


def _net(dims, acts):
    return mlp_desc.Net([(_T(), _T(), dims[l], dims[l + 1], acts[l], None) for l in range(len(dims) - 1)])


R3 = [RELU, RELU, NONE]
PAIR_SHAPES = [([K, 256, 256, 6], R3) for K in (16, 17, 48, 49, 64, 65)] + [
    ([16, 255, 255, 6], R3), ([16, 256, 255, 6], R3), ([64, 256, 256, 16], R3), ([64, 256, 256, 17], R3),
    ([16, 256, 256, 6], [RELU, TANH, NONE]), ([16, 256, 256, 6], [RELU, RELU, TANH]),
    ([16, 256, 256, 6], [TANH, RELU, NONE]), ([16, 256, 6], [RELU, NONE])]


def test_pairable_agrees_with_the_c_pair_check():
    """mlp_desc.pairable (which picks pair jobs: drpo_mlp_pair_ok over the nets' shapes) against
    csrc/mlp.hip pair_ok (which admits them), through a rows = 0 drpo_mlp_forward_multi call with
    pair = 1."""
    L = _lib.lib()
    verdicts = []
    cases = [(s, s) for s in PAIR_SHAPES] + [(PAIR_SHAPES[0], ([16, 256, 256, 4], R3)),    # two shapes
                                             (PAIR_SHAPES[0], ([16, 256, 256, 6], [RELU, TANH, NONE]))]
    for a, b in cases:
        rc = _multi(L.drpo_mlp_forward_multi, [_fwd_job([a, b], a[0][0], pair=1)], 0, 0)
        want = mlp_desc.pairable(_net(*a), _net(*b))
        assert rc == (OK if want else EINVAL), (a, b, _err())
        if not want:
            assert 'drpo_mlp_forward_multi: job 0: a pair job needs two 3-layer ReLU nets of one shape' in _err()
        verdicts.append(want)
    # K = 16, 49, 64 and out = 16 pair; everything else in the table does not
    assert verdicts == [True, False, False, True, True, False, False, False, True, False, False, False, False, False,
                        False, False]
