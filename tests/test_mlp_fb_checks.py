"""Host-side checks of the fused forward + backward launch (drpo_mlp_fb_multi,
csrc/mlp.hip), no GPU: every call has rows == 0 (accepted jobs return DRPO_OK before any
launch) or is refused by name before any launch. Pointers are dummies the host never
dereferences."""
import ctypes

import pytest

from drpo_amd import _abi, _lib, mlp_desc
from test_mlp_desc_checks import EINVAL, HEAD, NONE, OK, P, Q, RELU, TANH, TRUNK, _actor_head, _bwd_job, _err, \
    _fwd_job, _fwd_net

S1 = 21     # the post chain's input width: the 20 src[0] columns + the bound


def _launch():
    """The actor update's three jobs (sac_step.py 'a.fb'): forwards [certificate + bound +
    multiplier post chain, certificate, certificate, critic], one backward each."""
    ccm = _fwd_job([TRUNK, HEAD, HEAD], 20, trunk=1)
    ccm.ccb_out = P
    _fwd_net(ccm.post, [S1, 256, 256, 1], [RELU, RELU, NONE])
    fw = [ccm, _fwd_job([TRUNK, HEAD, HEAD], 20, trunk=1), _fwd_job([TRUNK, HEAD, HEAD], 20, trunk=1),
          _fwd_job([Q], 20)]
    bw = [_bwd_job([TRUNK, HEAD, HEAD], trunk=1, upstream=mlp_desc.UPSTREAM_ACTOR_CC, gout=0),
          _bwd_job([TRUNK, HEAD, HEAD], trunk=1, upstream=mlp_desc.UPSTREAM_SAFE_CC, gout=0),
          _bwd_job([Q], upstream=mlp_desc.UPSTREAM_NEG_MEAN, gout=0)]
    jobs = [((0, 1), 0), ((2,), 1), ((3,), 2)]
    h = _actor_head()
    h.lams = P
    return fw, bw, jobs, h


def _call(fw, bw, jobs, h):
    fa = (_abi.MlpFwd * len(fw))(*fw)
    ba = (_abi.MlpBwd * len(bw))(*bw)
    ja = (_abi.MlpFbJob * len(jobs))()
    for J, (fi, bi) in zip(ja, jobs):
        J.nfwd, J.bwd = len(fi), bi
        for q, i in enumerate(fi[:2]):
            J.fwd[q] = i
    return _lib.lib().drpo_mlp_fb_multi(fa, P, len(fw), ba, P, len(bw), ja, len(jobs), ctypes.byref(h), 0, 0, None)


def test_fb_accepts_the_actor_update_jobs():
    assert _call(*_launch()) == OK, _err()


def _dz(fw, bw, jobs, h):
    bw[2].net[0].L[1].dz = P


def _tanh(fw, bw, jobs, h):
    fw[3].net[0].L[0].act = bw[2].net[0].L[0].act = TANH


def _pair(fw, bw, jobs, h):
    q16 = ([16, 256, 256, 1], [RELU, RELU, NONE])     # a shape the pair job admits
    fw[3] = _fwd_job([q16, q16], 16, pair=1)


def _mismatch(fw, bw, jobs, h):
    bw[1].net[1].L[1].dout = 2


def _no_post(fw, bw, jobs, h):
    jobs[0] = ((1, 1), 0)


def _bad_index(fw, bw, jobs, h):
    jobs[2] = ((3,), 3)


def _bad_fwd_index(fw, bw, jobs, h):
    jobs[2] = ((4,), 2)


def _gout_upstream(fw, bw, jobs, h):
    bw[2] = _bwd_job([Q], upstream=mlp_desc.UPSTREAM_GOUT)


def _narrow_heads(fw, bw, jobs, h):
    head = ([256, 128, 3], [RELU, NONE])
    fw[2] = _fwd_job([TRUNK, head, head], 20, trunk=1)
    bw[1] = _bwd_job([TRUNK, head, head], trunk=1, upstream=mlp_desc.UPSTREAM_SAFE_CC, gout=0)


def _safe_with_chain(fw, bw, jobs, h):
    jobs[1] = ((0, 2), 1)


def _too_many(fw, bw, jobs, h):
    jobs.extend([((3,), 2), ((3,), 2)])


def _rows(fw, bw, jobs, h):
    fw[3].rows = 16


def _batched(fw, bw, jobs, h):
    fw[3].nbatch = 2


@pytest.mark.parametrize('spoil, message', [
    (_dz, 'job 2: net 0 layer 1: dz saves are not written here'),
    (_tanh, 'job 2: net 0 layer 0: hidden layers are ReLU and wider than 16, outputs identity'),
    (_pair, 'job 2: forward 0: one batch item, one net or a trunk job, no pair / head / head2 / pre'),
    (_mismatch, 'job 1: net 1 differs between the forward and the backward'),
    (_no_post, 'job 0: a first forward must end in a post chain with one output (the multiplier)'),
    (_bad_index, 'job 2: 1..2 forwards and a backward of the launch\'s arrays'),
    (_bad_fwd_index, 'job 2: forward index 4'),
    (_gout_upstream, 'job 2: a single net takes the -1/B upstream on one output, after one forward'),
    (_narrow_heads, 'job 1: a trunk job takes the constraint-critic upstream on paired 256-wide heads'),
    (_safe_with_chain, 'job 1: only the actor\'s certificate job chains the multiplier forward in front'),
    (_too_many, '1..4 jobs over forward and backward descriptor arrays'),
    (_rows, 'job 2: forward 0 has 16 rows, the actor head 0'),
    (_batched, 'job 2: forward 0: one batch item'),
])
def test_fb_refuses_malformed_jobs_by_name(spoil, message):
    fw, bw, jobs, h = _launch()
    spoil(fw, bw, jobs, h)
    assert _call(fw, bw, jobs, h) == EINVAL
    assert 'drpo_mlp_fb_multi: ' + message in _err()


def test_fb_needs_an_actor_head():
    fw, bw, jobs, h = _launch()
    h.C = 17
    assert _call(fw, bw, jobs, h) == EINVAL
    assert 'drpo_mlp_fb_multi: bad actor head' in _err()
