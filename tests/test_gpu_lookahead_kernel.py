"""drpo_rollout_lookahead (csrc/lookahead.hip) on synthetic rows, bit for bit against
lookahead_helpers.lookahead_reference (float32 compared as int32, no tolerance: both sides do the
same double operations in the same order and round once).

Shapes: B 37 (a partial last workgroup at any number of rows per workgroup), H 1, 3 and 128 (the
longest chain), C 1 and 2, both modes, discount 0, 0.99 and 1. The rows (lookahead_helpers.synthetic,
built by position) show every length 0..H terminated and not (at H 128, where 37 rows cannot, a
spread of lengths with 0 and H among them), h' on both sides of 0 (the offset) and of the bootstrap
(both arms of the max), a NaN, a +inf and a -inf terminal bootstrap on live rows (they propagate),
a NaN step bootstrap, and a NaN where a terminated row's bootstrap would be (it must not show);
assert_synthetic_shows_every_case holds the inputs to that before anything is compared."""
import ctypes

import numpy as np
import pytest
import torch

from drpo_amd import _abi, _lib
from gpu_helpers import DEV
from lookahead_helpers import (COST, REACH, SCALES, assert_bits, assert_synthetic_shows_every_case, lookahead_reference,
                               synthetic, weights)

pytestmark = pytest.mark.gpu

B = 37
SENTINEL = -7.25


def _launch(x, H, C, mode, gamma, value=True, certificate=True):
    """One drpo_rollout_lookahead call on the CPU tensors ``x``: (value, certificate), None for an
    output that was not given."""
    dev = {k: v.to(DEV).contiguous() for k, v in x.items()}
    n = len(x['lengths'])
    w = torch.from_numpy(weights(gamma, H)).to(DEV)
    out_v = torch.full((n, H + 1), SENTINEL, device=DEV) if value else None
    out_c = torch.full((n, H + 1, C), SENTINEL, device=DEV) if certificate else None
    d = _abi.RolloutLookahead()
    d.B, d.H, d.C, d.mode, d.gamma = n, H, C, mode, gamma
    for k, v in SCALES.items():
        setattr(d, k, v)
    for k, v in dev.items():
        setattr(d, k, v.data_ptr())
    if mode == REACH:
        d.violations = None                                   # may be null there
    d.weights = w.data_ptr()
    d.value = out_v.data_ptr() if value else None
    d.certificate = out_c.data_ptr() if certificate else None
    _lib.check(_lib.lib().drpo_rollout_lookahead(ctypes.byref(d), _lib.stream()), 'rollout_lookahead')
    torch.cuda.synchronize()
    return out_v, out_c


_INPUTS = {}


def _inputs(H, C):
    if (H, C) not in _INPUTS:
        x, cases = synthetic(B, H, C)
        assert_synthetic_shows_every_case(x, cases, H, C)
        _INPUTS[H, C] = x, cases
    return _INPUTS[H, C]


@pytest.mark.parametrize('gamma', [0.0, 0.99, 1.0])
@pytest.mark.parametrize('mode', [REACH, COST], ids=['reachability', 'cost'])
@pytest.mark.parametrize('C', [1, 2])
@pytest.mark.parametrize('H', [1, 3, 128])
def test_kernel_equals_the_reference(H, C, mode, gamma):
    x, cases = _inputs(H, C)
    want_v, want_c = lookahead_reference(**x, gamma=gamma, mode=mode, **SCALES)
    got_v, got_c = _launch(x, H, C, mode, gamma)
    assert_bits(got_v, want_v, 'value')
    assert_bits(got_c, want_c, 'certificate')
    # what the cases are there for
    assert np.isnan(want_v[cases['nan_boot']]).any() and np.isnan(want_c[cases['nan_boot']]).any()
    assert not np.isfinite(want_v[cases['pinf_boot']]).all() and not np.isfinite(want_v[cases['ninf_boot']]).all()
    assert np.isfinite(want_v[cases['nan_dead']]).all() and np.isfinite(want_c[cases['nan_dead']]).all()
    assert np.isnan(want_c[cases['nan_step'], 0]).all()
    # either output alone: the same values
    only_v, none = _launch(x, H, C, mode, gamma, certificate=False)
    assert none is None
    assert_bits(only_v, want_v, 'value alone')
    none, only_c = _launch(x, H, C, mode, gamma, value=False)
    assert none is None
    assert_bits(only_c, want_c, 'certificate alone')


@pytest.mark.parametrize('mode', [REACH, COST], ids=['reachability', 'cost'])
def test_lengths_outside_the_horizon_do_not_fault(mode):
    """lengths are clamped as read: 200 and -3 in memory index nothing outside the row. Only the
    return of the call and the other rows are required."""
    H, C = 3, 2
    x, _ = _inputs(H, C)
    x = dict(x, lengths=x['lengths'].clone())
    a, b = 5, 30
    x['lengths'][a], x['lengths'][b] = 200, -3
    want_v, want_c = lookahead_reference(**x, gamma=0.99, mode=mode, **SCALES)
    got_v, got_c = _launch(x, H, C, mode, 0.99)
    rows = np.array([i for i in range(B) if i not in (a, b)])
    assert_bits(got_v, want_v, 'value', rows)
    assert_bits(got_c, want_c, 'certificate', rows)
    assert not bool((got_v == SENTINEL).any()) and not bool((got_c == SENTINEL).any())     # every element written
