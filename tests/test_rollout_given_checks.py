"""Host-side checks of drpo_rollout_trajectories_given (csrc/rollout.hip), no GPU: every
call here is refused before any launch. The descriptor and its dummy pointers are
test_rollout_traj_checks.py's."""
import ctypes

import pytest

from drpo_amd import _abi, _lib
from test_rollout_traj_checks import EINVAL, P, _desc, _err, _out

WHO = 'drpo_rollout_trajectories_given:'
H = 3


def _given(steps, actions=P):
    g = _abi.RolloutGiven()
    g.actions, g.steps = actions, steps
    return g


def _call(d, g, t):
    return _lib.lib().drpo_rollout_trajectories_given(ctypes.byref(d), None if g is None else ctypes.byref(g),
                                                      None if t is None else ctypes.byref(t), None)


def test_struct_layout_and_version():
    L = _lib.lib()
    assert L.drpo_abi_sizeof(b'drpo_rollout_given_t') == ctypes.sizeof(_abi.RolloutGiven) == \
        2 * ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_version() >= 7             # the version that added the entry point


@pytest.mark.parametrize('steps, actions, fragment', [
    (H + 1, P, 'given steps 4 outside [0, horizon 3]'),
    (-1, P, 'given steps -1 outside [0, horizon 3]'),
    (2, None, 'given steps 2 need actions'),
])
def test_refuses_bad_given(steps, actions, fragment):
    assert _call(_desc(H=H), _given(steps, actions), _out()) == EINVAL
    assert _err().startswith(WHO) and fragment in _err(), _err()


@pytest.mark.parametrize('given', [None, 'zero steps'])
def test_no_given_reaches_the_later_refusals_of_drpo_rollout_trajectories(given):
    """given == NULL (and steps == 0, with or without actions) is drpo_rollout_trajectories:
    the same refusals, under this entry point's name."""
    g = None if given is None else _given(0, None)
    d = _desc(H=H)
    assert _call(d, g, _out(len=None)) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    assert _call(d, g, None) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    assert _call(d, g, _out(ret=P)) == EINVAL
    assert _err() == WHO + ' ret needs weights'
    d = _desc(H=129)
    assert _call(d, g, _out()) == EINVAL
    assert _err().startswith(WHO) and 'horizon <= 128' in _err()


def test_shared_checks_come_first_and_carry_the_name():
    d = _desc(H=H)
    d.engine = 1
    assert _call(d, _given(2), _out()) == EINVAL
    assert _err().startswith(WHO) and 'fused engine only' in _err()
    d = _desc(H=H)
    d.replay_ptr = 10
    assert _call(d, _given(H + 1), _out()) == EINVAL
    assert _err().startswith(WHO) and 'replay has 10 rows < batch 72' in _err()
