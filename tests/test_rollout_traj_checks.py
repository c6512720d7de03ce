"""Host-side descriptor checks of drpo_rollout_trajectories (csrc/rollout.hip), no GPU:
every call here is refused before any launch. Pointers are dummies the host never
dereferences (the members array is host memory and real)."""
import ctypes

import pytest

from drpo_amd import _abi, _lib

P = 0x1000          # a non-null pointer value (never dereferenced)
OK, EINVAL = 0, 1
WHO = 'drpo_rollout_trajectories:'


def _err():
    return _lib.lib().drpo_last_error().decode()


def _desc(H=3, buffer=False):
    """A quadrotor-shaped descriptor every shared check accepts. buffer=False leaves the
    virtual-buffer fields (vs .. vv, vptr, vcap) NULL / 0."""
    d = _abi.RolloutDesc()
    d.S, d.A, d.C, d.Ha, d.Hm, d.B, d.H = 12, 2, 2, 256, 200, 72, H
    d.env_id = 1
    for f in ('aW1', 'ab1', 'aW2', 'ab2', 'aW3', 'ab3', 'mW1', 'mb1', 'mW2', 'mb2', 'dW1', 'db1', 'dW2', 'db2',
              'lW1', 'lb1', 'lW2', 'lb2', 'norm_mean', 'norm_std', 'min_lv', 'max_lv', 'replay_states', 'workspace'):
        setattr(d, f, P)
    d.members = (ctypes.c_int * max(H, 1))()
    d.replay_ptr, d.replay_cap = 400, 1000
    if buffer:
        for f in ('vs', 'va', 'vs2', 'vr', 'vh', 'vd', 'vv', 'vptr'):
            setattr(d, f, P)
        d.vcap = 10 ** 6
    return d


def _out(**kw):
    t = _abi.RolloutTraj()
    t.len = P
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _call(d, t):
    return _lib.lib().drpo_rollout_trajectories(ctypes.byref(d), ctypes.byref(t), None)


def test_struct_layout_and_version():
    L = _lib.lib()
    assert L.drpo_abi_sizeof(b'drpo_rollout_traj_t') == ctypes.sizeof(_abi.RolloutTraj) == 12 * ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_version() >= 6             # the version that added the entry point


def test_refuses_a_horizon_above_128():
    d = _desc(H=129)
    assert _call(d, _out()) == EINVAL
    assert _err().startswith(WHO) and 'horizon <= 128' in _err()


def test_refuses_the_per_step_engine():
    d = _desc()
    d.engine = 1
    assert _call(d, _out()) == EINVAL
    assert _err().startswith(WHO) and 'fused engine only' in _err()


def test_refuses_recorded_draws_in_compacted_layout():
    d = _desc()
    d.eps_a = d.eps_m = P
    d.eps_layout = 0
    assert _call(d, _out()) == EINVAL
    assert _err().startswith(WHO) and 'eps_layout 1' in _err()


def test_refuses_a_null_len():
    d = _desc()
    assert _call(d, _out(len=None)) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    assert _lib.lib().drpo_rollout_trajectories(ctypes.byref(d), None, None) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()


def test_refuses_ret_without_weights():
    d = _desc()
    assert _call(d, _out(ret=P)) == EINVAL
    assert _err().startswith(WHO) and 'ret needs weights' in _err()


def test_null_buffer_fields_pass_where_drpo_rollout_refuses_them():
    """The same descriptor: drpo_rollout stops at its buffer checks, the new entry point
    runs through every shared check and stops only at its own last one (ret without
    weights), which comes after them all."""
    L = _lib.lib()
    d = _desc(buffer=False)
    assert L.drpo_rollout(ctypes.byref(d), None) == EINVAL
    assert _err().startswith('drpo_rollout:') and 'exceeds buffer capacity' in _err()
    d.vcap = 10 ** 6                                     # capacity given, pointer still NULL
    assert L.drpo_rollout(ctypes.byref(d), None) == EINVAL
    assert _err() == 'drpo_rollout: null pointer'
    d.vcap = 0
    assert _call(d, _out(ret=P)) == EINVAL
    assert _err() == WHO + ' ret needs weights'


@pytest.mark.parametrize('field, value, fragment', [
    ('S', 65, 'S=65 A=2 out of range'), ('Hm', 300, 'hidden dims'), ('env_id', 7, 'unknown env id 7'),
    ('C', 3, 'con_dim 3 does not match env 1'), ('B', 0, 'B=0 H=3 must be positive'),
    ('replay_states', None, 'null pointer'), ('replay_ptr', 10, 'replay has 10 rows < batch 72'),
    ('rows_per_tile', 8, 'rows_per_tile must be 16 or 32'), ('eps_a', P, 'eps_a and eps_m go together'),
])
def test_shared_checks_apply_with_the_entry_points_own_prefix(field, value, fragment):
    """drpo_rollout's shape, env and pointer checks, through the shared function: the same
    refusal from either entry point, each under its own name."""
    L = _lib.lib()
    for buffer, call, who in ((False, lambda d: _call(d, _out()), WHO),
                              (True, lambda d: L.drpo_rollout(ctypes.byref(d), None), 'drpo_rollout:')):
        d = _desc(buffer=buffer)
        setattr(d, field, value)
        if field == 'B' and buffer:
            fragment = 'exceeds buffer capacity'         # drpo_rollout's combined B / H / capacity check
        assert call(d) == EINVAL
        assert _err().startswith(who) and fragment in _err(), _err()
