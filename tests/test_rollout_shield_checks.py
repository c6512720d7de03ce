"""Host-side checks of drpo_rollout_trajectories_shielded (csrc/rollout.hip), no GPU: every
call here is refused before any launch. The descriptor and its dummy pointers are
test_rollout_traj_checks.py's."""
import ctypes

import pytest

from drpo_amd import _abi, _lib
from test_rollout_traj_checks import EINVAL, P, _desc, _err, _out

WHO = 'drpo_rollout_trajectories_shielded:'
H = 3
SAFE = ('sW1', 'sb1', 'sW2', 'sb2', 'sW3', 'sb3')
TRUNK_MEAN = ('cW1', 'cb1', 'cW2', 'cb2', 'qW1', 'qb1', 'qW2', 'qb2')
LOG_STD = ('zW1', 'zb1', 'zW2', 'zb2')


def _shield(**kw):
    """The quadrotor's shield (Hc 256, Cq 2, distributional), every check passing."""
    s = _abi.RolloutShield()
    for f in SAFE + TRUNK_MEAN + LOG_STD + ('interventions', 'certificate'):
        setattr(s, f, P)
    s.Hc, s.Cq, s.distributional = 256, 2, 1
    s.std_ratio, s.log_std_min, s.log_std_max, s.threshold = 2.0, -4.0, 4.0, -0.1
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _call(d, s, t):
    return _lib.lib().drpo_rollout_trajectories_shielded(ctypes.byref(d), None if s is None else ctypes.byref(s),
                                                         None if t is None else ctypes.byref(t), None)


def test_struct_layout_and_version():
    L = _lib.lib()
    assert L.drpo_abi_sizeof(b'drpo_rollout_shield_t') == ctypes.sizeof(_abi.RolloutShield)
    # 18 weight / bias pointers, 3 ints and 4 floats (padded to a pointer), 2 output pointers
    assert ctypes.sizeof(_abi.RolloutShield) == 20 * ctypes.sizeof(ctypes.c_void_p) + 32
    assert L.drpo_version() >= 8             # the version that added the entry point


@pytest.mark.parametrize('field, value, fragment', [
    ('Hc', 0, 'hidden width 0 outside 1..256'), ('Hc', 257, 'hidden width 257 outside 1..256'),
    ('Cq', 0, 'outputs 0 outside 1..8'), ('Cq', 9, 'outputs 9 outside 1..8'),
] + [(f, None, 'null safe-actor pointer') for f in SAFE]
  + [(f, None, 'null critic trunk / mean head pointer') for f in TRUNK_MEAN]
  + [(f, None, 'distributional shield needs the log-std head') for f in LOG_STD])
def test_refuses_bad_shield(field, value, fragment):
    assert _call(_desc(H=H), _shield(**{field: value}), _out()) == EINVAL
    assert _err().startswith(WHO) and fragment in _err(), _err()


def test_mean_only_shield_needs_no_log_std_head():
    """distributional == 0 with a NULL log-std head passes the shield's checks: the call
    stops at a later refusal of drpo_rollout_trajectories."""
    s = _shield(distributional=0, **{f: None for f in LOG_STD})
    assert _call(_desc(H=H), s, _out(ret=P)) == EINVAL
    assert _err() == WHO + ' ret needs weights'


@pytest.mark.parametrize('shield', [None, 'valid'])
def test_reaches_the_later_refusals_of_drpo_rollout_trajectories(shield):
    """shield == NULL is drpo_rollout_trajectories, and a valid shield adds no refusal: the
    same refusals, under this entry point's name."""
    s = None if shield is None else _shield()
    d = _desc(H=H)
    assert _call(d, s, _out(len=None)) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    assert _call(d, s, None) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    assert _call(d, s, _out(ret=P)) == EINVAL
    assert _err() == WHO + ' ret needs weights'
    d = _desc(H=129)
    assert _call(d, s, _out()) == EINVAL
    assert _err().startswith(WHO) and 'horizon <= 128' in _err()
    d = _desc(H=H)
    d.engine = 1
    assert _call(d, s, _out()) == EINVAL
    assert _err().startswith(WHO) and 'fused engine only' in _err()
    d = _desc(H=H)
    d.replay_ptr = 10
    assert _call(d, s, _out()) == EINVAL
    assert _err().startswith(WHO) and 'replay has 10 rows < batch 72' in _err()
