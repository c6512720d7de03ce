"""Host-side checks of drpo_rollout_trajectories_linear (csrc/rollout.hip) and of the Python
refusals of imagine(shield='linear'), no GPU: every call here is refused before any launch.
The descriptors and their dummy pointers are test_rollout_traj_checks.py's and
test_rollout_shield_checks.py's."""
import ctypes

import pytest
import torch

import drpo_amd
from drpo_amd import _abi, _lib
from test_host_logic import make_smbpo
from test_rollout_shield_checks import _shield
from test_rollout_traj_checks import EINVAL, P, _desc, _err, _out

WHO = 'drpo_rollout_trajectories_linear:'
H = 3


def _linear(K=11, blend=P):
    lin = _abi.RolloutLinear()
    lin.candidates, lin.blend = K, blend
    return lin


def _call(d, s, lin, t):
    by = lambda x: None if x is None else ctypes.byref(x)   # noqa: E731
    return _lib.lib().drpo_rollout_trajectories_linear(ctypes.byref(d), by(s), by(lin), by(t), None)


def test_struct_layout_and_version():
    L = _lib.lib()
    assert L.drpo_abi_sizeof(b'drpo_rollout_linear_t') == ctypes.sizeof(_abi.RolloutLinear)
    # an int (padded to a pointer) and the output pointer
    assert ctypes.sizeof(_abi.RolloutLinear) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_version() >= 9             # the version that added the entry point
    # drpo_rollout_shield_t did not change
    assert L.drpo_abi_sizeof(b'drpo_rollout_shield_t') == 20 * ctypes.sizeof(ctypes.c_void_p) + 32


@pytest.mark.parametrize('K', [1, 33, 0, -1])
def test_refuses_candidates_outside_2_to_32(K):
    assert _call(_desc(H=H), _shield(), _linear(K), _out()) == EINVAL
    assert _err() == f'{WHO} linear shield candidates {K} outside 2..32'


def test_refuses_linear_without_shield():
    assert _call(_desc(H=H), None, _linear(), _out()) == EINVAL
    assert _err().startswith(WHO) and 'linear without shield' in _err()


@pytest.mark.parametrize('K', [2, 11, 32])
@pytest.mark.parametrize('linear', [False, True])
def test_every_check_of_the_shielded_call_applies(linear, K):
    """linear == NULL is drpo_rollout_trajectories_shielded, and a valid linear adds no
    refusal: the shield's and the trajectory call's refusals, under this entry point's name."""
    lin = _linear(K) if linear else None
    assert _call(_desc(H=H), _shield(Hc=257), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'hidden width 257 outside 1..256' in _err()
    assert _call(_desc(H=H), _shield(sW2=None), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'null safe-actor pointer' in _err()
    assert _call(_desc(H=H), _shield(zW1=None), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'distributional shield needs the log-std head' in _err()
    # mean only, NULL log-std head: through the shield's checks to a later refusal
    s = _shield(distributional=0, zW1=None, zb1=None, zW2=None, zb2=None)
    assert _call(_desc(H=H), s, lin, _out(ret=P)) == EINVAL
    assert _err() == WHO + ' ret needs weights'
    assert _call(_desc(H=H), _shield(), lin, _out(len=None)) == EINVAL
    assert _err().startswith(WHO) and 'null len' in _err()
    assert _call(_desc(H=129), _shield(), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'horizon <= 128' in _err()
    d = _desc(H=H)
    d.engine = 1
    assert _call(d, _shield(), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'fused engine only' in _err()
    d = _desc(H=H)
    d.rows_per_tile = 8
    assert _call(d, _shield(), lin, _out()) == EINVAL
    assert _err().startswith(WHO) and 'rows_per_tile must be 16 or 32' in _err()


# ------------------------------------------------------------------ Python
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


def test_python_refusals(alg):
    """Each is a ValueError raised before anything touches a device (the trainer is on the
    CPU here: a call that got further would raise DrpoError, not ValueError)."""
    B, A = alg.rollout_batch_size, alg.action_dim
    s = torch.zeros(B, alg.state_dim)
    with pytest.raises(ValueError, match='shield with actions'):
        alg.imagine(s, actions=torch.zeros(B, 1, A), shield='linear')
    with pytest.raises(ValueError, match='shield with actions'):
        alg.imagine(s, actions=torch.zeros(B, 1, A), shield=('linear', 0.0, 5))
    with pytest.raises(ValueError, match='shield with a recorded tape'):
        alg.imagine(s, noise=drpo_amd.TapeNoise([]), shield='linear')
    for bad in ('safe', 'Linear', '', ('safe', 0.0), (), ('linear', 0.0, 11, 1)):
        with pytest.raises(ValueError, match='shield: '):
            alg.imagine(s, shield=bad)
    for K in (1, 33, 0, 11.0, True):
        with pytest.raises(ValueError, match='shield_candidates'):
            alg.imagine(s, shield=('linear', 0.0, K))
    with pytest.raises(ValueError, match='shield_uncertainty without shield'):
        alg.imagine(s, shield_uncertainty=True)


def test_python_refuses_the_bound_of_a_mean_only_critic(alg, monkeypatch):
    monkeypatch.setattr(alg.solver, 'distributional_qc', False)
    with pytest.raises(ValueError, match='not distributional'):
        alg.imagine(torch.zeros(4, alg.state_dim), shield='linear', shield_uncertainty=True)


def test_a_valid_linear_call_gets_past_the_refusals(alg):
    """... and stops where the compute path asks for device tensors."""
    for shield in ('linear', ('linear', 0.5), ('linear', 0.5, 2), ('linear', 0.5, 32), ['linear', None, None]):
        with pytest.raises(_lib.DrpoError, match='no CPU fallback'):
            alg.imagine(torch.zeros(4, alg.state_dim), shield=shield)
