"""Host-side checks of the halting entry points (csrc/rollout.hip), no GPU: drpo_rollout_stage,
drpo_rollout_emit_cut, drpo_rollout_trajectories_cut and the host-only
drpo_rollout_staging_offsets. Every call here is refused before any launch; pointers are
dummies the host never dereferences (the members array is host memory and real)."""
import ctypes
import math

import pytest

from drpo_amd import _abi, _lib
from test_rollout_traj_checks import EINVAL, OK, P, _desc, _err, _out

STAGE, EMIT, TRAJ = 'drpo_rollout_stage', 'drpo_rollout_emit_cut', 'drpo_rollout_trajectories_cut'


def _cut(**kw):
    c = _abi.RolloutCut()
    c.scores, c.row_stride, c.step_stride, c.threshold, c.halted_at = P, 1, 72, 0.5, P
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _call(entry, d, cut=None):
    """The entry point on descriptor ``d`` (cut: a RolloutCut, or None for a NULL one)."""
    L = _lib.lib()
    c = None if cut is None else ctypes.byref(cut)
    if entry == STAGE:
        return L.drpo_rollout_stage(ctypes.byref(d), None)
    if entry == EMIT:
        return L.drpo_rollout_emit_cut(ctypes.byref(d), c, None)
    return L.drpo_rollout_trajectories_cut(ctypes.byref(d), c, ctypes.byref(_out()), None)


def _desc_for(entry, **kw):
    return _desc(buffer=entry != TRAJ, **kw)


def test_struct_layout_and_version():
    L = _lib.lib()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_abi_sizeof(b'drpo_rollout_cut_t') == ctypes.sizeof(_abi.RolloutCut) == 2 * ptr + 16 + 8
    assert L.drpo_version() >= 11            # the version that added the entry points


@pytest.mark.parametrize('entry', [EMIT, TRAJ])
def test_refuses_a_null_cut_or_scores(entry):
    d = _desc_for(entry)
    assert _call(entry, d, None) == EINVAL
    assert _err().startswith(entry + ':') and 'null cut descriptor or scores' in _err()
    assert _call(entry, d, _cut(scores=None)) == EINVAL
    assert _err().startswith(entry + ':') and 'null cut descriptor or scores' in _err()


@pytest.mark.parametrize('entry', [EMIT, TRAJ])
@pytest.mark.parametrize('field', ['row_stride', 'step_stride'])
def test_refuses_a_zero_stride(entry, field):
    assert _call(entry, _desc_for(entry), _cut(**{field: 0})) == EINVAL
    assert _err().startswith(entry + ':') and 'must not be zero' in _err()


@pytest.mark.parametrize('entry', [EMIT, TRAJ])
def test_refuses_a_nan_threshold_and_takes_infinities(entry):
    d = _desc_for(entry)
    assert _call(entry, d, _cut(threshold=math.nan)) == EINVAL
    assert _err().startswith(entry + ':') and 'threshold is NaN' in _err()
    # an infinite threshold passes this check: the next refusal is another one
    d.engine = 1
    for thr in (math.inf, -math.inf):
        assert _call(entry, d, _cut(threshold=thr)) == EINVAL
        assert 'fused engine only' in _err()


@pytest.mark.parametrize('entry', [STAGE, EMIT, TRAJ])
def test_refuses_the_per_step_engine(entry):
    d = _desc_for(entry)
    d.engine = 1
    assert _call(entry, d, _cut()) == EINVAL
    assert _err().startswith(entry + ':') and 'fused engine only' in _err()


@pytest.mark.parametrize('entry', [STAGE, EMIT, TRAJ])
def test_refuses_a_horizon_above_the_fused_engines(entry):
    L = _lib.lib()
    assert L.drpo_abi_const(b'DRPO_ROLLOUT_FUSED_MAX_H') == 128
    d = _desc_for(entry, H=129)
    assert _call(entry, d, _cut()) == EINVAL
    assert _err().startswith(entry + ':') and 'horizon <= 128' in _err()


@pytest.mark.parametrize('entry', [STAGE, EMIT, TRAJ])
def test_refuses_recorded_draws_in_compacted_layout(entry):
    d = _desc_for(entry)
    d.eps_a = d.eps_m = P
    d.eps_layout = 0
    assert _call(entry, d, _cut()) == EINVAL
    assert _err().startswith(entry + ':') and 'eps_layout 1' in _err()


@pytest.mark.parametrize('entry', [STAGE, EMIT, TRAJ])
@pytest.mark.parametrize('field, value, fragment', [
    ('S', 65, 'S=65 A=2 out of range'), ('env_id', 7, 'unknown env id 7'), ('replay_states', None, 'null pointer'),
    ('replay_ptr', 10, 'replay has 10 rows < batch 72'), ('rows_per_tile', 8, 'rows_per_tile must be 16 or 32'),
])
def test_makes_drpo_rollouts_checks(entry, field, value, fragment):
    d = _desc_for(entry)
    setattr(d, field, value)
    assert _call(entry, d, _cut()) == EINVAL
    assert _err().startswith(entry + ':') and fragment in _err(), _err()


@pytest.mark.parametrize('entry', [STAGE, EMIT])
def test_the_buffer_entries_need_the_buffer(entry):
    d = _desc(buffer=False)
    assert _call(entry, d, _cut()) == EINVAL
    assert _err().startswith(entry + ':') and 'exceeds buffer capacity' in _err()


def test_trajectories_cut_checks_its_outputs():
    L = _lib.lib()
    d, c = _desc(), _cut()
    assert L.drpo_rollout_trajectories_cut(ctypes.byref(d), ctypes.byref(c), None, None) == EINVAL
    assert _err().startswith(TRAJ + ':') and 'null len' in _err()
    assert L.drpo_rollout_trajectories_cut(ctypes.byref(d), ctypes.byref(c), ctypes.byref(_out(ret=P)), None) == EINVAL
    assert _err().startswith(TRAJ + ':') and 'ret needs weights' in _err()


# ------------------------------------------------------------------ the workspace
def _offsets(B, S, H):
    o_s, o_a = ctypes.c_size_t(), ctypes.c_size_t()
    assert _lib.lib().drpo_rollout_staging_offsets(B, S, H, ctypes.byref(o_s), ctypes.byref(o_a)) == OK
    return o_s.value, o_a.value


@pytest.mark.parametrize('B, S, H', [(72, 12, 3), (4096, 12, 10), (1, 1, 1), (1040, 12, 128), (65536, 12, 80)])
def test_staging_offsets_lie_inside_the_workspace(B, S, H):
    L = _lib.lib()
    size = L.drpo_rollout_workspace_size(B, S, H)
    count = L.drpo_rollout_count_offset(B, S, H)
    o_s, o_a = _offsets(B, S, H)
    # the count, the staged states [H][B][S], their next states (as large), the actions ([H][B][<= 8])
    assert count + 8 <= o_s
    assert o_s % 256 == 0 and o_a % 256 == 0
    assert o_s + 2 * 4 * H * B * S <= o_a
    assert o_a + 4 * H * B * 8 <= size
    # and room behind everything for the cut's lengths, [B] int32
    assert o_a + 4 * H * B * 8 + 4 * B <= size


def test_staging_offsets_refuse_bad_arguments():
    L = _lib.lib()
    o = ctypes.c_size_t()
    for B, S, H in ((0, 12, 3), (72, 0, 3), (72, 12, 0)):
        assert L.drpo_rollout_staging_offsets(B, S, H, ctypes.byref(o), ctypes.byref(o)) == EINVAL
        assert _err().startswith('drpo_rollout_staging_offsets:')
    assert L.drpo_rollout_staging_offsets(72, 12, 3, None, ctypes.byref(o)) == EINVAL


def test_count_offset_did_not_move():
    """The cut's lengths are the last piece of the workspace: every earlier offset, the row
    count's among them, is the parent commit's (the values below)."""
    L = _lib.lib()
    assert L.drpo_rollout_count_offset(72, 12, 3) == COUNT_OFFSET_72_12_3
    assert L.drpo_rollout_count_offset(4096, 12, 10) == COUNT_OFFSET_4096_12_10


# ------------------------------------------------------------------ the Python request
def _alg(**kw):
    import types
    model = types.SimpleNamespace(_elite_inds=[0, 1])
    return types.SimpleNamespace(**dict({'env_params': {'env_id': 1}, 'model_ensemble': model, 'rollout_engine': 0}, **kw))


def test_halt_request_is_checked_before_any_device():
    """ops._halt_request, the one place rollout(halt=) and imagine(halt=) are refused: on objects
    that own no device memory at all."""
    import types

    import numpy as np

    from drpo_amd import ops
    device_noise, tape = types.SimpleNamespace(parity=False), types.SimpleNamespace(parity=True)
    assert ops._halt_request(_alg(), device_noise, None, True) is None
    assert ops._halt_request(_alg(), device_noise, 0.1, True) == float(np.float32(0.1))
    assert ops._halt_request(_alg(), device_noise, math.inf, True) == math.inf
    assert ops._halt_request(_alg(), device_noise, -1, False) == -1.0
    for bad, fragment in ((math.nan, 'NaN'), (True, 'None or a float'), ('0.5', 'None or a float')):
        with pytest.raises(ValueError, match=fragment):
            ops._halt_request(_alg(), device_noise, bad, True)
    with pytest.raises(ValueError, match='host round trip'):
        ops._halt_request(_alg(env_params=None), device_noise, 0.5, True)
    with pytest.raises(ValueError, match='no elites'):
        ops._halt_request(_alg(model_ensemble=types.SimpleNamespace()), device_noise, 0.5, False)
    with pytest.raises(ValueError, match='fused engine only'):
        ops._halt_request(_alg(rollout_engine=1), device_noise, 0.5, True)
    with pytest.raises(ValueError, match='fused engine only'):
        ops._halt_request(_alg(), tape, 0.5, True, eps_layout=0)
    # a tape indexed by original row drives the fused engine; imagine never runs engine 1
    assert ops._halt_request(_alg(), tape, 0.5, True, eps_layout=1) == 0.5
    assert ops._halt_request(_alg(rollout_engine=1), tape, 0.5, False) == 0.5


def test_config_field_is_optional_and_off_when_unset():
    import drpo_amd
    cfg = drpo_amd.SMBPO.Config()
    assert isinstance(cfg.rollout_halt_threshold, drpo_amd.Optional)
    cfg.verify()
    assert cfg.rollout_halt_threshold is None
    cfg = drpo_amd.SMBPO.Config()
    cfg.update({'rollout_halt_threshold': 0.25})
    cfg.verify()
    assert cfg.rollout_halt_threshold == 0.25
    with pytest.raises(AssertionError):
        drpo_amd.SMBPO.Config().update({'rollout_halt_threshold': 'high'})


COUNT_OFFSET_72_12_3 = 8984
COUNT_OFFSET_4096_12_10 = 428880
