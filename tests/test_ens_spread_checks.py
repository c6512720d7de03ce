"""Host-side checks of drpo_ens_spread (csrc/ensemble.hip) and the Python refusals of
BatchedGaussianEnsemble.disagreement and imagine(uncertainty=), no GPU: every call here is
refused before any launch. The pointers are dummies that are never followed."""
import ctypes

import pytest
import torch

from drpo_amd import _abi, _lib
from test_host_logic import make_smbpo

WHO = 'drpo_ens_spread:'
EINVAL = 1          # DRPO_EINVAL
P = 0x1000          # a non-null pointer; no refused call reads through it
OUTPUTS = ('mean', 'epistemic_std', 'aleatoric_std', 'disagreement', 'epistemic', 'aleatoric')


def _desc(**kw):
    d = _abi.EnsSpread()
    d.D = d.LVR = d.s = d.minlv = d.maxlv = d.zsel = d.scale = P
    d.n, d.S, d.Z, d.M = 8, 3, 7, 5
    for k in OUTPUTS:
        setattr(d, k, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(d):
    return _lib.lib().drpo_ens_spread(None if d is None else ctypes.byref(d), None)


def _err():
    return _lib.lib().drpo_last_error().decode()


def test_struct_layout_and_version():
    L = _lib.lib()
    assert L.drpo_abi_sizeof(b'drpo_ens_spread_t') == ctypes.sizeof(_abi.EnsSpread)
    assert L.drpo_version() >= 10            # the version that added the entry point


@pytest.mark.parametrize('M', [0, 33, -1])
def test_refuses_members_outside_1_to_32(M):
    assert _call(_desc(M=M)) == EINVAL
    assert _err() == f'{WHO} members M outside 1..32'


def test_refuses_null_arguments():
    assert _call(None) == EINVAL
    assert _err() == f'{WHO} null descriptor'
    assert _call(_desc(D=None)) == EINVAL
    assert _err() == f'{WHO} null D'
    assert _call(_desc(s=None)) == EINVAL
    assert _err().startswith(WHO) and 'mean needs s' in _err()
    for k in ('minlv', 'maxlv'):
        assert _call(_desc(**{k: None})) == EINVAL
        assert _err().startswith(WHO) and 'minlv and maxlv' in _err()


@pytest.mark.parametrize('out', ['aleatoric_std', 'aleatoric'])
def test_refuses_an_aleatoric_output_without_lvr(out):
    keep = {k: None for k in OUTPUTS if k != out}
    assert _call(_desc(LVR=None, **keep)) == EINVAL
    assert _err().startswith(WHO) and 'needs LVR' in _err()


def test_lvr_and_bounds_may_be_null_without_an_aleatoric_output():
    # through those checks to a later refusal
    d = _desc(LVR=None, minlv=None, maxlv=None, aleatoric_std=None, aleatoric=None, M=0)
    assert _call(d) == EINVAL
    assert _err() == f'{WHO} members M outside 1..32'
    d = _desc(s=None, mean=None, M=0)
    assert _call(d) == EINVAL
    assert _err() == f'{WHO} members M outside 1..32'


def test_refuses_no_output():
    assert _call(_desc(**{k: None for k in OUTPUTS})) == EINVAL
    assert _err() == f'{WHO} no output requested'


@pytest.mark.parametrize('kw', [dict(n=-1), dict(S=0), dict(Z=0)])
def test_refuses_bad_sizes(kw):
    assert _call(_desc(**kw)) == EINVAL
    assert _err().startswith(WHO) and 'out of range' in _err()


def test_refuses_more_than_32_members_without_zsel():
    assert _call(_desc(zsel=None, Z=33, M=32)) == EINVAL
    assert _err().startswith(WHO) and 'zsel NULL with Z=33 > 32' in _err()
    assert _call(_desc(zsel=None, Z=7, M=5)) == EINVAL          # NULL is members 0..Z-1
    assert _err().startswith(WHO) and 'M=5, Z=7' in _err()


@pytest.mark.parametrize('kw', [dict(), dict(zsel=None, M=7), dict(S=300), dict(M=32, Z=64)])
def test_no_rows_is_ok_without_a_launch(kw):
    assert _call(_desc(n=0, **kw)) == 0


# ------------------------------------------------------------------ Python
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


def test_python_refusals(alg):
    """Each is a ValueError raised before anything touches a device (the trainer is on the
    CPU here: a call that got further would raise DrpoError, not ValueError)."""
    m = alg.model_ensemble
    E, S, A = m.ensemble_size, alg.state_dim, alg.action_dim
    s, a = torch.zeros(4, S), torch.zeros(4, A)
    for bad in ('elite', 'ALL', [], [E], [-1], [0] * 33):
        with pytest.raises(ValueError, match='disagreement: '):
            m.disagreement(s, a, members=bad)
    assert '_elite_inds' not in m.__dict__                       # never fitted: no elites to default to
    with pytest.raises(ValueError, match='no elites'):
        m.disagreement(s, a)
    for n in (S - 1, S + 2, 1):
        with pytest.raises(ValueError, match='scale has'):
            m.disagreement(s, a, members='all', scale=torch.ones(n))
    for bad in ('x', 'elites', 1.5, 2):
        with pytest.raises(ValueError, match='uncertainty: '):
            alg.imagine(s, uncertainty=bad)


def test_a_valid_call_gets_past_the_refusals(alg):
    """... and stops where the compute path asks for device tensors."""
    m = alg.model_ensemble
    s, a = torch.zeros(4, alg.state_dim), torch.zeros(4, alg.action_dim)
    for kw in (dict(members='all'), dict(members=[0, 0, 2]), dict(members=range(m.ensemble_size)),
               dict(members='all', scale=torch.ones(alg.state_dim)),
               dict(members='all', scale=torch.ones(alg.state_dim + 1))):
        with pytest.raises(_lib.DrpoError, match='no CPU fallback'):
            m.disagreement(s, a, **kw)
    for u in (True, 'all', False, None):
        with pytest.raises(_lib.DrpoError, match='no CPU fallback'):
            alg.imagine(s, uncertainty=u)
