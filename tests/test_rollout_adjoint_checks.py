"""Gradients through imagined rollouts without a GPU: the reference of the GPU tests pinned against
autograd of the un-teacher-forced chain and a central finite difference, the struct, the version,
the path query, every refusal of drpo_rollout_adjoint (calls that fail before any launch; pointers
are dummies the host never dereferences), every Python refusal of SMBPO.imagine_vjp,
SMBPO.value_gradient and plan(refine=), and plan's argument resolution with refine off."""
import ctypes
import inspect
import math

import pytest
import torch

from drpo_amd import _abi, _lib, ops
from drpo_amd.rng import TapeNoise
from rollout_adjoint_helpers import cast_params, chain, random_params, vjp_reference
from test_host_logic import make_smbpo
from test_rollout_traj_checks import EINVAL, OK, P, _err

WHO = 'drpo_rollout_adjoint:'


# ------------------------------------------------------------------ 1. the reference
def _case(H, B=5, S=3, A=2, Hm=8, E=3, seed=0):
    gen = torch.Generator().manual_seed(seed)
    P64 = cast_params(random_params(E, S, A, Hm, gen, gain=2.0), torch.float64)
    s0 = torch.randn(B, S, generator=gen, dtype=torch.float64)
    actions = torch.rand(B, H, A, generator=gen, dtype=torch.float64) * 2 - 1
    members = [int(m) for m in torch.randint(0, E, (H,), generator=gen)]
    gs = torch.randn(B, H + 1, S, generator=gen, dtype=torch.float64)
    gr = torch.randn(B, H, generator=gen, dtype=torch.float64)
    return P64, s0, actions, members, gs, gr


def _objective(P64, s0, actions, members, gs, gr):
    states, rewards = chain(P64, s0, actions, members)
    return (gs * states).sum() + (gr * rewards).sum(), states


@pytest.mark.parametrize('H', [1, 3])
def test_reference_is_autograd_of_the_chain(H):
    """On the chain's own states the teacher-forced sweep is the chain's gradient."""
    P64, s0, actions, members, gs, gr = _case(H)
    s0g, ag = s0.clone().requires_grad_(True), actions.clone().requires_grad_(True)
    loss, states = _objective(P64, s0g, ag, members, gs, gr)
    want_s, want_a = torch.autograd.grad(loss, (s0g, ag))
    lengths = torch.full((len(s0),), H, dtype=torch.int32)
    ga, g0 = vjp_reference(P64, states.detach(), actions, lengths, members, gs, gr)
    assert float(want_a.abs().max()) > 1e-3 and float(want_s.abs().max()) > 1e-3
    assert torch.allclose(ga, want_a, rtol=1e-12, atol=1e-13) and torch.allclose(g0, want_s, rtol=1e-12, atol=1e-13)
    if H > 1:     # members differ per step, and the early steps see the later ones
        assert len(set(members)) > 1
        only_last = vjp_reference(P64, states.detach(), actions, lengths, members, None,
                                  torch.cat([torch.zeros_like(gr[:, :-1]), gr[:, -1:]], dim=1))[0]
        assert float(only_last[:, 0].abs().max()) > 0


def test_reference_against_a_central_difference():
    P64, s0, actions, members, gs, gr = _case(3, seed=1)
    H = 3
    states = chain(P64, s0, actions, members)[0]
    ga, g0 = vjp_reference(P64, states, actions, torch.full((len(s0),), H, dtype=torch.int32), members, gs, gr)
    h = 1e-6
    for (i, t, j) in [(0, 0, 0), (1, 1, 1), (4, 2, 0), (2, 0, 1)]:
        d = torch.zeros_like(actions)
        d[i, t, j] = h
        fd = (_objective(P64, s0, actions + d, members, gs, gr)[0] -
              _objective(P64, s0, actions - d, members, gs, gr)[0]) / (2 * h)
        assert abs(float(fd) - float(ga[i, t, j])) <= 1e-7 * max(1.0, abs(float(fd))), (i, t, j)
    for (i, j) in [(0, 0), (3, 2)]:
        d = torch.zeros_like(s0)
        d[i, j] = h
        fd = (_objective(P64, s0 + d, actions, members, gs, gr)[0] -
              _objective(P64, s0 - d, actions, members, gs, gr)[0]) / (2 * h)
        assert abs(float(fd) - float(g0[i, j])) <= 1e-7 * max(1.0, abs(float(fd))), (i, j)


def test_reference_lengths_and_nulls():
    """Rows that end early: a row's sweep starts at g_states[i][len], nothing beyond it is read
    (NaN there changes nothing), grad_actions beyond it is zero; a row of length 0 hands
    g_states[i][0] through; None is zeros; float32 is close to float64."""
    P64, s0, actions, members, gs, gr = _case(3, B=4, seed=2)
    H = 3
    states = chain(P64, s0, actions, members)[0]
    lengths = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    ga, g0 = vjp_reference(P64, states, actions, lengths, members, gs, gr)
    poisoned = gs.clone()
    for i, n in enumerate(lengths.tolist()):
        poisoned[i, n + 1:] = float('nan')
    gr_p = gr.clone()
    ga_p, g0_p = vjp_reference(P64, states, actions, lengths, members, poisoned, gr_p)
    assert torch.equal(ga, ga_p) and torch.equal(g0, g0_p)
    assert torch.equal(g0[0], gs[0, 0]) and not ga[0].any() and not ga[1, 1:].any() and not ga[2, 2:].any()
    assert ga[1, 0].any() and ga[2, 1].any() and ga[3, 2].any()
    # a row of length n is the full-length sweep of its first n steps
    for i, n in enumerate(lengths.tolist()):
        if n:
            sub = vjp_reference(P64, states[i:i + 1, :n + 1], actions[i:i + 1, :n], torch.tensor([n]), members[:n],
                                gs[i:i + 1, :n + 1], gr[i:i + 1, :n])
            # (other row counts, other BLAS blocking: equal to rounding, not to the bit)
            assert torch.allclose(sub[0][0], ga[i, :n], rtol=1e-12, atol=1e-14)
            assert torch.allclose(sub[1][0], g0[i], rtol=1e-12, atol=1e-14)
    z = vjp_reference(P64, states, actions, lengths, members, None, None)
    assert not z[0].any() and not z[1].any()
    a = vjp_reference(P64, states, actions, lengths, members, gs, None)
    b = vjp_reference(P64, states, actions, lengths, members, gs, torch.zeros_like(gr))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lo = vjp_reference(P64, states.float(), actions.float(), lengths, members, gs.float(), gr.float(), torch.float32)
    assert lo[0].dtype == torch.float32
    assert float((lo[0].double() - ga).abs().max()) <= 1e-4 * float(ga.abs().max())


# ------------------------------------------------------------------ 2. struct, version, path query, refusals
def test_struct_layout_version_and_path_query():
    L = _lib.lib()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert L.drpo_abi_sizeof(b'drpo_rollout_adjoint_t') == ctypes.sizeof(_abi.RolloutAdjoint) == 8 + 5 * 4 + 4 + 20 * ptr
    assert L.drpo_version() >= 17            # the version that added the entry point
    ok = lambda S, A, Hm: bool(L.drpo_rollout_adjoint_ok(S, A, Hm))
    assert ok(12, 2, 200) and ok(12, 2, 256) and ok(11, 2, 200) and ok(4, 1, 256) and ok(15, 8, 200) and ok(1, 1, 200)
    assert not ok(12, 2, 64) and not ok(12, 2, 144) and not ok(12, 2, 128) and not ok(12, 2, 0)
    assert not ok(16, 2, 200)                # S + 1 > 16
    assert not ok(0, 2, 200) and not ok(12, 0, 200) and not ok(15, 50, 200)      # S + A > 64


POINTERS = ('mW1', 'mb1', 'mW2', 'mb2', 'dW1', 'db1', 'mT1', 'mT2', 'dT1', 'dT2', 'norm_mean', 'norm_std',
            'states', 'actions', 'lengths', 'grad_actions', 'grad_start')
OPTIONAL = ('g_states', 'g_rewards')


def _desc(members=None, **kw):
    d = _abi.RolloutAdjoint()
    d.B, d.H, d.S, d.A, d.Hm, d.E = 0, 3, 12, 2, 200, 7
    for f in POINTERS + OPTIONAL:
        setattr(d, f, P)
    for k, v in kw.items():
        setattr(d, k, v)
    m = (ctypes.c_int * max(d.H, 1))(*(members if members is not None else [0] * max(d.H, 1)))
    d.members = m
    d._keep = m
    return d


def _call(d):
    return _lib.lib().drpo_rollout_adjoint(None if d is None else ctypes.byref(d), None)


def test_adjoint_refuses_null_pointers():
    assert _call(None) == EINVAL
    assert _err().startswith(WHO) and 'null descriptor' in _err()
    for f in POINTERS:
        assert _call(_desc(**{f: None})) == EINVAL, f
        assert _err().startswith(WHO) and 'null' in _err()
    d = _desc()
    d.members = None
    assert _call(d) == EINVAL and 'null members' in _err()
    for f in OPTIONAL:                       # NULL upstreams mean zeros
        assert _call(_desc(**{f: None})) == OK, f


@pytest.mark.parametrize('kw, fragment', [
    ({'H': 0}, 'H=0 outside 1..128'), ({'H': 129}, 'H=129 outside 1..128'), ({'H': -1}, 'outside 1..128'),
    ({'S': 16}, 'S + 1 <= 16'), ({'S': 0}, '1 <= S'), ({'A': 0}, '1 <= A'), ({'S': 15, 'A': 50}, 'S + A <= 64'),
    ({'Hm': 64}, '200 | 256'), ({'Hm': 144}, '200 | 256'), ({'Hm': 128}, '200 | 256'), ({'Hm': 0}, '200 | 256'),
    ({'B': -1}, 'B=-1 is negative'), ({'B': 16 * (2 ** 23 - 1) + 1}, 'exceeds one grid'), ({'B': 2 ** 40}, 'exceeds one grid'),
    ({'E': 0}, 'E=0'),
])
def test_adjoint_refuses_before_any_launch(kw, fragment):
    assert _call(_desc(**kw)) == EINVAL
    assert _err().startswith(WHO) and fragment in _err(), _err()


@pytest.mark.parametrize('members', [[0, 7, 0], [0, 0, -1], [99, 0, 0]])
def test_adjoint_refuses_a_member_outside_the_ensemble(members):
    assert _call(_desc(members=members)) == EINVAL
    assert _err().startswith(WHO) and 'outside an ensemble of 7' in _err(), _err()


def test_adjoint_of_no_row_is_ok_without_a_launch():
    for kw in ({}, {'H': 1}, {'H': 128}, {'Hm': 256}, {'S': 15, 'A': 8}, {'S': 1, 'A': 1}, {'g_states': None},
               {'g_rewards': None}):
        assert _call(_desc(**kw)) == OK, kw
    assert _call(_desc(members=[6, 0, 3])) == OK


# ------------------------------------------------------------------ 3. the Python refusals
@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


def _im(alg, B=4, H=3, members=0):
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    return ops.ImaginedRollout([members] * H if isinstance(members, int) else members, H,
                               states=z(B, H + 1, S), actions=z(B, H, A), rewards=z(B, H),
                               constraint_values=z(B, H, C), dones=z(B, H, dtype=torch.bool),
                               violations=z(B, H, dtype=torch.bool), lengths=torch.full((B,), H, dtype=torch.int32),
                               returns=z(B), max_constraint=z(B, C), first_violation=z(B, dtype=torch.int32),
                               terminated=z(B, dtype=torch.bool))


def test_imagine_vjp_refusals(alg, monkeypatch):
    calls = []
    monkeypatch.setattr(ops, '_vjp_fused', lambda *a, **k: calls.append('fused'))
    monkeypatch.setattr(ops, '_vjp_steps', lambda *a, **k: calls.append('steps'))
    im = _im(alg)
    S = alg.state_dim
    with pytest.raises(ValueError, match='one run'):
        alg.imagine_vjp(ops.ImaginedRollout.stack([im, im]))
    with pytest.raises(ValueError, match='grad_states'):
        alg.imagine_vjp(im, grad_states=torch.zeros(4, 3, S))
    with pytest.raises(ValueError, match='grad_states'):
        alg.imagine_vjp(im, grad_states=torch.zeros(5, 4, S))
    with pytest.raises(ValueError, match='grad_rewards'):
        alg.imagine_vjp(im, grad_rewards=torch.zeros(4, 4))
    with pytest.raises(ValueError, match='members'):
        alg.imagine_vjp(_im(alg, members=[0, 1]))
    with pytest.raises(ValueError, match='members'):
        alg.imagine_vjp(_im(alg, members=[0, 99, 0]))
    with pytest.raises(ValueError, match='members'):
        alg.imagine_vjp(_im(alg, members=[[0, 0, 0], [1, 1, 1]]))
    with pytest.raises(ValueError, match='path'):
        ops.rollout_vjp(alg, im, path='fast')
    assert calls == []


@pytest.fixture
def seen(monkeypatch):
    calls = []
    for name in ('plan_sample', 'plan_refit', '_terminal_critics', 'rollout_trajectories', 'lookahead', 'rollout_vjp',
                 'value_gradient', 'terminal_value_gradient'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    return calls


@pytest.mark.parametrize('kw, match', [
    ({'actions': torch.zeros(4, 2, 2)}, 'actions'),                       # K < horizon
    ({'actions': torch.zeros(4, 2)}, 'actions'),                          # [B, A] is K = 1
    ({'actions': torch.zeros(4, 3, 3)}, 'actions'),
    ({'members': None}, 'members'), ({'members': 'each'}, 'members'),
    ({'particles': [0, 1]}, 'particles'), ({'particles': 'elites'}, 'particles'),
    ({'noise': TapeNoise([])}, 'noise: a recorded tape'),
    ({'shield': True}, 'shield'), ({'shield': 'linear'}, 'shield'), ({'proposals': torch.zeros(4, 3, 2)}, 'proposals'),
    ({'halt': 0.5}, 'halt'), ({'model_noise': True}, 'model_noise'),
])
def test_value_gradient_refuses_before_any_device_work(alg, seen, kw, match):
    assert alg.action_dim == 2
    args = dict({'actions': torch.zeros(4, 3, 2), 'horizon': 3}, **kw)
    with pytest.raises(ValueError, match=match):
        alg.value_gradient(torch.zeros(4, alg.state_dim), **args)
    assert seen == [] and alg.__dict__.get('_gradient_noise') is None


@pytest.mark.parametrize('kw, match', [
    ({'refine': -1}, 'refine:'), ({'refine': 1.0}, 'refine:'), ({'refine': True}, 'refine:'),
    ({'refine_trials': 0}, 'refine_trials'), ({'refine_trials': 1024}, 'refine_trials'), ({'refine_trials': 2.0}, 'refine_trials'),
    ({'refine_step': 0.0}, 'refine_step'), ({'refine_step': -0.5}, 'refine_step'), ({'refine_step': math.inf}, 'refine_step'),
    ({'refine_step': math.nan}, 'refine_step'),
    ({'refine': 1, 'members': 0, 'steps': 2}, 'refine with steps=2'),
    ({'refine': 1}, 'refine with members=None'),
    ({'refine': 2, 'members': 0, 'model_noise': True}, 'refine with model_noise=True'),
    ({'refine': 1, 'particles': [0, 1]}, 'refine with particles='),
    ({'refine': 1, 'members': 0, 'safety_filter': True}, 'refine with safety_filter=True'),
    ({'refine': 1, 'members': 0, 'safety_filter': 'linear'}, 'refine with safety_filter='),
])
def test_plan_refine_refuses_before_any_device_work(alg, seen, kw, match):
    with pytest.raises(ValueError, match=match):
        alg.plan(torch.zeros(4, alg.state_dim), **dict({'horizon': 3, 'candidates': 8}, **kw))
    assert seen == [] and alg.__dict__.get('_plan_noise') is None
    if 'steps' not in kw:      # the controller checks the same settings once, without states
        with pytest.raises(ValueError, match=match):
            alg.mpc(**dict({'horizon': 3, 'candidates': 8}, **kw))


def test_plan_resolves_as_before_with_refine_off(alg):
    """refine=0 changes nothing of what plan's arguments resolve to; the other refine settings are
    then only checked."""
    s = torch.zeros(4, alg.state_dim)

    def resolve(**kw):
        bound = inspect.signature(alg.plan).bind(s, horizon=3, candidates=8, **kw)
        bound.apply_defaults()
        return alg._plan_checks(**bound.arguments)
    base = resolve()
    assert (base['refine'], base['refine_trials'], base['refine_step']) == (0, 8, 0.5)
    for kw in ({'refine': 0}, {'refine': 0, 'steps': 2}, {'refine': 0, 'model_noise': True},
               {'refine': 0, 'safety_filter': True}, {'refine': 0, 'particles': [0, 1]},
               {'refine_trials': 3, 'refine_step': 0.25}):
        q, want = resolve(**kw), resolve(**{k: v for k, v in kw.items() if not k.startswith('refine')})
        for k in want:
            if k.startswith('refine'):
                continue
            same = torch.equal(q[k], want[k]) if torch.is_tensor(want[k]) else q[k] == want[k]
            assert same, (kw, k)
        assert q['refine'] == 0
    on = resolve(refine=2, members=1, refine_trials=4, refine_step=0.25)
    assert (on['refine'], on['refine_trials'], on['refine_step']) == (2, 4, 0.25)
    assert ops.PlanResult.REFINE_FIELDS == ('refine_score', 'refine_accepted', 'refine_gradient')
    r = ops.PlanResult(**dict.fromkeys(ops.PlanResult.FIELDS, 0))
    assert r.refine_score is None and r.refine_accepted is None and r.refine_gradient is None
