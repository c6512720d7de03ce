"""drpo_rollout_adjoint (ops.rollout_vjp) against float64 autograd, the fused kernel and the
per-step path each.

Reference and tolerance: rollout_adjoint_helpers (vjp_reference teacher-forced at the stored
float32 states in float64, the same sweep in float32 for the bound's e32; check: the bound of
tests/test_gpu_mlp_shapes.py::check, max|got - ref64| <= max(4 e32, 32 * 2^-24 scale), and at
H = 1 every element within 1e-4 + 1e-4 |ref| too).

Shapes: B 1, 16, 17, 33 (one row, a full tile, a partial second tile, three tiles) x H 1, 2, 5 x
hidden 200 and 256 on quadrotor (S 12, A 2) and point-robot (S 11, A 2) dimensions, random
upstreams, members all equal and different per step. The nets are gpu_helpers._width_alg's with
the four weight matrices of the mean path scaled by 3 (raw initial weights all but ignore their
input: imagine_helpers) and a random normalizer. The rows that end early come from an imagine
run of imagine_helpers._action_scene whose rows die at every step, and from its imagine(halt=) twin.

Measured on an MI355X (a run with -s prints err / bound per tensor), the largest err / bound:
    fused   0.65      steps   0.57      fused against steps 0.54
The 4x margin was not needed."""
import pytest
import torch

import drpo_amd
from drpo_amd import ops
from gpu_helpers import DEV, _width_alg
from imagine_helpers import _action_scene
from rollout_adjoint_helpers import PRE, check, vjp_reference

gpu = pytest.mark.gpu

GAIN = 3.0
ROWS, HORIZONS = [1, 16, 17, 33], [1, 2, 5]
NETS = [('quadrotor', 200), ('quadrotor', 256), ('point-robot', 200), ('point-robot', 256)]
MEASURED = {'fused': [0.0], 'steps': [0.0], 'fused against steps': [0.0]}
_ALGS = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k, v in MEASURED.items():
        print(f'\nMEASURED {k}: max err / bound = {v[0]:.3f}')


def _alg(env, mh):
    """(trainer, its model's parameters on the CPU as the oracle names them), one per net: leave it as it is."""
    if (env, mh) not in _ALGS:
        alg = _width_alg(env, 64, mh)
        m = alg.model_ensemble
        gen = torch.Generator().manual_seed(3)
        m.state_normalizer.mean.copy_(torch.randn(alg.state_dim, generator=gen) * 0.1)
        m.state_normalizer.std.copy_(torch.rand(alg.state_dim, generator=gen) + 0.5)
        trunk, diff, _ = m.views()
        for W in (trunk[0][0], trunk[1][0], diff[0][0], diff[1][0]):
            W.mul_(GAIN)
        P = {k: v.detach().cpu().clone() for k, v in alg.state_dict().items() if k.startswith(PRE)}
        _ALGS[(env, mh)] = (alg, P)
    return _ALGS[(env, mh)]


def make_im(alg, states, actions, lengths, members):
    """An ImaginedRollout around the tensors the adjoint reads; everything else zero."""
    B, H, _ = actions.shape
    C = alg.con_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    return ops.ImaginedRollout(list(members), H, states=states.to(DEV), actions=actions.to(DEV), rewards=z(B, H),
                               constraint_values=z(B, H, C), dones=z(B, H, dtype=torch.bool),
                               violations=z(B, H, dtype=torch.bool), lengths=lengths.to(DEV), returns=z(B),
                               max_constraint=z(B, C), first_violation=z(B, dtype=torch.int32),
                               terminated=z(B, dtype=torch.bool))


def _inputs(alg, B, H, seed):
    gen = torch.Generator().manual_seed(seed)
    S, A = alg.state_dim, alg.action_dim
    states = torch.randn(B, H + 1, S, generator=gen)
    actions = torch.rand(B, H, A, generator=gen) * 2 - 1
    gs = torch.randn(B, H + 1, S, generator=gen)
    gr = torch.randn(B, H, generator=gen)
    return states, actions, torch.full((B,), H, dtype=torch.int32), gs, gr


def _dev(x):
    return None if x is None else x.to(DEV)


def _run(alg, im, gs, gr, path):
    out = ops.rollout_vjp(alg, im, _dev(gs), _dev(gr), path=path)
    torch.cuda.synchronize()
    return out


def _refs(P, states, actions, lengths, members, gs, gr):
    r64 = vjp_reference(P, states, actions, lengths, members, gs, gr, torch.float64)
    r32 = vjp_reference(P, states, actions, lengths, members, gs, gr, torch.float32)
    return r64, r32


def _check_all(tag, alg, P, states, actions, lengths, members, gs, gr, ceiling):
    """fused and steps against ref64, and fused against steps, each within the bound."""
    r64, r32 = _refs(P, states, actions, lengths, members, gs, gr)
    assert float(r64[0].abs().max()) > 1e-3, 'the scene shows nothing: a zero gradient'
    im = make_im(alg, states, actions, lengths, members)
    got = {}
    for path in ('fused', 'steps'):
        got[path] = _run(alg, im, gs, gr, path)
        for name, g, a, b in zip(('grad_actions', 'grad_start'), got[path], r64, r32):
            check(f'{tag} {path} {name}', g, a, b, ceiling=ceiling, measured=MEASURED[path])
    _check_pair(tag, got['fused'], got['steps'], r64, r32)
    return got


def _check_pair(tag, fused, steps, r64, r32):
    """fused against steps under the same bound (e32 and the scale's floor as against ref64)"""
    for name, f, s, a, b in zip(('grad_actions', 'grad_start'), fused, steps, r64, r32):
        s = s.detach().double().cpu()
        check(f'{tag} fused against steps {name}', f, s, s + (b.double() - a), measured=MEASURED['fused against steps'])


@gpu
@pytest.mark.parametrize('H', HORIZONS)
@pytest.mark.parametrize('B', ROWS)
@pytest.mark.parametrize('env, mh', NETS)
def test_adjoint_against_float64(env, mh, B, H):
    alg, P = _alg(env, mh)
    assert ops.rollout_adjoint_ok(alg)
    E = alg.model_ensemble.ensemble_size
    states, actions, lengths, gs, gr = _inputs(alg, B, H, 1000 * B + H)
    vary = [(2 * t + 1) % E for t in range(H)]
    assert H == 1 or len(set(vary)) > 1
    _check_all(f'{env} {mh} B{B} H{H} members vary', alg, P, states, actions, lengths, vary, gs, gr, H == 1)
    if B == 17:
        _check_all(f'{env} {mh} B{B} H{H} members same', alg, P, states, actions, lengths, [E - 1] * H, gs, gr, H == 1)


def _bits(x):
    return x.detach().cpu().view(torch.int32)


@gpu
@pytest.mark.parametrize('path', ['fused', 'steps'])
def test_null_upstreams_are_zeros_and_the_vjp_is_linear(path):
    alg, P = _alg('quadrotor', 200)
    B, H = 33, 5
    states, actions, lengths, gs, gr = _inputs(alg, B, H, 77)
    lengths = torch.tensor([(5 * i) % (H + 1) for i in range(B)], dtype=torch.int32)
    im = make_im(alg, states, actions, lengths, [0, 1, 2, 1, 0])
    for a, b in (((None, gr), (torch.zeros_like(gs), gr)), ((gs, None), (gs, torch.zeros_like(gr))),
                 ((None, None), (torch.zeros_like(gs), torch.zeros_like(gr)))):
        x, y = _run(alg, im, *a, path), _run(alg, im, *b, path)
        assert torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[1]), _bits(y[1]))
    none = _run(alg, im, None, None, path)
    assert not none[0].any() and not none[1].any()
    # scaling the upstream by a power of two is exact
    one, two = _run(alg, im, gs, gr, path), _run(alg, im, 2 * gs, 2 * gr, path)
    assert one[0].any()
    assert torch.equal(_bits(2 * one[0]), _bits(two[0])) and torch.equal(_bits(2 * one[1]), _bits(two[1]))


def _guarded(shape, guard=64):
    n = 1
    for d in shape:
        n *= d
    base = torch.full((n + 2 * guard,), float('nan'), device=DEV)
    return base, base[guard:guard + n].view(*shape)


@gpu
@pytest.mark.parametrize('B, H', [(1, 1), (17, 2), (33, 5)])
def test_every_element_is_written_and_nothing_else(B, H):
    alg, P = _alg('point-robot', 256)
    S, A = alg.state_dim, alg.action_dim
    states, actions, lengths, gs, gr = _inputs(alg, B, H, 5 * B + H)
    lengths = torch.tensor([(3 * i + H) % (H + 1) for i in range(B)], dtype=torch.int32)
    args = ops._vjp_inputs(alg, make_im(alg, states, actions, lengths, [1] * H), gs.to(DEV), gr.to(DEV))
    (ba, ga), (b0, g0) = _guarded((B, H, A)), _guarded((B, S))
    ops._vjp_fused(alg, *args, out=(ga, g0))
    torch.cuda.synchronize()
    for base, inner in ((ba, ga), (b0, g0)):
        assert torch.isfinite(inner).all()
        assert torch.isnan(base[:64]).all() and torch.isnan(base[64 + inner.numel():]).all()
    im = make_im(alg, states, actions, lengths, [1] * H)
    free = ops.rollout_vjp(alg, im, gs.to(DEV), gr.to(DEV), path='fused')
    assert torch.equal(_bits(free[0]), _bits(ga)) and torch.equal(_bits(free[1]), _bits(g0))
    r64, r32 = _refs(P, states, actions, lengths, [1] * H, gs, gr)
    steps = _run(alg, im, gs, gr, 'steps')
    for name, f, s, a, b in zip(('grad_actions', 'grad_start'), (ga, g0), steps, r64, r32):
        check(f'guarded B{B} H{H} fused {name}', f, a, b, ceiling=H == 1, measured=MEASURED['fused'])
        check(f'guarded B{B} H{H} steps {name}', s, a, b, ceiling=H == 1, measured=MEASURED['steps'])
    _check_pair(f'guarded B{B} H{H}', (ga, g0), steps, r64, r32)


def _take(im, idx):
    idx = torch.as_tensor(idx, device=DEV)
    return ops.ImaginedRollout(im.members, im.given_steps,
                               **{k: getattr(im, k).index_select(0, idx).contiguous() for k in im.TENSORS})


@gpu
def test_rows_that_end_early():
    """Rows of an imagine run whose rows die at every step and of its imagine(halt=) twin: one tile
    with lengths 0 (halted at step 0), 1, H-1 and H, then a tile whose rows are all dead. g_states
    beyond a row's length is NaN."""
    alg, rep, P = _action_scene(DEV)
    B, H = 72, 3
    S, A = alg.state_dim, alg.action_dim
    assert ops.rollout_adjoint_ok(alg)
    gen = torch.Generator().manual_seed(8)
    start = torch.from_numpy(rep['states'][2:400:5][:B].copy())
    given = torch.rand(B, H, A, generator=gen) * 2 - 1
    members = [3, 0, 6]
    kw = dict(actions=given, members=members, deterministic=True, model_noise=False)
    first = alg.imagine(start, horizon=H, uncertainty=True, noise=drpo_amd.DeviceNoise(1), **kw)
    thr = float(first.disagreement[:, 0].median())
    halted = alg.imagine(start, horizon=H, halt=thr, noise=drpo_amd.DeviceNoise(1), **kw)
    # the pool: the dying rows of the unhalted run (lengths 1..H), then the halted run's (0..H-1)
    im = ops.ImaginedRollout(members, H, **{k: torch.cat([getattr(first, k), getattr(halted, k)]) for k in first.TENSORS})
    assert bool((halted.halted_at == 0).any()) and not first.lengths.eq(0).any()
    lens = im.lengths.cpu()
    by_len = {n: torch.nonzero(lens == n).flatten().tolist() for n in range(H + 1)}
    print('lengths of the pool:', {n: len(v) for n, v in by_len.items()})
    assert all(by_len[n] for n in (0, 1, H - 1, H)), 'the scene must show rows of length 0, 1, H-1 and H'
    tile = [i for n in (0, 1, 2, 3) for i in by_len[n][:4]]
    tile = (tile * 16)[:16]
    rows = tile + by_len[0][:1] * 16
    sub = _take(im, rows)
    n = len(rows)
    assert set(sub.lengths[:16].tolist()) == {0, 1, 2, 3} and not sub.lengths[16:].any()
    gs = torch.randn(n, H + 1, S, generator=gen)
    gr = torch.randn(n, H, generator=gen)
    for i, ln in enumerate(sub.lengths.tolist()):
        gs[i, ln + 1:] = float('nan')
    states, actions, lengths = sub.states.cpu(), sub.actions.cpu(), sub.lengths.cpu()
    r64, r32 = _refs(P, states, actions, lengths, members, gs, gr)
    got = {}
    for path in ('fused', 'steps'):
        ga, g0 = got[path] = _run(alg, sub, gs, gr, path)
        check(f'early rows {path} grad_actions', ga, r64[0], r32[0], measured=MEASURED[path])
        check(f'early rows {path} grad_start', g0, r64[1], r32[1], measured=MEASURED[path])
        ga, g0 = ga.cpu(), g0.cpu()
        for i, ln in enumerate(lengths.tolist()):
            assert not ga[i, ln:].any(), (path, i, ln)                     # exactly zero beyond the length
            assert ln == 0 or ga[i, :ln].any()
        assert torch.equal(_bits(g0[16:]), _bits(gs[16:, 0]))              # the dead tile: g_states[:, 0]
        assert not ga[16:].any()
    _check_pair('early rows', got['fused'], got['steps'], r64, r32)


@gpu
@pytest.mark.parametrize('mh', [64, 144])
def test_other_widths_take_the_steps_path(mh, monkeypatch):
    """(No fused run to compare with at these widths: the entry point refuses them.)"""
    alg, P = _alg('quadrotor', mh)
    assert not ops.rollout_adjoint_ok(alg)
    B, H = 17, 2
    states, actions, lengths, gs, gr = _inputs(alg, B, H, mh)
    members = [2, 0]
    im = make_im(alg, states, actions, lengths, members)
    with pytest.raises(ValueError, match="path='fused'"):
        ops.rollout_vjp(alg, im, path='fused')
    monkeypatch.setattr(ops, '_vjp_fused', lambda *a, **k: pytest.fail('the fused kernel ran at an unadmitted width'))
    got = _run(alg, im, gs, gr, None)
    r64, r32 = _refs(P, states, actions, lengths, members, gs, gr)
    check(f'width {mh} grad_actions', got[0], r64[0], r32[0], measured=MEASURED['steps'])
    check(f'width {mh} grad_start', got[1], r64[1], r32[1], measured=MEASURED['steps'])
    # SMBPO.imagine_vjp is the same call
    via = alg.imagine_vjp(im, gs.to(DEV), gr.to(DEV))
    assert torch.equal(_bits(via[0]), _bits(got[0])) and torch.equal(_bits(via[1]), _bits(got[1]))
