"""The host path that ops.rollout and ops.rollout_trajectories share, no GPU: the order in which
it consumes a noise object (_start_states, _members_and_draws), the members check, the shield
request (_shield_request and the shorthand SMBPO.imagine translates for it),
ImaginedRollout.stack over the optional groups, and the descriptor cache (_rollout_static)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drpo_amd
from drpo_amd import ops
from test_host_logic import make_smbpo

S, A, B, H = 4, 2, 5, 3
ELITES = [4, 1, 6]


class RecordingNoise:
    """A device-noise stand-in that logs every call a rollout may make on it."""
    parity = False

    def __init__(self):
        self.log = []

    @property
    def seed(self):
        self.log.append(('seed',))
        return 7

    def np_choice(self, high, size):
        self.log.append(('np_choice', high, size))

    def choice(self, n):
        self.log.append(('choice', n))
        return len(self.log) % n

    def next(self):
        self.log.append(('next',))
        return 1


def _stubs(pointer=8, capacity=10):
    rb = SimpleNamespace(_states=torch.zeros(capacity, S), pointer=pointer, capacity=capacity)
    alg = SimpleNamespace(replay_buffer=SimpleNamespace(_module=rb), rollout_batch_size=B, state_dim=S)
    return alg, SimpleNamespace(_elite_inds=list(ELITES), ensemble_size=7)


# ------------------------------------------------------------------ 1. noise order
def test_noise_order_without_start_states_and_members():
    alg, model = _stubs()
    noise = RecordingNoise()
    src, ptr, cap, init_idx, b = ops._start_states(alg, None, noise, 'cpu')
    assert src is alg.replay_buffer._module._states and (ptr, cap, init_idx, b) == (8, 10, None, B)
    members, counts, eps_a, eps_m = ops._members_and_draws(model, noise, H, B, A, S + 1, 'cpu')
    assert noise.log == [('np_choice', 8, B)] + [('choice', 3)] * H
    assert len(members) == H and set(members) <= set(ELITES) and counts is None and eps_a is None and eps_m is None
    # a full buffer offers its capacity
    alg, _ = _stubs(pointer=13)
    noise = RecordingNoise()
    ops._start_states(alg, None, noise, 'cpu')
    assert noise.log == [('np_choice', 10, B)]


def test_noise_order_with_start_states_and_members():
    alg, model = _stubs()
    noise = RecordingNoise()
    s = torch.arange(7 * S, dtype=torch.float64).reshape(7, S)
    src, ptr, cap, init_idx, b = ops._start_states(alg, s, noise, 'cpu')
    assert src.dtype == torch.float32 and torch.equal(src, s.float()) and (ptr, cap, b) == (7, 7, 7)
    assert init_idx.dtype == torch.int64 and init_idx.tolist() == list(range(7))
    members, counts, eps_a, eps_m = ops._members_and_draws(model, noise, H, 7, A, S + 1, 'cpu', members=2)
    assert members == [2] * H and counts is None and eps_a is None and eps_m is None
    assert noise.log == []
    with pytest.raises(AssertionError, match='state_dim'):
        ops._start_states(alg, torch.zeros(7, S + 1), noise, 'cpu')
    with pytest.raises(AssertionError, match='state_dim'):
        ops._start_states(alg, torch.zeros(S), noise, 'cpu')


def _tape(rows, picks):
    g = np.random.RandomState(3)
    entries = []
    for n, k in zip(rows, picks):
        entries += [('normal', g.randn(n, A).astype(np.float32)), ('choice', k),
                    ('randn_like', g.randn(n, S + 1).astype(np.float32))]
    return entries


def test_tape_supplies_members_counts_and_zero_padded_draws():
    _, model = _stubs()
    entries = _tape([5, 4, 2], [2, 0, 1])
    tape = drpo_amd.TapeNoise(entries)
    members, counts, eps_a, eps_m = ops._members_and_draws(model, tape, H, B, A, S + 1, 'cpu')
    assert tape.done()
    assert members == [ELITES[2], ELITES[0], ELITES[1]] and counts == [5, 4, 2]
    assert eps_a.shape == (H, B, A) and eps_m.shape == (H, B, S + 1) and eps_a.dtype == eps_m.dtype == torch.float32
    for t, n in enumerate(counts):
        assert np.array_equal(eps_a[t, :n].numpy(), entries[3 * t][1])
        assert np.array_equal(eps_m[t, :n].numpy(), entries[3 * t + 2][1])
        assert not eps_a[t, n:].any() and not eps_m[t, n:].any()
    with pytest.raises(AssertionError, match='a tape supplies its own'):
        ops._members_and_draws(model, drpo_amd.TapeNoise(entries), H, B, A, S + 1, 'cpu', members=2)


def test_short_tape_pads_the_members_with_0():
    _, model = _stubs()
    tape = drpo_amd.TapeNoise(_tape([5, 4], [1, 2]))
    members, counts, eps_a, eps_m = ops._members_and_draws(model, tape, H, B, A, S + 1, 'cpu')
    assert tape.done() and members == [ELITES[1], ELITES[2], 0] and counts == [5, 4]
    assert not eps_a[2].any() and not eps_m[2].any() and bool(eps_a[1, :4].any())


# ------------------------------------------------------------------ 2. members
def test_members_check():
    _, model = _stubs()
    E = model.ensemble_size
    for bad in (E, -1, np.bool_(True), '1', None, 1.0, np.float32(1), [0, 1.0, 2], [0, E, 2]):
        with pytest.raises(ValueError, match='not a member index'):
            ops._traj_members(model, [bad] * H if not isinstance(bad, list) else bad, H)
    for bad in (E, -1, 1.0):                                   # a single value stands for every step
        with pytest.raises((ValueError, TypeError)):
            ops._traj_members(model, bad, H)
    for bad in ([0] * (H - 1), [0] * (H + 1), []):
        with pytest.raises(ValueError, match=f'entries for horizon {H}'):
            ops._traj_members(model, bad, H)
    got = ops._traj_members(model, np.int64(3), H)
    assert got == [3] * H and all(type(m) is int for m in got)
    got = ops._traj_members(model, np.array([0, 6, 2], np.int32), H)
    assert got == [0, 6, 2] and all(type(m) is int for m in got)
    assert ops._traj_members(model, (5, 0, 5), H) == [5, 0, 5]


# ------------------------------------------------------------------ 3. the shield request
DEVICE, TAPE = RecordingNoise(), drpo_amd.TapeNoise([])
ACTIONS = torch.zeros(B, 1, A)
# (distributional critic, noise, actions, shield, candidates, uncertainty) -> (threshold, candidates, dist) or the text
REQUESTS = [
    ((True, DEVICE, None, None, None, None), None),
    ((True, TAPE, ACTIONS, None, None, None), None),
    ((True, DEVICE, None, 0.5, None, None), (0.5, None, True)),         # the threshold shield: distributional_qc
    ((False, DEVICE, None, 0.5, None, None), (0.5, None, False)),
    ((True, DEVICE, None, 0.5, None, False), (0.5, None, False)),       # an explicit value overrides it
    ((True, DEVICE, None, 0.5, 11, None), (0.5, 11, False)),            # the linear shield: the mean
    ((False, DEVICE, None, 0.5, 11, None), (0.5, 11, False)),
    ((True, DEVICE, None, 0.5, 11, True), (0.5, 11, True)),
    ((True, DEVICE, None, -float('inf'), 2, None), (-float('inf'), 2, False)),
    ((True, DEVICE, None, 1, np.int64(32), 1), (1.0, 32, True)),
    ((True, DEVICE, ACTIONS, 0.5, None, None), 'shield with actions'),
    ((True, DEVICE, ACTIONS, 0.0, 5, None), 'shield with actions'),
    ((True, TAPE, None, 0.0, None, None), 'shield with a recorded tape'),
    ((True, TAPE, None, 0.0, 11, None), 'shield with a recorded tape'),
    ((True, DEVICE, None, 0.0, 1, None), 'shield_candidates'),
    ((True, DEVICE, None, 0.0, 33, None), 'shield_candidates'),
    ((True, DEVICE, None, 0.0, 0, None), 'shield_candidates'),
    ((True, DEVICE, None, 0.0, 11.0, None), 'shield_candidates'),
    ((True, DEVICE, None, 0.0, True, None), 'shield_candidates'),
    ((True, DEVICE, None, None, None, True), 'shield_uncertainty without shield'),
    ((True, DEVICE, None, None, None, False), 'shield_uncertainty without shield'),
    ((True, DEVICE, None, None, 11, None), 'without shield'),
    ((False, DEVICE, None, 0.0, None, True), 'not distributional'),
    ((False, DEVICE, None, 0.0, 11, True), 'not distributional'),
]


@pytest.mark.parametrize('args,want', REQUESTS, ids=[str(i) for i in range(len(REQUESTS))])
def test_shield_request(args, want):
    alg = SimpleNamespace(solver=SimpleNamespace(distributional_qc=args[0]))
    if isinstance(want, str):
        with pytest.raises(ValueError, match=want):
            ops._shield_request(alg, *args[1:])
        return
    got = ops._shield_request(alg, *args[1:])
    assert got == want
    if want is not None:
        assert type(got[0]) is float and type(got[2]) is bool and (got[1] is None or type(got[1]) is int)


@pytest.fixture(scope='module')
def alg():
    return make_smbpo('point-robot')


def test_imagine_translates_the_shield_shorthand(alg, monkeypatch):
    """SMBPO.imagine hands ops a threshold and a candidate count, and shield_uncertainty as given."""
    seen = []
    monkeypatch.setattr(ops, 'rollout_trajectories', lambda *a, **kw: seen.append(kw))
    s = torch.zeros(4, alg.state_dim)
    thr = float(alg.safe_shield_threshold)
    for shield, want in [(None, (None, None)), (False, (None, None)), (True, (thr, None)), (0.25, (0.25, None)),
                         (0, (0.0, None)), ('linear', (thr, 11)), (('linear',), (thr, 11)),
                         (('linear', 0.5), (0.5, 11)), (('linear', 0.5, 5), (0.5, 5)),
                         (['linear', None, None], (thr, 11)), (('linear', None, 33), (thr, 33))]:
        for unc in (None, False, True):
            seen.clear()
            alg.imagine(s, shield=shield, shield_uncertainty=unc)
            kw = seen[0]
            assert (kw.get('shield'), kw.get('shield_candidates')) == want, shield
            assert kw['shield_uncertainty'] is unc
    for bad in ('safe', 'Linear', '', ('safe', 0.0), (), ('linear', 0.0, 11, 1)):
        with pytest.raises(ValueError, match='shield: '):
            alg.imagine(s, shield=bad)


# ------------------------------------------------------------------ 4. ImaginedRollout.stack
GROUPS = ops.ImaginedRollout.GROUPS
SCALARS = {'shield_threshold': 0.5, 'shield_candidates': 11}


def _run(seed, groups):
    g = torch.Generator().manual_seed(seed)

    def rand(shape, dtype):
        x = torch.rand(shape, generator=g)
        return x if dtype == torch.float32 else (x * 3).to(dtype)
    im = ops.ImaginedRollout([seed] * H, 1, **{name: rand(shape, dt) for name, shape, dt, _ in
                                               ops._traj_spec(2, H, S, A, 2)})
    im.lengths = torch.tensor([H, 2], dtype=torch.int32)
    shapes = {'max_disagreement': (2,)}
    dtypes = {'interventions': torch.bool, 'blend': torch.uint8}
    for group in groups:
        per_run, scalars = GROUPS[group]
        im.set_group(group, **{k: rand(shapes.get(k, (2, H)), dtypes.get(k, torch.float32)) for k in per_run},
                     **{k: SCALARS[k] for k in scalars})
    return im


@pytest.mark.parametrize('groups', [(), ('shield',), ('linear',), ('uncertainty',), tuple(GROUPS)],
                         ids=lambda g: '+'.join(g) or 'none')
def test_stack(groups):
    runs = [_run(seed, groups) for seed in (1, 2, 3)]
    out = ops.ImaginedRollout.stack(runs)
    assert out.members == [[1] * H, [2] * H, [3] * H] and out.given_steps == 1
    for k in ops.ImaginedRollout.TENSORS:
        assert torch.equal(getattr(out, k), torch.stack([getattr(r, k) for r in runs])), k
    for group, (per_run, scalars) in GROUPS.items():
        for k in per_run:
            want = torch.stack([getattr(r, k) for r in runs]) if group in groups else None
            got = getattr(out, k)
            assert (got is None) if want is None else (got.dtype == want.dtype and torch.equal(got, want)), k
        for k in scalars:
            assert getattr(out, k) == (SCALARS[k] if group in groups else None), k
    assert out.mask.shape == (3, 2, H) and torch.equal(out.mask, torch.stack([r.mask for r in runs]))
    if 'uncertainty' in groups:
        for thr in (-1.0, 0.5, 2.0):
            assert torch.equal(out.first_uncertain(thr), torch.stack([r.first_uncertain(thr) for r in runs]))
    else:
        with pytest.raises(ValueError, match='first_uncertain needs'):
            out.first_uncertain(0.5)


def test_a_group_is_set_whole():
    im = _run(1, ())
    with pytest.raises(AssertionError):
        im.set_group('shield', interventions=torch.zeros(2, H, dtype=torch.bool))
    with pytest.raises(KeyError):
        im.set_group('shields')


# ------------------------------------------------------------------ 5. the descriptor cache
def test_descriptor_cache(alg, monkeypatch):
    built = []
    build = ops._rollout_desc

    def counted(alg, policy, B, H, ws_name):
        built.append(ws_name)
        return build(alg, policy, B, H, ws_name)
    monkeypatch.setattr(ops, '_rollout_desc', counted)
    monkeypatch.setattr(alg, '_ws', {})
    for name in ('_rollout_desc_cache', '_rollout_traj_desc_cache'):
        monkeypatch.setitem(alg.__dict__, name, {})
    for buffer, cache, prefix in ((True, '_rollout_desc_cache', 'rollout.'), (False, '_rollout_traj_desc_cache',
                                                                              'rollout_traj.')):
        built.clear()
        first = ops._rollout_static(alg, alg.actor, 16, H, buffer)
        assert ops._rollout_static(alg, alg.actor, 16, H, buffer) is first and built == [f'{prefix}16.{H}']
        d, members, count, _ = first
        assert (d.B, d.H, len(members)) == (16, H, H)
        if buffer:
            assert d.vs == alg.virt_buffer._module._states.data_ptr()
            assert count.dtype == torch.int64 and count.dim() == 0
        else:
            assert not d.vs and not d.vptr and count is None
        for b in range(17, 24):                                   # a changed B builds again: 8 entries
            assert ops._rollout_static(alg, alg.actor, b, H, buffer)[0].B == b
        assert len(built) == 8 and len(alg.__dict__[cache]) == 8
        assert ops._rollout_static(alg, alg.actor, 16, H, buffer) is first and len(built) == 8
        ops._rollout_static(alg, alg.actor, 16, H + 1, buffer)    # the ninth key clears the cache
        assert len(built) == 9 and len(alg.__dict__[cache]) == 1
        assert ops._rollout_static(alg, alg.actor, 16, H, buffer) is not first and len(built) == 10
    # the two entries never share a descriptor or a workspace
    a, b = (ops._rollout_static(alg, alg.actor, 16, H, buffer)[0] for buffer in (True, False))
    assert a is not b and a.workspace != b.workspace
    names = set(alg._ws)
    assert f'rollout.16.{H}' in names and f'rollout_traj.16.{H}' in names
    assert all(n.startswith(('rollout.', 'rollout_traj.')) for n in names)
