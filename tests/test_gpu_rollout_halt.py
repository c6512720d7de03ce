"""Halting rollouts where the ensemble disagrees: ops._cut_trajectories, SMBPO.imagine(halt=) and
SMBPO.rollout(halt=) (drpo_rollout_trajectories_cut, drpo_rollout_stage, drpo_rollout_emit_cut).

Scenes (imagine_helpers): _scene(16) / _scene(32), B 72, H 3, natural lengths 1, 2, 3 and a
partial last tile, whose members are one model (disagreement 0: the scene of the synthetic scores
and of the limits), and _action_scene, whose members really disagree. Test 5 builds the smallest
shape that takes the scan + emit tail.

Everything is compared bit for bit (float32 as int32): a halted run against
halt_helpers.cut_reference of the unhalted run with the same seed, and the rows rollout(halt=)
writes against flatten(imagine(halt=)). No tolerance is involved: halting is a post-pass that
recomputes no step, and the returns are summed in the reference's order in float64."""
import numpy as np
import pytest
import torch

import bench
import drpo_amd
from drpo_amd import _lib, ops
from gpu_helpers import COMP, DEV
from halt_helpers import assert_cut, cut_reference, run_of
from imagine_helpers import B, H, INF, SEED, _action_scene, _imagine, _scene, assert_same, bits, flatten

pytestmark = pytest.mark.gpu

UNC = ('disagreement', 'epistemic', 'aleatoric', 'max_disagreement')
NAN = float('nan')
SENTINEL = -7.25


def _weights(alg, h=H):
    return np.power(np.float64(alg.solver.discount), np.arange(h, dtype=np.float64))


def _between_live_scores(im):
    """A threshold halfway between two adjacent distinct finite live scores at the median, so that
    no score equals it (also not after its rounding to float32)."""
    live = im.disagreement[im.mask]
    u = torch.unique(live[torch.isfinite(live)]).cpu().double()
    assert len(u) >= 4
    k = len(u) // 2
    thr = float(np.float32((u[k - 1] + u[k]) / 2))
    assert float(u[k - 1]) < thr < float(u[k]), 'two adjacent float32 scores at the median'
    return thr


def _check_optional_groups(got, plain, names):
    """zero at and beyond the new lengths, the unhalted run's values before them"""
    mask = got.mask
    for k in names:
        x, y = getattr(got, k), getattr(plain, k)
        assert x.dtype == y.dtype and x.shape == y.shape == mask.shape, k
        assert not bool(x[~mask].any()), k
        assert torch.equal(bits(x[mask]), bits(y[mask])), k


# ------------------------------------------------------------------ 1. synthetic scores
def _synthetic_scores(lengths, thr):
    """[B, H] scores, by the position j of a row among the rows of its natural length L:
    j % 8 = 0 nothing over; 1 over at step 0; 2 over at step 1; 3 over at step 2 (a step at or
    beyond L has no effect); 4 equal to thr at step 0; 5 NaN at step L - 1; 6 +inf at step 0;
    7 over at steps 0 and 1 (the first counts)."""
    sc = torch.full((B, H), 0.5 * thr)
    seen = {}
    for i, L in enumerate(lengths.tolist()):
        j = seen[L] = seen.get(L, -1) + 1
        p = j % 8
        if p in (1, 2, 3):
            sc[i, p - 1] = 2 * thr
        elif p == 4:
            sc[i, 0] = thr
        elif p == 5:
            sc[i, L - 1] = NAN
        elif p == 6:
            sc[i, 0] = INF
        elif p == 7:
            sc[i, 0] = sc[i, 1] = 3 * thr
    return sc


@pytest.mark.parametrize('rpt', [16, 32])
def test_synthetic_scores_through_cut_trajectories(rpt):
    alg = _scene(rpt)
    thr = 1.0
    plain = _imagine(alg, uncertainty=True)
    im = _imagine(alg, uncertainty=True)
    assert_same(plain, im)
    length = plain.lengths.cpu()
    sc = _synthetic_scores(length, thr)
    ref = cut_reference(plain, sc, thr, _weights(alg))

    # the scene shows every case
    halted_at, L = ref['halted_at'], length.long()
    steps = torch.arange(H)
    live = steps[None] < L[:, None]
    assert set(halted_at.tolist()) == {-1, 0, 1, 2}
    for n in (1, 2, 3):
        assert bool(((L == n) & (halted_at >= 0)).any()) and bool(((L == n) & (halted_at < 0)).any()), n
    assert bool((((sc > thr) & ~live).any(-1) & (halted_at < 0)).any())        # over only at or beyond the length
    assert bool((((sc == thr) & live).any(-1) & (halted_at < 0)).any())        # equal: no halt
    nan_at = torch.isnan(sc) & live
    assert bool(nan_at.any()) and bool((halted_at[nan_at.any(-1)] == nan_at.long().argmax(-1)[nan_at.any(-1)]).all())
    inf_at = torch.isinf(sc) & live
    assert bool(inf_at.any()) and bool((halted_at[inf_at.any(-1)] == 0).all())
    assert 0 in ref['lengths'].tolist() and bool((ref['lengths'] == L.int()).any())

    # [B][H] order at one tile height, a transposed view of [H][B] storage at the other
    dev_sc = sc.to(DEV) if rpt == 16 else sc.t().contiguous().to(DEV).t()
    assert dev_sc.stride() == ((H, 1) if rpt == 16 else (1, B))
    out = ops._cut_trajectories(alg, alg.actor, im, dev_sc, thr)
    torch.cuda.synchronize()
    assert out is im and im.halt_threshold == thr
    assert_cut(im, ref)


# ------------------------------------------------------------------ 2. limits
@pytest.mark.parametrize('rpt', [16, 32])
def test_limits_of_the_threshold(rpt):
    alg = _scene(rpt)
    plain = _imagine(alg, uncertainty=True)
    n0 = drpo_amd.DeviceNoise(SEED)
    alg.imagine(noise=n0, uncertainty=True)

    n1 = drpo_amd.DeviceNoise(SEED)
    none = alg.imagine(noise=n1, halt=INF)
    torch.cuda.synchronize()
    assert_same(plain, none)
    assert_same(plain, none, UNC)
    assert none.halted_at.dtype == torch.int32 and none.halted_at.tolist() == [-1] * B and none.halt_threshold == INF
    assert n1.ctr == n0.ctr

    n2 = drpo_amd.DeviceNoise(SEED)
    every = alg.imagine(noise=n2, halt=-1.0)                 # disagreement >= 0: every row halts at step 0
    torch.cuda.synchronize()
    assert n2.ctr == n0.ctr
    assert every.halted_at.tolist() == [0] * B and every.lengths.tolist() == [0] * B
    assert torch.equal(bits(every.states[:, 0]), bits(plain.states[:, 0]))
    assert not bool(every.states[:, 1:].any())
    for k in ('actions', 'rewards', 'constraint_values', 'dones', 'violations', 'returns', 'terminated') + UNC:
        assert not bool(getattr(every, k).any()), k
    assert bool((every.max_constraint == -INF).all())
    assert every.first_violation.tolist() == [-1] * B
    assert_cut(every, cut_reference(plain, plain.disagreement, -1.0, _weights(alg)))


# ------------------------------------------------------------------ 3. real disagreement
_ACTION = {}


def _disagreeing():
    if 'v' not in _ACTION:
        _ACTION['v'] = _action_scene(DEV)[0]
    return _ACTION['v']


def _given():
    g = torch.Generator().manual_seed(31)
    return torch.tanh(torch.randn(B, 2, 2, generator=g)).to(DEV)


@pytest.mark.parametrize('case', ['policy', 'linear', 'actions'])
def test_real_disagreement_equals_the_reference(case):
    alg = _disagreeing()
    kw = {'policy': {}, 'linear': {'shield': 'linear'}, 'actions': {'actions': _given()}}[case]
    plain = _imagine(alg, uncertainty=True, **kw)
    assert len(set(plain.lengths.tolist())) > 1
    thr = _between_live_scores(plain)
    im = _imagine(alg, halt=thr, **kw)
    ref = cut_reference(plain, plain.disagreement, thr, _weights(alg))
    halted = ref['halted_at'] >= 0
    print(f'{case}: thr {thr:.6g}, {int(halted.sum())} of {B} rows halted, at {sorted(set(ref["halted_at"].tolist()))}')
    assert bool(halted.any()) and bool((~halted).any())
    assert_cut(im, ref)
    assert im.halt_threshold == thr and im.members == plain.members and im.given_steps == plain.given_steps
    groups = UNC[:3] + (('interventions', 'certificate', 'blend') if case == 'linear' else ())
    _check_optional_groups(im, plain, groups)
    if case == 'linear':
        assert im.shield_candidates == plain.shield_candidates and im.shield_threshold == plain.shield_threshold


def test_each_member_is_cut_on_its_own():
    alg = _disagreeing()
    plain = _imagine(alg, uncertainty=True, members='each')
    E = len(alg.model_ensemble._elite_inds)
    assert plain.rewards.shape == (E, B, H)
    thr = _between_live_scores(plain)
    im = _imagine(alg, halt=thr, members='each')
    assert im.halted_at.shape == (E, B) and im.halt_threshold == thr and im.members == plain.members
    distinct = set()
    for e in range(E):
        ref = cut_reference(run_of(plain, e), plain.disagreement[e], thr, _weights(alg))
        assert_cut(run_of(im, e), ref)
        distinct.add(tuple(ref['halted_at'].tolist()))
    assert len(distinct) > 1                                   # the runs do not halt alike


# ------------------------------------------------------------------ 4. the buffer path
def _sentinel(vb, pointer):
    for k in COMP:
        buf = vb._bufs[k]
        buf.fill_(SENTINEL if buf.dtype.is_floating_point else 1)
    vb._set_pointer(pointer)


def _check_buffer(vb, p0, n, want=None):
    """rows p0 .. p0 + n - 1 (mod capacity) hold ``want`` (by component), every other row the sentinel"""
    cap = vb.capacity
    idx = (torch.arange(n, device=DEV) + p0) % cap
    outside = torch.ones(cap, dtype=torch.bool, device=DEV)
    outside[idx] = False
    for k in COMP:
        buf = vb._bufs[k]
        rest = buf[outside]
        fill = torch.full_like(rest, SENTINEL if buf.dtype.is_floating_point else 1)
        assert torch.equal(rest, fill), k
        if want is not None:
            x, y = buf[idx].cpu(), want[k]
            assert x.dtype == y.dtype, k
            assert torch.equal(bits(x), bits(y.reshape(x.shape))), k
    assert vb.pointer == p0 + n


def _buffer_against_imagine(alg, thr, p0, **rollout_kw):
    vb = alg.virt_buffer._module
    _sentinel(vb, p0)
    res = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED), **rollout_kw)
    im = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), halt=thr)
    torch.cuda.synchronize()
    rows = flatten(im)
    n = len(rows['rewards'])
    assert n == int(im.lengths.sum()) == len(res)
    _check_buffer(vb, p0, n, rows)
    assert res.halted_at.dtype == torch.int32 and torch.equal(res.halted_at, im.halted_at)
    return n, im


@pytest.mark.parametrize('rpt', [16, 32])
def test_rollout_writes_the_halted_trajectories(rpt):
    alg = _disagreeing()
    vb = alg.virt_buffer._module
    cap = vb.capacity
    try:
        alg.rows_per_tile = rpt
        plain = _imagine(alg, uncertainty=True)
        thr = _between_live_scores(plain)
        n, im = _buffer_against_imagine(alg, thr, 40, halt=thr)
        halted = im.halted_at >= 0
        assert 0 < n < int(plain.lengths.sum()) and bool(halted.any()) and bool((~halted).any())
        # a ring wrap: the pointer a few rows short of the capacity
        assert n > 10
        _buffer_against_imagine(alg, thr, cap - 5, halt=thr)
        # the config's default is the argument's
        assert not isinstance(alg.rollout_halt_threshold, float)
        alg.rollout_halt_threshold = thr
        try:
            _buffer_against_imagine(alg, thr, 7)
            off = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED), halt=None)    # an explicit None: off
            assert off.halted_at is None and len(off) == int(plain.lengths.sum())
        finally:
            alg.rollout_halt_threshold = None

        # +inf: the plain rollout's buffer and pointer, bit for bit
        _sentinel(vb, 11)
        a = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED))
        torch.cuda.synchronize()
        want = {f: getattr(vb, f).clone() for f in ops._VB_FIELDS}
        assert a.halted_at is None and len(a) == int(plain.lengths.sum())
        _sentinel(vb, 11)
        b = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED), halt=INF)
        torch.cuda.synchronize()
        assert len(b) == len(a) and b.halted_at.tolist() == [-1] * B
        for f in ops._VB_FIELDS:
            x, y = getattr(vb, f), want[f]
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), f

        # -1: nothing is written and the pointer stays
        _sentinel(vb, 11)
        c = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED), halt=-1.0)
        torch.cuda.synchronize()
        assert len(c) == 0 and c.halted_at.tolist() == [0] * B
        _check_buffer(vb, 11, 0)
    finally:
        alg.rows_per_tile = 16


# ------------------------------------------------------------------ 5. the scan + emit tail
def test_the_scan_and_emit_tail():
    """The smallest shape whose H * tiles exceeds the one-launch tail's 8192 counts: H 128,
    B 1040 at 16-row tiles (65 tiles, the last one full: 8320 counts)."""
    Bs, Hs = 1040, 128
    assert Hs * (Bs // 16) > 8192 >= Hs * ((Bs - 16) // 16)
    alg = bench.make_alg(DEV, Bs, Hs, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 2000, np.random.RandomState(0))
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    m = alg.model_ensemble
    m.state_normalizer.fit(alg.replay_buffer.get('states'))
    m._elite_inds = [3, 0, 6, 2, 5]
    alg.rollout_engine, alg.rows_per_tile = 2, 16
    plain = alg.imagine(noise=drpo_amd.DeviceNoise(SEED), uncertainty=True)
    thr = _between_live_scores(plain)
    n, im = _buffer_against_imagine(alg, thr, 123, halt=thr)
    halted = im.halted_at >= 0
    print(f'scan + emit: thr {thr:.6g}, {int(halted.sum())} of {Bs} rows halted, {n} of {int(plain.lengths.sum())} rows kept')
    assert bool(halted.any()) and bool((~halted).any())
    assert_cut(im, cut_reference(plain, plain.disagreement, thr, _weights(alg, Hs)))


# ------------------------------------------------------------------ 6. off means off
def test_off_means_off(monkeypatch):
    alg = _disagreeing()
    L = _lib.lib()
    calls = []

    def spy(name):
        f = getattr(L, name)

        def wrapped(*a):
            calls.append(name)
            return f(*a)
        monkeypatch.setattr(L, name, wrapped)
    for name in ('drpo_rollout_stage', 'drpo_rollout_emit_cut', 'drpo_rollout_trajectories_cut', 'drpo_rollout'):
        spy(name)
    alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED))
    alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED), halt=None)
    alg.imagine(noise=drpo_amd.DeviceNoise(SEED), uncertainty=True)
    torch.cuda.synchronize()
    assert calls == ['drpo_rollout', 'drpo_rollout']
    del calls[:]
    alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(SEED), halt=0.5)
    alg.imagine(noise=drpo_amd.DeviceNoise(SEED), halt=0.5)
    torch.cuda.synchronize()
    assert calls == ['drpo_rollout_stage', 'drpo_rollout_emit_cut', 'drpo_rollout_trajectories_cut']
