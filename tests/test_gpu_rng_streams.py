"""The device random streams against the bit-exact host model (tests/rng_model.py).

* raw words and indices, exactly: drpo_sample_batch and drpo_ens_gather_steps on buffers
  whose rows hold their own number;
* the normals value by value: drpo_policy_head (mode 0, zero ``raw``) returns its draws in
  ``e``; |e - z64| <= C_HW * 2^-24 * m with m = sqrt(-2 ln u1), the Box-Muller radius
  (v_sin_f32 / v_cos_f32 are absolutely accurate near their zeros, not relatively, so the
  bound scales with the radius and not with |z64|), at every site, and at the edge words
  u1 = 1, u1 = 2^-24, u2 = 1, u2 = 1/4 and 1/2 (+- 2^-24);
* the sites that have no draw output (drpo_cc_dist, drpo_ens_head, the fused heads of
  drpo_mlp_forward_multi, and the critic update's launches with sites 1, 2 and 7): the
  device-noise run equals, bit for bit, the run on recorded draws equal to those
  drpo_policy_head returns for the same (seed, ctr, site, idx);
* the rollout engines' keying: with zero weights every draw can be recovered from the
  trajectories and is compared with the model's normal at (row, (t << 8) | kind, q, ctr);
* the permutation: drpo_sample_without_replacement and the rollout's start rows equal the
  model's, including the five calls at which the capped walk repeated an index.

Measured figures: profiles/rng_streams/README.md (``pytest -s`` prints them)."""
import ctypes

import numpy as np
import pytest
import torch

import drpo_amd
import fake_envs
import rng_model as M
from drpo_amd import _lib, ops
from drpo_amd._abi import BufferView
from drpo_amd.envs import ConstraintProgram
from gpu_helpers import C_HW, C_LIBM, DEV, U32, error_ratio, ulp32
from test_rng_model import CE_SEED, COUNTEREXAMPLES, CountingNoise

pytestmark = pytest.mark.gpu

SEEDS = [0x1234567, 0x9E3779B97F4A7C15]       # the second one has bits 32..63 set
CTRS = [1, 0x89ABCDEF]


def ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------
# raw words and indices
# ---------------------------------------------------------------------------
_ROWS = {}


def row_numbers(n):
    """[n, 1] float32 whose row i holds i (exact below 2^24), and n zero bytes"""
    if n not in _ROWS:
        _ROWS[n] = (torch.arange(n, device=DEV, dtype=torch.float32).reshape(n, 1).contiguous(),
                    torch.zeros(n, dtype=torch.uint8, device=DEV))
    return _ROWS[n]


def buffer_view(n_alloc, length, ptr_dev=None, cap=0):
    """a drpo_buffer_view_t over the row-number buffer: every float component reads it"""
    rows, flags = row_numbers(n_alloc)
    v = BufferView()
    v.s = v.a = v.s2 = v.r = v.h = rows.data_ptr()
    v.d = v.v = flags.data_ptr()
    v.len, v.cap = length, cap
    v.ptr_dev = 0 if ptr_dev is None else ptr_dev.data_ptr()
    return v


def sample_batch(real, virt, n_real, B, seed, ctr):
    out = [torch.full((B, 1), -1.0, device=DEV) for _ in range(3)] + [torch.full((B,), -1.0, device=DEV)]
    flags = [torch.full((B,), 7, dtype=torch.uint8, device=DEV) for _ in range(2)]
    h = torch.full((B, 1), -1.0, device=DEV)
    s, a, s2, r = out
    _lib.check(_lib.lib().drpo_sample_batch(ctypes.byref(real), ctypes.byref(virt), n_real, B, 1, 1, 1, None, None, seed,
                                            ctr, 0.0, 0.0, 1.0, 0.0, ptr(s), ptr(a), ptr(s2), ptr(r), ptr(flags[0]),
                                            ptr(flags[1]), ptr(h), _lib.stream()), 'sample_batch')
    torch.cuda.synchronize()
    assert not bool(flags[0].any()) and not bool(flags[1].any())
    return [x.reshape(B).cpu().numpy().astype(np.int64) for x in (s, a, s2, r, h)]


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('ctr', CTRS)
def test_sample_batch_rows_equal_the_model(seed, ctr):
    """B = 130 (two 64-thread blocks and two threads of a third), 65 real and 65 virtual
    rows. len = 2^20: the row is the top 20 bits of x; len = 1000: all 32 bits enter the
    product. A negative len reads the device pointer: 700 (below cap 1000) and 5000 (above)."""
    B, n_real = 130, 65
    big = 1 << 20
    p_lo = torch.tensor([700], dtype=torch.int64, device=DEV)
    p_hi = torch.tensor([5000], dtype=torch.int64, device=DEV)
    cases = [(buffer_view(big, big), buffer_view(big, 1000), big, 1000),
             (buffer_view(big, 1000), buffer_view(big, big), 1000, big),
             (buffer_view(big, -1, p_lo, 1000), buffer_view(big, -1, p_hi, 1000), 700, 1000),
             (buffer_view(big, -1, p_hi, 1000), buffer_view(big, -1, p_lo, 1000), 1000, 700)]
    for real, virt, len_r, len_v in cases:
        want = M.sample_batch_rows(seed, ctr, n_real, B, len_r, len_v)
        assert want[:n_real].max() < len_r and want[n_real:].max() < len_v
        for got in sample_batch(real, virt, n_real, B, seed, ctr):
            assert np.array_equal(got, want), (len_r, len_v)
    # top 20 bits of x at len = 2^20
    w = M.philox_words(seed, M.site_sample_batch(n_real, B, ctr))
    assert np.array_equal(M.sample_batch_rows(seed, ctr, n_real, B, big, big), w[:, 0].astype(np.int64) >> 12)
    # the real and the virtual half draw differently at equal j
    assert not np.array_equal(want[:n_real], want[n_real:])


def gather(cap, pointer, rows, steps, seed, ctr, dev_ptr):
    buf, _ = row_numbers(cap)
    p = torch.tensor([pointer], dtype=torch.int64, device=DEV)
    xs, xa = (torch.full((steps * rows, 1), -1.0, device=DEV) for _ in range(2))
    xt = torch.full((steps * rows, 2), -1.0, device=DEV)
    _lib.check(_lib.lib().drpo_ens_gather_steps(ptr(buf), ptr(buf), ptr(buf), ptr(buf), 0 if dev_ptr else pointer,
                                                ptr(p) if dev_ptr else None, cap, rows, steps, None, seed, ctr, 1, 1,
                                                ptr(xs), ptr(xa), ptr(xt), _lib.stream()), 'gather')
    torch.cuda.synchronize()
    cols = [xs[:, 0], xa[:, 0], xt[:, 0], xt[:, 1]]
    return [c.cpu().numpy().astype(np.int64) for c in cols]


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('ctr', [1, 0xFFFFFFFE])      # the second one wraps: ctr + step passes 2^32
def test_gather_rows_equal_the_model(seed, ctr):
    """rows = 96, steps = 4. cap = 2^20 full and unwrapped: the row is the low 20 bits of x
    (y drops out of (y << 32 | x) mod 2^20); cap = 1000 with the pointer at 1234: n = 1000
    does not divide 2^32, so y enters, and the chronological index is turned by 234."""
    rows, steps = 96, 4
    big = 1 << 20
    for cap, pointer in ((big, big), (1000, 1234), (1000, 700)):
        want = M.gather_rows(seed, ctr, rows, steps, pointer, cap)
        for dev_ptr in (False, True):
            for got in gather(cap, pointer, rows, steps, seed, ctr, dev_ptr):
                assert np.array_equal(got, want), (cap, pointer, dev_ptr)
    w = M.philox_words(seed, M.site_gather(rows, steps, ctr)).astype(np.int64)
    assert np.array_equal(M.gather_rows(seed, ctr, rows, steps, big, big), w[:, 0] & (big - 1))
    # y is used: the rows differ from those of x alone at n = 1000
    assert not np.array_equal(M.gather_rows(seed, ctr, rows, steps, 1000, 1000), w[:, 0] % 1000)


# ---------------------------------------------------------------------------
# normals, value by value
# ---------------------------------------------------------------------------
def head_draws(B, A, seed, ctr, site):
    """the draws of drpo_policy_head, mode 0, zero raw: e [B * A] float32 on the device"""
    raw = torch.zeros(B, 2 * A, device=DEV)
    e = torch.full((B, A), float('nan'), device=DEV)
    a = torch.empty(B, A, device=DEV)
    _lib.check(_lib.lib().drpo_policy_head(ptr(raw), B, A, 0, None, seed, ctr, site, ptr(a), None, None, ptr(e), None,
                                           _lib.stream()), 'policy_head')
    torch.cuda.synchronize()
    return e.reshape(-1)


def normals_ratio(name, got, seed, ctr, site, idx):
    z, m = M.normal_at(seed, ctr, site, idx)
    return error_ratio(name, got, torch.from_numpy(z), torch.from_numpy(m), C_HW)


NORMAL_SITES = [M.SITE_PI_NEXT, M.SITE_SAFE_NEXT, M.SITE_PI_RS, M.SITE_SAFE_RS, M.SITE_TARGET, M.SITE_PI_MULT,
                M.SITE_ACT, M.SITE_CC_DIST, M.SITE_ENS_HEAD]


@pytest.mark.parametrize('A', [1, 3, 6])
def test_normals_equal_the_model_at_every_site(A):
    """At least 4099 elements (every lane, 1025 counters, a partial 64-row block): B = 4099
    at A = 1, 1367 at A = 3 (4101 elements), 684 at A = 6 (4104)."""
    B = -(-4099 // A)
    idx = np.arange(B * A)
    worst = 0.0
    for seed in SEEDS:
        for ctr in CTRS:
            for site in NORMAL_SITES:
                got = head_draws(B, A, seed, ctr, site)
                worst = max(worst, normals_ratio(f'normal_at A={A} seed={seed:#x} ctr={ctr:#x} site={site:#x}', got,
                                                 seed, ctr, site, idx))
    print(f'edge-ratio normals A={A}: worst over seeds, counters and sites {worst:.3g}')
    assert worst <= 1.0
    # sites, counters and seeds address different draws
    a, b, c, d = (head_draws(B, A, *k) for k in ((SEEDS[0], 1, 1), (SEEDS[0], 1, 2), (SEEDS[0], 2, 1), (SEEDS[1], 1, 1)))
    assert not (torch.equal(a, b) or torch.equal(a, c) or torch.equal(a, d))


# (seed, site, ctr, counter, pair, u * 2^24 of the word): found by a search of ctr = 1, 2, ...
# over the 1024 counters of idx < 4096 with the model (profiles/rng_streams/README.md);
# pair 0 is lanes 0, 1 (words x, y), pair 1 lanes 2, 3 (words z, w)
EDGE_SEED, EDGE_SITE = 0x9E3779B97F4A7C15, 5
EDGE_WORDS = {
    'u1 = 1': (3153, 596, 1, 'radius', 1 << 24),
    'u1 = 2^-24': (7907, 34, 0, 'radius', 1),
    'u2 = 1': (17894, 365, 1, 'angle', 1 << 24),
    'u2 = 1/4 + 2^-24': (1444, 492, 0, 'angle', (1 << 22) + 1),
    'u2 = 1/2 - 2^-24': (484, 286, 0, 'angle', (1 << 23) - 1),
}


@pytest.mark.parametrize('case', list(EDGE_WORDS))
def test_normals_at_the_edge_words(case):
    ctr, counter, pair, which, u24 = EDGE_WORDS[case]
    w = M.philox_words(EDGE_SEED, M._words(counter, 0, EDGE_SITE, ctr))
    word = int(w[2 * pair + (0 if which == 'radius' else 1)])
    assert (word >> 8) + 1 == u24, 'the model no longer finds the edge word there'
    idx = np.array([4 * counter + 2 * pair, 4 * counter + 2 * pair + 1])
    z, m = M.normal_at(EDGE_SEED, ctr, EDGE_SITE, idx)
    got = head_draws(1024, 4, EDGE_SEED, ctr, EDGE_SITE)
    assert bool(torch.isfinite(got).all())
    pairv = got[torch.from_numpy(idx).to(DEV)].cpu().double()
    print(f'{case}: model {z[0]:.9g} {z[1]:.9g} (radius {m[0]:.9g}), device {pairv[0].item():.9g} {pairv[1].item():.9g}')
    ratio = error_ratio(f'edge word {case}', pairv, torch.from_numpy(z), torch.from_numpy(m), C_HW)
    assert ratio <= 1.0
    if case == 'u1 = 1':
        assert m[0] == 0 and bool((pairv == 0).all())            # -0 * cos: +-0, never NaN
    if case == 'u1 = 2^-24':
        assert abs(m[0] - np.sqrt(48 * np.log(2.0))) < 1e-12     # 5.768: the largest radius there is
    # and the whole launch around the edge
    assert normals_ratio(f'edge launch {case}', got, EDGE_SEED, ctr, EDGE_SITE, np.arange(4096)) <= 1.0


# ---------------------------------------------------------------------------
# sites without a draw output
# ---------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('seed,ctr', [(SEEDS[0], 1), (SEEDS[1], 0x89ABCDEF)])
def test_cc_dist_draws_are_site_cc01(seed, ctr):
    """mode 1 on recorded draws equal to site 0xcc01's against device noise: the same
    instructions on the same words, so equal bit for bit (the +-2 clamp included)."""
    n = 4099
    g = torch.Generator().manual_seed(3)
    mu, ls = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    e = head_draws(n, 1, seed, ctr, M.SITE_CC_DIST)
    assert int((e.abs() > 2).sum()) > 50                         # the clamp acts (4.6 % of the draws)
    outs = []
    for eps in (e, None):
        sd, q = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        _lib.check(_lib.lib().drpo_cc_dist(ptr(mu), ptr(ls), n, 1, 2.0, -5.0, 2.0, ptr(eps), seed, ctr, ptr(sd), ptr(q),
                                           _lib.stream()), 'cc_dist')
        outs.append((sd, q))
    torch.cuda.synchronize()
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    other = head_draws(n, 1, seed, ctr, M.SITE_CC_DIST + 1)      # a neighbouring site would not pass
    assert not torch.equal(other, e)


@pytest.mark.parametrize('seed,ctr', [(SEEDS[0], 1), (SEEDS[1], 0x89ABCDEF)])
def test_ens_head_draws_are_site_e5a1_over_the_output_index(seed, ctr):
    """Z = 3 output members through a zsel map, n = 67, S = 3: element (zo, row, k) draws at
    index (zo * n + row) * (S + 1) + k, the member offset included."""
    Zin, Zo, n, S = 3, 3, 67, 3
    S1 = S + 1
    D, LV = torch.zeros(Zin, n, S1, device=DEV), torch.zeros(Zin, n, S1, device=DEV)
    s = torch.zeros(n, S, device=DEV)
    lo, hi = torch.full((S1,), -30., device=DEV), torch.full((S1,), 30., device=DEV)
    zsel = torch.tensor([2, 0, 2], dtype=torch.int32, device=DEV)
    e = head_draws(Zo * n * S1, 1, seed, ctr, M.SITE_ENS_HEAD)
    assert np.array_equal(np.concatenate([M.ens_head_index(z, n, S) for z in range(Zo)]), np.arange(Zo * n * S1))
    outs = []
    for eps in (e, None):
        s2, r = torch.empty(Zo, n, S, device=DEV), torch.empty(Zo, n, device=DEV)
        _lib.check(_lib.lib().drpo_ens_head(ptr(D), ptr(LV), ptr(s), 0, n, S, Zo, ptr(lo), ptr(hi), ptr(zsel), ptr(eps),
                                            seed, ctr, None, None, ptr(s2), ptr(r), _lib.stream()), 'ens_head')
        outs.append((s2, r))
    torch.cuda.synchronize()
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    s2 = outs[1][0]
    assert not torch.equal(s2[0], s2[2])                          # members 0 and 2 read the same input member
    # the values themselves: std = sqrt(exp(lv)) with lv the soft clamp of 0 into [-30, 30]
    x = torch.cat([s2, outs[1][1][..., None]], -1).reshape(-1).cpu().double()
    lv = 30 - np.log1p(np.exp(30.0))
    lv = -30 + np.log1p(np.exp(lv + 30))
    z, m = M.normal_at(seed, ctr, M.SITE_ENS_HEAD, np.arange(Zo * n * S1))
    sd = np.sqrt(np.exp(lv))
    assert error_ratio('ens_head draws', x, torch.from_numpy(z * sd), torch.from_numpy(m * sd), C_HW + C_LIBM) <= 1.0


FUSED_SITES = [(M.SITE_PI_NEXT, 1), (M.SITE_SAFE_NEXT, 1), (M.SITE_PI_RS, 2), (M.SITE_SAFE_RS, 2), (M.SITE_PI_MULT, 2)]


@pytest.mark.parametrize('A', [1, 6])
def test_fused_heads_draw_at_their_sites(A):
    """The squashed-Gaussian head fused into drpo_mlp_forward_multi at the sites of
    sac_step.py (1, 2: sample; 5, 6, 8: rsample), on the smallest net the descriptor checks
    admit (test_gpu_rowwise_fused.identity_net, [2A -> 2A]), 33 rows (two full 16-row tiles
    and one row): the launch with ``eps`` pointing at site's draws and the launch with
    ``eps`` null write the same a, logp, u and e bit for bit."""
    from drpo_amd import _abi
    from drpo_amd.mlp_desc import fill_fwd, with_head
    from test_gpu_rowwise_fused import dev_copy, identity_net
    rows = 33
    seed, ctr = SEEDS[1], 0x89ABCDEF
    g = torch.Generator().manual_seed(A)
    raw = torch.randn(rows, 2 * A, generator=g).to(DEV)
    for site, mode in FUSED_SITES:
        e = head_draws(rows, A, seed, ctr, site).reshape(rows, A).contiguous()
        outs = []
        for eps in (e, None):
            net = identity_net(2 * A)
            o = {k: torch.full((rows,) if k == 'logp' else (rows, A), float('nan'), device=DEV)
                 for k in ('a', 'logp', 'u', 'e')}
            d = fill_fwd([net], [(raw, 2 * A), (None, 0), (None, 0)], rows)
            with_head(d, mode, A, eps, site, **o)
            arr = (_abi.MlpFwd * 1)(d)
            dcopy = dev_copy(arr)
            _lib.check(_lib.lib().drpo_mlp_forward_multi(arr, dcopy.data_ptr(), 1, seed, ctr, _lib.stream()),
                       'forward_multi')
            torch.cuda.synchronize()
            outs.append(o)
        for k in ('a', 'logp', 'u', 'e'):
            assert bool(torch.isfinite(outs[1][k]).all()), (site, k)
            assert torch.equal(bits(outs[0][k]), bits(outs[1][k])), (site, k)
        assert torch.equal(bits(outs[1]['e']), bits(e))
    assert not torch.equal(head_draws(rows, A, seed, ctr, 1), head_draws(rows, A, seed, ctr, 2))


# ---------------------------------------------------------------------------
# the permutation on the device
# ---------------------------------------------------------------------------
def device_prp(N, B, seed, ctr):
    out = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().drpo_sample_without_replacement(ptr(out), B, N, seed, ctr, _lib.stream()), 'prp')
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('N,B', [(1, 1), (2, 2), (5, 5), (17, 17), (257, 257), (4097, 4097), (100000, 4096)])
def test_device_permutation_equals_the_model(N, B):
    for seed, ctr in ((0x1234567, 1), (2 ** 64 - 1, 2 ** 32 - 1), (0xDEADBEEF12345, 40)):
        got = device_prp(N, B, seed, ctr)
        assert np.array_equal(got, M.sample_without_replacement(N, B, seed, ctr)), (seed, ctr)
        assert len(np.unique(got)) == B and got.min() >= 0 and got.max() < N
    # seed bits 56..63 and ctr bits 32.. do not enter
    assert np.array_equal(device_prp(N, B, 0x1234567 | (0xA5 << 56), 1 + (3 << 32)), device_prp(N, B, 0x1234567, 1))


@pytest.mark.parametrize('N,ctr,row,value', COUNTEREXAMPLES)
def test_device_permutation_counterexamples(N, ctr, row, value):
    """The calls at which the 64-step walk fell back to x % N and returned `value` twice:
    N distinct values now (N - 1 before), equal to the uncapped model."""
    got = device_prp(N, N, CE_SEED, ctr)
    print(f'N = {N}, ctr = {ctr}: {len(np.unique(got))} distinct values, row {row} -> {got[row]}')
    assert len(np.unique(got)) == N
    assert np.array_equal(got, M.sample_without_replacement(N, N, CE_SEED, ctr))
    assert got[row] != value and int((got == value).sum()) == 1


# ---------------------------------------------------------------------------
# rollout keying, by recovering each draw
# ---------------------------------------------------------------------------
BOUND = 1000.0      # the env's safe set and live set: |s0| <= 1000
RB, RH = 70, 4      # four 16-row tiles and one of 6 / two 32-row tiles and one of 6
A_STD_RAW = float(np.log(0.3227 / 0.6773))      # log-std -6 + 10 * sigmoid = -2.773: std 2^-4
_WIDE = {}


def fresh_alg(S, A):
    """A trainer (default widths, E = 7) on an env of S states, A actions and wide bounds"""
    class WideEnv(fake_envs._Env):
        drpo_constraint_program = staticmethod(
            lambda: ConstraintProgram().affine([0], [1.0], -BOUND).done_box((0,), -BOUND, BOUND))
    WideEnv.S, WideEnv.A, WideEnv.C = S, A, 1
    torch.manual_seed(5)
    cfg = drpo_amd.SMBPO.Config()
    cfg.update({'horizon': RH, 'rollout_batch_size': RB, 'buffer_max': 4096})
    alg = drpo_amd.SMBPO(cfg, lambda id=None: WideEnv(), None, 1, device=DEV)
    assert alg.env_params['env_id'] == 4 and (alg.state_dim, alg.action_dim) == (S, A)
    return alg


def wide_alg(S, A):
    """fresh_alg with zero weights in the actor, the safe actor and every member: mu = 0,
    action std 2^-4, the members' std between 2^-7 and 2^-5 per output (from the biases
    alone), next state = state + std * eps."""
    if (S, A) in _WIDE:
        return _WIDE[(S, A)]
    alg = fresh_alg(S, A)
    for pol in (alg.actor, alg.actor_safe):
        pol.group.data.zero_()
        pol.group.view(f'net.{2 * (pol.spec.n_layers - 1)}.bias')[A:].fill_(A_STD_RAW)
    m = alg.model_ensemble
    for net in m.views():
        for W, b in net:
            W.zero_()
            b.zero_()
    m.views()[2][-1][1][:] = torch.linspace(-8.5, -7.3, S + 1, device=DEV)     # raw log-var per output
    m._elite_inds = list(range(min(5, m.ensemble_size)))
    m.state_normalizer.mean.zero_()
    m.state_normalizer.std.fill_(1.0)
    _WIDE[(S, A)] = alg
    return alg


def kernel_std(alg, B):
    """The kernels' own std per element, from a run on recorded draws all equal to 1 from
    zero start states: states[:, 1] = 0 + std * 1 and rewards = std exactly, actions =
    tanh(std_a). ((B, S + 1) model std, (B, A) atanh of the ones-action), float64."""
    S, A = alg.state_dim, alg.action_dim
    ones = alg_run(alg, torch.zeros(B, S, device=DEV), horizon=1, members=0,
                   eps_a=torch.ones(1, B, A, device=DEV), eps_m=torch.ones(1, B, S + 1, device=DEV), eps_layout=1)
    sd = torch.cat([ones.states[:, 1], ones.rewards[:, :1]], 1).cpu().double().numpy()
    assert sd.min() >= 2.0 ** -7 and sd.max() <= 2.0 ** -5, (sd.min(), sd.max())
    a1 = ones.actions[:, 0].cpu().double().numpy()
    assert abs(a1 - 2.0 ** -4).max() < 2.0 ** -9
    return sd, np.arctanh(a1), a1


def alg_run(alg, start, rpt=0, **kw):
    alg.rows_per_tile = rpt
    kw.setdefault('horizon', RH)
    kw.setdefault('members', [0, 1, 2, 0][:kw['horizon']])
    im = ops.rollout_trajectories(alg, alg.actor, start, kw.pop('noise', drpo_amd.DeviceNoise(1)), **kw)
    torch.cuda.synchronize()
    return im


def start_states(B, S):
    g = torch.Generator().manual_seed(9)
    return (torch.rand(B, S, generator=g) * 2 - 1).to(DEV)        # 999 inside the bounds


def fast_tanh_terms(a):
    """absolute terms of fast_tanh = 1 - 2 / (e^{2u} + 1) at the action a = tanh(u)"""
    return 1.0 + (1.0 - a)


def check_model_draws(name, im, sd, seed, ctr, key_rows=None, steps=None):
    """eps_m = (s[t+1] - s[t]) / std and reward / std against the model's kind 1 normals:
    the normals' bound plus ulp32(s[t+1]) / std (the rounding of the sum)."""
    st = im.states.cpu().double().numpy()
    rw = im.rewards.cpu().double().numpy()
    B, S = st.shape[0], st.shape[2]
    worst = 0.0
    for t in (range(im.rewards.shape[1]) if steps is None else steps):
        rows = np.arange(B) if key_rows is None else key_rows[t]
        live = rows >= 0
        z, m = M.rollout_normals(seed, ctr, rows[live], t, 1, S + 1)
        nxt = np.concatenate([st[live, t + 1], rw[live, t:t + 1]], 1)
        cur = np.concatenate([st[live, t], np.zeros((live.sum(), 1))], 1)
        eps = (nxt - cur) / sd[live]
        bound = C_HW * U32 * m + ulp32(torch.from_numpy(nxt)).numpy() / sd[live]
        worst = max(worst, float((np.abs(eps - z) / bound).max()))
    print(f'edge-ratio {name} model draws: max err/bound {worst:.3g}')
    return worst


def check_action_draws(name, im, w1, a1, seed, ctr, fused, key_rows=None, steps=None, rows_mask=None):
    """eps_a = atanh(a) / atanh(a_ones) against the model's kind 0 normals: the normals'
    bound plus C_LIBM * 2^-24 * |eps| (tanhf and the two roundings). The fused engine
    squashes with fast_tanh = 1 - 2 / (e^{2u} + 1), whose error is absolute, C_HW * 2^-24 *
    (1 + 2 / (e^{2u} + 1)): divided by d a / d eps = (1 - a^2) * atanh(a_ones) for the action,
    and the same term of a_ones times |eps| / a_ones (profiles/rng_streams/README.md)."""
    ac = im.actions.cpu().double().numpy()
    B, A = ac.shape[0], ac.shape[2]
    worst = 0.0
    for t in (range(ac.shape[1]) if steps is None else steps):
        rows = np.arange(B) if key_rows is None else key_rows[t]
        live = rows >= 0
        if rows_mask is not None:
            live = live & rows_mask[:, t]
        z, m = M.rollout_normals(seed, ctr, rows[live], t, 0, A)
        a = ac[live, t]
        eps = np.arctanh(a) / w1[live]
        bound = C_HW * U32 * m + C_LIBM * U32 * np.abs(z)
        if fused:
            bound = bound + C_HW * U32 * (fast_tanh_terms(a) / ((1 - a * a) * w1[live]) +
                                          fast_tanh_terms(a1[live]) / a1[live] * np.abs(z))
        worst = max(worst, float((np.abs(eps - z) / bound).max()))
    print(f'edge-ratio {name} action draws: max err/bound {worst:.3g}')
    return worst


ROLL_SEED, ROLL_CTR = 0x9E3779B97F4A7C15, 0x12345


@pytest.mark.parametrize('rpt', [0, 16, 32])
@pytest.mark.parametrize('S,A', [(3, 2), (12, 6)])
def test_fused_engine_draws_are_keyed_by_row_step_kind_q(S, A, rpt):
    """rollout_trajectories plain: B = 70 (a partial last tile), H = 4, q = 0 (A = 2) and
    0, 1 (A = 6), q up to 0 (S = 3) and 3 (S = 12). No row can end: the total displacement
    is at most 4 * 5.77 * 2^-5 < 1 with the bound 999 away."""
    alg = wide_alg(S, A)
    sd, w1, a1 = kernel_std(alg, RB)
    im = alg_run(alg, start_states(RB, S), rpt, noise=drpo_amd.DeviceNoise(ROLL_SEED), ctr=ROLL_CTR)
    assert bool((im.lengths == RH).all())
    name = f'fused S={S} A={A} rpt={rpt}'
    assert check_model_draws(name, im, sd, ROLL_SEED, ROLL_CTR) <= 1.0
    assert check_action_draws(name, im, w1, a1, ROLL_SEED, ROLL_CTR, fused=True) <= 1.0


@pytest.mark.parametrize('K', [1, RH])
@pytest.mark.parametrize('S,A', [(3, 2), (12, 6)])
def test_given_actions_leave_every_other_draw_in_place(S, A, K):
    alg = wide_alg(S, A)
    sd, w1, a1 = kernel_std(alg, RB)
    g = torch.Generator().manual_seed(4)
    given = (torch.rand(RB, K, A, generator=g) - 0.5).to(DEV).contiguous()
    im = alg_run(alg, start_states(RB, S), noise=drpo_amd.DeviceNoise(ROLL_SEED), ctr=ROLL_CTR, actions=given)
    assert bool((im.lengths == RH).all()) and im.given_steps == K
    assert torch.equal(bits(im.actions[:, :K]), bits(given))
    name = f'given K={K} S={S} A={A}'
    assert check_model_draws(name, im, sd, ROLL_SEED, ROLL_CTR) <= 1.0
    if K < RH:
        assert check_action_draws(name, im, w1, a1, ROLL_SEED, ROLL_CTR, fused=True, steps=range(K, RH)) <= 1.0


@pytest.mark.parametrize('S,A', [(3, 2), (12, 6)])
def test_shield_moves_no_draw(S, A):
    """A threshold no row reaches (+inf) and one every row reaches (-inf): the model draws
    are the model's in both, and the action draws of the rows without an intervention
    (every row at +inf, none at -inf) are the model's."""
    alg = wide_alg(S, A)
    sd, w1, a1 = kernel_std(alg, RB)
    for thr in (float('inf'), float('-inf')):
        im = alg_run(alg, start_states(RB, S), noise=drpo_amd.DeviceNoise(ROLL_SEED), ctr=ROLL_CTR, shield=thr)
        assert bool((im.lengths == RH).all())
        assert bool(im.interventions.all()) == (thr < 0) and bool(im.interventions.any()) == (thr < 0)
        name = f'shield {thr} S={S} A={A}'
        assert check_model_draws(name, im, sd, ROLL_SEED, ROLL_CTR) <= 1.0
        if thr > 0:
            assert check_action_draws(name, im, w1, a1, ROLL_SEED, ROLL_CTR, fused=True,
                                      rows_mask=~im.interventions.cpu().numpy()) <= 1.0
        else:
            assert float(im.actions.abs().max()) <= 4 * U32         # fast_tanh(mu_safe = 0), no draw


@pytest.mark.parametrize('S,A', [(3, 2), (12, 6)])
def test_step_engine_keys_by_the_compacted_row(S, A):
    """drpo_rollout, engine 1, B = 70, H = 2, row 37 starts outside the live set and ends
    at step 0: at step 1 the rows after it are keyed one lower (their rank among the live
    rows), the rows before it by their own number."""
    alg = wide_alg(S, A)
    sd, w1, a1 = kernel_std(alg, RB)
    dead = 37
    start = start_states(RB, S)
    start[dead, 0] = 2 * BOUND
    H = 2
    alg.horizon, alg.rollout_engine, alg.rows_per_tile = H, 1, 0
    alg.model_ensemble._elite_inds = [0]
    vb = alg.virt_buffer
    try:
        noise = drpo_amd.DeviceNoise(ROLL_SEED)
        noise.ctr = ROLL_CTR - 1
        n0 = len(vb)
        out = ops.rollout(alg, alg.actor, start, noise)
        torch.cuda.synchronize()
    finally:
        alg.horizon, alg.rollout_engine = RH, 0
        alg.model_ensemble._elite_inds = list(range(5))
    assert noise.ctr == ROLL_CTR
    got = out.get(as_dict=True)
    assert len(out) == 2 * RB - 1
    done0 = got['dones'][:RB].cpu().numpy()
    assert done0.tolist() == [i == dead for i in range(RB)]
    alive1 = ~done0
    key_rows = [np.arange(RB), M.step_engine_key_rows(alive1)]
    assert key_rows[1][dead] == -1 and key_rows[1][dead - 1] == dead - 1 and key_rows[1][dead + 1] == dead
    # the buffer holds step 0's 70 rows, then step 1's 69 in the order of their rank
    worst_m = worst_a = 0.0
    for t, (lo, rows) in enumerate(((0, np.arange(RB)), (RB, np.flatnonzero(alive1)))):
        n = len(rows)
        s, s2 = got['states'][lo:lo + n].cpu().double().numpy(), got['next_states'][lo:lo + n].cpu().double().numpy()
        r, a = got['rewards'][lo:lo + n].cpu().double().numpy(), got['actions'][lo:lo + n].cpu().double().numpy()
        if t == 1:
            assert np.array_equal(s, prev_next[rows])              # row order: the survivors, in order
        prev_next = s2
        keys = key_rows[t][rows]
        z, m = M.rollout_normals(ROLL_SEED, ROLL_CTR, keys, t, 1, S + 1)
        nxt, cur = np.concatenate([s2, r[:, None]], 1), np.concatenate([s, np.zeros((n, 1))], 1)
        eps = (nxt - cur) / sd[rows]
        # the step engine's std is libm's sqrtf(expf(lv)), the ones run's fast_exp(lv / 2):
        # C_HW * 2^-24 * |lv| / 2 apart relatively (|lv| <= 10)
        bound = C_HW * U32 * m + ulp32(torch.from_numpy(nxt)).numpy() / sd[rows] + C_HW * U32 * 5 * np.abs(z)
        worst_m = max(worst_m, float((np.abs(eps - z) / bound).max()))
        za, ma = M.rollout_normals(ROLL_SEED, ROLL_CTR, keys, t, 0, A)
        ea = np.arctanh(a) / w1[rows]
        bound = (C_HW * U32 * ma + C_LIBM * U32 * np.abs(za) +
                 C_HW * U32 * fast_tanh_terms(a1[rows]) / a1[rows] * np.abs(za))   # a_ones is the fused engine's
        worst_a = max(worst_a, float((np.abs(ea - za) / bound).max()))
        if t == 1:      # keyed by the original row the later rows would be wrong by order 1
            zo, _ = M.rollout_normals(ROLL_SEED, ROLL_CTR, rows, t, 1, S + 1)
            assert np.abs(eps - zo)[rows > dead].max() > 0.5
    print(f'edge-ratio step engine S={S} A={A}: model draws {worst_m:.3g}, action draws {worst_a:.3g}')
    assert worst_m <= 1.0 and worst_a <= 1.0


# ---------------------------------------------------------------------------
# a rollout's start rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('wrapped', [False, True])
def test_rollout_start_rows_equal_the_model(wrapped):
    """257 replay rows whose first state component is the (physical) row number, B = 256, the
    call that takes ctr 431086 of seed 0x1234567: the capped walk gave rows 125 and one
    other the same start state. Unwrapped, and wrapped (capacity 257, pointer 357)."""
    S, A, N, B = 3, 2, 257, 256
    alg = wide_alg(S, A)
    N_, ctr, row, value = COUNTEREXAMPLES[0]
    assert N_ == N
    rb = alg.replay_buffer._module
    saved = (rb._states, rb.capacity, rb._host_ptr, rb._pointer.clone())
    states = torch.zeros(N, S, device=DEV)
    states[:, 0] = torch.arange(N, device=DEV)
    pointer = 357 if wrapped else N
    try:
        rb._states, rb.capacity = states, N
        rb._set_pointer(pointer)
        alg.rollout_batch_size = B
        noise = CountingNoise(CE_SEED)
        noise.ctr = ctr - 1
        im = alg_run(alg, None, horizon=1, members=0, noise=noise)
    finally:
        rb._states, rb.capacity = saved[0], saved[1]
        rb._set_pointer(int(saved[3]))
        alg.rollout_batch_size = RB
    assert noise.taken == [ctr]                                      # one counter per launch
    got = im.states[:, 0, 0].cpu().numpy().astype(np.int64)
    want = M.chrono_to_phys(M.sample_without_replacement(N, B, CE_SEED, ctr), pointer, N)
    assert np.array_equal(got, want)
    assert len(np.unique(got)) == B
    capped = M.chrono_to_phys(M.prp_index_capped(np.arange(B), N, CE_SEED, ctr)[0], pointer, N)
    assert len(np.unique(capped)) == B - 1 and got[row] != capped[row]


# ---------------------------------------------------------------------------
# one counter per launch
# ---------------------------------------------------------------------------
def test_fit_advances_the_counter_by_the_steps_of_a_chunk():
    """ensemble_engine.fit gathers a chunk of k steps in one launch with ctr .. ctr + k - 1 and
    takes k counters for it, then one for the holdout gather: steps + 1 in all, consecutive."""
    alg = fresh_alg(3, 2)
    g = np.random.RandomState(0)
    n = 600
    alg.replay_buffer.extend(states=torch.from_numpy(g.randn(n, 3).astype(np.float32)).to(DEV),
                             actions=torch.from_numpy(g.uniform(-1, 1, (n, 2)).astype(np.float32)).to(DEV),
                             next_states=torch.from_numpy(g.randn(n, 3).astype(np.float32)).to(DEV),
                             rewards=torch.from_numpy(g.randn(n).astype(np.float32)).to(DEV),
                             dones=torch.zeros(n, dtype=torch.bool, device=DEV),
                             violations=torch.zeros(n, dtype=torch.bool, device=DEV),
                             constraint_values=torch.zeros(n, device=DEV))
    noise = CountingNoise(7)
    noise.ctr = 100
    alg.model_ensemble.fit(alg.replay_buffer, steps=5, noise=noise)
    torch.cuda.synchronize()
    assert noise.taken == list(range(101, 107))


def test_each_drawing_op_takes_one_counter():
    """ops.policy_act (site 9) and the constraint critic's sampled forward (site 0xcc01) take
    one counter each, and policy_act's action is the model's draw at that counter."""
    alg = wide_alg(3, 2)
    noise = CountingNoise(ROLL_SEED)
    noise.ctr = 41
    s = start_states(RB, 3)
    a = ops.policy_act(alg.actor, s, False, noise)
    assert noise.taken == [42]
    z, m = M.normal_at(ROLL_SEED, 42, M.SITE_ACT, np.arange(RB * 2))
    std = np.exp(-6 + 10 / (1 + np.exp(-A_STD_RAW)))
    ref = np.tanh(z * std)
    # tanhf, expf, the sigmoid and the product: C_LIBM roundings of |u| <= |a| / (1 - a^2), plus the draw's
    bound = (C_LIBM * np.abs(z * std) + C_HW * m * std) * U32
    err = np.abs(a.reshape(-1).cpu().double().numpy() - ref)
    print(f'edge-ratio policy_act site 9: max err/bound {float((err / bound).max()):.3g}')
    assert float((err / bound).max()) <= 1.0
    mu, sd, q = ops.constraint_critic_forward(alg.constraint_critic, s, a, sample=True, noise=noise)
    torch.cuda.synchronize()
    assert noise.taken == [42, 43]
    e = head_draws(q.numel(), 1, ROLL_SEED, 43, M.SITE_CC_DIST).reshape(q.shape).clamp(-2, 2)
    ref = mu.double() + e.double() * sd.double()                # the kernel may contract it into an FMA: 1 ulp
    assert bool(((q.double() - ref).abs() <= 2 * U32 * (mu.abs() + (e * sd).abs()).double()).all())
    assert float((q - mu).abs().max()) > 0


# ---------------------------------------------------------------------------
# the critic update's sites in the production launch: 1, 2 (chained heads) and 7
# ---------------------------------------------------------------------------
def recorded_site_noise(seed, ctr0, normal_sites, randn_sites):
    """A DeviceNoise whose host hooks hand the kernels, as recorded draws, what the kernels
    would draw themselves at the counter the step is about to take: the k-th normal() the
    draws of normal_sites[k], the k-th used randn_like() those of randn_sites[k]
    (drpo_policy_head returns them for any site)."""
    from drpo_amd.rng import DeviceNoise

    class Recorded(DeviceNoise):
        def __init__(self):
            super().__init__(seed, rank=0, world=1)
            self.ctr = ctr0
            self.todo = [list(normal_sites), list(randn_sites)]

        def _draws(self, shape, site):
            shape = tuple(shape)
            A = shape[1] if len(shape) > 1 else 1
            return head_draws(shape[0], A, self.seed, self.ctr + 1, site).reshape(shape).cpu().numpy()

        def normal(self, shape):
            return self._draws(shape, self.todo[0].pop(0))

        def randn_like(self, shape, used=True):
            return self._draws(shape, self.todo[1].pop(0)) if used else None
    return Recorded()


def test_critic_update_draws_at_sites_1_2_and_7():
    """One update_critic (distributional certificate, B = 40: two full 16-row tiles and one of
    8) on device noise, and on recorded draws equal to sites 1 (a' ~ pi(s'), with its
    log-prob), 2 (a'_safe) and 7 (the clamped target noise) at the step's counter: both losses
    and every critic parameter after the step are equal bit for bit."""
    import bench
    from drpo_amd.rng import DeviceNoise
    from test_gpu_configs import _sac_batch
    B, seed, ctr0 = 40, SEEDS[1], 0x89ABCDEE
    res = []
    for recorded in (False, True):
        torch.manual_seed(5)
        alg = bench.make_alg(DEV, B, 3, 3, 5, bench.QUAD_JSON)
        sol = alg.solver
        assert sol.distributional_qc and sol.qc_under_uncertainty
        batch = [b.to(DEV) for b in _sac_batch(alg, 'quadrotor', bench.QUAD_JSON, B, 3)]
        if recorded:
            noise = recorded_site_noise(seed, ctr0, [M.SITE_PI_NEXT, M.SITE_SAFE_NEXT], [M.SITE_TARGET])
        else:
            noise = DeviceNoise(seed, rank=0, world=1)
            noise.ctr = ctr0
        lq, lqc = sol.update_critic(*batch, noise=noise)
        torch.cuda.synchronize()
        assert noise.ctr == ctr0 + 1                                  # one counter for the whole step
        if recorded:
            assert noise.todo == [[], []]
        res.append((lq.clone(), lqc.clone(), sol.critic_group.data.clone()))
    (lq0, lqc0, p0), (lq1, lqc1, p1) = res
    assert bool(torch.isfinite(lq0)) and bool(torch.isfinite(lqc0))
    assert torch.equal(bits(lq0.reshape(1)), bits(lq1.reshape(1)))
    assert torch.equal(bits(lqc0.reshape(1)), bits(lqc1.reshape(1)))
    assert torch.equal(bits(p0), bits(p1))
