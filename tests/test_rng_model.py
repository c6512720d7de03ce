"""The host model of the device random streams (tests/rng_model.py) against what is known
without a device: the Random123 known answers, the permutation property of the cycle walk
(and the five calls at which the capped walk repeated an index), the uniformity of the
samples, and the disjointness of the counters that the draw sites of one training
iteration address. The GPU side of the same model is tests/test_gpu_rng_streams.py."""
import numpy as np
import pytest

import rng_model as M

KNOWN_ANSWERS = [     # Random123 kat_vectors, philox4x32 10 rounds: counter, key, result
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     'd16cfe09 94fdcceb 5001e420 24126ea1'),
]

# seed 0x1234567, B = N: the capped walk's fallback at row i returned `value`, which
# another row of the same call returns too
COUNTEREXAMPLES = [(257, 431086, 125, 153), (1025, 54677, 868, 914), (4097, 32881, 496, 3556),
                   (16385, 4749, 2802, 10668), (65537, 181, 63202, 35596)]
CE_SEED = 0x1234567


def hexwords(w):
    return ' '.join('%08x' % int(v) for v in w)


@pytest.mark.parametrize('counter,key,want', KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    assert hexwords(M.philox4x32_10(np.array(counter, dtype=np.uint64), key)) == want
    # vectorised: the same answer in every row of a batch, next to other counters
    batch = np.array([counter, (1, 2, 3, 4), counter], dtype=np.uint64)
    out = M.philox4x32_10(batch, key)
    assert hexwords(out[0]) == want and hexwords(out[2]) == want and hexwords(out[1]) != want
    # the answers depend on every bit of the round constants (one bit of the second one)
    assert hexwords(M.philox4x32_10(np.array(counter, dtype=np.uint64), key, m1=M.PHILOX_M1 ^ 1)) != want


def test_key_is_seed_low_high():
    c = np.array([5, 6, 7, 8], dtype=np.uint64)
    seed = 0xa4093822 | (0x299f31d0 << 32)
    assert M.philox_key(seed) == (0xa4093822, 0x299f31d0)
    assert np.array_equal(M.philox_words(seed, c), M.philox4x32_10(c, (0xa4093822, 0x299f31d0)))


def test_unit_and_normals():
    assert M.unit(0) == 2.0 ** -24 and M.unit(0xff) == 2.0 ** -24 and M.unit(0x100) == 2.0 ** -23
    assert M.unit(0xffffffff) == 1.0 and M.unit(0xffffff00) == 1.0 and M.unit(0x7fffff00) == 0.5
    w = np.array([[0xffffff00, 0x3fffff00, 0, 0x7fffff00]], dtype=np.uint32)   # u = 1, 1/4, 2^-24, 1/2
    z, m = M.normals_of_words(w)
    r = np.sqrt(2 * 24 * np.log(2.0))                                        # 5.768
    assert m[0, 0] == 0 and m[0, 1] == 0 and abs(m[0, 2] - r) < 1e-12
    assert z[0, 0] == 0 and z[0, 1] == 0
    assert abs(z[0, 2] + r) < 1e-12 and abs(z[0, 3]) < 1e-14               # cos(pi) = -1, sin(pi) = 0
    # 2^17 draws: mean, variance and the share beyond 3 sigma, each within 5 standard errors
    z, _ = M.normals(77, M.normal_at_words(np.arange(0, 1 << 17, 4), 3, 1)[0])
    z = z.ravel()
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    p = 0.0026998
    assert abs((np.abs(z) > 3).mean() - p) < 5 * np.sqrt(p / n)


PRP_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 65536, 65537, 100000]
PRP_PAIRS = [(0, 0), (0x1234567, 1), (0xDEADBEEF12345, 40), (2 ** 64 - 1, 2 ** 32 - 1)]


@pytest.mark.parametrize('N', PRP_SIZES)
def test_prp_is_a_permutation(N):
    for seed, ctr in PRP_PAIRS:
        out, steps = M.prp_index(np.arange(N), N, seed, ctr)
        assert np.array_equal(np.sort(out), np.arange(N)), (N, seed, ctr)
        # these calls never reach the old cap, so the capped walk agrees on them
        assert steps.max() <= 64
        assert np.array_equal(M.prp_index_capped(np.arange(N), N, seed, ctr)[0], out)
        # the first B outputs of a call do not depend on B
        assert np.array_equal(M.sample_without_replacement(N, (N + 1) // 2, seed, ctr), out[:(N + 1) // 2])


@pytest.mark.parametrize('N,ctr,row,value', COUNTEREXAMPLES)
def test_capped_walk_repeats_an_index(N, ctr, row, value):
    i = np.arange(N)
    capped, csteps = M.prp_index_capped(i, N, CE_SEED, ctr)
    out, steps = M.prp_index(i, N, CE_SEED, ctr)
    assert steps[row] > 64 and csteps[row] == 65            # the fallback was taken at that row only
    assert (csteps == 65).sum() == 1
    assert capped[row] == value
    twin = np.flatnonzero(capped == value)
    assert len(twin) == 2 and row in twin                    # exactly one other row returns it too
    assert len(np.unique(capped)) == N - 1
    assert np.array_equal(np.sort(out), i)                   # the uncapped walk: N distinct values
    other = i != row
    assert np.array_equal(out[other], capped[other])         # and nothing else moved
    assert out[row] != value


def test_sampling_is_unbiased():
    """N = 1000, B = 100, ctr = 1..4000: how often each index is included and how often
    it comes first against the uniform expectation (chi-square, 999 degrees of freedom,
    normal approximation, |z| <= 4), and the overlap of consecutive samples against
    B^2 / N (4 standard errors)."""
    N, B, seed, K = 1000, 100, 0xDEADBEEF12345, 4000
    samples = np.stack([M.sample_without_replacement(N, B, seed, c) for c in range(1, K + 1)])
    assert all(len(np.unique(s)) == B for s in samples)

    def z_of(counts, expect):
        chi2 = ((counts - expect) ** 2 / expect).sum()
        return (chi2 - (N - 1)) / np.sqrt(2.0 * (N - 1))

    # (an inclusion count is binomial, variance K p (1 - p) with p = B / N = 0.1, so the
    # expected statistic is nearer 900 than 999: the plain form leans to the negative side by
    # about 2, inside the bound. Values of this model: -0.77 and -0.40.)
    incl = np.bincount(samples.ravel(), minlength=N).astype(np.float64)
    z_incl = z_of(incl, K * B / N)
    first = np.bincount(samples[:, 0], minlength=N).astype(np.float64)
    z_first = z_of(first, K / N)
    print(f'chi-square z: inclusion {z_incl:.2f}, first {z_first:.2f}')
    assert abs(z_incl) <= 4 and abs(z_first) <= 4

    # ctr = 1..1000 against its successor: measured 10.18 +- 0.089
    ov = np.array([len(np.intersect1d(samples[c], samples[c + 1])) for c in range(1000)], dtype=np.float64)
    se = ov.std(ddof=1) / np.sqrt(len(ov))
    print(f'overlap of consecutive samples: {ov.mean():.2f} +- {se:.3f} (expected {B * B / N})')
    assert abs(ov.mean() - B * B / N) <= 4 * se


# ---------------------------------------------------------------------------
# disjoint streams
# ---------------------------------------------------------------------------
def keyset(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return {tuple(int(v) for v in r) for r in w}


def assert_unique(words, lanes=None):
    """no two draws of one launch share (counter, lane)"""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    if lanes is not None:
        w = np.concatenate([w, np.asarray(lanes, dtype=np.uint64).reshape(-1, 1)], 1)
    assert len(np.unique(w, axis=0)) == len(w)


SHAPES = [(64, A, S) for A in (2, 6) for S in (3, 12)]     # B, A, S; H = 3, Z = 2 below
H, Z, CTR = 3, 2, 1000


def launches(B, A, S, ctr):
    """the draw sites of one small training iteration, each as (words, lanes or None)"""
    out = {f'policy_head site {s}': M.site_policy_head(B, A, s, ctr)
           for s in (M.SITE_PI_NEXT, M.SITE_SAFE_NEXT, M.SITE_PI_RS, M.SITE_SAFE_RS, M.SITE_PI_MULT, M.SITE_ACT)}
    out['target noise'] = M.site_target_noise(B, A, ctr)
    out['cc_dist'] = M.site_cc_dist(B * 2, ctr)
    out['ens_head'] = M.site_ens_head(Z, B, S, ctr)
    out['gather'] = (M.site_gather(B, 4, ctr), None)
    out['sample_batch'] = (M.site_sample_batch(B // 4, B, ctr), None)
    out['rollout'] = (M.site_rollout(B, H, A, S, ctr), None)
    return out


@pytest.mark.parametrize('B,A,S', SHAPES)
def test_no_two_draws_of_a_launch_share_a_counter(B, A, S):
    for name, (w, lanes) in launches(B, A, S, CTR).items():
        assert_unique(w, lanes)


@pytest.mark.parametrize('B,A,S', SHAPES)
def test_sites_that_share_a_counter_value_do_not_overlap(B, A, S):
    """The safe-SAC update hands ONE ctr to several launches (sac_step.py: the heads 1, 2
    and the target noise 7 in update_critic; 5, 6 in the actor update; 8 in the
    multiplier update), so those sites must be disjoint among themselves at equal
    (seed, ctr). So must the index draws, the ensemble head and drpo_cc_dist against
    everything, whoever passes their ctr: the third word alone separates them."""
    L = launches(B, A, S, CTR)
    third_word_sites = [k for k in L if k != 'rollout']
    for i, a in enumerate(third_word_sites):
        for b in third_word_sites[i + 1:]:
            assert not (keyset(L[a][0]) & keyset(L[b][0])), (a, b)
    # the gather uses ctr .. ctr + steps - 1; no other site has its third word
    for c in range(CTR, CTR + 4):
        for k in third_word_sites:
            if k != 'gather':
                assert not (keyset(L['gather'][0]) & keyset(launches(B, A, S, c)[k][0])), (k, c)


@pytest.mark.parametrize('B,A,S', SHAPES)
def test_rollout_kinds_at_t0_against_normal_at_sites(B, A, S):
    """Both have a zero second word at t = 0 (kind 0: (row, 0, q, ctr); normal_at:
    (idx >> 2, 0, site, ctr)), and the rollout's third word q runs over 0 .. 3 where the
    policy heads' sites are 1, 2, 5 ...: at A > 4 the action draws of q = 1 ARE the
    counters of site 1 (elements 4 row .. 4 row + 3). Kind 1 has the second word 1 at
    t = 0 and (t << 8) | 1 later, kind 0 has t << 8 >= 256 later; normal_at's second word is
    idx >> 34, zero below 2^34 elements. So the only separation of a rollout from the
    normal_at sites is its own ctr: ops.rollout and ops.rollout_trajectories take one
    noise.next() per launch (test_gpu_rng_streams.py counts them)."""
    roll = M.site_rollout(B, 1, A, S, CTR)
    kind0 = keyset(roll[roll[:, 1] == 0])
    kind1 = keyset(roll[roll[:, 1] == 1])
    assert len(kind0) + len(kind1) == len(roll)
    L = launches(B, A, S, CTR)
    hit = {k for k in L if k != 'rollout' and kind0 & keyset(L[k][0])}
    # q = 0 matches no site (there is no site 0); q = 1 (A > 4) matches site 1 and nothing else
    assert hit == ({'policy_head site 1'} if A > 4 else set()), hit
    assert not any(kind1 & keyset(L[k][0]) for k in L if k != 'rollout')
    # with its own counter value the rollout is disjoint from every site
    own = keyset(M.site_rollout(B, H, A, S, CTR + 1))
    assert not any(own & keyset(L[k][0]) for k in L if k != 'rollout')
    # later steps and wide states (q up to 16 at S = 64) never reach a normal_at site either
    # way: second word >= 256
    late = M.site_rollout(B, H, A, S, CTR)
    late = late[late[:, 1] >= 256]
    assert len(late) and not any(keyset(late) & keyset(L[k][0]) for k in L if k != 'rollout')


def test_gather_of_k_steps_uses_k_counter_values():
    """A chunked gather of k steps draws with ctr, ctr + 1, ..., ctr + k - 1: the launch
    after it must start at ctr + k (ensemble_engine.fit takes k noise.next() per chunk)."""
    rows, k = 96, 4
    chunk = keyset(M.site_gather(rows, k, CTR))
    per_step = [keyset(M.site_gather(rows, 1, CTR + s)) for s in range(k)]
    assert chunk == set().union(*per_step) and len(chunk) == k * rows
    assert chunk & keyset(M.site_gather(rows, 1, CTR + 1))             # an advance by 1 would repeat rows
    assert not (chunk & keyset(M.site_gather(rows, k, CTR + k)))       # an advance by k does not
    # and the row values of step s are those of a one-step gather at ctr + s
    got = M.gather_rows(5, CTR, rows, k, 1234, 1000).reshape(k, rows)
    for s in range(k):
        assert np.array_equal(got[s], M.gather_rows(5, CTR + s, rows, 1, 1234, 1000))
    assert not np.array_equal(got[0], got[1])


class CountingNoise:
    """What the draw sites need of a DeviceNoise, counting the counters handed out."""

    def __new__(cls, seed=0):
        from drpo_amd.rng import DeviceNoise

        class Counting(DeviceNoise):
            def __init__(self, seed):
                super().__init__(seed, rank=0, world=1)
                self.taken = []

            def next(self):
                c = super().next()
                self.taken.append(c)
                return c
        return Counting(seed)


def test_device_noise_hands_out_each_counter_once():
    nz = CountingNoise(11)
    got = [nz.next() for _ in range(5)]
    assert got == [1, 2, 3, 4, 5] == nz.taken and nz.ctr == 5
    assert nz.collection() is nz                   # single process: one stream, one counter
    nz.rand((1, 2))                                # the host warm-up draw takes a counter too
    assert nz.taken[-1] == 6


def test_step_engine_key_rows():
    alive = np.array([True, True, False, True, False, True])
    assert M.step_engine_key_rows(alive).tolist() == [0, 1, -1, 2, -1, 3]
    assert M.step_engine_key_rows(np.ones(4, bool)).tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------------------
# key properties (pinned, not changed here)
# ---------------------------------------------------------------------------
def test_seed_bits_56_to_63_do_not_enter_the_prp_keys():
    for seed in (0, 0x1234567, 0x00FFFFFFFFFFFFFF):
        for hi in (1, 0x80, 0xFF):
            assert M.prp_keys(seed | (hi << 56), 9) == M.prp_keys(seed, 9)
        assert M.prp_keys(seed ^ (1 << 55), 9) != M.prp_keys(seed, 9)     # bit 55 does enter
    # ... while Philox takes all 64 bits of the seed
    c = np.array([1, 2, 3, 4], dtype=np.uint64)
    assert not np.array_equal(M.philox_words(1 << 63, c), M.philox_words(0, c))


def test_only_the_low_32_bits_of_ctr_are_used():
    ctr = 12345
    assert M.prp_keys(7, ctr) == M.prp_keys(7, ctr + 2 ** 32)
    idx = np.arange(40)
    for w in (M.normal_at_words(idx, 5, ctr)[0], M.site_gather(8, 3, ctr), M.site_sample_batch(3, 9, ctr),
              M.site_rollout(20, 2, 6, 12, ctr)):
        assert np.all(w[:, 3] >= ctr) and np.all(w[:, 3] < ctr + 3)
    assert np.array_equal(M.normal_at_words(idx, 5, ctr)[0], M.normal_at_words(idx, 5, ctr + 2 ** 32)[0])
    assert np.array_equal(M.site_gather(8, 3, ctr), M.site_gather(8, 3, ctr + 2 ** 32))
    assert np.array_equal(M.site_gather(8, 2, 2 ** 32 - 1)[:, 3], np.repeat([2 ** 32 - 1, 0], 8))   # wraps
    assert np.array_equal(M.site_sample_batch(3, 9, ctr), M.site_sample_batch(3, 9, ctr + 2 ** 32))
    assert np.array_equal(M.site_rollout(20, 2, 6, 12, ctr), M.site_rollout(20, 2, 6, 12, ctr + 2 ** 32))
