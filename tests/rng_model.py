"""Bit-exact host model of the device random streams (numpy integers only, no device).

What the kernels draw is a pure function of (seed, ctr, site, index):

* ``philox4x32_10``: the counter generator of csrc/common.hpp (``philox``), the standard
  Philox4x32-10 of Random123. The key is ``(seed & 0xffffffff, seed >> 32)``.
* ``unit`` / ``normals``: the map of a 32-bit word to (0, 1] (``u32_to_unit``) and the
  four Box-Muller normals of a counter (``philox_normal4``), here in float64.
* ``prp_keys`` / ``hb_for`` / ``prp_index``: the keyed Feistel permutation of
  csrc/prp.hpp with its cycle walk. ``prp_index_capped`` is the walk as it was before it
  lost its cap (64 steps, then ``x % N``): kept for the counterexamples of
  tests/test_rng_model.py only.
* one function per draw site, returning the four counter words of every draw the site
  makes in one launch (and, for the normals, the lane of the element among the four).

Two properties the code has, stated here and pinned by tests/test_rng_model.py:

* ``prp_keys`` reads the seed byte-shifted by 0, 8, 16 and 24 bits and truncated to 32
  bits, so it sees seed bits 0..55: bits 56..63 do not enter the permutation.
* every site truncates ``ctr`` to 32 bits (``(uint32_t)ctr``; the gather adds the step
  first), so ``ctr`` and ``ctr + 2^32`` address the same draws.

Counter layout, (word 0, word 1, word 2, word 3), as read from the kernels:

=====================  ==========================================================
``normal_at``          ``(idx >> 2, idx >> 34, site, ctr)``, lane ``idx & 3``
                       sites 1, 2, 5, 6, 8 (sac_step.py), 9 (ops.policy_act),
                       7 (critic_rows.hpp, clamped to +-2), 0xcc01 (drpo_cc_dist)
``drpo_ens_head``      ``normal_at`` with site 0xe5a1, idx the OUTPUT index
                       ``(zo * n + row) * (S + 1) + k`` (member offset included)
``drpo_ens_gather``    ``(i, i >> 32, 0xe5e3b1, ctr + step)``; chronological row
                       ``((y << 32) | x) mod n``, then ``chrono_to_phys``
``drpo_sample_batch``  ``(j, 0 real | 1 virtual, 0x5a4d11, ctr)``; row
                       ``(x * len) >> 32``
rollout engines        ``(row, (t << 8) | kind, q, ctr)``: kind 0 the action
                       dimensions 4q..4q+3, kind 1 the model outputs 4q..4q+3
=====================  ==========================================================

"row" of the rollout engines: the fused-horizon engine (engine 2, and every
``rollout_trajectories`` entry point) keeps a batch row in its tile for the whole horizon,
so row is the ORIGINAL batch row at every step. The step engine (engine 1) compacts the
live rows before every step and keys by ``row0 + r`` AFTER compaction: at step t a row is
keyed by its rank among the rows still alive (ranks keep the original order), so a row
that ends shifts every later row down by one from the next step on.
"""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

SITE_PI_NEXT, SITE_SAFE_NEXT, SITE_PI_RS, SITE_SAFE_RS, SITE_TARGET, SITE_PI_MULT, SITE_ACT = 1, 2, 5, 6, 7, 8, 9
SITE_CC_DIST = 0xcc01
SITE_ENS_HEAD = 0xe5a1
SITE_GATHER = 0xe5e3b1
SITE_SAMPLE_BATCH = 0x5a4d11
NORMAL_AT_SITES = (SITE_PI_NEXT, SITE_SAFE_NEXT, SITE_PI_RS, SITE_SAFE_RS, SITE_TARGET, SITE_PI_MULT, SITE_ACT,
                   SITE_CC_DIST, SITE_ENS_HEAD)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & M32, seed >> 32


def philox4x32_10(counter, key, m1=PHILOX_M1):
    """counter: [..., 4] 32-bit words, key: (k0, k1) -> [..., 4] uint32. Vectorised.
    (m1: the second multiplier, a parameter only so that a test can show that the known
    answers depend on it.)"""
    c = _u64(counter) & _u64(M32)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m32 = _u64(M32)
    for _ in range(10):
        p0 = _u64(PHILOX_M0) * c0          # 32 x 32 -> 64 bits, exact in uint64
        p1 = _u64(m1) * c2
        hi0, lo0 = p0 >> _u64(32), p0 & m32
        hi1, lo1 = p1 >> _u64(32), p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ _u64(k0), lo1, hi0 ^ c3 ^ _u64(k1), lo0
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def philox_words(seed, counter):
    """The four output words of every counter [..., 4] under ``seed``."""
    return philox4x32_10(counter, philox_key(seed))


def unit(v):
    """u32_to_unit: ((v >> 8) + 1) / 2^24, in (0, 1]; exact in float32 and float64."""
    return ((_u64(v) >> _u64(8)) + _u64(1)).astype(np.float64) / 16777216.0


def box_muller_radius(words):
    """m = sqrt(-2 ln u1), sqrt(-2 ln u3) of output words [..., 4] -> [..., 2] float64"""
    w = np.asarray(words)
    return np.sqrt(-2.0 * np.log(unit(w[..., [0, 2]])))


def normals_of_words(words):
    """The four float64 normals of output words [..., 4]: m1 cos, m1 sin, m2 cos, m2 sin
    (angles 2 pi u2, 2 pi u4), and the radius of each: ([..., 4], [..., 4])."""
    w = np.asarray(words)
    m = box_muller_radius(w)
    ang = 2.0 * np.pi * unit(w[..., [1, 3]])
    z = np.stack([m[..., 0] * np.cos(ang[..., 0]), m[..., 0] * np.sin(ang[..., 0]),
                  m[..., 1] * np.cos(ang[..., 1]), m[..., 1] * np.sin(ang[..., 1])], -1)
    return z, np.repeat(m, 2, axis=-1)


def normals(seed, counter):
    """philox_normal4 in float64: (z [..., 4], radius [..., 4])"""
    return normals_of_words(philox_words(seed, counter))


def _words(c0, c1, c2, c3):
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    return (np.stack([c0, c1, c2, c3], -1) & _u64(M32)).astype(np.uint32)


# ---------------------------------------------------------------------------
# draw sites: counter words of every draw of one launch
# ---------------------------------------------------------------------------
def normal_at_words(idx, site, ctr):
    """normal_at(idx): (words [n, 4], lane [n])"""
    idx = _u64(idx)
    return _words(idx >> _u64(2), idx >> _u64(34), site, int(ctr) & M32), (idx & _u64(3)).astype(np.int64)


def normal_at(seed, ctr, site, idx):
    """float64 value and Box-Muller radius of normal_at at every idx"""
    w, lane = normal_at_words(idx, site, ctr)
    z, m = normals(seed, w)
    k = np.arange(len(lane))
    return z[k, lane], m[k, lane]


def site_policy_head(B, A, site, ctr):
    """squashed_gaussian_row (drpo_policy_head and the fused heads): element i * A + d"""
    return normal_at_words(np.arange(B * A), site, ctr)


def site_target_noise(B, A, ctr):
    """critic_rows.hpp: the clamped target noise, site 7, element k of [B, A]"""
    return normal_at_words(np.arange(B * A), SITE_TARGET, ctr)


def site_cc_dist(n, ctr):
    """drpo_cc_dist mode 1: element i of rows * C"""
    return normal_at_words(np.arange(n), SITE_CC_DIST, ctr)


def ens_head_index(zo, n, S):
    """output indices of member slot zo: (zo * n + row) * (S + 1) + k"""
    return zo * n * (S + 1) + np.arange(n * (S + 1))


def site_ens_head(Z, n, S, ctr):
    """drpo_ens_head with Z output members: dst = (zo * n + row) * (S + 1) + k"""
    return normal_at_words(np.arange(Z * n * (S + 1)), SITE_ENS_HEAD, ctr)


def site_gather(rows, steps, ctr):
    """drpo_ens_gather_steps: one draw per (step, row): (i, i >> 32, site, ctr + step)"""
    st, i = np.divmod(np.arange(steps * rows), rows)
    i = _u64(i)
    return _words(i, i >> _u64(32), SITE_GATHER, (int(ctr) + st) & M32)


def site_sample_batch(n_real, B, ctr):
    """drpo_sample_batch: rows [0, n_real) real (j = i), the others virtual (j = i - n_real)"""
    i = np.arange(B)
    virt = i >= n_real
    return _words(np.where(virt, i - n_real, i), virt.astype(np.int64), SITE_SAMPLE_BATCH, int(ctr) & M32)


def rollout_words(row, t, kind, q, ctr):
    return _words(row, (_u64(t) << _u64(8)) | _u64(kind), q, int(ctr) & M32)


def site_rollout(B, H, A, S, ctr, rows_per_tile=16):
    """Every counter one rollout launch (either engine) can touch: all tile rows (the
    padding rows of the last tile draw too and are discarded), every step, both kinds."""
    nrow = -(-B // rows_per_tile) * rows_per_tile
    na, nm = (A + 3) // 4, (S + 1 + 3) // 4
    out = []
    for kind, nq in ((0, na), (1, nm)):
        row, t, q = np.meshgrid(np.arange(nrow), np.arange(H), np.arange(nq), indexing='ij')
        out.append(rollout_words(row.ravel(), t.ravel(), kind, q.ravel(), ctr))
    return np.concatenate(out)


def rollout_normals(seed, ctr, rows, t, kind, n):
    """float64 normals and radii [len(rows), n] of elements 0..n-1 (action dimensions for
    kind 0, model outputs for kind 1) of the given key rows at step t"""
    rows = np.asarray(rows)
    nq = (n + 3) // 4
    r, q = np.meshgrid(rows, np.arange(nq), indexing='ij')
    z, m = normals(seed, rollout_words(r.ravel(), t, kind, q.ravel(), ctr))
    return z.reshape(len(rows), nq * 4)[:, :n], m.reshape(len(rows), nq * 4)[:, :n]


def step_engine_key_rows(alive_before):
    """Step engine: the key row of every ORIGINAL batch row at one step, given which rows
    are alive when the step begins (bool [B]): its rank among the live rows; -1 where the
    row has ended."""
    alive = np.asarray(alive_before, dtype=bool)
    return np.where(alive, np.cumsum(alive) - 1, -1)


# ---------------------------------------------------------------------------
# index draws
# ---------------------------------------------------------------------------
def chrono_to_phys(j, ptr, cap):
    j = np.asarray(j, dtype=np.int64)
    return (ptr % cap + j) % cap if ptr > cap else j


def gather_rows(seed, ctr, rows, steps, ptr, cap):
    """physical replay row of every (step, row) of drpo_ens_gather_steps: [steps * rows]"""
    n = min(ptr, cap)
    w = philox_words(seed, site_gather(rows, steps, ctr)).astype(np.uint64)
    x64 = (w[:, 1] << _u64(32)) | w[:, 0]
    return chrono_to_phys((x64 % _u64(n)).astype(np.int64), ptr, cap)


def sample_batch_rows(seed, ctr, n_real, B, len_real, len_virt):
    """buffer row of every output row of drpo_sample_batch: (x * len) >> 32"""
    w = philox_words(seed, site_sample_batch(n_real, B, ctr)).astype(np.uint64)
    ln = np.where(np.arange(B) >= n_real, len_virt, len_real).astype(np.uint64)
    return ((w[:, 0] * ln) >> _u64(32)).astype(np.int64)      # x < 2^32, len < 2^31: exact in uint64


# ---------------------------------------------------------------------------
# keyed Feistel permutation (csrc/prp.hpp)
# ---------------------------------------------------------------------------
def prp_keys(seed, ctr):
    """key[i] = uint32(seed >> 8 i) * 0x9E3779B9 + uint32(ctr) * (2 i + 1) + i. Seed bits
    56..63 never enter (the largest shift is 24, then 32 bits are kept), and only the
    low 32 bits of ctr do."""
    seed, c = int(seed) & 0xFFFFFFFFFFFFFFFF, int(ctr) & M32
    return [((((seed >> (8 * i)) & M32) * 0x9E3779B9) + c * (2 * i + 1) + i) & M32 for i in range(4)]


def hb_for(n):
    b = 1
    while (1 << (2 * b)) < n:
        b += 1
    return b


def _prp_round(r, k):
    m32 = _u64(M32)
    h = ((r * _u64(0x9E3779B1)) & m32) ^ _u64(k)
    h ^= h >> _u64(15)
    h = (h * _u64(0x85EBCA77)) & m32
    h ^= h >> _u64(13)
    h = (h * _u64(0xC2B2AE3D)) & m32
    h ^= h >> _u64(16)
    return h


def _feistel(x, hb, key):
    mask = _u64((1 << hb) - 1)
    L, R = (x >> _u64(hb)) & mask, x & mask
    for k in key:
        L, R = R, L ^ (_prp_round(R, k) & mask)
    return (L << _u64(hb)) | R


def prp_index(i, N, seed, ctr, cap=None):
    """prp_index for every i (array) -> (index [n] int64, walk length [n]). cap=None: the
    walk ends when it lands in [0, N). cap=k: the walk as it was before, at most k steps
    and then ``x % N``."""
    key, hb = prp_keys(seed, ctr), hb_for(N)
    x = _u64(i).copy()
    assert x.size == 0 or int(x.max()) < N, 'the walk is defined for i < N only'
    out = np.zeros(x.shape, dtype=np.int64)
    steps = np.zeros(x.shape, dtype=np.int64)
    live = np.arange(x.size)
    it = 0
    while live.size and (cap is None or it < cap):
        x = _feistel(x, hb, key)
        it += 1
        done = x < _u64(N)
        out[live[done]] = x[done].astype(np.int64)
        steps[live[done]] = it
        live, x = live[~done], x[~done]
    if live.size:                                       # capped walk only
        out[live] = (x % _u64(N)).astype(np.int64)
        steps[live] = cap + 1                           # marks the fallback
    return out, steps


def prp_index_capped(i, N, seed, ctr):
    """the 64-step walk with the ``x % N`` fallback: not a permutation (test_rng_model.py)"""
    return prp_index(i, N, seed, ctr, cap=64)


def sample_without_replacement(N, B, seed, ctr):
    return prp_index(np.arange(B), N, seed, ctr)[0]
