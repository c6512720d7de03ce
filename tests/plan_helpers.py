"""What the tests of planning on the model share (drpo_plan_sample, drpo_plan_refit, SMBPO.plan):
the two definitions of include/drpo_hip.h restated in float64, the synthetic candidates and the
comparisons.

plan_refit_reference. Scores come from lookahead_helpers.lookahead_reference with zero step_q /
step_qc, entry H (at k = H a row's bootstrap is its terminal one, so the step values are never
read). The order, the elites and the weights are plain Python on the float32 values; the refit is
one numpy float64 operation per step of the definition, in candidate order (numpy's elementwise
operations round once and fuse nothing)."""
import math

import numpy as np
import torch

import rng_model
from lookahead_helpers import NAN, lookahead_reference

INF = float('inf')
THRESHOLD = -0.125          # exact in float32: a certificate can equal it
PER_STATE = ('best', 'n_feasible', 'best_score', 'best_cert', 'best_feasible')
PER_ROW = ('score', 'cert', 'rank', 'weight')


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def plan_scores(x, *, gamma, mode, scales):
    """(score [B], cert [B]) float32: entry H of the lookahead of the rows ``x`` (a dict of
    rewards, constraint_values, dones, violations, lengths, terminated, terminal_q, terminal_qc),
    and the maximum over the critic's outputs, a NaN staying, canonical."""
    B, H = tuple(x['rewards'].shape)
    C = int(x['terminal_qc'].shape[-1])
    v, c = lookahead_reference(x['rewards'], x['constraint_values'], x['dones'], x['violations'], x['lengths'],
                               x['terminated'], torch.zeros(B, H), torch.zeros(B, H, C), x['terminal_q'],
                               x['terminal_qc'], gamma=gamma, mode=mode, **scales)
    score, last = v[:, H].copy(), c[:, H]
    cert = last[:, 0].copy()
    for k in range(1, C):
        nan = np.isnan(cert) | np.isnan(last[:, k])
        cert = np.where(nan, np.float32(NAN), np.maximum(cert, last[:, k]))
    return score, cert.astype(np.float32)


def plan_order(score, cert, threshold):
    """Of one state's N float32 scores and certs: (order: the n of rank 0, 1, ..; cls [N]: 0
    feasible, 1 valid and not feasible, 2 invalid; key [N] float: score, -cert, 0)."""
    N = len(score)
    thr = float(np.float32(threshold))
    cls, key = [], []
    for n in range(N):
        s, c = float(score[n]), float(cert[n])
        if s != s or c != c:
            cls.append(2), key.append(0.0)
        elif c <= thr:
            cls.append(0), key.append(s)
        else:
            cls.append(1), key.append(-c)
    order = sorted(range(N), key=lambda n: (cls[n], -key[n], n))     # (-0.0 and 0.0 compare equal: the lower n)
    return order, cls, key


def plan_refit_reference(x, cand, mean_in, std_in, *, N, gamma, mode, scales, threshold, elites, temperature,
                         momentum, min_std, scores=None, flip_ties=False, ignore_feasibility=False):
    """drpo_plan_refit on CPU tensors: a dict of numpy arrays named as ops.plan_refit's. ``scores``:
    (score, cert) of plan_scores, if the caller has them. flip_ties / ignore_feasibility: the two
    wrong definitions of the mutation check (profiles/plan/README.md), never the reference."""
    cand, mean_in, std_in = (_np(t).astype(np.float32) for t in (cand, mean_in, std_in))
    P, K, A = mean_in.shape
    assert cand.shape == (P * N, K, A)
    score, cert = plan_scores(x, gamma=gamma, mode=mode, scales=scales) if scores is None else scores
    thr = float(np.float32(threshold)) if not ignore_feasibility else INF
    out = {'score': score.reshape(P, N), 'cert': cert.reshape(P, N), 'rank': np.zeros((P, N), np.int32),
           'weight': np.zeros((P, N), np.float32), 'best': np.zeros(P, np.int32), 'n_feasible': np.zeros(P, np.int32),
           'best_score': np.zeros(P, np.float32), 'best_cert': np.zeros(P, np.float32),
           'best_feasible': np.zeros(P, bool), 'mean': mean_in.copy(), 'std': std_in.copy(),
           'best_actions': np.zeros((P, K, A), np.float32)}
    keep = 1.0 - float(momentum)
    for p in range(P):
        s, c = out['score'][p], out['cert'][p]
        order, cls, key = plan_order(s, c, thr)
        if flip_ties:
            order = sorted(range(N), key=lambda n: (cls[n], -key[n], -n))
        for pos, n in enumerate(order):
            out['rank'][p, n] = pos
        nf, nv = cls.count(0), N - cls.count(2)
        best = order[0] if nv else 0
        Ke = min(elites, nf if nf > 0 else nv)
        w = [0.0] * N
        for n in order[:Ke]:
            diff = 0.0 if key[n] == key[best] else key[n] - key[best]
            w[n] = 1.0 if math.isinf(temperature) else math.exp(diff / temperature)
        out['weight'][p] = np.asarray(w, np.float64).astype(np.float32)
        out['best'][p], out['n_feasible'][p] = best, nf
        out['best_score'][p], out['best_cert'][p], out['best_feasible'][p] = s[best], c[best], cls[best] == 0
        rows = cand[p * N:(p + 1) * N].astype(np.float64)
        out['best_actions'][p] = cand[p * N + best]
        sw, swx = 0.0, np.zeros((K, A))
        for n in range(N):
            if w[n] > 0.0:
                sw = sw + w[n]
                swx = swx + w[n] * rows[n]
        if not sw > 0.0:
            continue
        m = swx / sw
        sv = np.zeros((K, A))
        for n in range(N):
            if w[n] > 0.0:
                dx = rows[n] - m
                sv = sv + w[n] * (dx * dx)
        sd = keep * np.sqrt(sv / sw) + float(momentum) * std_in[p].astype(np.float64)
        out['mean'][p] = (keep * m + float(momentum) * mean_in[p].astype(np.float64)).astype(np.float32)
        out['std'][p] = np.where(sd < min_std, min_std, sd).astype(np.float32)
    return out


def plan_sample_reference(mean, std, incumbent, *, N, seed, ctr, lo=-1.0, hi=1.0):
    """drpo_plan_sample in float64: (cand [P * N, K, A] float64, with candidate 0 the incumbent
    as float32 bits; the Box-Muller radius of every draw, the same shape)."""
    mean, std, incumbent = (_np(t).astype(np.float32) for t in (mean, std, incumbent))
    P, K, A = mean.shape
    total = P * N * K * A
    z, radius = rng_model.normal_at(seed, ctr, rng_model_site(), np.arange(total))
    z, radius = z.reshape(P, N, K, A), radius.reshape(P, N, K, A)
    x = std[:, None].astype(np.float64) * z + mean[:, None].astype(np.float64)
    x = np.minimum(np.maximum(x, np.float64(np.float32(lo))), np.float64(np.float32(hi)))
    x[:, 0] = incumbent
    return x.reshape(P * N, K, A), radius.reshape(P * N, K, A)


def rng_model_site():
    from drpo_amd import _abi
    return _abi.PLAN_SITE


# ------------------------------------------------------------------ synthetic candidates
SCALES = dict(reward_scale=0.5, alive_bonus=1.0, constraint_scale=10.0, constraint_offset=0.5)
P_STATES = 5


def synthetic_plan(N, H, K, A, C, seed=0):
    """Inputs of drpo_plan_refit for P_STATES start states, built by position: (x, cand, mean_in,
    std_in) as CPU tensors. A 'controlled' row has length 0 and is not terminated, so that its score
    is its terminal_q and its cert its largest terminal_qc, whatever the mode.
      state 0  controlled rows, every cert above THRESHOLD (several equal): no feasible row
      state 1  controlled rows, the last one alone feasible
      state 2  controlled feasible rows whose scores come in equal pairs (n, n + 1)
      state 3  a NaN score on the even rows, a NaN cert on the odd ones: no valid row
      state 4  row 0 controlled with cert == THRESHOLD; rows 1.. as a rollout leaves them, lengths
               H, H, 0, 1, .. terminated (with the done bit at the last step) and not; from N 6 on
               rows 4 and 5 are controlled with a NaN score and a NaN cert among valid rows"""
    P, B = P_STATES, P_STATES * N
    g = torch.Generator().manual_seed(100000 * N + 1000 * H + 10 * C + A + seed)
    lengths = torch.zeros(B, dtype=torch.int32)
    terminated = torch.zeros(B, dtype=torch.bool)
    rewards = torch.randn(B, H, generator=g)
    cvals = 0.05 * torch.randn(B, H, C, generator=g) - 0.02
    terminal_q = 3 * torch.randn(B, generator=g)
    terminal_qc = 0.5 * torch.randn(B, C, generator=g) - 0.3
    violations = torch.rand(B, H, generator=g) < 0.15
    dones = torch.zeros(B, H, dtype=torch.bool)

    def controlled(r, score, cert):
        lengths[r], terminated[r], terminal_q[r] = 0, False, score
        terminal_qc[r] = cert - 1.0 if cert == cert else cert
        terminal_qc[r, (r % C)] = cert                      # the largest output, in any column
    for n in range(N):
        controlled(0 * N + n, float(terminal_q[n]), THRESHOLD + 0.25 * (1 + (n * 7) % 5))
        controlled(1 * N + n, float(terminal_q[N + n]), THRESHOLD - 1.0 if n == N - 1 else THRESHOLD + 0.5 + n % 3)
        controlled(2 * N + n, float(((n // 2) * 3) % 7) - 2.0, THRESHOLD - 0.5 - (n % 3))
        controlled(3 * N + n, NAN if n % 2 == 0 else 1.0, NAN if n % 2 == 1 else THRESHOLD - 1.0)
    r0 = 4 * N
    controlled(r0, 1.0, THRESHOLD)
    for n in range(1, N):
        r = r0 + n
        lengths[r] = H if n <= 2 else (n - 3) % (H + 1)
        terminated[r] = bool(n % 2 == 1 and lengths[r] > 0)
        if terminated[r]:
            dones[r, int(lengths[r]) - 1] = True
    if N >= 6:
        controlled(r0 + 4, NAN, THRESHOLD - 1.0)
        controlled(r0 + 5, 0.5, NAN)
    mask = torch.arange(H) < lengths.unsqueeze(-1)           # as ImaginedRollout holds them: zero beyond the length
    rewards, violations, cvals = rewards * mask, violations & mask, cvals * mask.unsqueeze(-1)
    x = dict(rewards=rewards, constraint_values=cvals, dones=dones, violations=violations, lengths=lengths,
             terminated=terminated, terminal_q=terminal_q, terminal_qc=terminal_qc)
    cand = torch.rand(B, K, A, generator=g) * 2 - 1
    mean_in = torch.rand(P, K, A, generator=g) - 0.5
    std_in = torch.rand(P, K, A, generator=g) * 0.5 + 0.1
    return x, cand, mean_in, std_in


def assert_plan_synthetic_shows_every_case(x, ref, N, H, elites):
    """Otherwise the comparison shows nothing. ``ref``: plan_refit_reference's outputs for ``x``
    at THRESHOLD."""
    thr = np.float32(THRESHOLD)
    score, cert, nf = ref['score'], ref['cert'], ref['n_feasible']
    valid = ~np.isnan(score) & ~np.isnan(cert)
    nv = valid.sum(1)
    assert ((nf == 0) & (nv > 0)).any(), 'a state with no feasible row'
    assert (nf == 1).any(), 'a state with exactly one feasible row'
    if elites > 1:
        assert ((nf > 0) & (nf < elites)).any(), 'n_feasible < elites'
    tie = False
    for p in range(len(nf)):
        _, cls, key = plan_order(score[p], cert[p], thr)
        seen = {(c, k) for c, k in zip(cls, key) if c == 0}
        tie |= len(seen) < cls.count(0)
    assert tie, 'equal scores among feasible rows'
    assert (np.isnan(score) & ~np.isnan(cert)).any() and (np.isnan(cert) & ~np.isnan(score)).any()
    assert (nv == 0).any(), 'a state with no valid row'
    at = np.argwhere(valid & (cert == thr))
    assert len(at) and all(ref['rank'][p, n] < nf[p] for p, n in at), 'a cert equal to the threshold is feasible'
    n, term = x['lengths'].numpy(), x['terminated'].numpy()
    assert int(n.min()) == 0 and int(n.max()) == H and term.any() and (~term).any()
    if N - 6 >= H + 1:
        assert set(n.tolist()) == set(range(H + 1))


def bits(a):
    a = _np(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.bool_ or w.dtype == np.bool_:
        g, w = g.astype(np.int32), w.astype(np.int32)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}'
