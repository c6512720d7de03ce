"""What the tests of planning over ensemble particles share (drpo_plan_refit_particles,
SMBPO.plan(particles=)): the definition of include/drpo_hip.h restated in float64 on plan_helpers'
pieces, and the synthetic member-major inputs.

plan_particles_reference. The member values are plan_helpers.plan_scores on the G * B flat rows
(a row's values depend on nothing but the row). The aggregation (particle_aggregate) is written out
literally, a Python loop per candidate: the members sorted by (score, j), the first T added one
after the other as doubles, one division, one rounding to float32; the certificate's maximum
with a NaN staying, or its ordered sum over G; the spread from the ordered mean. Steps b-e are
plan_helpers.plan_refit_reference on the aggregated float32 values."""
import math

import numpy as np
import torch

from plan_helpers import THRESHOLD, _np, plan_refit_reference, plan_scores, synthetic_plan

QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _f32(x):
    """a float64 rounded to float32 once, a NaN as the canonical quiet NaN"""
    with np.errstate(over='ignore', invalid='ignore'):
        f = np.float32(x)
    return QNAN if f != f else f


def particle_aggregate(member_score, member_cert, score_tail, cert_mode):
    """(score [B], cert [B], spread [B]) float32 of member_score / member_cert [G, B] float32."""
    ms, mc = _np(member_score).astype(np.float32), _np(member_cert).astype(np.float32)
    G, B = ms.shape
    T = int(score_tail)
    assert 1 <= T <= G and cert_mode in (0, 1)
    score, cert, spread = (np.zeros(B, np.float32) for _ in range(3))
    ms64, mc64 = ms.astype(np.float64).T.tolist(), mc.astype(np.float64).T.tolist()
    for r in range(B):
        s, c = ms64[r], mc64[r]          # Python floats: IEEE doubles, one rounding per operation
        # score: the T lowest in (score, j) order, added in that order
        if any(v != v for v in s):
            score[r] = QNAN
        else:
            order = sorted(range(G), key=lambda j: (s[j], j))
            acc = 0.0
            for j in order[:T]:
                acc = acc + s[j]
            score[r] = _f32(acc / float(T))
        # cert
        if cert_mode == 0:
            top = c[0]
            for j in range(1, G):
                top = top if top != top else (c[j] if c[j] != c[j] else (c[j] if top < c[j] else top))
            cert[r] = _f32(top)
        else:
            acc = 0.0
            for j in range(G):
                acc = acc + c[j]
            cert[r] = _f32(acc / float(G))
        # spread
        acc = 0.0
        for j in range(G):
            acc = acc + s[j]
        m = acc / float(G)
        sq = 0.0
        for j in range(G):
            dx = s[j] + (-m)
            sq = sq + dx * dx
        spread[r] = _f32(math.sqrt(sq / float(G)) if sq == sq else sq)
    return score, cert, spread


def plan_particles_reference(x, cand, mean_in, std_in, *, G, N, score_tail, cert_mode, gamma, mode, scales, threshold,
                             elites, temperature, momentum, min_std, member_values=None):
    """drpo_plan_refit_particles on CPU tensors: ``x`` as plan_refit_reference's with G * P * N
    rows, member-major. Returns plan_refit_reference's dict plus member_score, member_cert
    [G, P, N] and score_spread [P, N]. member_values: (member_score, member_cert) [G * B] of
    plan_scores, if the caller has them."""
    P = _np(mean_in).shape[0]
    B = P * N
    ms, mc = plan_scores(x, gamma=gamma, mode=mode, scales=scales) if member_values is None else member_values
    assert ms.shape == (G * B,)
    ms, mc = ms.reshape(G, B), mc.reshape(G, B)
    score, cert, spread = particle_aggregate(ms, mc, score_tail, cert_mode)
    out = plan_refit_reference(None, cand, mean_in, std_in, N=N, gamma=gamma, mode=mode, scales=scales,
                               threshold=threshold, elites=elites, temperature=temperature, momentum=momentum,
                               min_std=min_std, scores=(score, cert))
    out.update(member_score=ms.reshape(G, P, N).copy(), member_cert=mc.reshape(G, P, N).copy(),
               score_spread=spread.reshape(P, N))
    return out


# ------------------------------------------------------------------ synthetic particles
def synthetic_particles(G, N, H, K, A, C):
    """Inputs of drpo_plan_refit_particles: member 0 is plan_helpers.synthetic_plan itself, and
    member j >= 1 the same construction under another seed (the rows built by position keep their
    controlled values: equal across the members, so the aggregated states keep the cases of
    synthetic_plan), then edited where the members must differ. (x member-major, cand, mean_in,
    std_in) as CPU tensors. With row = state * N + n, a 'controlled' row of synthetic_plan (length
    0, not terminated: its score is terminal_q, its cert the largest terminal_qc):
      state 1, rows n < N - 1   member j's score is 1 + 0.5 n - 0.25 ((3 j + n) % 4): the members'
                         order differs from candidate to candidate, and from G 5 on members
                         share a score (G >= 2)
      state 1, row N - 1 the one feasible row: member G - 1's cert is above THRESHOLD, so under
                         cert_mode 0 the state has no feasible row (G >= 2)
      state 2, row 0     member G - 1's score is +inf, row 1: -inf, (G >= 2; the mean is +-inf,
                         the spread NaN)
      state 2, row 2     member G // 2's score is NaN among valid members (G >= 2)
      state 2, row 3     +inf in member 0 and -inf in member G - 1 (G >= 2, N >= 4): a NaN mean"""
    runs = [synthetic_plan(N, H, K, A, C, seed=7 * j) for j in range(G)]
    x0, cand, mean_in, std_in = runs[0]
    x = {k: torch.cat([r[0][k] for r in runs]) for k in x0}
    B = x0['rewards'].shape[0]
    if G >= 2:
        for j in range(G):
            for n in range(N - 1):
                x['terminal_q'][j * B + N + n] = 1.0 + 0.5 * n - 0.25 * ((j * 3 + n) % 4)
        last = (G - 1) * B
        x['terminal_qc'][last + N + N - 1] = THRESHOLD + 0.5
        x['terminal_q'][last + 2 * N + 0] = float('inf')
        x['terminal_q'][last + 2 * N + 1] = -float('inf')
        if N > 2:
            x['terminal_q'][(G // 2) * B + 2 * N + 2] = float('nan')
        if N > 3:
            x['terminal_q'][0 * B + 2 * N + 3] = float('inf')
            x['terminal_q'][last + 2 * N + 3] = -float('inf')
    return x, cand, mean_in, std_in


def assert_particles_synthetic_shows_every_case(ref, G, N, T, cert_mode):
    """On the reference alone: the member-level cases the comparison is about."""
    ms, mc = ref['member_score'], ref['member_cert']
    if G < 2:
        return
    thr = np.float32(THRESHOLD)
    finite = np.isfinite(ms).all(0)
    # equal member scores within a candidate, and member orders that differ between candidates
    ties = [(p, n) for p in range(ms.shape[1]) for n in range(N)
            if finite[p, n] and len(set(ms[:, p, n].tolist())) < G]
    assert ties, 'equal member scores'
    orders = {tuple(np.argsort(ms[:, 1, n], kind='stable').tolist()) for n in range(N - 1)}
    assert len(orders) > 1 or N <= 2, 'the members order the candidates differently'
    assert np.isposinf(ms).any() and np.isneginf(ms).any(), '+-inf member scores'
    if N > 2:
        col = ms[:, 2, 2]
        assert np.isnan(col).sum() == 1 and np.isnan(ref['score'][2, 2]), 'a NaN in one member'
    # a row feasible under every member but one
    col = mc[:, 1, N - 1]
    assert (col <= thr).sum() == G - 1, 'a member that does not certify'
    if cert_mode == 0:
        assert ref['n_feasible'][1] == 0, 'so the state has no feasible row'
    if T < G:
        differ = (ref['score'] != particle_aggregate(ms.reshape(G, -1), mc.reshape(G, -1), G, cert_mode)[0]
                  .reshape(ref['score'].shape)) & finite
        assert differ.any(), 'the tail differs from the mean'
