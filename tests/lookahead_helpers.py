"""What the tests of the model-based lookahead share (drpo_rollout_lookahead, ops.lookahead,
SMBPO.imagine(lookahead=)): the definition in plain float64 loops, the synthetic rows and the
comparisons.

lookahead_reference is the contract of include/drpo_hip.h restated: every add and multiply is one
Python float (IEEE double, round to nearest, nothing contracted) operation in the order the header
gives, the result rounded to float32 once, a NaN result stored as the canonical quiet NaN
(0x7FC00000). The kernel is held to it bit for bit (float32 compared as int32)."""
import numpy as np
import torch

REACH, COST = 0, 1
NAN, INF = float('nan'), float('inf')
QNAN_BITS = 0x7FC00000


def weights(gamma, H):
    """w[k] = gamma ** k, k = 0..H, formed as SMBPO.imagine forms the weights of ``returns``."""
    return np.power(np.float64(gamma), np.arange(H + 1, dtype=np.float64))


def _maximum(a, b):
    """torch.maximum on two doubles: a NaN in either operand stays."""
    if a != a:
        return a
    if b != b:
        return b
    return b if a < b else a


def _store(x):
    """float64 array -> float32, rounded once, NaNs canonical"""
    with np.errstate(over='ignore', invalid='ignore'):
        out = np.asarray(x, np.float64).astype(np.float32)
    out[np.isnan(out)] = np.float32(NAN)
    return out


def lookahead_reference(rewards, constraint_values, dones, violations, lengths, terminated, step_q, step_qc,
                        terminal_q, terminal_qc, *, gamma, mode, reward_scale, alive_bonus, constraint_scale,
                        constraint_offset, w=None):
    """(value [B, H+1], certificate [B, H+1, C]) float32 numpy arrays from CPU tensors / arrays:
    rewards [B, H], constraint_values [B, H, C] (unused in COST mode, may be None), dones and
    violations [B, H] (violations unused in REACH mode, may be None), lengths [B] (clamped to
    0..H), terminated [B], step_q [B, H], step_qc [B, H, C], terminal_q [B], terminal_qc [B, C]."""
    def lst(x):
        return None if x is None else (x.detach().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).tolist()
    B, H = tuple(rewards.shape)
    C = int(step_qc.shape[-1])
    g = float(gamma)
    w = (weights(g, H) if w is None else np.asarray(w, np.float64)).tolist()
    assert len(w) == H + 1
    one_minus_g = 1.0 - g
    rs, ab, cs, co = float(reward_scale), float(alive_bonus), float(constraint_scale), float(constraint_offset)
    r_, h_, d_, v_ = lst(rewards), lst(constraint_values), lst(dones), lst(violations)
    len_, term_ = lst(lengths), lst(terminated)
    sq, sqc, tq, tqc = lst(step_q), lst(step_qc), lst(terminal_q), lst(terminal_qc)
    value = np.zeros((B, H + 1), np.float64)
    cert = np.zeros((B, H + 1, C), np.float64)
    for i in range(B):
        n = min(max(int(len_[i]), 0), H)
        term = bool(term_[i])
        # the preprocessed steps (src/smbpo.py:260-270), in double
        rp, hp = [], []
        for t in range(n):
            r = float(r_[i][t])
            if rs != 0.0:
                r = r * rs
            if ab != 0.0:
                r = r + ab
            rp.append(r)
            if mode == REACH:
                row = []
                for c in range(C):
                    h = float(h_[i][t][c]) * cs
                    h = h + (1.0 if h > 0.0 else 0.0) * co
                    row.append(h)
                hp.append(row)
        for k in range(H + 1):
            kk = min(k, n)
            boot = kk < n or not term
            acc = 0.0
            for t in range(kk):
                acc = acc + w[t] * rp[t]
            if boot:
                q = float(sq[i][kk]) if kk < n else float(tq[i])
                acc = acc + w[kk] * q
            value[i, k] = acc
            for c in range(C):
                # a terminated row has no bootstrap: the scan starts from 0.0, which its last
                # step's done select replaces
                x = (float(sqc[i][kk][c]) if kk < n else float(tqc[i][c])) if boot else 0.0
                for t in range(kk - 1, -1, -1):
                    if mode == REACH:
                        h = hp[t][c]
                        x = h if d_[i][t] else one_minus_g * h + g * _maximum(h, x)
                    else:
                        v = 1.0 if v_[i][t] else 0.0
                        x = v if d_[i][t] else v + g * x
                cert[i, k, c] = x
    return _store(value), _store(cert)


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def assert_bits(got, want, what, rows=None):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape)
    if rows is not None:
        g, w = g[rows], w[rows]
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} elements differ, first at {bad[0].tolist()}'


# ------------------------------------------------------------------ synthetic rows
def synthetic(B, H, C, seed=0):
    """Inputs of drpo_rollout_lookahead built by position, as a dict of CPU tensors, and the row
    indices of its special cases. Row i: length i % (H + 1) (every length 0..H for B > H + 1, else
    a spread of them), terminated on every other pass over the lengths (terminated rows carry the
    done bit at their last step). Constraint values on both sides of zero and of the bootstraps."""
    g = torch.Generator().manual_seed(1000 * H + 10 * C + seed)
    lengths = torch.tensor([(i * (1 if B > H + 1 else max(1, (H + 1) // B))) % (H + 1) for i in range(B)],
                           dtype=torch.int32)
    if H + 1 > B:       # the longest chain is always there
        lengths[-1], lengths[-2] = H, H
    terminated = torch.tensor([(i // (H + 1) + i) % 2 == 1 for i in range(B)])
    if H + 1 > B:
        terminated[-1], terminated[-2] = False, True
    rewards = torch.randn(B, H, generator=g)
    cvals = 0.05 * torch.randn(B, H, C, generator=g)              # h' = 10 h ~ N(0, 0.5): both signs
    step_q = 3 * torch.randn(B, H, generator=g)
    step_qc = 0.5 * torch.randn(B, H, C, generator=g)             # both sides of h'
    terminal_q = 3 * torch.randn(B, generator=g)
    terminal_qc = 0.5 * torch.randn(B, C, generator=g)
    dones = torch.zeros(B, H, dtype=torch.bool)
    violations = torch.rand(B, H, generator=g) < 0.3
    mask = torch.arange(H) < lengths.unsqueeze(-1)
    for i in range(B):
        n = int(lengths[i])
        if terminated[i] and n > 0:
            dones[i, n - 1] = True
    # as ImaginedRollout holds them: zero at and beyond the length
    rewards, violations = rewards * mask, violations & mask
    cvals, step_q, step_qc = cvals * mask.unsqueeze(-1), step_q * mask, step_qc * mask.unsqueeze(-1)
    live = [i for i in range(B) if not terminated[i]]
    dead = [i for i in range(B) if terminated[i] and lengths[i] > 0]
    cases = {}
    # a NaN and the two infinities as the terminal bootstrap of live rows (they propagate)
    picks = [i for i in live if lengths[i] == min(H, 1)] + live
    cases['nan_boot'], cases['pinf_boot'], cases['ninf_boot'] = picks[0], live[-1], live[-2]
    assert len({cases['nan_boot'], cases['pinf_boot'], cases['ninf_boot']}) == 3
    terminal_qc[cases['nan_boot']] = NAN
    terminal_q[cases['nan_boot']] = NAN
    terminal_qc[cases['pinf_boot']] = INF
    terminal_q[cases['pinf_boot']] = INF
    terminal_qc[cases['ninf_boot']] = -INF
    terminal_q[cases['ninf_boot']] = -INF
    # a NaN where a terminated row's bootstrap would be (must not reach the output)
    cases['nan_dead'] = dead[0]
    terminal_qc[dead[0]] = NAN
    terminal_q[dead[0]] = NAN
    # a NaN step bootstrap on a live step of a long row: entry kk of that row alone
    long_rows = [i for i in range(B) if lengths[i] >= 1 and i not in cases.values()]
    cases['nan_step'] = long_rows[0]
    step_qc[long_rows[0], 0] = NAN
    return dict(rewards=rewards, constraint_values=cvals, dones=dones, violations=violations, lengths=lengths,
                terminated=terminated, step_q=step_q, step_qc=step_qc, terminal_q=terminal_q,
                terminal_qc=terminal_qc), cases


SCALES = dict(reward_scale=0.5, alive_bonus=1.0, constraint_scale=10.0, constraint_offset=0.5)


def assert_synthetic_shows_every_case(x, cases, H, C):
    """Otherwise the comparison shows nothing (the cases of the module docstring of
    test_gpu_lookahead_kernel.py)."""
    n, term = x['lengths'].numpy(), x['terminated'].numpy()
    B = len(n)
    if B > 2 * (H + 1):
        assert {(int(a), bool(b)) for a, b in zip(n, term)} >= {(k, t) for k in range(H + 1) for t in (False, True)}
    assert int(n.max()) == H and int(n.min()) == 0 and term.any() and (~term).any()
    mask = np.arange(H) < n[:, None]
    hp = x['constraint_values'].double().numpy() * SCALES['constraint_scale']
    assert (hp[mask] > 0).any() and (hp[mask] < 0).any()                      # the offset applies and does not
    # both arms of the max at the last step of some row: h' above and below the bootstrap
    above = below = False
    for i in range(B):
        if n[i] >= 1 and not term[i]:
            boot = x['terminal_qc'][i].double().numpy()
            h = hp[i, n[i] - 1] + (hp[i, n[i] - 1] > 0) * SCALES['constraint_offset']
            above |= bool((h > boot).any())
            below |= bool((h < boot).any())
    assert above and below
    assert torch.isnan(x['terminal_qc'][cases['nan_boot']]).all() and not term[cases['nan_boot']]
    assert (x['terminal_qc'][cases['pinf_boot']] == INF).all() and not term[cases['pinf_boot']]
    assert (x['terminal_qc'][cases['ninf_boot']] == -INF).all() and not term[cases['ninf_boot']]
    assert torch.isnan(x['terminal_qc'][cases['nan_dead']]).all() and term[cases['nan_dead']] and \
        n[cases['nan_dead']] >= 1
    assert torch.isnan(x['step_qc'][cases['nan_step'], 0]).all() and n[cases['nan_step']] >= 1
