"""What the tests of drpo_rollout_adjoint share (tests/test_rollout_adjoint_checks.py,
tests/test_gpu_rollout_adjoint.py, tests/test_gpu_value_gradient.py): the definition of the header
as torch autograd on the CPU, and the bound the kernel is held to.

vjp_reference is the reverse sweep of include/drpo_hip.h above drpo_rollout_adjoint_t, step by
step: at every stored (states[:, t], actions[:, t]) it runs oracle.ens_forward1's mean (the
deterministic model step: next state = s + diff[:S], reward = diff[S]) with the ensemble's
parameters cast to ``dtype`` and backs the step's upstream [lam | g_r] through it with
torch.autograd. Teacher-forced at the stored states: the Jacobians are taken where the GPU's
trajectory is, so no trajectory divergence enters the comparison. float64 is the reference
(ref64), float32 the same sweep by torch on the CPU (ref32), whose error sizes the bound.

Tolerance (check): the project's own, tests/test_gpu_mlp_shapes.py::check. Per compared tensor
    max|got - ref64| <= max(4 * e32, 32 * 2^-24 * scale),   e32 = max|ref32 - ref64|, scale = max|ref64|
(4x: the MFMA k-chunk order against the CPU's sums; the floor: the hardware exp / rcp of
fast_sigmoid), and at H = 1 every element within 1e-4 + 1e-4 |ref| as well."""
import torch

from oracle import drpo_oracle as O

PRE = 'model_ensemble.'


def cast_params(P, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in P.items()}


def step_mean(P, s, a, member):
    """[n, S+1]: the deterministic model step's next state and reward (ens_forward1's mean)."""
    return O.ens_forward1(P, PRE, s, a, member)[0]


def vjp_reference(P, states, actions, lengths, members, g_states=None, g_rewards=None, dtype=torch.float64):
    """(grad_actions [B, H, A], grad_start [B, S]) in ``dtype``: the definition. states [B, H+1, S],
    actions [B, H, A], lengths [B] (clamped to 0..H), members H ints; g_states [B, H+1, S] and
    g_rewards [B, H] or None (zeros). Entries of g_states beyond a row's length are never read."""
    P = cast_params(P, dtype)
    B, H1, S = states.shape
    H, A = H1 - 1, actions.shape[2]
    lens = lengths.to(torch.int64).clamp(0, H)
    gs = torch.zeros(B, H + 1, S, dtype=dtype) if g_states is None else g_states.to(dtype)
    gr = torch.zeros(B, H, dtype=dtype) if g_rewards is None else g_rewards.to(dtype)
    rows = torch.arange(B)
    lam = gs[rows, lens]                                   # g_states[i][len]
    ga = torch.zeros(B, H, A, dtype=dtype)
    for t in range(H - 1, -1, -1):
        live = lens > t
        if not bool(live.any()):
            continue
        s = states[live, t].to(dtype).clone().requires_grad_(True)
        a = actions[live, t].to(dtype).clone().requires_grad_(True)
        with torch.enable_grad():
            out = step_mean(P, s, a, members[t])
        up = torch.cat([lam[live], gr[live, t].unsqueeze(1)], dim=1)
        ds, da = torch.autograd.grad(out, (s, a), grad_outputs=up)
        ga[live, t] = da
        lam = lam.clone()
        lam[live] = gs[live, t] + ds                     # ds = lam + J_s^T [lam, g_r] / (std + 1e-6)
    return ga, lam


def chain(P, s0, actions, members):
    """The un-teacher-forced chain in the dtype of its inputs: (states [B, H+1, S], rewards [B, H])."""
    states, rewards, s = [s0], [], s0
    for t in range(actions.shape[1]):
        out = step_mean(P, s, actions[:, t], members[t])
        s = out[:, :-1]
        states.append(s)
        rewards.append(out[:, -1])
    return torch.stack(states, dim=1), torch.stack(rewards, dim=1)


def random_params(E, S, A, Hm, gen, gain=1.0):
    """An ensemble's parameters as the oracle names them: uniform(+-gain / sqrt(din)) weights."""
    P = {}

    def layer(prefix, i, din, dout):
        k = gain / din ** 0.5
        P[f'{PRE}{prefix}{i}.weight'] = (torch.rand(E, dout, din, generator=gen) * 2 - 1) * k
        P[f'{PRE}{prefix}{i}.bias'] = (torch.rand(E, dout, generator=gen) * 2 - 1) * k
    layer('trunk.', 0, S + A, Hm)
    layer('trunk.', 2, Hm, Hm)
    for head in ('diff_head.', 'log_var_head.'):
        layer(head, 0, Hm, Hm)
        layer(head, 2, Hm, S + 1)
    P[PRE + 'min_log_var'] = torch.full((S + 1,), -10.0)
    P[PRE + 'max_log_var'] = torch.full((S + 1,), 1.0)
    P[PRE + 'state_normalizer.mean'] = torch.randn(S, generator=gen) * 0.1
    P[PRE + 'state_normalizer.std'] = torch.rand(S, generator=gen) + 0.5
    return P


def check(what, got, ref64, ref32, ceiling=False, measured=None):
    """The header's bound for one tensor; prints the figures before it asserts. Returns err / bound."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    assert torch.isfinite(got).all(), f'{what}: not finite'
    scale = float(ref64.abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    err = float((got - ref64).abs().max())
    bound = max(4 * e32, 32 * 2.0 ** -24 * scale)
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
    print(f'{what}: err {err:.3e} scale {scale:.3e} e32 {e32:.3e} bound {bound:.3e} err/bound {ratio:.3f}')
    if measured is not None:
        measured[0] = max(measured[0], ratio)
    assert err <= bound, f'{what}: max err {err:.3e} > {bound:.3e} (scale {scale:.3e}, e32 {e32:.3e})'
    if ceiling:
        assert bool(((got - ref64).abs() <= 1e-4 + 1e-4 * ref64.abs()).all()), f'{what}: past the fp32 ceiling'
    return ratio
