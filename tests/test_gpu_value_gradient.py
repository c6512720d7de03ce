"""SMBPO.value_gradient against float64 autograd of the whole objective, on the action scene of the
imagine tests (imagine_helpers._action_scene: a model that answers to its actions, rows that leave
the z bound at every step).

Reference: the objective is sum_{t<len} discount^t reward_scale r_t + discount^len Q_k(s_len,
tanh(mu(s_len))) for the rows that did not terminate, with r_t and s_len from the float64 chain of
the model step (rollout_adjoint_helpers.vjp_reference, teacher-forced at the GPU's stored states),
the float64 twin critics and policy of the oracle, and k the critic the GPU selected
(ValueGradient.critic_index), so no argmin flips. ref32 is the same pipeline in float32 on the CPU.
Bound: rollout_adjoint_helpers.check, the bound of tests/test_gpu_mlp_shapes.py::check.

Measured on an MI355X (a run with -s prints the figures): the largest err / bound 0.28; the
directional check skipped 0 of 17 rows (a row whose length changes under the perturbation would count
as skipped too)."""
import pytest
import torch

import drpo_amd
from drpo_amd import ops
from gpu_helpers import DEV
from imagine_helpers import _action_scene, _params
from oracle import drpo_oracle as O
from rollout_adjoint_helpers import cast_params, check, vjp_reference
from test_gpu_imagine_lookahead import _virtual

pytestmark = pytest.mark.gpu

B = 17
MEMBERS = {3: [3, 0, 6], 1: [3]}
_SCENE = []


def _scene():
    if not _SCENE:
        alg, rep, _ = _action_scene(DEV)
        _SCENE.append((alg, rep, _params(alg)))
    return _SCENE[0]


def _inputs(rep, H, seed=21):
    gen = torch.Generator().manual_seed(seed)
    states = torch.from_numpy(rep['states'][10:400:23][:B].copy())        # z over the whole range
    actions = torch.rand(B, H, 2, generator=gen) - 0.5
    return states, actions


def _terminal_gradient(P, s_last, index, weight, dtype):
    """d/ds sum_i weight_i Q_index_i(s_i, tanh(mu(s_i))) with the oracle's nets in ``dtype``."""
    P = cast_params(P, dtype)
    s = s_last.to(dtype).clone().requires_grad_(True)
    with torch.enable_grad():
        a = O.policy_mean(P, 'actor.net.', s)
        q = torch.stack(O.critic_all(P, 'critic.', s, a))                 # [n_critics, n]
        picked = q.gather(0, index.view(1, -1)).squeeze(0)
        (g,) = torch.autograd.grad((weight.to(dtype) * picked).sum(), s)
    return g


def _reference(alg, P, vg, H, gamma, members, dtype, every_row_terminal=False):
    im = vg.imagined
    states, actions, lengths = im.states.cpu(), im.actions.cpu(), im.lengths.cpu()
    lens = lengths.to(torch.int64).clamp(0, H)
    alive = ~im.terminated.cpu().view(torch.bool) | every_row_terminal
    w = torch.tensor([gamma ** k for k in range(H + 1)], dtype=torch.float64)
    last = states[torch.arange(B), lens]
    g_last = _terminal_gradient(P, last, vg.critic_index.cpu(), torch.where(alive, w[lens], 0.0), dtype)
    gs = torch.zeros(B, H + 1, states.shape[2], dtype=dtype)
    gs[torch.arange(B), lens] = g_last
    scale = float(alg.reward_scale)
    gr = (w[:H] * scale).to(dtype).expand(B, H) * (torch.arange(H) < lens.unsqueeze(1))
    return vjp_reference(P, states, actions, lengths, members, gs, gr, dtype)


@pytest.mark.parametrize('H', [3, 1])
def test_value_gradient_against_float64(H):
    alg, rep, P = _scene()
    states, actions = _inputs(rep, H)
    gamma = float(alg.solver.discount)
    vg = alg.value_gradient(states, actions, horizon=H, members=MEMBERS[H])
    torch.cuda.synchronize()
    assert tuple(vg.grad_actions.shape) == (B, H, 2) and tuple(vg.grad_states.shape) == (B, alg.state_dim)
    assert tuple(vg.value.shape) == (B,) and vg.imagined.given_steps == H
    term = vg.imagined.terminated.cpu().view(torch.bool)
    print(f'H {H}: lengths {vg.imagined.lengths.cpu().tolist()}, terminated {int(term.sum())} of {B}')
    assert term.any() and (~term).any(), 'the scene must show terminated rows and rows cut by the horizon'
    r64 = _reference(alg, P, vg, H, gamma, MEMBERS[H], torch.float64)
    r32 = _reference(alg, P, vg, H, gamma, MEMBERS[H], torch.float32)
    assert float(r64[0].abs().max()) > 1e-3
    check(f'H {H} grad_actions', vg.grad_actions, r64[0], r32[0], ceiling=H == 1)
    check(f'H {H} grad_states', vg.grad_states, r64[1], r32[1], ceiling=H == 1)
    # terminated rows get no terminal term: with one, the reference would be somewhere else
    wrong = _reference(alg, P, vg, H, gamma, MEMBERS[H], torch.float64, every_row_terminal=True)
    gap = (wrong[1] - r64[1]).abs()[term].max()
    err = (vg.grad_states.cpu().double() - r64[1]).abs()[term].max()
    print(f'H {H}: a terminal term on the terminated rows would move grad_states by {float(gap):.3e} (error {float(err):.3e})')
    assert float(gap) > 100 * float(err)
    # the value is imagine(lookahead=)'s, from the same kind of run, bit for bit
    im = alg.imagine(states, horizon=H, actions=actions, lookahead=True, deterministic=True, model_noise=False,
                     members=MEMBERS[H], noise=drpo_amd.DeviceNoise(4))
    assert torch.equal(vg.value.cpu().view(torch.int32), im.value_lookahead[:, H].cpu().view(torch.int32))
    assert torch.equal(vg.imagined.states, im.states)


def test_the_gradient_is_an_ascent_direction():
    """On the device: for eps = 2^-7 and d = g / max|g|, value(a + eps d) - value(a - eps d) has the
    sign of 2 eps <g, d> on every row whose |<g, d>| exceeds the float32 noise of the value,
    64 * 2^-24 |value| / eps; at most a quarter of the rows may fall under it."""
    alg, rep, P = _scene()
    H = 3
    states, actions = _inputs(rep, H)
    kw = dict(horizon=H, members=MEMBERS[H])
    vg = alg.value_gradient(states, actions, **kw)
    g = vg.grad_actions
    gmax = g.abs().amax(dim=(1, 2)).clamp_min(1e-30)
    d = g / gmax.view(B, 1, 1)
    eps = 2.0 ** -7
    a = actions.to(DEV)
    up, down = alg.value_gradient(states, a + eps * d, **kw), alg.value_gradient(states, a - eps * d, **kw)
    torch.cuda.synchronize()
    slope = (g * d).sum(dim=(1, 2)).cpu().double()
    diff = (up.value - down.value).cpu().double()
    noise = 64 * 2.0 ** -24 * vg.value.cpu().double().abs() / eps
    same_run = (up.imagined.lengths == vg.imagined.lengths).cpu() & (down.imagined.lengths == vg.imagined.lengths).cpu()
    tested = (slope.abs() > noise) & same_run
    print(f'directional check: skipped {int((~tested).sum())} of {B} rows; slope {slope.tolist()}; '
          f'difference / (2 eps) {(diff / (2 * eps)).tolist()}')
    assert int((~tested).sum()) <= B // 4
    assert bool((torch.sign(diff[tested]) == torch.sign(slope[tested])).all())


def test_value_gradient_leaves_the_training_state_alone():
    alg, rep, P = _scene()
    states, actions = _inputs(rep, 3)
    alg.imagine(states)                                       # (so that imagine's private stream exists)
    torch.cuda.synchronize()
    before = _virtual(alg)
    ctrs = (alg.noise.ctr, alg._imagine_noise.ctr)
    replay = {k: alg.replay_buffer.get(k).clone() for k in ('states', 'actions', 'rewards')}
    alg.value_gradient(states, actions, horizon=3, members=0)
    torch.cuda.synchronize()
    assert (alg.noise.ctr, alg._imagine_noise.ctr) == ctrs
    after = _virtual(alg)
    assert before[1:] == after[1:]
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    for k, v in replay.items():
        assert torch.equal(alg.replay_buffer.get(k), v), k
