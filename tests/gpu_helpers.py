"""Shared helpers for the GPU parity tests."""
import itertools
import random

import numpy as np
import pytest
import torch

import drpo_amd
import env_programs as EP
import fake_envs
from drpo_amd import envs, ops
from fake_envs import ENVS
from oracle import drpo_oracle as O

DEV = torch.device('cuda')
COMP = O.COMPONENTS


def small_smbpo(d, env, factory=None):
    cfg = drpo_amd.SMBPO.Config()
    E, H, B = int(d['meta/E']), int(d['meta/H']), int(d['meta/B'])
    hid, mh = int(d['meta/hidden']), int(d['meta/model_hidden'])
    cfg.update({'horizon': H, 'rollout_batch_size': B, 'buffer_max': int(d['meta/buffer_max']),
                'steps_per_epoch': 2, 'solver_updates_per_step': 10,
                'model_cfg': {'ensemble_size': E, 'num_elites': int(d['meta/num_elites']), 'hidden_dim': mh,
                              'batch_size': int(d['meta/model_batch']), 'holdout_size': int(d['meta/model_batch'])},
                'sac_cfg': {'batch_size': int(d['meta/sac_batch']), 'hidden_dim': hid,
                            'critic_cfg': {'hidden_dim': hid}, 'constraint_critic_cfg': {'hidden_dim': hid},
                            'mlp_multiplier_cfg': {'hidden_dim': hid},
                            'qc_under_uncertainty': bool(d['meta/uncertainty']),
                            'distributional_qc': bool(d['meta/distributional']), 'target_entropy': -2.0,
                            'penalty_lb': -1.0, 'actor_lr': 1e-4},
                'reward_scale': 2.0, 'alive_bonus': 2.0, 'constraint_offset': 0.5, 'constraint_scale': 10.0})
    flags = {k[len('flag/'):]: d[k].item() for k in d.files if k.startswith('flag/')}
    if flags:                          # solver-flag fixtures (make_golden.SOLVER_FLAG_CASES)
        cfg.update({'sac_cfg': flags})
    return drpo_amd.SMBPO(cfg, factory or (lambda id=None: ENVS[env]()), None, 1, device=DEV)


def load_sd(alg, d, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(np.array(d[k])) for k in d.files if k.startswith(prefix)}
    sd.pop('log_alpha', None)
    missing, unexpected = alg.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected


def fill_replay(alg, d):
    rows = {k: torch.from_numpy(d['replay/' + k]).to(DEV) for k in COMP}
    half = len(rows['states']) // 2
    alg.replay_buffer.extend(**{k: v[:half] for k, v in rows.items()})
    alg.replay_buffer.extend(**{k: v[half:] for k, v in rows.items()})


def close(a, b, tol=1e-4, msg=''):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    if a.dtype == bool or b.dtype == bool:
        np.testing.assert_array_equal(a, b, err_msg=msg)
    else:
        np.testing.assert_allclose(a, b, rtol=tol, atol=tol, err_msg=msg)


# ---------------------------------------------------------------------------
# scenes and tapes that more than one test module builds
# ---------------------------------------------------------------------------
def original_row_tape(entries, ref, B):
    """Re-index the reference's per-step draws (row k of step t = k-th surviving row)
    by original batch row: step t's arrays become [B, dim], row i = trajectory i
    (zeros for rows already done). Survivors follow from the oracle's dones:
    step t+1 keeps step t's rows with done == 0, in order (src/smbpo.py:243-246)."""
    ids = np.arange(B)
    out, off, t_rows = [], 0, None
    dones = np.asarray(ref['dones']).astype(bool)
    for kind, v in entries:
        if kind == 'normal':               # eps_a of a step: [n_t, A]
            n = v.shape[0]
            assert n == len(ids)
            full = np.zeros((B, v.shape[1]), np.float32)
            full[ids] = v
            out.append((kind, full))
            t_rows = n
        elif kind == 'randn_like':         # eps_m of the same step: [n_t, S+1]
            full = np.zeros((B, v.shape[1]), np.float32)
            full[ids] = v
            out.append((kind, full))
            ids = ids[~dones[off:off + t_rows]]
            off += t_rows
        else:
            out.append((kind, v))
    assert off == len(dones)
    return out


def _fill(alg, env, N, seed):
    import bench
    rep = bench.synth_replay(env, N, np.random.RandomState(seed))
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    return rep


WIDTH_E, WIDTH_B, WIDTH_H = 3, 256, 4          # the shapes of test_gpu_widths.py


def _width_alg(env, hid, mh, seed=5):
    import bench
    E, B, H = WIDTH_E, WIDTH_B, WIDTH_H
    torch.manual_seed(seed)
    extra = {'model_cfg': {'ensemble_size': E, 'num_elites': E, 'hidden_dim': mh},
             'sac_cfg': {'hidden_dim': hid, 'critic_cfg': {'hidden_dim': hid},
                         'constraint_critic_cfg': {'hidden_dim': hid}, 'mlp_multiplier_cfg': {'hidden_dim': hid}}}
    alg = bench.make_alg(DEV, B, H, E, seed, bench.ENV_JSON[env], extra=extra, env=env)
    sd = alg.state_dict()
    assert alg.model_ensemble.hidden_dim == mh and alg.model_ensemble.ensemble_size == E
    for k in ('solver.actor.net.0.weight', 'solver.critic.qs.0.0.weight', 'solver.constraint_critic.trunk.0.weight',
              'solver.constraint_critic.mean_head.0.weight', 'solver.multiplier.lam.0.weight'):
        assert sd[k].shape[0] == hid, (k, tuple(sd[k].shape))
    return alg


def _no_host_env(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the host round trip ran for an env with a constraint program')
    monkeypatch.setattr(ops, 'rollout_host_env', refuse)


class ProgramQuadrotor(envs.ShapeEnv):
    """ShapeEnv('quadrotor') without the built-in id: dims plus the program."""
    drpo_constraint_program = staticmethod(EP.quadrotor_program)

    def __init__(self, name, id=None):
        super().__init__(name)
        assert name == 'quadrotor'
        del self.drpo_env_id


def _drifting_quadrotor_alg(rpt):
    """bench.make_alg quadrotor, E 7, B 72, H 3. The model is put in bench's steady
    mode (next state = state + tiny noise) with a +0.1 per-step drift on z, and the
    replay's z is spread over [0.6, 1.6]: rows leave the z <= 1.5 constraint at step 0,
    1 and 2 by their starting height, the lower ones survive the horizon."""
    import bench
    random.seed(11)
    alg = bench.make_alg(DEV, 72, 3, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 400, np.random.RandomState(0))
    rep['states'][:, 2] = np.linspace(0.6, 1.6, 400, dtype=np.float32)
    rep['states'][:, [0, 4]] *= 0.1            # well inside the x and pitch bounds
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    _, diff, _ = alg.model_ensemble.views()
    diff[-1][1][..., 2] = 0.1
    alg.rollout_engine, alg.rows_per_tile = 2, rpt
    return alg


class CustomEnv(fake_envs._Env):
    S, A, C, T = 9, 2, 3, 100
    drpo_constraint_program = staticmethod(EP.custom_program)


@pytest.fixture
def custom_oracle_env():
    prog = EP.custom_program()
    O.ENV_CONSTRAINTS['_custom_program'] = prog.evaluate_numpy
    yield '_custom_program'
    del O.ENV_CONSTRAINTS['_custom_program']


# ---------------------------------------------------------------------------
# float64 comparisons under a per-element error model (tests/test_gpu_rowwise_*.py)
# ---------------------------------------------------------------------------
U32 = 2.0 ** -24        # unit roundoff of float32
C_LIBM = 8              # a handful of correctly-rounded operations, each under 1 ulp
C_HW = 32               # chains of up to ~8 v_exp_f32 / v_log_f32 / v_rcp_f32 results (1 ulp each) and the adds between
TINY32 = 2.0 ** -126    # smallest normal float32: a result or an intermediate under it may be flushed to 0


def f64(x):
    return x.detach().cpu().double()


def sp64(x):
    """torch softplus (beta 1, threshold 20) in float64: the reference's own formula"""
    return torch.nn.functional.softplus(x)


def error_ratio(name, got, ref, terms, c, exp_arg=None):
    """max |got - ref| / bound with bound = c * 2^-24 * (terms + |ref| * exp_arg) + 2^-126, all float64
    on the CPU: ``terms`` the sum of the absolute terms of the float64 formula, ``exp_arg`` the largest
    |argument| of an exp whose result scales the value. The relative model has no meaning under the
    smallest normal float32: the GPU flushes denormal results and operands of its transcendentals to
    zero (sigmoid(-100) = 3.7e-44 becomes 0, and with it a gradient of -1e-44), so one 2^-126 is allowed
    absolutely. Prints the ratio and returns it."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(ref).all(), name + ': reference not finite'
    assert torch.isfinite(got).all(), name + ': kernel output not finite'
    bound = c * U32 * (terms + (ref.abs() * exp_arg if exp_arg is not None else 0.0)) + TINY32
    bound = torch.broadcast_to(torch.as_tensor(bound, dtype=torch.float64).detach(), ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
    worst = ratio.max().item() if ratio.numel() else 0.0
    k = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    print(f'edge-ratio {name}: max err/bound {worst:.3g} (err {err.reshape(-1)[k].item():.3g}, '
          f'ref {ref.reshape(-1)[k].item():.6g}, flat index {k})')
    return worst


def within(name, got, ref, terms, c, exp_arg=None):
    worst = error_ratio(name, got, ref, terms, c, exp_arg)
    assert worst <= 1.0, f'{name}: error is {worst:.3g} x its bound'


def ulp32(x):
    """float32 spacing at |x| (float64 tensor in, float64 tensor out)"""
    a = np.abs(f64(x).numpy()).astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


SPREAD_OUTPUTS = ('mean', 'epistemic_std', 'aleatoric_std', 'disagreement', 'epistemic', 'aleatoric')


def spread_statistics(d, lv, exp_arg, s0, w, absd):
    """drpo_ens_spread's float64 formulas over members [M, n, S+1] and their bounds' (terms,
    exp_arg), as the docstring of test_gpu_ens_spread.py states them: d the members' differences
    with absolute terms absd, lv their clamped log-variances with exp arguments exp_arg,
    s0 = [s, 0], w the column weights."""
    M, n, _ = d.shape
    f = max(1.0, M / 8)
    dbar = d.mean(0)
    evar, avar = ((d - dbar) ** 2).mean(0), lv.exp().mean(0)
    t_col = absd.max(0).values + f * absd.mean(0)
    dis, t_dis = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for m1, m2 in itertools.combinations(range(M), 2):
        dis = torch.maximum(dis, (w * (d[m1] - d[m2])).norm(dim=-1))
        t_dis = torch.maximum(t_dis, (w * (absd[m1] + absd[m2])).norm(dim=-1))
    ref = {'mean': s0 + dbar, 'epistemic_std': evar.sqrt(), 'aleatoric_std': avar.sqrt(), 'disagreement': dis,
           'epistemic': (w * w * evar).sum(-1).sqrt(), 'aleatoric': (w * w * avar).sum(-1).sqrt()}
    model = {'mean': (s0.abs() + f * absd.mean(0), None),
             'epistemic_std': (t_col + ref['epistemic_std'], None),
             'aleatoric_std': (ref['aleatoric_std'], exp_arg.max(0).values),
             'disagreement': (t_dis + dis, None),
             'epistemic': ((w * t_col).norm(dim=-1) + ref['epistemic'], None),
             'aleatoric': (ref['aleatoric'], exp_arg.max(0).values.max(-1).values)}
    return ref, model
