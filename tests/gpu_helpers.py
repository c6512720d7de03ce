"""Shared helpers for the GPU parity tests."""
import numpy as np
import torch

import drpo_amd
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

