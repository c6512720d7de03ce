"""Constraint programs on the device (drpo_env_program_t, env id 4): the stand-alone
launch, both rollout engines against the reference fixtures and the oracle with an
environment the build only knows through its program, the program against the
built-in id under device noise with rows dying, and the robust critic target.

Tolerances: h is compared as float32 to atol 1e-6 (|h| < 16, so one float32 ulp is
<= 9.5e-7; the interpreter and evaluate_numpy do the same double operations in the
same order). Where the program and a built-in id do the same double operations
(quadrotor, cartpole) the outputs must be identical bit for bit; the point-robot
built-in may contract dx*dx + dy*dy into a fused multiply-add, which the interpreter
never does, hence atol 1e-6 there. Rollouts use the tolerances of the tests they mirror."""
import numpy as np
import pytest
import torch

import drpo_amd
import env_programs as EP
import fake_envs
import pr_env
from conftest import load_golden
from drpo_amd import envs, ops
from gpu_helpers import (COMP, DEV, CustomEnv, ProgramQuadrotor, _drifting_quadrotor_alg, _no_host_env,  # noqa: F401
                         close, custom_oracle_env, fill_replay, load_sd, original_row_tape, small_smbpo)
from oracle import drpo_oracle as O

pytestmark = pytest.mark.gpu


def _program_params(prog):
    return dict(env_id=envs.ENV_PROGRAM, con_dim=prog.C, tracking_surr_start=47, tracking_n_surr=1, thr0=0.0,
                thr1=0.0, program=prog)


# ------------------------------------------------------------------ 1. stand-alone launch
@pytest.mark.parametrize('name', ['point-robot', 'quadrotor', 'cartpole', 'custom'])
def test_standalone_program_launch(name):
    make, states = EP.CASES[name]
    prog, s = make(), states()
    st = torch.from_numpy(s).to(DEV)
    done, viol, h = ops.env_constraints(_program_params(prog), st)
    torch.cuda.synchronize()
    h = h.reshape(len(s), prog.C)
    rd, rv, rh = prog.evaluate_numpy(s)
    np.testing.assert_array_equal(done.cpu().numpy(), rd)
    np.testing.assert_array_equal(viol.cpu().numpy(), rv)
    np.testing.assert_allclose(h.cpu().numpy(), rh, rtol=0, atol=1e-6)
    assert 0 < int(rd.sum()) < len(s) and 0 < int(rv.sum()) < len(s)
    if name == 'custom':
        return
    bd, bv, bh = ops.env_constraints(envs.device_env_params(name), st)   # the built-in id
    bh = bh.reshape(len(s), prog.C)
    assert torch.equal(done, bd) and torch.equal(viol, bv)
    if name == 'point-robot':
        np.testing.assert_allclose(h.cpu().numpy(), bh.cpu().numpy(), rtol=0, atol=1e-6)
    else:
        assert torch.equal(h.view(torch.int32), bh.view(torch.int32))


def test_builtin_entry_refuses_program_id():
    from drpo_amd import _lib
    s = torch.zeros(4, 11, device=DEV)
    p = dict(envs.device_env_params('point-robot'), env_id=envs.ENV_PROGRAM)
    with pytest.raises(_lib.DrpoError, match='drpo_env_constraints_program'):
        ops.env_constraints(p, s)
    prog = EP.custom_program()                       # reads state index 8
    with pytest.raises(ValueError, match='state index 8'):
        ops.env_constraints(_program_params(prog), torch.zeros(4, 8, device=DEV))


# ------------------------------------------------------------------ 2. engine 1, reference fixture
def _load_rollout_fixture(alg, d):
    load_sd(alg, d, 'sd/')
    fill_replay(alg, d)
    m = alg.model_ensemble
    m.state_normalizer.mean.copy_(torch.from_numpy(d['model/norm_mean']))
    m.state_normalizer.std.copy_(torch.from_numpy(d['model/norm_std']))
    m._elite_inds = list(d['model/elite_inds'])


def test_step_engine_program_matches_reference_fixture(monkeypatch):
    """The set-up of test_rollout_host_env_fallback_matches_reference_fixture, but the
    unknown class carries the point-robot program: it stays on the device."""
    class MyPointRobot(pr_env.PointRobot):
        drpo_constraint_program = staticmethod(EP.point_robot_program)

    _no_host_env(monkeypatch)
    d = load_golden('rollout_point-robot')
    alg = small_smbpo(d, 'point-robot', factory=lambda id=None: MyPointRobot())
    assert alg.env_params['env_id'] == 4
    _load_rollout_fixture(alg, d)
    tape = drpo_amd.TapeNoise.from_npz(d, 'tape')
    alg.rollout(alg.actor, noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    n = int(d['out/n'])
    assert len(alg.virt_buffer) == n
    got = alg.virt_buffer.get(as_dict=True)
    for k in COMP:
        close(got[k], d['out/' + k], msg=k)


# ------------------------------------------------------------------ 3. engine 2, production widths
class MyQuadrotor(fake_envs.QuadrotorWrapperEnv):     # unknown class name: only its program says what it is
    drpo_constraint_program = staticmethod(EP.quadrotor_program)


def test_fused_engine_program_matches_reference_fixture_full_width(monkeypatch):
    """rollout_fullwidth_quad (actor 256, members 200, B 64, H 2) driven as
    test_fused_engine_matches_reference_fixture_full_width drives it: the program
    instantiation of the persist kernel on the LDS-resident-actor, paired-heads path."""
    _no_host_env(monkeypatch)
    d = load_golden('rollout_fullwidth_quad')
    alg = small_smbpo(d, 'quadrotor', factory=lambda id=None: MyQuadrotor())
    assert alg.env_params['env_id'] == 4 and alg.env_params['con_dim'] == 2
    _load_rollout_fixture(alg, d)
    entries = drpo_amd.TapeNoise.from_npz(d, 'tape').entries
    tape = drpo_amd.TapeNoise(original_row_tape(entries, {'dones': d['out/dones']}, alg.rollout_batch_size))
    alg.rollout_engine = 2
    out = ops.rollout(alg, alg.actor, None, tape, eps_layout=1)
    torch.cuda.synchronize()
    assert tape.done() and len(out) == int(d['out/n'])
    got = alg.virt_buffer.get(as_dict=True)
    for k in COMP:
        close(got[k], d['out/' + k], tol=2e-4, msg=k)


# ------------------------------------------------------------------ 4. program against built-in
@pytest.mark.parametrize('rpt', [16, 32])
def test_fused_engine_program_equals_builtin_device_noise(monkeypatch, rpt):
    """Philox draws are keyed by row and step, so the program and the built-in id see
    the same numbers: all seven components and the row count identical bit for bit.
    B = 72: four full 16-row tiles and one of 8 rows / two 32-row tiles and one of 8."""
    _no_host_env(monkeypatch)
    outs = []
    for standin in (None, ProgramQuadrotor):
        with monkeypatch.context() as mp:
            if standin is not None:
                mp.setattr(envs, 'ShapeEnv', standin)
            alg = _drifting_quadrotor_alg(rpt)
        assert alg.env_params['env_id'] == (1 if standin is None else 4)
        out = alg.rollout(alg.actor, noise=drpo_amd.DeviceNoise(1234))
        torch.cuda.synchronize()
        outs.append((len(out), out.get(as_dict=True)))
    (n0, a), (n1, b) = outs
    assert n0 == n1
    # the buffer holds step 0's 72 rows, then step 1's survivors, then step 2's
    done = a['dones']
    n_1 = int((~done[:72]).sum())
    n_2 = int((~done[72:72 + n_1]).sum())
    assert n0 == 72 + n_1 + n_2
    assert bool(done[:72 + n_1].any()), 'no row finished before the last step'
    assert n_2 > 0 and bool((~done[72 + n_1:]).any()), 'no row survived the horizon'
    for k in COMP:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


@pytest.mark.parametrize('engine', [1, 2])
def test_custom_program_rollout_matches_oracle(monkeypatch, custom_oracle_env, engine):
    """S = 9, C = 3 (no built-in has these dims) at default widths, B 72, H 3, against the
    oracle's rollout with evaluate_numpy as its constraint functions: the recorded draws
    drive the per-step engine, and re-indexed by original row the fused engine."""
    _no_host_env(monkeypatch)
    B, H = 72, 3
    torch.manual_seed(5)
    cfg = drpo_amd.SMBPO.Config()
    cfg.update({'horizon': H, 'rollout_batch_size': B, 'buffer_max': 20000})
    alg = drpo_amd.SMBPO(cfg, lambda id=None: CustomEnv(), None, 1, device=DEV)
    assert alg.env_params['env_id'] == 4 and (alg.state_dim, alg.con_dim) == (9, 3)
    states = EP.custom_states()
    N = len(states)
    rng = np.random.RandomState(3)
    rows = dict(states=states, actions=rng.uniform(-1, 1, (N, 2)).astype(np.float32), next_states=states,
                rewards=rng.normal(0, 1, N).astype(np.float32), dones=np.zeros(N, bool), violations=np.zeros(N, bool),
                constraint_values=np.zeros((N, 3), np.float32))
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rows.items()})
    m = alg.model_ensemble
    st = torch.from_numpy(states)
    mean, std = O.normalizer_fit(st)
    m.state_normalizer.mean.copy_(mean)
    m.state_normalizer.std.copy_(std)
    m._elite_inds = [3, 0, 6, 2, 5]
    sd = {k: v.detach().cpu() for k, v in alg.state_dict().items()}
    P = {k[len('solver.'):]: v for k, v in sd.items() if k.startswith('solver.actor.')}
    P.update({k: v for k, v in sd.items() if k.startswith('model_ensemble.')})
    live = O.LiveRNG()
    ref = O.rollout(P, 'actor.net.', 'model_ensemble.', m._elite_inds, st, custom_oracle_env, B, H, live)
    n = len(ref['states'])
    assert B < n < B * H and bool(ref['dones'][:B].any())      # rows die, rows survive
    if engine == 1:
        out = alg.rollout(alg.actor, noise=drpo_amd.TapeNoise(live.entries))
    else:
        tape = drpo_amd.TapeNoise(original_row_tape(live.entries, ref, B))
        out = ops.rollout(alg, alg.actor, None, tape, eps_layout=1)
    torch.cuda.synchronize()
    assert len(out) == n
    got = out.get(as_dict=True)
    for k in COMP:
        close(got[k], ref[k], tol=2e-4, msg=k)


# ------------------------------------------------------------------ 5. robust critic target
def test_robust_critic_target_uses_program():
    """One update_critic with qc_under_uncertainty (ssac_robust_point): the model-predicted
    done flags of the certificate target come from the program launch, never from the
    env's host check_done. Tolerances of test_ssac_updates_match_reference."""
    from test_gpu_sac import check_params, solver_sd

    class MyPointRobot(fake_envs.PointRobot):
        drpo_constraint_program = staticmethod(EP.point_robot_program)

        def check_done(self, states):
            raise AssertionError('the host check_done ran for an env with a constraint program')

    d = load_golden('ssac_robust_point')
    alg = small_smbpo(d, 'point-robot', factory=lambda id=None: MyPointRobot())
    sol = alg.solver
    assert sol.qc_under_uncertainty and not sol.distributional_qc
    sd0 = solver_sd(d, 'sd0/')
    sol.log_alpha.fill_(float(sd0.pop('log_alpha')))
    missing, unexpected = sol.load_state_dict(sd0, strict=False)
    assert not unexpected
    alg.model_ensemble._elite_inds = list(d['model/elite_inds'])
    batch = [torch.from_numpy(d['in/' + k]).to(DEV) for k in ['s', 'a', 's2', 'r', 'd', 'v', 'h']]
    tape = drpo_amd.TapeNoise.from_npz(d, 'critic_tape')
    lq, lqc = sol.update_critic(*batch, noise=tape)
    torch.cuda.synchronize()
    assert tape.done()
    np.testing.assert_allclose(lq.item(), float(d['out/lq']), rtol=1e-4)
    np.testing.assert_allclose(lqc.item(), float(d['out/lqc']), rtol=1e-4)
    check_params(sol, solver_sd(d, 'sd1/'), 'after update_critic')
