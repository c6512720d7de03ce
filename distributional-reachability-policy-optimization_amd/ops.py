"""Host glue: turns the reference-API calls into C-ABI launches (libdrpo_hip.so).

Everything here only marshals pointers, shapes and noise; all arithmetic runs in
the HIP kernels. No CPU fallback: a missing library or non-device tensors raise.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._abi import RolloutDesc
from .mlp_desc import Net, fill_fwd, spec_layers


def _dev(x, device, dtype=None):
    t = torch.as_tensor(x, device=device)
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------
# rollout (src/smbpo.py:229-249)
# ---------------------------------------------------------------------------
def _tape_rollout_noise(noise, H, B, A, S1):
    """Parity mode: pull the reference's rollout draws from the tape. Returns (elite picks,
    per-step row counts, eps_a [H,B,A], eps_m [H,B,S1])."""
    eps_a = np.zeros((H, B, A), np.float32)
    eps_m = np.zeros((H, B, S1), np.float32)
    ks, ns = [], []
    for t in range(H):
        if noise.peek() != 'normal':
            break
        ea = noise._take('normal')
        k = noise.choice(None)
        em = noise._take('randn_like')
        n = ea.shape[0]
        assert em.shape == (n, S1) and ea.shape == (n, A)
        eps_a[t, :n], eps_m[t, :n] = ea, em
        ks.append(k)
        ns.append(n)
    return ks, ns, eps_a, eps_m


class EventTimer:
    """Pool of HIP events recorded by the library around its dominant kernels."""

    def __init__(self, n):
        L = _lib.lib()
        self.events = (ctypes.c_void_p * n)()
        for i in range(n):
            ev = ctypes.c_void_p()
            _lib.check(L.drpo_event_create(ctypes.byref(ev)), 'event_create')
            self.events[i] = ev
        self.n = n

    def elapsed_pairs(self, npairs):
        """ms between events (2i, 2i+1) for i < npairs (call after synchronize)."""
        L = _lib.lib()
        out = []
        for i in range(npairs):
            ms = ctypes.c_float()
            _lib.check(L.drpo_event_elapsed_ms(ctypes.byref(ms), self.events[2 * i], self.events[2 * i + 1]), 'elapsed')
            out.append(ms.value)
        return out


_VB_FIELDS = ('_states', '_actions', '_next_states', '_rewards', '_constraint_values', '_dones', '_violations',
              '_pointer')
_ROLLOUT_CACHE_MAX = 8


def _rollout_static(alg, policy, B, H, buffer):
    """The per-(shapes, parameter groups, buffers) part of a rollout descriptor: the
    packed-mirror and bias pointers, env parameters, normalizer / log-var bound and the
    workspace. Built once and cached on ``alg``; per call only the members, the noise, the
    initial-state source and the events change (_fill_call). (Building it took ~20 tensor
    views per call: most of the call's host time.)
    buffer=True, drpo_rollout's entry: with the virtual-buffer pointers, which are part of
    the key, and the workspace's row count. buffer=False, the drpo_rollout_trajectories*
    calls' entry: a cache, descriptor and workspace of its own (never the one drpo_rollout's
    pointers live in), the virtual-buffer fields NULL, no count. Returns (descriptor, its
    members array, the count or None, the uploaded program or None: kept alive here)."""
    # every device pointer the descriptor stores is part of the key (a buffer reallocated
    # under one of them must never leave a stale pointer behind)
    key = _rollout_key(alg, policy, B, H)
    if buffer:
        vb = alg.virt_buffer._module
        key += (vb.capacity,) + tuple(getattr(vb, f).data_ptr() for f in _VB_FIELDS)
    cache = alg.__dict__.setdefault('_rollout_desc_cache' if buffer else '_rollout_traj_desc_cache', {})
    hit = cache.get(key)
    if hit is not None:
        return hit
    if len(cache) >= _ROLLOUT_CACHE_MAX:   # (B, H) or buffers changed: drop the old entries
        cache.clear()
    d, members, ws, prog = _rollout_desc(alg, policy, B, H, f'rollout.{B}.{H}' if buffer else f'rollout_traj.{B}.{H}')
    count = None
    if buffer:
        d.vs, d.va, d.vs2, d.vr = vb._states.data_ptr(), vb._actions.data_ptr(), vb._next_states.data_ptr(), \
            vb._rewards.data_ptr()
        d.vh, d.vd, d.vv = vb._constraint_values.data_ptr(), vb._dones.data_ptr(), vb._violations.data_ptr()
        d.vptr, d.vcap = vb._pointer.data_ptr(), vb.capacity
        off = _lib.lib().drpo_rollout_count_offset(B, alg.state_dim, H)
        count = ws[off:off + 8].view(torch.int64)[0]
    hit = cache[key] = (d, members, count, prog)
    return hit


def _rollout_key(alg, policy, B, H):
    """The device pointers and shapes of _rollout_desc, as a cache key."""
    model = alg.model_ensemble
    pg, mg = policy.group, model.group
    norm = model.state_normalizer
    return (id(policy), B, H, pg.data.data_ptr(), pg.packed.data_ptr(), mg.data.data_ptr(), mg.packed.data_ptr(),
            norm.mean.data_ptr(), norm.std.data_ptr(), model.min_log_var.data_ptr(), model.max_log_var.data_ptr())


def _rollout_desc(alg, policy, B, H, ws_name):
    """A rollout descriptor without the virtual-buffer fields, on a workspace of its own
    (``ws_name``): what drpo_rollout and drpo_rollout_trajectories read alike. Returns
    (descriptor, its members array, the workspace, the uploaded program or None)."""
    model = alg.model_ensemble
    pg, mg = policy.group, model.group
    norm = model.state_normalizer
    L = _lib.lib()
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim
    pa = [(pg.pview(f'net.{2 * i}.weight')[0], pg.view(f'net.{2 * i}.bias')) for i in range(policy.spec.n_layers)]

    def mviews(prefix, spec):   # packed mirrors of member 0 (the kernel adds member * packed size)
        return [(mg.pview(f'{prefix}{2 * i}.weight')[0], mg.view(f'{prefix}{2 * i}.bias'))
                for i in range(spec.n_layers)]
    trunk, diff, logv = (mviews('trunk.', model.trunk_spec), mviews('diff_head.', model.diff_spec),
                         mviews('log_var_head.', model.logvar_spec))
    ep = alg.env_params
    d = RolloutDesc()
    d.S, d.A, d.C, d.Ha, d.Hm, d.B, d.H = S, A, C, policy.spec.dims[1], model.hidden_dim, B, H
    d.env_id, d.tracking_surr_start, d.tracking_n_surr = ep['env_id'], ep['tracking_surr_start'], ep['tracking_n_surr']
    d.env_thr0, d.env_thr1 = ep['thr0'], ep['thr1']
    # constraint program (env id 4): checked against S and uploaded once, cached on the program
    prog = ep['program'].device(alg.device, S) if 'program' in ep else None
    d.env_program = 0 if prog is None else prog.data_ptr()
    (d.aW1, d.ab1), (d.aW2, d.ab2), (d.aW3, d.ab3) = [(W.data_ptr(), b.data_ptr()) for W, b in pa]
    (d.mW1, d.mb1), (d.mW2, d.mb2) = [(W.data_ptr(), b.data_ptr()) for W, b in trunk]
    (d.dW1, d.db1), (d.dW2, d.db2) = [(W.data_ptr(), b.data_ptr()) for W, b in diff]
    (d.lW1, d.lb1), (d.lW2, d.lb2) = [(W.data_ptr(), b.data_ptr()) for W, b in logv]
    d.norm_mean, d.norm_std = norm.mean.data_ptr(), norm.std.data_ptr()
    d.min_lv, d.max_lv = model.min_log_var.data_ptr(), model.max_log_var.data_ptr()
    # a workspace of its own per entry (the cached pointers must never see it reallocated)
    ws = alg._workspace(ws_name, L.drpo_rollout_workspace_size(B, S, H))
    d.workspace = ws.data_ptr()
    members = (ctypes.c_int * H)()
    d.members = members
    return d, members, ws, prog


def _start_states(alg, initial_states, noise, dev):
    """Where a rollout starts: the given rows (the reference rolls out exactly
    len(initial_states) rows, src/smbpo.py:230-233), else rollout_batch_size chronological
    replay indices (np.random.choice without replacement; None from a device noise, whose
    kernel draws them). Returns (source tensor, src_ptr, src_cap, init_idx, B)."""
    if initial_states is not None:
        src = initial_states.contiguous().float()
        assert src.dim() == 2 and src.shape[1] == alg.state_dim, 'initial_states must be [n, state_dim]'
        B = len(src)
        return src, B, B, torch.arange(B, device=dev, dtype=torch.int64), B
    rb, B = alg.replay_buffer._module, alg.rollout_batch_size
    ptr, cap = rb.pointer, rb.capacity
    idx = noise.np_choice(min(ptr, cap), B)
    return rb._states, ptr, cap, None if idx is None else _dev(idx, dev, torch.int64), B


def _members_and_draws(model, noise, H, B, A, S1, dev, members=None, eps_a=None, eps_m=None):
    """The ensemble member of each step and the recorded draws of a rollout. Returns (the H
    members, the tape's per-step row counts or None, eps_a [H, B, A] and eps_m [H, B, S1] on
    ``dev`` or None for both: the kernel draws).

    A tape supplies its own (_tape_rollout_noise), rows beyond a step's count and steps beyond
    the tape zero (member 0). Otherwise ``members`` (an int or H ints), else one random elite
    per step, checked, and the caller's eps_a / eps_m, checked.

    The order in which a rollout consumes its noise object. rollout(noise=n) and
    imagine(noise=n) are equal row for row because both keep it:
      1. _start_states: np_choice, only when no start states were given;
      2. here: the tape reads, or H times choice(len(elites)), those only when ``members`` is None;
      3. the caller: next(), only when no ``ctr`` was given.
    SMBPO.imagine takes its next() for members='each', deterministic and model_noise=False
    before any of these."""
    if noise.parity:
        assert members is None and eps_a is None and eps_m is None, 'a tape supplies its own members and draws'
        ks, ns, ea, em = _tape_rollout_noise(noise, H, B, A, S1)
        return [model._elite_inds[k] for k in ks] + [0] * (H - len(ks)), ns, _dev(ea, dev), _dev(em, dev)
    if members is None:
        elites = model._elite_inds
        members = [elites[noise.choice(len(elites))] for _ in range(H)]
    assert (eps_a is None) == (eps_m is None), 'eps_a and eps_m go together'
    if eps_a is not None:
        assert eps_a.dtype == eps_m.dtype == torch.float32 and eps_a.is_contiguous() and eps_m.is_contiguous() \
            and eps_a.shape == (H, B, A) and eps_m.shape == (H, B, S1), 'eps_a [H, B, A] / eps_m [H, B, S+1] float32'
    return _traj_members(model, members, H), None, eps_a, eps_m


def _traj_members(model, members, H):
    """members as an int (every step) or a sequence of H ints, checked against the
    ensemble size here: the descriptor does not carry it."""
    mem = [members] * H if isinstance(members, (int, np.integer)) else list(members)
    if len(mem) != H:
        raise ValueError(f'members: {len(mem)} entries for horizon {H}')
    E = model.ensemble_size
    for m in mem:
        if not isinstance(m, (int, np.integer)) or not 0 <= m < E:
            raise ValueError(f'members: {m!r} is not a member index of an ensemble of {E}')
    return [int(m) for m in mem]


def _particles_request(model, particles, members, noise):
    """imagine(particles=) / plan(particles=) checked: None (off), else the member index of every
    particle, 1..PLAN_MAX_PARTICLES ints ('elites': every elite in _elite_inds order; repeats are
    allowed). Not with ``members`` (a particle is a member) or a recorded tape."""
    if particles is None:
        return None
    if members is not None:
        raise ValueError('particles together with members: a particle keeps its own member for the whole horizon')
    if noise is not None and noise.parity:
        raise ValueError('particles with a recorded tape: a tape fixes the members and the draws of one run')
    E = model.ensemble_size
    if isinstance(particles, str):
        if particles != 'elites':
            raise ValueError(f"particles: {particles!r} (None, 'elites' or 1..{PLAN_MAX_PARTICLES} member indices)")
        ms = list(model._elite_inds)
    else:
        try:
            ms = list(particles)
        except TypeError:
            raise ValueError(f"particles: {particles!r} (None, 'elites' or 1..{PLAN_MAX_PARTICLES} member indices)")
    if not 1 <= len(ms) <= PLAN_MAX_PARTICLES:
        raise ValueError(f'particles: {len(ms)} members (1..{PLAN_MAX_PARTICLES})')
    for m in ms:
        if not isinstance(m, (int, np.integer)) or isinstance(m, bool) or not 0 <= m < E:
            raise ValueError(f'particles: {m!r} is not a member index of an ensemble of {E}')
    return [int(m) for m in ms]


def _fill_call(d, marr, alg, noise, start, members, eps_a, eps_m, ctr, engine, eps_layout, timer):
    """The per-call fields of a cached descriptor (_rollout_static), for drpo_rollout and the
    drpo_rollout_trajectories* calls alike. ``start``: _start_states' tuple. ``timer``: an
    EventTimer or None (engine 2 records one pair, around the fused kernel; engine 1 one per step)."""
    src, src_ptr, src_cap, init_idx, _ = start
    marr[:] = members
    d.replay_states, d.replay_ptr, d.replay_cap = src.data_ptr(), src_ptr, src_cap
    d.init_idx = 0 if init_idx is None else init_idx.data_ptr()
    d.eps_a = 0 if eps_a is None else eps_a.data_ptr()
    d.eps_m = 0 if eps_m is None else eps_m.data_ptr()
    d.seed, d.ctr = noise.seed, ctr
    d.rows_per_tile = getattr(alg, 'rows_per_tile', 0)
    d.engine, d.eps_layout = engine, (eps_layout if eps_a is not None else 0)
    d.step_events = timer.events if timer is not None else None
    if timer is not None:   # (the engine the library runs for this descriptor)
        timer.pairs = 1 if _lib.lib().drpo_rollout_engine(ctypes.byref(d)) == 2 else len(marr)


def _halt_request(alg, noise, halt, buffer, eps_layout=1):
    """Every refusal of a halt threshold (rollout(halt=), imagine(halt=)), before anything
    touches a device. buffer: the virtual-buffer path, which halts on the fused engine only.
    Returns None (off) or the threshold as the kernel compares it, rounded to float32."""
    if halt is None:
        return None
    if isinstance(halt, bool) or not isinstance(halt, (int, float, np.integer, np.floating)):
        raise ValueError(f'halt: {halt!r} (None or a float threshold on the ensemble\'s disagreement)')
    thr = float(np.float32(halt))
    if thr != thr:
        raise ValueError('halt: the threshold is NaN')
    if alg.env_params is None:
        raise ValueError('halt needs the constraint functions on the device: the host round trip of an env without '
                         'them stages nothing to cut')
    if not alg.model_ensemble.__dict__.get('_elite_inds'):
        raise ValueError('halt: the model has no elites before its first fit, so no disagreement to halt on')
    if buffer and (getattr(alg, 'rollout_engine', 0) == 1 or (noise.parity and eps_layout == 0)):
        raise ValueError('halt runs the fused engine only: not rollout_engine 1, and not a recorded tape whose draws '
                         'are indexed by the compacted row of each step (eps_layout 0), which needs it')
    return thr


def _staged_rows(alg, ws_name, B, H):
    """The fused engine's staged (states [H * B, S], actions [H * B, A]) as views of the
    workspace ``ws_name`` (step-major, original row; slots of steps a row did not live hold
    stale floats)."""
    S, A = alg.state_dim, alg.action_dim
    L = _lib.lib()
    ws = alg._workspace(ws_name, L.drpo_rollout_workspace_size(B, S, H))
    o_s, o_a = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(L.drpo_rollout_staging_offsets(B, S, H, ctypes.byref(o_s), ctypes.byref(o_a)), 'rollout_staging_offsets')
    n = H * B
    return (ws[o_s.value:o_s.value + 4 * n * S].view(torch.float32).view(n, S),
            ws[o_a.value:o_a.value + 4 * n * A].view(torch.float32).view(n, A))


def _cut_desc(scores, row_stride, step_stride, thr, B, dev):
    """drpo_rollout_cut_t over ``scores`` with a fresh halted_at [B]. Returns (descriptor, halted_at)."""
    from ._abi import RolloutCut
    cut = RolloutCut()
    halted_at = torch.empty(B, dtype=torch.int32, device=dev)
    cut.scores, cut.row_stride, cut.step_stride = scores.data_ptr(), row_stride, step_stride
    cut.threshold, cut.halted_at = thr, halted_at.data_ptr()
    return cut, halted_at


def rollout(alg, policy, initial_states, noise, timer=None, eps_layout=0, halt=None):
    """One imagined rollout (src/smbpo.py:229-249) into alg.virt_buffer.

    Engine (``alg.rollout_engine``, 0 = auto, the library's choice: drpo_rollout_engine):
    2 = fused horizon kernel (default for device noise), 1 = one launch per horizon step
    (used for recorded reference draws, which are indexed by the compacted row of each step). ``eps_layout=1``
    marks a tape whose per-step draws are indexed by the original batch row
    ([B] rows every step), which drives engine 2 with recorded draws.

    halt: None, or a float threshold on the elites' disagreement (model.disagreement, the
    model's normalised state units): a row stops at the first step of its life whose
    disagreement at (state, action) is not <= halt, and that step and every later one of the
    row are not written into the buffer (drpo_rollout_stage, one disagreement pass over the
    H * B staged rows, drpo_rollout_emit_cut). The steps kept are bit-identical to the
    unhalted call's, no draw is made or moved, nothing syncs; the result carries
    ``halted_at`` ([B] int32 on the device, -1: not halted). Fused engine only."""
    H, model, vb = alg.horizon, alg.model_ensemble, alg.virt_buffer._module
    thr = _halt_request(alg, noise, halt, True, eps_layout)
    _lib.require_device(policy.group.data, model.group.data, vb._states, initial_states)
    start = _start_states(alg, initial_states, noise, alg.device)
    B = start[-1]
    assert B * H <= vb.capacity, 'We do not support extending by more than buffer capacity'
    members, ns, eps_a, eps_m = _members_and_draws(model, noise, H, B, alg.action_dim, alg.state_dim + 1, alg.device)
    ctr = noise.next()
    start_ptr = vb.pointer if vb._host_ptr is not None else None
    policy.group.ensure_packed()
    model.group.ensure_packed()
    d, marr, count, _ = _rollout_static(alg, policy, B, H, buffer=True)
    _fill_call(d, marr, alg, noise, start, members, eps_a, eps_m, ctr,
               getattr(alg, 'rollout_engine', 0) if thr is None else 2, eps_layout, timer)
    L = _lib.lib()
    if thr is None:
        _lib.check(L.drpo_rollout(ctypes.byref(d), _lib.stream()), 'rollout')
        vb._device_advanced()
        return _RolloutResult(vb, start_ptr, count, ns)
    _lib.check(L.drpo_rollout_stage(ctypes.byref(d), _lib.stream()), 'rollout_stage')
    # never-staged slots hold stale floats: their scores are computed and never read
    s, a = _staged_rows(alg, f'rollout.{B}.{H}', B, H)
    scores = model.disagreement(s, a, outputs=('disagreement',)).disagreement
    cut, halted_at = _cut_desc(scores, 1, B, thr, B, alg.device)
    _lib.check(L.drpo_rollout_emit_cut(ctypes.byref(d), ctypes.byref(cut), _lib.stream()), 'rollout_emit_cut')
    vb._device_advanced()
    return _RolloutResult(vb, start_ptr, count, ns, halted_at)


# the fused engine's horizon limit (DRPO_ROLLOUT_FUSED_MAX_H; read at import, before the
# library loads: tests/test_path_queries.py pins it to drpo_abi_const)
TRAJ_MAX_H = 128


def _traj_spec(B, H, S, A, C):
    """ImaginedRollout's tensors as the kernel writes them: (name, shape, dtype, field of drpo_rollout_traj_t)."""
    f32, i32, b8 = torch.float32, torch.int32, torch.bool
    return (('states', (B, H + 1, S), f32, 'states'), ('actions', (B, H, A), f32, 'actions'),
            ('rewards', (B, H), f32, 'rewards'), ('constraint_values', (B, H, C), f32, 'constraint_values'),
            ('dones', (B, H), b8, 'dones'), ('violations', (B, H), b8, 'violations'), ('lengths', (B,), i32, 'len'),
            ('returns', (B,), f32, 'ret'), ('max_constraint', (B, C), f32, 'hmax'),
            ('first_violation', (B,), i32, 'first_violation'), ('terminated', (B,), b8, 'terminated'))


class ImaginedRollout:
    """Imagined trajectories, one per start state (row i of every tensor is the rollout
    from start state i). With B rows, horizon H:

      states [B, H+1, S]         states[i, t] at the start of step t, states[i, lengths[i]] the last next state
      actions [B, H, A], rewards [B, H], constraint_values [B, H, C]
      dones, violations [B, H]   bool
      lengths [B] int32          steps the row lived, 1..H (0..H under imagine(halt=))
      returns [B]                sum_t weights[t] * rewards[i, t] (weights: discount ** t)
      max_constraint [B, C]      max over the row's steps of constraint_values
      first_violation [B] int32  first step with a violation, -1 if none
      terminated [B] bool        the row ended with done (False: cut by the horizon)
      mask [B, H] bool           t < lengths[i]

    Everything at or beyond a row's length is zero. ``members`` is the ensemble member
    of each step. members='each' stacks the runs on a new leading axis, and so does particles=
    (one run per particle, a member index each; ``particle_launches`` then says how many horizon
    launches made them, None otherwise). ``given_steps``:
    the leading steps whose actions the caller gave (0: every action is the policy's),
    executed as given (imagine(actions=)) or proposed to the shield (imagine(proposals=):
    ``actions`` then holds what the shield let the row execute, ``certificate`` at those steps
    the proposal's).

    Under the shield (imagine(shield=)) three attributes are set, None otherwise:
      interventions [B, H] bool  the step took the safe actor's action
      certificate [B, H]         the constraint critic's certificate of the actor's action
      shield_threshold           the threshold the certificate was compared with
    Under the linear shield (imagine(shield='linear')) two more, None otherwise:
      blend [B, H] uint8         j of the action taken: 0 the policy's, K-1 the safe actor's,
                                 between them the blend with share blend / (K-1) of the safe
                                 action; interventions is blend != 0
      shield_candidates          K
    With imagine(uncertainty=) four more, None otherwise (EnsembleSpread's per-row numbers
    at (states[i, t], actions[i, t]), in the model's normalised state units):
      disagreement, epistemic, aleatoric [B, H]   zero at and beyond a row's length
      max_disagreement [B]       the largest disagreement over the row's steps
    With imagine(halt=) two more, None otherwise; every tensor above then describes the
    trajectories as cut (a row halted at step 0 has length 0: states[i, 0] its start state,
    returns 0, max_constraint -inf, terminated False):
      halted_at [B] int32        the step whose disagreement was not <= the threshold, where
                                 the row stops (its new length), -1 if it was not halted
      halt_threshold             the threshold, as compared (float32)
    With imagine(lookahead=) seven more, None otherwise (C: the constraint critic's outputs,
    con_dim, or 1 for a 'cost' solver; drpo_rollout_lookahead has the definition):
      step_q [B, H]              min over solver.critic's nets at (states[i, t], actions[i, t]); 0 at
                                 and beyond the length
      step_qc [B, H, C]          solver.constraint_critic (its mean or its bound) at the same rows,
                                 always with the C axis; 0 at and beyond the length
      terminal_q [B]             min Q at (states[i, lengths[i]], the policy's mean action there); 0
                                 for terminated rows
      terminal_qc [B, C]         Qc at (states[i, lengths[i]], actor_safe's mean action there); 0 for
                                 terminated rows
      value_lookahead [B, H+1]   entry k: sum_{t<k} discount^t r'_t + discount^k min Q after k steps,
                                 in the critics' reward units; entries beyond the length repeat
      certificate_lookahead [B, H+1, C]   entry k: the constraint critic's backup unrolled k steps
                                 along the trajectory, closed with Qc
      lookahead_kind             'mean' or 'bound'"""
    TENSORS = tuple(s[0] for s in _traj_spec(0, 0, 0, 0, 0))
    # the optional groups: name -> (per-run tensors, which stack stacks; scalars, which it copies)
    GROUPS = {'shield': (('interventions', 'certificate'), ('shield_threshold',)),
              'linear': (('blend',), ('shield_candidates',)),
              'uncertainty': (('disagreement', 'epistemic', 'aleatoric', 'max_disagreement'), ())}
    # the group of the post-pass that rewrites the core tensors (imagine(halt=)); set and stacked like GROUPS
    HALT_GROUP = {'halt': (('halted_at',), ('halt_threshold',))}
    # the group of the critics' post-pass (imagine(lookahead=)), which runs after the cut; set and stacked alike
    LOOKAHEAD_GROUP = {'lookahead': (('step_q', 'step_qc', 'terminal_q', 'terminal_qc', 'value_lookahead',
                                      'certificate_lookahead'), ('lookahead_kind',))}
    _ALL_GROUPS = dict(GROUPS, **HALT_GROUP, **LOOKAHEAD_GROUP)
    _UNSET = dict.fromkeys(k for per_run, scalars in _ALL_GROUPS.values() for k in per_run + scalars)

    def __init__(self, members, given_steps=0, **tensors):
        assert set(tensors) == set(self.TENSORS)
        self.members = members
        self.given_steps = given_steps
        self.particle_launches = None
        self.__dict__.update(self._UNSET, **tensors)

    def set_group(self, group, **values):
        """Set every attribute of one optional group."""
        per_run, scalars = self._ALL_GROUPS[group]
        assert set(values) == set(per_run + scalars), (group, sorted(values))
        self.__dict__.update(values)

    @property
    def mask(self):
        H = self.rewards.shape[-1]
        return torch.arange(H, device=self.lengths.device) < self.lengths.unsqueeze(-1)

    def first_uncertain(self, threshold):
        """[B] int32: the first step of the row's life whose disagreement exceeds
        ``threshold``, -1 if none (first_violation's counterpart; needs uncertainty=)."""
        if self.disagreement is None:
            raise ValueError('first_uncertain needs imagine(uncertainty=)')
        over = (self.disagreement > threshold) & self.mask
        first = over.to(torch.int32).argmax(dim=-1).to(torch.int32)
        return torch.where(over.any(dim=-1), first, torch.full_like(first, -1))

    @classmethod
    def stack(cls, runs):
        out = cls([r.members for r in runs], runs[0].given_steps,
                  **{k: torch.stack([getattr(r, k) for r in runs]) for k in cls.TENSORS})
        for group, (per_run, scalars) in cls._ALL_GROUPS.items():
            if getattr(runs[0], per_run[0]) is not None:
                out.set_group(group, **{k: torch.stack([getattr(r, k) for r in runs]) for k in per_run},
                              **{k: getattr(runs[0], k) for k in scalars})
        return out

    def flat_runs(self):
        """Of G stacked runs (members='each', particles=): the core tensors with the leading
        axes [G, B] merged to G * B rows, run-major, as views (no copy); no optional group."""
        return ImaginedRollout(self.members, self.given_steps,
                               **{k: getattr(self, k).flatten(0, 1) for k in self.TENSORS})


class EnsembleSpread:
    """How far the ensemble members' predictions for n rows (s, a) are apart
    (BatchedGaussianEnsemble.disagreement, drpo_ens_spread), over the member list
    ``members``. Per column k of [next state | reward]:

      mean [n, S+1]            the mean prediction over the members
      epistemic_std [n, S+1]   population std of the members' means
      aleatoric_std [n, S+1]   root of the mean predicted variance; the squares of the two
                               stds add up to the mixture's predictive variance
    and per row, with the column weights ``scale`` of the call:
      disagreement [n]         the largest distance between two members' predictions (0 for one member)
      epistemic [n]            sqrt(sum_k scale_k^2 epistemic_std_k^2)
      aleatoric [n]            sqrt(sum_k scale_k^2 aleatoric_std_k^2)"""
    TENSORS = ('mean', 'epistemic_std', 'aleatoric_std', 'disagreement', 'epistemic', 'aleatoric')

    def __init__(self, members, mean, epistemic_std, aleatoric_std, disagreement, epistemic, aleatoric):
        self.members = members
        self.mean, self.epistemic_std, self.aleatoric_std = mean, epistemic_std, aleatoric_std
        self.disagreement, self.epistemic, self.aleatoric = disagreement, epistemic, aleatoric


class ModelRolloutError:
    """The k-step open-loop model error on real episode segments (SMBPO.model_rollout_error).
    With n segments of k steps:

      starts [n] int64       chronological replay index of each segment's first row
      imagined               the ImaginedRollout from states[starts] under the segments' real actions
      state_error [n, k]     || (imagined.states[:, t+1] - real next_states[starts+t]) / (state_std + 1e-7) ||_2
      reward_error [n, k]    | imagined.rewards[:, t] - real rewards[starts+t] |
      alive [n, k] bool      the imagined mask; both errors are NaN where it is False
    With uncertainty=True, None otherwise:
      disagreement, epistemic [n, k]   EnsembleSpread's over the elites at (imagined.states[:, t],
                             actions[:, t]) with the weights 1 / (state_std + 1e-7) of state_error
                             (reward weight 0), so in its units; NaN where alive is False

    members='each' adds a leading elite axis to everything but ``starts``."""

    def __init__(self, starts, imagined, state_error, reward_error, alive, disagreement=None, epistemic=None):
        self.starts, self.imagined = starts, imagined
        self.state_error, self.reward_error, self.alive = state_error, reward_error, alive
        self.disagreement, self.epistemic = disagreement, epistemic

    def deciles(self, t):
        """Deciles (0, 10, .., 100 %) of state_error[..., t] over the rows alive at step t."""
        e = self.state_error[..., t][self.alive[..., t]]
        return torch.quantile(e, torch.linspace(0, 1, 11, device=e.device, dtype=e.dtype))


def _shield_request(alg, noise, actions, shield, candidates, uncertainty):
    """Every refusal and default of rollout_trajectories' shield arguments (its docstring), before
    anything touches a device. Returns None without a shield, else (threshold, the linear
    shield's candidates or None, whether the certificate is the critic's distributional bound)."""
    if shield is None:
        if candidates is not None or uncertainty is not None:
            raise ValueError('shield_candidates / shield_uncertainty without shield')
        return None
    if actions is not None:
        raise ValueError('shield with actions: a given action is taken as it is (to have the shield judge '
                         'given actions, pass them as proposals=)')
    if noise.parity:
        raise ValueError('shield with a recorded tape: the reference rollout a tape records has no shield')
    if candidates is not None and not (isinstance(candidates, (int, np.integer)) and
                                       not isinstance(candidates, bool) and 2 <= candidates <= 32):
        raise ValueError(f'shield_candidates: {candidates!r} (an int, 2..32)')
    if uncertainty and not alg.solver.distributional_qc:
        raise ValueError('shield_uncertainty: the constraint critic is not distributional')
    if uncertainty is None:
        uncertainty = alg.solver.distributional_qc and candidates is None
    return float(shield), None if candidates is None else int(candidates), bool(uncertainty)


def _proposal_request(noise, actions, proposals, shield):
    """Every refusal of rollout_trajectories' ``proposals`` (its docstring), before anything
    touches a device. Returns whether the call is the proposals form."""
    if proposals is None:
        return False
    if actions is not None:
        raise ValueError('proposals with actions: a leading step is either executed as given (actions=) or '
                         'proposed to the shield (proposals=), not both')
    if shield is None:
        raise ValueError('proposals without shield: a proposal is what the shield judges; actions= executes the '
                         'given actions as they are')
    if noise.parity:
        raise ValueError('proposals with a recorded tape: a tape fixes the policy\'s draws, and the reference '
                         'rollout it records has no shield')
    return True


def _shield_desc(alg, policy, B, H, threshold, dist):
    """drpo_rollout_shield_t of alg's shield: alg.actor_safe, alg.constraint_critic (dist:
    its distributional bound; False: its mean, the log-std head left out), fresh [B, H]
    outputs. Refuses what the kernels do not run. Returns (descriptor, (interventions
    uint8, certificate))."""
    from ._abi import RolloutShield
    safe, cc = alg.actor_safe, alg.constraint_critic
    if safe.spec.dims != policy.spec.dims:
        raise ValueError(f'shield: the safe actor\'s layers {safe.spec.dims} are not the policy\'s {policy.spec.dims}')
    Hc, Cq = cc.hidden_dim, cc.output_dim
    if cc.trunk_layers != 2 or cc.head_layers != 1:
        raise ValueError(f'shield: the kernels run the reference\'s ConstraintCritic (trunk_layers 2, head_layers 1), '
                         f'not {cc.trunk_layers} / {cc.head_layers}')
    if not (1 <= Hc <= 256 and 1 <= Cq <= 8):
        raise ValueError(f'shield: constraint critic hidden width {Hc} / outputs {Cq} outside 1..256 / 1..8')
    _lib.require_device(safe.group.data, cc.group.data)
    safe.group.ensure_packed()
    cc.group.ensure_packed()

    def views(g, prefix, n):
        return [x for i in range(n) for x in (g.pview(f'{prefix}{2 * i}.weight')[0].data_ptr(),
                                              g.view(f'{prefix}{2 * i}.bias').data_ptr())]
    sh = RolloutShield()
    sh.sW1, sh.sb1, sh.sW2, sh.sb2, sh.sW3, sh.sb3 = views(safe.group, 'net.', 3)
    sh.cW1, sh.cb1, sh.cW2, sh.cb2 = views(cc.group, cc.prefix + 'trunk.', 2)
    sh.qW1, sh.qb1, sh.qW2, sh.qb2 = views(cc.group, cc.prefix + 'mean_head.', 2)
    if dist:
        sh.zW1, sh.zb1, sh.zW2, sh.zb2 = views(cc.group, cc.prefix + 'log_std_head.', 2)
    sh.Hc, sh.Cq, sh.distributional = Hc, Cq, int(dist)
    sh.std_ratio, sh.log_std_min, sh.log_std_max = float(cc.std_ratio), float(cc.log_std_min), float(cc.log_std_max)
    sh.threshold = threshold
    dev = alg.device
    keep = (torch.empty(B, H, dtype=torch.uint8, device=dev), torch.empty(B, H, dtype=torch.float32, device=dev))
    sh.interventions, sh.certificate = keep[0].data_ptr(), keep[1].data_ptr()
    return sh, keep


def _given_actions(actions, B, H, A, name='actions'):
    """rollout_trajectories' ``actions`` (or, under ``name``, its ``proposals``) checked. Returns
    (actions [B, K, A] or None, K; 0 without)."""
    if actions is None:
        return None, 0
    if not torch.is_tensor(actions) or actions.dtype != torch.float32 or not actions.is_contiguous():
        raise ValueError(f'{name}: a contiguous float32 tensor [B, K, A] (or [B, A])')
    _lib.require_device(actions)
    if actions.dim() == 2:
        actions = actions.unsqueeze(1)
    if actions.dim() != 3 or actions.shape[2] != A:
        raise ValueError(f'{name}: shape {tuple(actions.shape)} is not [B, K, {A}]')
    if actions.shape[0] != B:
        raise ValueError(f'{name}: {actions.shape[0]} rows for {B} trajectories')
    K = actions.shape[1]
    if not 1 <= K <= H:
        raise ValueError(f'{name}: {K} given steps, need 1 <= K <= horizon {H}')
    return actions, K


def _traj_outputs(out, spec, dev):
    """The tensors of ``spec`` (_traj_spec): those of ``out``, checked, and fresh ones for the rest."""
    out = {} if out is None else dict(out)
    names = set(ImaginedRollout.TENSORS)
    assert set(out) <= names, f'out: unknown names {sorted(set(out) - names)}'
    res = {}
    for name, shape, dt, _ in spec:
        t = out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=dev)
        else:
            _lib.require_device(t)
            assert (t.dtype == dt or (dt == torch.bool and t.dtype == torch.uint8)) and tuple(t.shape) == shape and \
                t.is_contiguous(), f'out[{name!r}]: need contiguous {dt} {shape}'
        res[name] = t
    return res


def rollout_trajectories(alg, policy, initial_states, noise, *, members=None, eps_a=None, eps_m=None, eps_layout=1,
                         weights=None, out=None, horizon=None, ctr=None, actions=None, timer=None, shield=None,
                         shield_candidates=None, shield_uncertainty=None, proposals=None):
    """One imagined rollout (src/smbpo.py:229-249) kept per trajectory: the fused horizon
    kernel and the trajectory tail (drpo_rollout_trajectories). Never touches
    alg.virt_buffer. Mirrors ``rollout``: the same start states, members and draws for
    the same noise object, so row i here is the trajectory whose surviving steps
    ``rollout`` writes into the buffer.

    members: None = one random elite per step (from ``noise``, as ``rollout``), an int, or
    H ints. eps_a [H, B, A] / eps_m [H, B, S+1]: recorded draws on the device, indexed by
    original row (eps_layout 1); a TapeNoise in that layout supplies its own. weights: H
    float64 per-step weights of ``returns`` (default ones). out: dict of preallocated
    tensors by ImaginedRollout name. horizon: default alg.horizon. ctr: the noise counter
    (default: the next one of ``noise``).

    actions: a contiguous float32 device tensor [B, K, A] (or [B, A]: K = 1), 1 <= K <=
    horizon: steps 0 .. K-1 of trajectory i take actions[i, t] in place of the policy's
    action, as given (post-tanh; neither clamped nor squashed), and the policy acts from
    step K on (drpo_rollout_trajectories_given). No other draw moves. timer: an
    EventTimer whose first pair brackets the horizon kernel.

    shield: a float threshold: every step runs the real-environment controller's safety
    shield (src/smbpo.py:124-136) inside the kernel (drpo_rollout_trajectories_shielded):
    the certificate of the policy's action from alg.constraint_critic (its quantile bound
    when the solver's distributional_qc is set, else its mean; the maximum over its
    outputs), and alg.actor_safe's mean action where it exceeds the threshold. The result
    carries interventions, certificate and shield_threshold. No draw is made or moved. Not
    with ``actions`` or a recorded tape.

    shield_candidates: K, 2..32, with ``shield``: the evaluation's linear shield instead
    (src/sampling.py:430-437, drpo_rollout_trajectories_linear): of the K blends between the
    policy's action (j = 0) and the safe actor's (j = K-1), drpo_shield_mix's candidates,
    the one closest to the policy's whose certificate is <= the threshold, the safe action
    if none is. The result carries blend and shield_candidates too.
    shield_uncertainty: whether the certificate is the critic's distributional bound.
    Default: solver.distributional_qc for the threshold shield, False for the linear one
    (the evaluation scores its candidates by the mean). True needs a distributional critic.

    proposals: ``actions``' shape and checks, with ``shield`` (either one): steps 0 .. K-1 of
    trajectory i propose proposals[i, t] to the shield in place of the policy's sample, as
    _shielded_action passes a proposed action through the certificate, and take what the
    shield lets through (drpo_rollout_trajectories_proposed): the proposal, or the safe
    actor's action (the linear shield: the first passing blend between the two). The result's
    ``actions`` are the executed ones, ``certificate`` at a given step is the proposal's,
    ``given_steps`` is K. No draw is made or moved. Not with ``actions``, without ``shield``
    (that is ``actions``) or with a recorded tape."""
    from ._abi import RolloutGiven, RolloutLinear, RolloutTraj
    dev = alg.device
    H = alg.horizon if horizon is None else int(horizon)
    if not 1 <= H <= TRAJ_MAX_H:
        raise ValueError(f'horizon {H}: imagined trajectories run the fused engine, 1 <= horizon <= {TRAJ_MAX_H}')
    S, A, C, model = alg.state_dim, alg.action_dim, alg.con_dim, alg.model_ensemble
    # the requests, checked
    if actions is not None and noise.parity:
        raise ValueError('actions with a recorded tape: a tape fixes the policy\'s draws')
    proposed = _proposal_request(noise, actions, proposals, shield)
    request = _shield_request(alg, noise, actions, shield, shield_candidates, shield_uncertainty)
    _lib.require_device(policy.group.data, model.group.data, initial_states)

    # inputs (the noise object is consumed here, in _members_and_draws' order)
    start = _start_states(alg, initial_states, noise, dev)
    B = start[-1]
    actions, K = _given_actions(proposals, B, H, A, 'proposals') if proposed else _given_actions(actions, B, H, A)
    _lib.require_device(eps_a, eps_m)
    mem, _, eps_a, eps_m = _members_and_draws(model, noise, H, B, A, S + 1, dev, members, eps_a, eps_m)
    ctr = noise.next() if ctr is None else ctr
    w = torch.ones(H, dtype=torch.float64, device=dev) if weights is None else \
        torch.as_tensor(weights, dtype=torch.float64).to(dev).contiguous()
    assert w.shape == (H,), 'weights: one float64 per step'

    # outputs
    spec = _traj_spec(B, H, S, A, C)
    res = _traj_outputs(out, spec, dev)
    im = ImaginedRollout(mem, K, **res)
    im._weights = w     # (kept for _cut_trajectories, which sums the returns again)

    # descriptors
    policy.group.ensure_packed()
    model.group.ensure_packed()
    d, marr, _, _ = _rollout_static(alg, policy, B, H, buffer=False)
    _fill_call(d, marr, alg, noise, start, mem, eps_a, eps_m, ctr, 2, eps_layout, timer)
    t = RolloutTraj()
    for name, _, _, field in spec:
        setattr(t, field, res[name].data_ptr())
    t.weights = w.data_ptr()
    entry, extra = 'rollout_trajectories', ()     # the entry point of csrc/rollout.hip and its own descriptors
    if K:
        given = RolloutGiven()
        given.actions, given.steps = actions.data_ptr(), K
        entry, extra = 'rollout_trajectories_given', (given,)
    if request is not None:
        threshold, candidates, dist = request
        sh, (interventions, certificate) = _shield_desc(alg, policy, B, H, threshold, dist)
        im.set_group('shield', interventions=interventions.view(torch.bool), certificate=certificate,
                     shield_threshold=threshold)
        entry, extra = 'rollout_trajectories_shielded', (sh,)
        if candidates is not None:
            lin = RolloutLinear()
            blend = torch.empty(B, H, dtype=torch.uint8, device=dev)
            lin.candidates, lin.blend = candidates, blend.data_ptr()
            im.set_group('linear', blend=blend, shield_candidates=candidates)
            entry, extra = 'rollout_trajectories_linear', (sh, lin)
        if proposed:      # (NULL linear: the threshold shield)
            entry, extra = 'rollout_trajectories_proposed', (given, sh, lin if candidates is not None else None)

    # launch
    launch = getattr(_lib.lib(), 'drpo_' + entry)
    _lib.check(launch(ctypes.byref(d), *(None if x is None else ctypes.byref(x) for x in extra), ctypes.byref(t),
                      _lib.stream()), entry)
    return im


def _cut_trajectories(alg, policy, im, scores, thr):
    """Cuts the trajectories of ``im`` in place where ``scores`` [B, H] (float32, on the device,
    any non-zero strides) is not <= ``thr`` within a row's life (drpo_rollout_trajectories_cut;
    imagine(halt=) passes im.disagreement): rewrites the core tensors from the staging, masks
    the optional groups with the new lengths and sets the group 'halt'. Valid only directly
    after the rollout_trajectories call that made ``im`` (a single run: under members='each'
    each run before the next), whose staging it reads."""
    from ._abi import RolloutTraj
    B, H = im.rewards.shape
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim
    _lib.require_device(scores)
    if scores.dtype != torch.float32 or tuple(scores.shape) != (B, H):
        raise ValueError(f'scores: float32 [{B}, {H}], not {scores.dtype} {tuple(scores.shape)}')
    if 0 in scores.stride():
        scores = scores.contiguous()
    thr = float(np.float32(thr))
    d, _, _, _ = _rollout_static(alg, policy, B, H, buffer=False)
    t = RolloutTraj()
    for name, _, _, field in _traj_spec(B, H, S, A, C):
        setattr(t, field, getattr(im, name).data_ptr())
    t.weights = im._weights.data_ptr()
    cut, halted_at = _cut_desc(scores, scores.stride(0), scores.stride(1), thr, B, alg.device)
    _lib.check(_lib.lib().drpo_rollout_trajectories_cut(ctypes.byref(d), ctypes.byref(cut), ctypes.byref(t),
                                                        _lib.stream()), 'rollout_trajectories_cut')
    # the optional groups' [B, H] tensors: zero at and beyond the new lengths
    mask = im.mask
    for group in ('shield', 'linear', 'uncertainty'):
        for k in ImaginedRollout.GROUPS[group][0]:
            v = getattr(im, k)
            if v is not None and v.shape == mask.shape:
                setattr(im, k, torch.where(mask, v, torch.zeros_like(v)))
    if im.disagreement is not None:
        im.max_disagreement = im.disagreement.max(dim=-1).values
    im.set_group('halt', halted_at=halted_at, halt_threshold=thr)
    return im


_NO_DRAW = None     # the noise object of lookahead's drpo_cc_dist call, which draws nothing


def _lookahead_request(alg, lookahead):
    """imagine(lookahead=) checked: None (off), 'mean' or 'bound'."""
    if lookahead is None or lookahead is False:
        return None
    if lookahead is True:
        return 'mean'
    if isinstance(lookahead, str) and lookahead == 'bound':
        if not alg.solver.distributional_qc:
            raise ValueError("lookahead='bound' needs a distributional constraint critic (solver.distributional_qc)")
        return 'bound'
    raise ValueError(f"lookahead: {lookahead!r} (None, True or 'bound')")


def _critic_forwards(alg, kind):
    """(qmin, qc) of the lookahead: the stand-alone forwards of solver.critic (min over its nets)
    and solver.constraint_critic (kind 'mean': its mean, 'bound': mean + std_ratio * std; always
    [rows, C]). Neither draws."""
    global _NO_DRAW
    assert kind in ('mean', 'bound'), kind
    sol, cc = alg.solver, alg.solver.constraint_critic
    C = cc.output_dim
    if kind == 'bound' and _NO_DRAW is None:
        from .rng import DeviceNoise
        _NO_DRAW = DeviceNoise(0, rank=0, world=1)

    def qc(s, a):
        q = constraint_critic_forward(cc, s, a, uncertainty=kind == 'bound', noise=_NO_DRAW)
        return q.reshape(-1, C)

    def qmin(s, a):
        qs = critic_all(sol.critic, s, a)
        q = qs[0]
        for other in qs[1:]:
            q = torch.min(q, other)
        return q
    return qmin, qc


def _terminal_critics(alg, policy, im, kind, forwards=None):
    """(terminal_q [B], terminal_qc [B, C]) of the imagined trajectories ``im``: the two critics at
    the state a row ends in, states[i, lengths[i]], under ``policy``'s and actor_safe's mean
    action; zero for terminated rows. What ops.lookahead closes its expansions with and all that
    SMBPO.plan's score (k = H) needs of the critics. forwards: _critic_forwards(alg, kind), if the
    caller has them."""
    qmin, qc = _critic_forwards(alg, kind) if forwards is None else forwards
    B, H = im.rewards.shape
    S = alg.state_dim
    zero = 0.0      # (a scalar operand of torch.where: no fill launch)
    at = im.lengths.clamp(0, H).to(torch.int64).reshape(B, 1, 1).expand(B, 1, S)
    last = torch.gather(im.states, 1, at).reshape(B, S)
    alive = ~im.terminated.view(torch.bool)
    terminal_q = torch.where(alive, qmin(last, policy.act(last, eval=True)).reshape(B), zero)
    terminal_qc = torch.where(alive.unsqueeze(-1), qc(last, alg.actor_safe.act(last, eval=True)), zero)
    return terminal_q, terminal_qc


def _lookahead_scales(alg, reward_scale=None, alive_bonus=None, constraint_scale=None, constraint_offset=None):
    """The four scales of the critics' training units (src/smbpo.py:260-270): the trainer's config
    where not given."""
    cfg = {'reward_scale': reward_scale, 'alive_bonus': alive_bonus, 'constraint_scale': constraint_scale,
           'constraint_offset': constraint_offset}
    return {k: float(getattr(alg, k) if v is None else v) for k, v in cfg.items()}


def lookahead(alg, policy, im, kind, gamma, *, reward_scale=None, alive_bonus=None, constraint_scale=None,
              constraint_offset=None):
    """What the two critics say along and at the end of the imagined trajectories ``im`` (one
    run, cut or not): fills the group 'lookahead' (imagine(lookahead=)). The stand-alone
    forwards of solver.critic (min over its nets) and solver.constraint_critic (kind 'mean': its
    mean, 'bound': mean + std_ratio * std) at every (states[i, t], actions[i, t]) and at the
    state a row ends in (under ``policy``'s and actor_safe's mean action; _terminal_critics),
    masked to zero beyond the lengths and for terminated rows; then one drpo_rollout_lookahead
    launch for the k-step expansions, k = 0..H. Dead rows are evaluated and masked, not
    compacted. Makes no draw and moves no counter. gamma: the discount; the four scales
    (src/smbpo.py:260-270) default to the trainer's config."""
    from ._abi import RolloutLookahead
    assert kind in ('mean', 'bound'), kind
    sol, cc = alg.solver, alg.solver.constraint_critic
    B, H = im.rewards.shape
    S, A, C = alg.state_dim, alg.action_dim, cc.output_dim
    dev = im.rewards.device
    _lib.require_device(im.rewards, im.states, im.actions)
    cfg = _lookahead_scales(alg, reward_scale, alive_bonus, constraint_scale, constraint_offset)
    qmin, qc = _critic_forwards(alg, kind)

    mask = im.mask
    s, a = im.states[:, :-1].reshape(B * H, S), im.actions.reshape(B * H, A)
    zero = torch.zeros((), device=dev)
    step_q = torch.where(mask, qmin(s, a).reshape(B, H), zero)
    step_qc = torch.where(mask.unsqueeze(-1), qc(s, a).reshape(B, H, C), zero)
    terminal_q, terminal_qc = _terminal_critics(alg, policy, im, kind, (qmin, qc))

    w = torch.as_tensor(np.power(np.float64(gamma), np.arange(H + 1, dtype=np.float64))).to(dev)
    value = torch.empty(B, H + 1, device=dev)
    cert = torch.empty(B, H + 1, C, device=dev)
    keep = [t.contiguous() for t in (im.rewards, im.constraint_values, im.dones, im.violations, im.lengths,
                                     im.terminated, step_q, step_qc, terminal_q, terminal_qc)]
    d = RolloutLookahead()
    d.B, d.H, d.C, d.mode, d.gamma = B, H, C, 0 if sol.constrained_fcn == 'reachability' else 1, float(gamma)
    for k, v in cfg.items():
        setattr(d, k, v)
    if d.mode == 0:
        assert tuple(im.constraint_values.shape) == (B, H, C), 'constraint_values: one column per critic output'
    (d.rewards, d.constraint_values, d.dones, d.violations, d.lengths, d.terminated, d.step_q, d.step_qc,
     d.terminal_q, d.terminal_qc) = (t.data_ptr() for t in keep)
    d.weights, d.value, d.certificate = w.data_ptr(), value.data_ptr(), cert.data_ptr()
    _lib.check(_lib.lib().drpo_rollout_lookahead(ctypes.byref(d), _lib.stream()), 'rollout_lookahead')
    im.set_group('lookahead', step_q=step_q, step_qc=step_qc, terminal_q=terminal_q, terminal_qc=terminal_qc,
                 value_lookahead=value, certificate_lookahead=cert, lookahead_kind=kind)
    return im


# ---------------------------------------------------------------------------
# gradients through imagined rollouts (drpo_rollout_adjoint)
# ---------------------------------------------------------------------------
# which implementation rollout_vjp(path=None) takes where the fused kernel admits the shapes: the
# fused launch, whose p90 is below the per-step path's p10 at 512 and at 4096 rows
# (profiles/rollout_adjoint: 212 / 228 us against 800 / 845 us)
VJP_DEFAULT_PATH = 'fused'


def rollout_adjoint_ok(alg):
    """Whether drpo_rollout_adjoint admits the trainer's model (drpo_rollout_adjoint_ok: the
    condition the entry point itself checks)."""
    return bool(_lib.lib().drpo_rollout_adjoint_ok(alg.state_dim, alg.action_dim, alg.model_ensemble.hidden_dim))


def _vjp_inputs(alg, im, grad_states, grad_rewards):
    """The stored run and the upstream gradients of rollout_vjp as contiguous float32 device
    tensors, shapes checked. Returns (states, actions, lengths, g_states or None, g_rewards or
    None, members)."""
    if im.rewards.dim() != 2:
        raise ValueError('rollout_vjp: im must be one run, not stacked runs')
    B, H = im.rewards.shape
    S, A = alg.state_dim, alg.action_dim
    members = _traj_members(alg.model_ensemble, im.members, H)
    states, actions = im.states.contiguous(), im.actions.contiguous()
    lengths = im.lengths.contiguous()
    if tuple(states.shape) != (B, H + 1, S) or tuple(actions.shape) != (B, H, A) or tuple(lengths.shape) != (B,) \
            or states.dtype != torch.float32 or actions.dtype != torch.float32 or lengths.dtype != torch.int32:
        raise ValueError('rollout_vjp: im holds states [B, H+1, S], actions [B, H, A] float32 and lengths [B] int32')
    gs = gr = None
    if grad_states is not None:
        if tuple(grad_states.shape) != (B, H + 1, S):
            raise ValueError(f'grad_states: shape {tuple(grad_states.shape)}, not {(B, H + 1, S)}')
        gs = grad_states.contiguous().float()
    if grad_rewards is not None:
        if tuple(grad_rewards.shape) != (B, H):
            raise ValueError(f'grad_rewards: shape {tuple(grad_rewards.shape)}, not {(B, H)}')
        gr = grad_rewards.contiguous().float()
    _lib.require_device(*[t for t in (states, actions, lengths, gs, gr) if t is not None])
    return states, actions, lengths, gs, gr, members


def _vjp_fused(alg, states, actions, lengths, gs, gr, members, out=None):
    """drpo_rollout_adjoint: the whole reverse sweep in one launch. out: (grad_actions, grad_start)
    buffers to write (contiguous float32 [B, H, A] and [B, S]); None: fresh ones."""
    from ._abi import RolloutAdjoint
    model = alg.model_ensemble
    mg, norm = model.group, model.state_normalizer
    mg.ensure_packed()
    B, H1, S = states.shape
    H, A = H1 - 1, actions.shape[2]
    dev = states.device
    ga, g0 = (torch.empty(B, H, A, device=dev), torch.empty(B, S, device=dev)) if out is None else out
    assert ga.is_contiguous() and g0.is_contiguous() and tuple(ga.shape) == (B, H, A) and tuple(g0.shape) == (B, S)

    def fwd(key):
        return mg.pview(key + '.weight')[0].data_ptr(), mg.view(key + '.bias').data_ptr()

    def tr(key):
        return mg.pview(key + '.weight', True)[0].data_ptr()
    d = RolloutAdjoint()
    d.B, d.H, d.S, d.A, d.Hm, d.E = B, H, S, A, model.hidden_dim, model.ensemble_size
    (d.mW1, d.mb1), (d.mW2, d.mb2), (d.dW1, d.db1) = fwd('trunk.0'), fwd('trunk.2'), fwd('diff_head.0')
    d.mT1, d.mT2, d.dT1, d.dT2 = tr('trunk.0'), tr('trunk.2'), tr('diff_head.0'), tr('diff_head.2')
    d.norm_mean, d.norm_std = norm.mean.data_ptr(), norm.std.data_ptr()
    marr = (ctypes.c_int * H)(*members)
    d.members = marr
    d.states, d.actions, d.lengths = states.data_ptr(), actions.data_ptr(), lengths.data_ptr()
    d.g_states, d.g_rewards = _lib.ptr(gs), _lib.ptr(gr)
    d.grad_actions, d.grad_start = ga.data_ptr(), g0.data_ptr()
    _lib.check(_lib.lib().drpo_rollout_adjoint(ctypes.byref(d), _lib.stream()), 'rollout_adjoint')
    return ga, g0


def _vjp_steps(alg, states, actions, lengths, gs, gr, members):
    """The same definition composed from the stand-alone launches, H times: the member's trunk and
    diff head forward with its pre-activation saves (drpo_mlp_forward), then its backward-data
    from the upstream [lam | g_r] to all S + A input columns (drpo_mlp_backward); the lam update
    in torch. No host sync: every step runs over all rows, a row's dead steps masked."""
    from .mlp_desc import UPSTREAM_GOUT, fill_bwd
    L = _lib.lib()
    model = alg.model_ensemble
    eng, norm = model.engine, model.state_normalizer
    model.group.ensure_packed()
    B, H1, S = states.shape
    H, A = H1 - 1, actions.shape[2]
    dev = states.device
    Hm = model.hidden_dim
    if gs is None:
        gs = torch.zeros(B, H + 1, S, device=dev)
    if gr is None:
        gr = torch.zeros(B, H, device=dev)
    lens = lengths.clamp(0, H).to(torch.int64).unsqueeze(-1)
    scale = norm.std + 1e-6
    ga = torch.empty(B, H, A, device=dev)
    lam = torch.zeros(B, S, device=dev)
    zero = 0.0      # (a scalar operand of torch.where: no fill launch)
    dx = torch.empty(B, S + A, device=dev)
    saves = [torch.empty(B, Hm, device=dev) for _ in range(3)]
    out = torch.empty(B, S + 1, device=dev)
    for t in range(H - 1, -1, -1):
        nets, _ = eng._nets(member=members[t])
        trunk, diff = nets[0], nets[1]
        trunk.sz[0], trunk.sz[1], diff.sz[0], diff.sy[1] = saves[0], saves[1], saves[2], out
        st, at = states[:, t], actions[:, t]
        f = fill_fwd([trunk, diff], [(st, S), (at, A)], B, trunk=True, norm=(norm.mean, norm.std))
        f.ld[0], f.ld[1] = (H + 1) * S, H * A     # rows of the trajectory-major tensors
        _lib.check(L.drpo_mlp_forward(ctypes.byref(f), _lib.stream()), 'mlp_forward')
        active = t < lens
        used = torch.where(t == lens - 1, gs[:, t + 1], lam)
        gout = torch.where(active, torch.cat([used, gr[:, t:t + 1]], dim=1), zero)
        b = fill_bwd([trunk, diff], [None, gout], B, trunk=True, dx={0: (dx, 0, S + A, False)},
                     upstream=UPSTREAM_GOUT)
        _lib.check(L.drpo_mlp_backward(ctypes.byref(b), _lib.stream()), 'mlp_backward')
        ga[:, t] = torch.where(active, dx[:, S:], zero)
        lam = torch.where(active, (gs[:, t] + used) + dx[:, :S] / scale, lam)
    g0 = torch.where(lens == 0, gs[:, 0], lam)
    return ga, g0


def rollout_vjp(alg, im, grad_states=None, grad_rewards=None, *, path=None):
    """The vector-Jacobian product of the imagined rollout ``im`` (one run of the deterministic
    model step: imagine(model_noise=False)): upstream gradients grad_states [B, H+1, S] and
    grad_rewards [B, H] (None: zeros) backed along the stored trajectories to (grad_actions
    [B, H, A], grad_start [B, S]); drpo_rollout_adjoint has the definition. Lengths, dones and
    constraint checks are constants; nothing is drawn.
    path: 'fused' the one-launch kernel (a ValueError where drpo_rollout_adjoint_ok refuses the
    model's shapes), 'steps' the same definition from H forward + backward launches, None
    VJP_DEFAULT_PATH where the fused kernel admits the shapes and 'steps' elsewhere."""
    if path not in (None, 'fused', 'steps'):
        raise ValueError(f"path: {path!r} (None, 'fused' or 'steps')")
    args = _vjp_inputs(alg, im, grad_states, grad_rewards)
    ok = rollout_adjoint_ok(alg)
    if path == 'fused' and not ok:
        raise ValueError(f"path='fused': drpo_rollout_adjoint does not take S={alg.state_dim}, A={alg.action_dim}, "
                         f"hidden width {alg.model_ensemble.hidden_dim} (path='steps' does)")
    if path is None:
        path = VJP_DEFAULT_PATH if ok else 'steps'
    return (_vjp_fused if path == 'fused' else _vjp_steps)(alg, *args)


class ValueGradient:
    """What SMBPO.value_gradient found for B rows under H given actions, all from one run:

      grad_actions [B, H, A]     d value / d actions (zero at and beyond a row's length)
      grad_states [B, S]         d value / d start state
      value [B]                  the run's value_lookahead[:, H]: sum_{t<len} discount^t r'_t, closed
                                 with discount^len min Q at the state a row ends in unless it terminated
      imagined                   the ImaginedRollout of the run (with its lookahead group)
      critic_index [B] int64     the critic whose Q was the minimum at the row's last state (the
                                 one differentiated; a constant of the gradient)"""

    def __init__(self, grad_actions, grad_states, value, imagined, critic_index):
        self.grad_actions, self.grad_states, self.value = grad_actions, grad_states, value
        self.imagined, self.critic_index = imagined, critic_index


def _saved_net(group, prefix, spec, rows):
    """_net with the saves a backward reads: every hidden layer's y and z, and the output."""
    net = _net(group, prefix, spec, rows)
    dev = group.data.device
    for l, lay in enumerate(net.layers[:-1]):
        net.sy[l] = torch.empty(rows, lay.dout, device=dev)
        net.sz[l] = torch.empty(rows, lay.dout, device=dev)
    return net


def _backward_dx(nets, gouts, rows, din):
    """One drpo_mlp_backward of up to three nets on one input (DRPO_UPSTREAM_GOUT): each net's
    gradient with respect to all ``din`` input columns, [rows, din] per net."""
    from .mlp_desc import UPSTREAM_GOUT, fill_bwd
    dxs = [torch.empty(rows, din, device=g.device) for g in gouts]
    b = fill_bwd(nets, gouts, rows, dx={j: (dx, 0, din, False) for j, dx in enumerate(dxs)}, upstream=UPSTREAM_GOUT)
    _lib.check(_lib.lib().drpo_mlp_backward(ctypes.byref(b), _lib.stream()), 'mlp_backward')
    return dxs


def terminal_value_gradient(alg, policy, last, weight):
    """weight[i] * d/ds min_k Q_k(s, tanh(mu(s))) at the rows s = last[i] ([n, S]; mu: ``policy``'s
    mean, Q_k: solver.critic's nets), the minimising critic selected per row as a constant (ties:
    the lower k). The stand-alone forwards with their saves, then drpo_mlp_backward of the
    critics to their state and action columns, (1 - a^2) in torch, and the policy net's backward
    with that on its mu columns and zeros on its log-std columns. Returns (gradient [n, S], the
    selected critic [n] int64). A zero weight gives an exactly zero row."""
    L = _lib.lib()
    critic = alg.solver.critic
    last, weight = last.contiguous(), weight.contiguous()
    _lib.require_device(policy.group.data, critic.group.data, last, weight)
    n, S = last.shape
    A = policy.action_dim
    pnet = _saved_net(policy.group, 'net.', policy.spec, n)
    _mlp([pnet], [(last, S)], n)
    a = torch.empty(n, A, device=last.device)
    _lib.check(L.drpo_policy_head(_lib.ptr(pnet.sy[-1]), n, A, 2, None, 0, 0, 0, None, None, None, None, _lib.ptr(a),
                                  _lib.stream()), 'policy_head')
    nets = [_saved_net(critic.group, f'{critic.prefix}qs.{i}.', critic.spec, n) for i in range(critic.n_critics)]
    for k in range(0, len(nets), 3):
        _mlp(nets[k:k + 3], [(last, S), (a, A)], n)
    index = torch.stack([net.sy[-1].reshape(n) for net in nets]).argmin(dim=0)
    zero = 0.0      # (a scalar operand of torch.where: no fill launch)
    d = None
    for k in range(0, len(nets), 3):
        chunk = nets[k:k + 3]
        gouts = [torch.where(index == k + j, weight, zero).reshape(n, 1) for j in range(len(chunk))]
        for dx in _backward_dx(chunk, gouts, n, S + A):
            d = dx if d is None else d + dx
    g_mu = d[:, S:] * (1.0 - a * a)
    (d_pi,) = _backward_dx([pnet], [torch.cat([g_mu, torch.zeros_like(g_mu)], dim=1)], n, S)
    return d[:, :S] + d_pi, index


def value_gradient(alg, policy, im, gamma):
    """The gradient of ``im``'s value_lookahead[:, H] (one deterministic run under H given actions,
    with its lookahead group) with respect to the actions and the start states: the upstream
    g_rewards[i][t] = gamma^t * reward_scale and, for rows that did not terminate, g_states[i][len]
    = gamma^len * terminal_value_gradient, backed through the run by rollout_vjp. Returns a
    ValueGradient. No host sync."""
    B, H = im.rewards.shape
    S = alg.state_dim
    dev = im.rewards.device
    lens = im.lengths.clamp(0, H).to(torch.int64)
    w = np.power(np.float64(gamma), np.arange(H + 1, dtype=np.float64))
    scale = float(alg.reward_scale) if float(alg.reward_scale) != 0 else 1.0    # (drpo_rollout_lookahead's r')
    zero = 0.0
    gr = torch.where(im.mask, torch.as_tensor((w[:H] * scale).astype(np.float32)).to(dev).expand(B, H), zero)
    alive = ~im.terminated.view(torch.bool)
    weight = torch.where(alive, torch.as_tensor(w.astype(np.float32)).to(dev)[lens], zero)
    at = lens.reshape(B, 1, 1).expand(B, 1, S)
    last = torch.gather(im.states, 1, at).reshape(B, S)
    g_last, index = terminal_value_gradient(alg, policy, last, weight)
    gs = torch.zeros(B, H + 1, S, device=dev).scatter_(1, at, g_last.unsqueeze(1))
    ga, g0 = rollout_vjp(alg, im, gs, gr)
    return ValueGradient(ga, g0, im.value_lookahead[:, H], im, index)


# ---------------------------------------------------------------------------
# planning on the model (SMBPO.plan): the two launches of an iteration
# ---------------------------------------------------------------------------
# the limits and the draw site of csrc/plan.hip (literals so that this module imports before the
# library loads: tests/test_plan_checks.py pins them to drpo_abi_const)
PLAN_MAX_CANDIDATES = 1024
PLAN_SITE = 0x91a7
PLAN_MAX_PARTICLES = 32


class PlanResult:
    """What SMBPO.plan found for P start states, N candidates of K given steps each:

      actions [P, K, A]          the best action sequence of the last iteration (its rank 0)
      action [P, A]              actions[:, 0], the action to take now
      score [P]                  its planning score, value_lookahead[:, H] of its trajectory
      certificate [P]            the largest of its certificate_lookahead[:, H, :]
      feasible [P] bool          certificate <= threshold (and neither is NaN)
      n_feasible [P] int32       feasible candidates of the last iteration
      mean, std [P, K, A]        the sampling distribution after the last refit
      history_score, history_certificate, history_feasible [iterations, P]   the best row of each iteration
    and of the last iteration:
      candidates [P, N, K, A]; scores, certificates [P, N]; ranks [P, N] int32 (0 the best)
      imagined                   the ImaginedRollout of its P * N rows (row p * N + n)
    ``threshold`` is the certificate threshold as compared (float32), ``lookahead_kind`` 'mean'
    or 'bound'.

    Under plan(safety_filter=) every candidate ran behind the shield, and ``actions`` /
    ``action`` stay the proposals. Four more, None otherwise, of the best row:
      executed_actions [P, H, A] what the shield let it execute (all H steps of its trajectory)
      safe_action [P, A]         executed_actions[:, 0], the action to hand to the environment
      interventions [P, H] bool  the steps at which the shield stepped in
      filter_threshold           the shield's threshold, as imagine's shield_threshold

    How the call drew and started, None from a caller that does not say (MPC_FIELDS):
      noise_beta                 the lag-1 correlation of the candidates' noise (0.0: white)
      warm_started               whether it started from a previous result (plan(warm_start=))
      shift                      the steps that warm start dropped, None for a cold start

    Under plan(particles=) every candidate ran under each of G ensemble members, and ``scores`` /
    ``certificates`` / ``ranks``, the best row and the history are of the aggregate over them
    (drpo_plan_refit_particles). ``imagined`` has the leading axis G; executed_actions is
    [G, P, H, A] and interventions [G, P, H] (the best row under each member), safe_action
    executed_actions[0, :, 0]: step 0 is the same in every group. Six more, None otherwise
    (PARTICLE_FIELDS):
      particles                  the member index of each particle, G ints
      risk, cert_risk            as given: 'mean', 'worst' or ('cvar', alpha); 'max' or 'mean'
      member_scores, member_certificates [G, P, N]   each member's score and certificate
      score_spread [P, N]        the members' population std of a candidate's score

    Under plan(refine=R) ``actions`` / ``action``, ``score``, ``certificate`` and ``feasible`` are the
    refined incumbent's (the other per-candidate fields stay the last sampling iteration's). Three
    more, None otherwise (REFINE_FIELDS):
      refine_score [R + 1, P]    the incumbent's score before and after each round
      refine_accepted [R, P] int32   the trial j a round took (step refine_step * 2^-j), -1: none
      refine_gradient [P, K, A]  the last round's gradient of the incumbent's value"""
    FIELDS =('actions', 'action', 'score', 'certificate', 'feasible', 'n_feasible', 'mean', 'std', 'history_score',
              'history_certificate', 'history_feasible', 'candidates', 'scores', 'certificates', 'ranks', 'imagined',
              'threshold', 'lookahead_kind')
    FILTER_FIELDS = ('executed_actions', 'safe_action', 'interventions', 'filter_threshold')

    MPC_FIELDS = ('noise_beta', 'warm_started', 'shift')
    PARTICLE_FIELDS = ('particles', 'risk', 'cert_risk', 'member_scores', 'member_certificates', 'score_spread')
    REFINE_FIELDS = ('refine_score', 'refine_accepted', 'refine_gradient')

    def __init__(self, executed_actions=None, safe_action=None, interventions=None, filter_threshold=None,
                 noise_beta=None, warm_started=None, shift=None, particles=None, risk=None, cert_risk=None,
                 member_scores=None, member_certificates=None, score_spread=None, refine_score=None,
                 refine_accepted=None, refine_gradient=None, **fields):
        assert set(fields) == set(self.FIELDS), sorted(set(fields) ^ set(self.FIELDS))
        self.__dict__.update(fields, executed_actions=executed_actions, safe_action=safe_action,
                             interventions=interventions, filter_threshold=filter_threshold,
                             noise_beta=noise_beta, warm_started=warm_started, shift=shift,
                             particles=particles, risk=risk, cert_risk=cert_risk, member_scores=member_scores,
                             member_certificates=member_certificates, score_spread=score_spread,
                             refine_score=refine_score, refine_accepted=refine_accepted,
                             refine_gradient=refine_gradient)


def plan_sample(mean, std, incumbent, candidates, seed, ctr, lo=-1.0, hi=1.0, corr=0.0):
    """The candidates of one planning iteration (drpo_plan_sample): [P * N, K, A] from mean, std
    and incumbent (contiguous float32 device tensors [P, K, A]). Candidate 0 of every state is
    its incumbent; the others are mean + std * z clamped to [lo, hi], z the Philox normals of
    (seed, ctr, PLAN_SITE). lo / hi default to the post-tanh range. corr in (0, 1): the noise of
    a candidate is AR(1) along its steps with that lag-1 correlation and unit variance
    (drpo_plan_sample_ar, over the same draws); corr == 0 is the white launch itself."""
    from ._abi import PlanSample, PlanSampleAr
    _lib.require_device(mean, std, incumbent)
    P, K, A = mean.shape
    for t in (mean, std, incumbent):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (P, K, A), 'plan_sample: [P, K, A]'
    cand = torch.empty(P * int(candidates), K, A, device=mean.device)
    white = corr == 0
    d = PlanSample() if white else PlanSampleAr()
    d.P, d.N, d.K, d.A, d.lo, d.hi = P, int(candidates), K, A, float(lo), float(hi)
    d.seed, d.ctr = int(seed) & 0xFFFFFFFFFFFFFFFF, int(ctr) & 0xFFFFFFFFFFFFFFFF
    d.mean, d.std, d.incumbent, d.cand = mean.data_ptr(), std.data_ptr(), incumbent.data_ptr(), cand.data_ptr()
    if white:
        _lib.check(_lib.lib().drpo_plan_sample(ctypes.byref(d), _lib.stream()), 'plan_sample')
    else:
        d.corr, d.innov = float(corr), math.sqrt(1.0 - float(corr) * float(corr))
        _lib.check(_lib.lib().drpo_plan_sample_ar(ctypes.byref(d), _lib.stream()), 'plan_sample_ar')
    return cand


def plan_shift(mean, std, incumbent, *, shift, fresh_std, std_floor, reset=None, tail=None):
    """The warm start of the next control step (drpo_plan_shift, one launch): three fresh
    [P, K, A] tensors (mean, std, incumbent) from those of the previous step, moved ``shift``
    steps towards the front. The kept steps' std is raised to ``std_floor``; the fresh steps at
    the end repeat the last kept step (or ``tail`` [P, A]) with std ``fresh_std``. States whose
    ``reset`` [P] (bool) is set start cold: zero (or ``tail``) and ``fresh_std`` at every step."""
    from ._abi import PlanShift
    P, K, A = mean.shape
    for t in (mean, std, incumbent):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (P, K, A), 'plan_shift: [P, K, A]'
    keep = [mean, std, incumbent]
    d = PlanShift()
    if reset is not None:
        assert reset.dtype in (torch.bool, torch.uint8) and reset.is_contiguous() and tuple(reset.shape) == (P,), \
            'plan_shift: reset is [P] bool'
        keep.append(reset)
        d.reset = reset.data_ptr()
    if tail is not None:
        assert tail.dtype == torch.float32 and tail.is_contiguous() and tuple(tail.shape) == (P, A), \
            'plan_shift: tail is [P, A]'
        keep.append(tail)
        d.tail = tail.data_ptr()
    _lib.require_device(*keep)
    out = [torch.empty(P, K, A, device=mean.device) for _ in range(3)]
    d.P, d.K, d.A, d.shift, d.fresh_std, d.std_floor = P, K, A, int(shift), float(fresh_std), float(std_floor)
    d.mean, d.std, d.incumbent = mean.data_ptr(), std.data_ptr(), incumbent.data_ptr()
    d.mean_out, d.std_out, d.incumbent_out = (t.data_ptr() for t in out)
    _lib.check(_lib.lib().drpo_plan_shift(ctypes.byref(d), _lib.stream()), 'plan_shift')
    return tuple(out)


class PlanController:
    """Receding-horizon control on SMBPO.plan (SMBPO.mpc builds one): one plan per act(), warm
    started from the previous one.

      act(states, reset=None)   actions [P, A] on the device for the P states, in the same order
                                at every call. A cold plan on the first call, after reset() and
                                when P changes; else plan(warm_start=last, shift=shift, reset=).
                                ``reset`` [P] bool: the states that do not continue the previous
                                call's (a new episode), which start cold.
      reset()                   forget the last result: the next act() starts cold.
      last                      the PlanResult of the last act(); steps: the calls so far.

    The action is the result's safe_action under safety_filter, else its action. fallback='safe':
    a state whose best row is not feasible takes the safe actor's mean action instead (a select
    on the device); fallback=None: the planner's action whatever its certificate. Nothing syncs
    with the host. The draws come from the ``noise`` given to mpc(), else from plan's private
    stream: the trainer's stream, the buffers and steps_sampled do not move."""

    def __init__(self, alg, fallback, shift, warm_std, plan_kwargs):
        self.alg, self.fallback, self.shift, self.warm_std = alg, fallback, shift, warm_std
        self.plan_kwargs = dict(plan_kwargs)
        self.last, self.steps = None, 0

    def reset(self):
        self.last = None

    def act(self, states, reset=None):
        alg = self.alg
        states = torch.as_tensor(states, dtype=torch.float32).reshape(-1, alg.state_dim)
        warm = self.last is not None and len(self.last.actions) == len(states)
        if warm:
            res = alg.plan(states, warm_start=self.last, shift=self.shift, warm_std=self.warm_std, reset=reset,
                           **self.plan_kwargs)
        else:
            kw = dict(self.plan_kwargs)
            tail = kw.pop('tail', None)
            if tail is not None:        # what plan_shift gives a reset state: the tail at every step
                K = kw.get('steps') or kw.get('horizon') or alg.horizon
                kw['init'] = torch.as_tensor(tail, dtype=torch.float32).unsqueeze(1).repeat(1, K, 1)
            res = alg.plan(states, **kw)
        action = res.action if res.safe_action is None else res.safe_action
        if self.fallback == 'safe':
            safe = alg.solver.actor_safe.act(states.to(alg.device), eval=True)
            action = torch.where(res.feasible.unsqueeze(-1), action, safe)
        self.last = res
        self.steps += 1
        return action


def plan_refit(alg, im, terminal_q, terminal_qc, cand, mean, std, gamma, *, candidates, threshold, elites,
               temperature, momentum, min_std, reward_scale=None, alive_bonus=None, constraint_scale=None,
               constraint_offset=None, particles=None, score_tail=None, cert_mode=0):
    """Scores, ranks and refits one planning iteration (drpo_plan_refit) on the run ``im`` of
    P * N rows under ``cand`` [P * N, K, A], with the terminal critics' values of
    _terminal_critics. mean / std [P, K, A] are read, not written. Returns a dict of fresh
    tensors: mean, std, best_actions [P, K, A]; best, n_feasible (int32), best_score, best_cert,
    best_feasible (bool) [P]; score, cert, rank (int32), weight [P, N].
    particles=G: ``im`` and the terminal values hold G runs of the P * N rows, run-major
    (ImaginedRollout.flat_runs of the stacked runs), and the launch is drpo_plan_refit_particles:
    the score is the mean of the ``score_tail`` (default G) lowest member scores, the cert the
    members' maximum (cert_mode 0) or mean (1). Three more tensors come back: member_score,
    member_cert [G, P, N] and score_spread [P, N]."""
    from ._abi import PlanRefit, PlanRefitParticles
    sol = alg.solver
    B, H = im.rewards.shape
    N = int(candidates)
    P, K, A = mean.shape
    C = sol.constraint_critic.output_dim
    G = None if particles is None else int(particles)
    if G is not None:
        assert G >= 1 and B == G * P * N, 'plan_refit: particles runs of P * N rows each'
        B //= G
    assert B == P * N and tuple(cand.shape) == (B, K, A), 'plan_refit: cand is [P * N, K, A]'
    dev = im.rewards.device
    w = torch.as_tensor(np.power(np.float64(gamma), np.arange(H + 1, dtype=np.float64))).to(dev)
    keep = [t.contiguous() for t in (im.rewards, im.constraint_values, im.dones, im.violations, im.lengths,
                                     im.terminated, terminal_q, terminal_qc, cand, mean, std)]
    _lib.require_device(*keep)
    f32, i32 = torch.float32, torch.int32
    out = {'mean': torch.empty(P, K, A, device=dev), 'std': torch.empty(P, K, A, device=dev),
           'best_actions': torch.empty(P, K, A, device=dev), 'best': torch.empty(P, dtype=i32, device=dev),
           'n_feasible': torch.empty(P, dtype=i32, device=dev), 'best_score': torch.empty(P, device=dev),
           'best_cert': torch.empty(P, device=dev), 'best_feasible': torch.empty(P, dtype=torch.uint8, device=dev),
           'score': torch.empty(P, N, device=dev), 'cert': torch.empty(P, N, device=dev),
           'rank': torch.empty(P, N, dtype=i32, device=dev), 'weight': torch.empty(P, N, device=dev)}
    d = PlanRefit() if G is None else PlanRefitParticles()
    if G is not None:
        out.update(member_score=torch.empty(G, P, N, device=dev), member_cert=torch.empty(G, P, N, device=dev),
                   score_spread=torch.empty(P, N, device=dev))
        d.G, d.score_tail, d.cert_mode = G, G if score_tail is None else int(score_tail), int(cert_mode)
    d.P, d.N, d.H, d.K, d.A, d.C, d.elites = P, N, H, K, A, C, int(elites)
    d.mode, d.gamma = 0 if sol.constrained_fcn == 'reachability' else 1, float(gamma)
    for k, v in _lookahead_scales(alg, reward_scale, alive_bonus, constraint_scale, constraint_offset).items():
        setattr(d, k, v)
    d.temperature, d.momentum, d.min_std, d.threshold = float(temperature), float(momentum), float(min_std), threshold
    if d.mode == 0:
        assert tuple(im.constraint_values.shape) == (im.rewards.shape[0], H, C), \
            'constraint_values: one column per critic output'
    (d.rewards, d.constraint_values, d.dones, d.violations, d.lengths, d.terminated, d.terminal_q, d.terminal_qc,
     d.cand, d.mean_in, d.std_in) = (t.data_ptr() for t in keep)
    d.weights = w.data_ptr()
    d.mean_out, d.std_out = out['mean'].data_ptr(), out['std'].data_ptr()
    for k in out:
        if k not in ('mean', 'std'):
            setattr(d, k, out[k].data_ptr())
    if G is None:
        _lib.check(_lib.lib().drpo_plan_refit(ctypes.byref(d), _lib.stream()), 'plan_refit')
    else:
        _lib.check(_lib.lib().drpo_plan_refit_particles(ctypes.byref(d), _lib.stream()), 'plan_refit_particles')
    out['best_feasible'] = out['best_feasible'].view(torch.bool)
    return out


def rollout_host_env(alg, policy, initial_states, noise):
    """SMBPO.rollout (src/smbpo.py:229-249) for an env WITHOUT device constraint
    functions (envs.device_env_params returned None): the policy sample and the
    elite-member sample run on the HIP kernels, and the env's own numpy
    check_done / check_violation / get_constraint_values are called on the host each
    step -- the reference's round trip (src/smbpo.py:63-65), kept only for such envs."""
    from .buffers import ConstraintSafetySampleBuffer
    from .torch_util import torchify
    dev = alg.device
    B, H = alg.rollout_batch_size, alg.horizon
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim
    model, env = alg.model_ensemble, alg.real_env
    if initial_states is None:
        real = alg.replay_buffer.get('states', device=dev)
        idx = noise.np_choice(len(real), B)
        if idx is None:
            L = _lib.lib()
            idx_t = torch.empty(B, dtype=torch.int64, device=dev)
            _lib.check(L.drpo_sample_without_replacement(_lib.ptr(idx_t), B, len(real), noise.seed, noise.next(),
                                                         _lib.stream()), 'sample_without_replacement')
        else:
            idx_t = _dev(idx, dev, torch.int64)
        states = real.index_select(0, idx_t)
    else:
        states = initial_states.to(dev).float()
        B = len(states)
    buf = ConstraintSafetySampleBuffer(S, A, B * H, con_dim=C, device=dev)
    for t in range(H):
        actions = policy.act(states, eval=False, noise=noise)
        next_states, rewards = model.sample(states, actions, noise=noise)
        s2 = next_states.cpu().numpy()
        dones = torchify(env.check_done(s2), to_device=False).to(dev)
        viols = torchify(env.check_violation(s2), to_device=False).to(dev)
        h = torchify(env.get_constraint_values(s2), to_device=False).to(dev)
        buf.extend(states=states, actions=actions, next_states=next_states, rewards=rewards,
                   dones=dones.reshape(-1), violations=viols.reshape(-1), constraint_values=h.reshape(len(s2), *(
                       [] if C == 1 else [C])))
        continues = ~dones.reshape(-1).bool()
        if int(continues.sum()) == 0:
            break
        states = next_states[continues]
    alg.virt_buffer.extend(**buf.get(as_dict=True, device=dev))
    return buf


class _RolloutResult:
    def __init__(self, vb, start_ptr, count, tape_counts=None, halted_at=None):
        self.vb, self._start, self._count, self.tape_counts = vb, start_ptr, count, tape_counts
        self.halted_at = halted_at     # rollout(halt=): device int32 [B], the step each row halted at, -1 if none

    def __len__(self):
        return int(self._count.item())

    def get(self, *names, as_dict=False, device=None):
        vb = self.vb
        names = names or vb.COMPONENT_NAMES
        n = len(self)
        end = vb.pointer
        start = end - n
        idx = (torch.arange(n, device=vb.device) + start) % vb.capacity
        out = [vb._bufs[k][idx] for k in names]
        if device is not None:
            out = [o.to(device) for o in out]
        if as_dict:
            return dict(zip(names, out))
        return out if len(out) > 1 else out[0]


# ---------------------------------------------------------------------------
# constraints / normalizer
# ---------------------------------------------------------------------------
def env_constraints(env_params, states, out=None):
    """Batched (done, violation, constraint_value) on the device; C==1 squeezed like torchify(np.squeeze(...)).
    out: preallocated contiguous device tensors (done[n], violation[n], h[n, C]) to write instead of new
    ones; done / violation bool or uint8."""
    L = _lib.lib()
    _lib.require_device(states)
    states = states.contiguous().float()
    n, S = states.shape
    C = env_params['con_dim']
    if out is None:
        out = (torch.empty(n, dtype=torch.bool, device=states.device),
               torch.empty(n, dtype=torch.bool, device=states.device),
               torch.empty(n, C, dtype=torch.float32, device=states.device))
    done, viol, h = out
    _lib.require_device(done, viol, h)
    assert done.dtype in (torch.bool, torch.uint8) and viol.dtype in (torch.bool, torch.uint8) and \
        h.dtype == torch.float32, 'env_constraints: out dtypes'
    assert done.numel() == n and viol.numel() == n and h.numel() == n * C and \
        done.is_contiguous() and viol.is_contiguous() and h.is_contiguous(), 'env_constraints: out shapes'
    if 'program' in env_params:
        # a user-defined env's constraint program (env id 4): checked against S on its upload
        prog = env_params['program'].device(states.device, S)
        _lib.check(L.drpo_env_constraints_program(_lib.ptr(prog), C, _lib.ptr(states), n, S, _lib.ptr(done),
                                                  _lib.ptr(viol), _lib.ptr(h), _lib.stream()),
                   'env_constraints_program')
    else:
        _lib.check(L.drpo_env_constraints(env_params['env_id'], env_params['tracking_surr_start'],
                                          env_params['tracking_n_surr'], env_params['thr0'],
                                          env_params['thr1'], _lib.ptr(states), n, S, _lib.ptr(done),
                                          _lib.ptr(viol), _lib.ptr(h), _lib.stream()), 'env_constraints')
    return done, viol, (h[:, 0] if C == 1 and h.dim() == 2 else h)


def normalizer_fit(X, mean, std):
    L = _lib.lib()
    _lib.require_device(X, mean, std)
    X = X.contiguous()
    N, S = X.shape
    ws = torch.empty(max(8, L.drpo_normalizer_workspace_size(N, S)), dtype=torch.uint8, device=X.device)
    _lib.check(L.drpo_normalizer_fit(_lib.ptr(X), N, S, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(ws), _lib.stream()),
               'normalizer_fit')


def normalize(x, mean, std, eps):
    L = _lib.lib()
    _lib.require_device(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    S = x.shape[-1]
    _lib.check(L.drpo_normalize(_lib.ptr(x), _lib.ptr(mean), _lib.ptr(std), float(eps), _lib.ptr(y),
                                x.numel() // S, S, _lib.stream()), 'normalize')
    return y


# ---------------------------------------------------------------------------
# stand-alone network forwards (policy act/distr, critics, multiplier): one fused
# MLP launch + one head launch each. Used outside the fused SAC step (real-env
# acting, evaluation, diagnostics) -- src/policy.py:76-100, src/ssac.py:17-111.
# ---------------------------------------------------------------------------
_default_noise = None


def default_noise():
    global _default_noise
    if _default_noise is None:
        from .rng import DeviceNoise
        _default_noise = DeviceNoise(torch.initial_seed() ^ 0xAC7)
    return _default_noise


def _mlp(nets, srcs, rows, trunk=False, norm=None, nbatch=1, sstride=None):
    L = _lib.lib()
    d = fill_fwd(nets, srcs, rows, trunk=trunk, norm=norm, nbatch=nbatch, sstride=sstride)
    _lib.check(L.drpo_mlp_forward(ctypes.byref(d), _lib.stream()), 'mlp_forward')


def _net(group, prefix, spec, out_rows=None):
    group.ensure_packed()
    net = Net(spec_layers(group, prefix, spec))
    if out_rows is not None:
        net.sy[-1] = torch.empty(out_rows, net.dout, device=group.data.device)
    return net


def _flat2(x, dim):
    x = x.contiguous().float()
    return x.reshape(-1, dim), x.shape[:-1]


def policy_raw(policy, states):
    _lib.require_device(policy.group.data, states)
    s, lead = _flat2(states, policy.state_dim)
    net = _net(policy.group, 'net.', policy.spec, len(s))
    _mlp([net], [(s, policy.state_dim)], len(s))
    return net.sy[-1], lead


def policy_act(policy, states, eval, noise=None):
    """TorchPolicy.act (src/policy.py:76-79): eval -> tanh(mu), else distr.sample()."""
    L = _lib.lib()
    raw, lead = policy_raw(policy, states)
    n, A = raw.shape[0], policy.action_dim
    a = torch.empty(n, A, device=raw.device)
    if eval:
        _lib.check(L.drpo_policy_head(_lib.ptr(raw), n, A, 2, None, 0, 0, 0, None, None, None, None, _lib.ptr(a),
                                      _lib.stream()), 'policy_head')
    else:
        noise = default_noise() if noise is None else noise
        eps = noise.normal((n, A))
        eps_t = None if eps is None else _dev(eps, raw.device)
        _lib.check(L.drpo_policy_head(_lib.ptr(raw), n, A, 0, _lib.ptr(eps_t), noise.seed, noise.next(), 9,
                                      _lib.ptr(a), None, None, None, None, _lib.stream()), 'policy_head')
    return a.reshape(*lead, A)


def policy_params(policy, states):
    """(loc, scale) of the squashed Gaussian (src/policy.py:88-97)."""
    L = _lib.lib()
    raw, lead = policy_raw(policy, states)
    n, A = raw.shape[0], policy.action_dim
    mu, sd = torch.empty(n, A, device=raw.device), torch.empty(n, A, device=raw.device)
    _lib.check(L.drpo_policy_head(_lib.ptr(raw), n, A, 3, None, 0, 0, 0, None, None, _lib.ptr(mu), _lib.ptr(sd),
                                  None, _lib.stream()), 'policy_head')
    return mu.reshape(*lead, A), sd.reshape(*lead, A)


def critic_all(critic, state, action, which=None):
    """CriticEnsemble.all (src/ssac.py:30-32): every Q net in one launch (grid.y = net);
    ``which`` restricts to a subset (random_choice, :38-40)."""
    _lib.require_device(critic.group.data, state, action)
    s, lead = _flat2(state, state.shape[-1])
    a, _ = _flat2(action, action.shape[-1])
    n = len(s)
    which = range(critic.n_critics) if which is None else which
    nets = [_net(critic.group, f'{critic.prefix}qs.{i}.', critic.spec, n) for i in which]
    for k in range(0, len(nets), 3):
        _mlp(nets[k:k + 3], [(s, s.shape[1]), (a, a.shape[1])], n)
    return [net.sy[-1].reshape(*lead) for net in nets]


def constraint_critic_forward(cc, state, action, uncertainty=False, sample=False, noise=None, repeat=1):
    """ConstraintCritic.forward (src/ssac.py:64-92): trunk + both heads in one launch,
    then the log-std clamp / quantile bound / clipped sample.

    repeat=K scores K action sets against the same states in ONE launch: ``action`` is
    [K*n, A] (set-major) and the states are read K times through a zero batch stride
    (the linear shield's candidates, src/sampling.py:430-437)."""
    assert not (uncertainty and sample), 'Uncertainty bound and sample cannot be True simultaneously.'
    L = _lib.lib()
    _lib.require_device(cc.group.data, state, action)
    s, lead = _flat2(state, state.shape[-1])
    a, _ = _flat2(action, action.shape[-1])
    if repeat > 1:
        assert len(a) == repeat * len(s), 'repeat: actions must be [repeat * n, A]'
        lead = (len(a),)
    n, C = len(a), cc.output_dim
    rows = len(s)
    trunk = _net(cc.group, cc.prefix + 'trunk.', cc.trunk_spec)
    mean = _net(cc.group, cc.prefix + 'mean_head.', cc.mean_spec, n)
    nets = [trunk, mean]
    if uncertainty or sample:
        nets.append(_net(cc.group, cc.prefix + 'log_std_head.', cc.logstd_spec, n))
    sstride = [0, rows * a.shape[1], 0] if repeat > 1 else None
    _mlp(nets, [(s, s.shape[1]), (a, a.shape[1])], rows, trunk=True, nbatch=repeat, sstride=sstride)
    shape = (*lead, C) if C > 1 else tuple(lead)
    mu = mean.sy[-1]
    if not (uncertainty or sample):
        return mu.reshape(shape)
    noise = default_noise() if noise is None else noise
    eps = noise.randn_like((n, C) if C > 1 else (n,), used=sample)
    eps_t = None if eps is None else _dev(eps, mu.device).reshape(n, C)
    q = torch.empty(n, C, device=mu.device)
    sd = torch.empty(n, C, device=mu.device) if sample else None
    _lib.check(L.drpo_cc_dist(_lib.ptr(mu), _lib.ptr(nets[2].sy[-1]), n * C, 1 if sample else 0, float(cc.std_ratio),
                              float(cc.log_std_min), float(cc.log_std_max), _lib.ptr(eps_t), noise.seed,
                              noise.next(), _lib.ptr(sd), _lib.ptr(q), _lib.stream()), 'cc_dist')
    if uncertainty:
        return q.reshape(shape)
    return mu.reshape(shape), sd.reshape(shape), q.reshape(shape)


# ---------------------------------------------------------------------------
# safety shields (src/smbpo.py:127-136, src/sampling.py:423-439)
# ---------------------------------------------------------------------------
SHIELD_NONE, SHIELD_THRESHOLD, SHIELD_LINEAR = 0, 1, 2


def shield_mix(a_perf, a_safe, K=11):
    """[K, n, A] candidates a_safe*(K-1-i)/(K-1) + a_perf*(1-(K-1-i)/(K-1))."""
    L = _lib.lib()
    _lib.require_device(a_perf, a_safe)
    a_perf, a_safe = a_perf.contiguous().float(), a_safe.contiguous().float()
    n, A = a_perf.shape
    mixes = torch.empty(K, n, A, device=a_perf.device)
    _lib.check(L.drpo_shield_mix(_lib.ptr(a_perf), _lib.ptr(a_safe), n, A, K, _lib.ptr(mixes), _lib.stream()),
               'shield_mix')
    return mixes


def shield_select(q, mode, threshold, a_perf, a_safe, mixes=None):
    """Per-row shield decision on the device; q [n(,C)] (mode 1) or [K*n(,C)] (mode 2)."""
    L = _lib.lib()
    _lib.require_device(q, a_perf, a_safe)
    a_perf, a_safe = a_perf.contiguous().float(), a_safe.contiguous().float()
    n, A = a_perf.shape
    K = 1 if mixes is None else mixes.shape[0]
    q = q.contiguous().float()
    C = q.numel() // (K * n) if mode == SHIELD_LINEAR else q.numel() // max(n, 1)
    out = torch.empty_like(a_perf)
    _lib.check(L.drpo_shield_select(_lib.ptr(q), K, n, max(C, 1), A, mode, float(threshold), _lib.ptr(a_perf),
                                    _lib.ptr(a_safe), _lib.ptr(mixes), _lib.ptr(out), _lib.stream()), 'shield_select')
    return out


def multiplier_forward(mult, state, Qc):
    """MLPMultiplier.forward (src/ssac.py:106-111)."""
    L = _lib.lib()
    _lib.require_device(mult.group.data, state, Qc)
    s, lead = _flat2(state, state.shape[-1])
    q = Qc.contiguous().float().reshape(-1, 1)
    n = len(s)
    net = _net(mult.group, 'lam.', mult.spec, n)
    _mlp([net], [(s, s.shape[1]), (q, 1)], n)
    lam = torch.empty(n, device=s.device)
    _lib.check(L.drpo_multiplier_out(n, _lib.ptr(net.sy[-1]), float(mult.upper_bound), _lib.ptr(lam), _lib.stream()),
               'multiplier_out')
    return lam.reshape(*lead)
