"""Model-based safe RL trainer (src/smbpo.py:21-440) on the HIP hot path.

The hot path -- rollout (fused horizon kernel, csrc/rollout.hip), update_solver
(SAC engine, sac_step.py) and update_models (ensemble fit) -- runs on the device
with no host synchronisation inside a rollout. Around it, the trainer keeps the
reference's driver surface so main.py's loop (setup -> evaluate -> epoch ->
evaluate, main.py:29-72) runs against it unchanged:

  step_generator   real-env collection (src/smbpo.py:111-212). The safety shield's
                   decision (qc > threshold -> safe action, :127-136) is taken on the
                   device (drpo_shield_select); the env-info consistency asserts
                   (:158-163) use the device constraint functions.
  setup / epoch    src/smbpo.py:293-325
  evaluate         linear-shield batched evaluation (src/smbpo.py:421-440 ->
                   sampling.sample_episodes_batched): the 11 shield candidates are
                   scored by ONE constraint-critic launch per step.
  log_statistics   src/smbpo.py:327-419 on the stand-alone HIP network forwards.

Constructor signature, Config fields, buffers and state_dict layout follow the
reference; ``noise`` (DeviceNoise by default, TapeNoise for parity replays)
supplies every random draw.
"""
import numpy as np
import torch

from .buffers import ConstraintSafetySampleBuffer, DummyModuleWrapper
from .checkpoint import CheckpointableData
from .config import BaseConfig, Configurable, Optional
from .distributed import GradReducer
from .dynamics import BatchedGaussianEnsemble
from .envs import ProductEnv, device_env_params, env_dims, get_max_episode_steps  # noqa: F401
from .log import default_log as log, TabularLog
from .policy import UniformPolicy
from .rng import DeviceNoise
from .ssac import SSAC
from .torch_util import Module, device as default_device, pythonic_mean

N_EVAL_TRAJ = 10
LOSS_AVERAGE_WINDOW = 10
BATCH_MAP_ROWS = 1000      # src/util.py:74 batch_map default


def deciles(a):
    """src/torch_util.py:63-65 (numpy quantiles on the host)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    q = np.quantile(a, [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
    return torch.from_numpy(np.asarray(q))


class SMBPO(Configurable, Module):
    class Config(BaseConfig):
        sac_cfg = SSAC.Config()
        model_cfg = BatchedGaussianEnsemble.Config()
        model_initial_steps = 10000
        model_steps = 2000
        model_update_period = 250
        save_trajectories = False
        horizon = 10
        alive_bonus = 1.0
        buffer_min = 5000
        buffer_max = 10 ** 6
        steps_per_epoch = 1000
        rollout_batch_size = 100
        solver_updates_per_step = 10
        real_fraction = 0.1
        action_clip_gap = 1e-6
        reward_scale = 1.
        mode = 'train'
        constraint_scale = 10.
        constraint_offset = 0.
        safe_shield = True
        safe_shield_threshold = -0.1
        eval_shield_threshold = -0.05
        eval_shield_type = "linear"
        # rollout(halt=)'s default: rows stop where the elites' disagreement exceeds it; unset: off
        rollout_halt_threshold = Optional(float)

    def __init__(self, config, env_factory, data=None, epochs=1, device=default_device, noise_seed=None):
        Configurable.__init__(self, config)
        Module.__init__(self)
        self.data = data if data is not None else CheckpointableData()
        self.device = device
        self.env_factory = env_factory
        self.episode_log = TabularLog(log.dir, 'episodes.csv') if log.dir is not None else None
        self.real_env = env_factory()
        self._eval_env = None
        self.state_dim, self.action_dim, self.con_dim = env_dims(self.real_env)
        # device constraint fns for known envs; None keeps the env's numpy fns (host round trip)
        self.env_params = device_env_params(self.real_env)
        if self.env_params is not None:
            assert self.env_params['con_dim'] == self.con_dim, 'env con_dim does not match the device constraint fns'
        self.model_ensemble = BatchedGaussianEnsemble(self.model_cfg, self.state_dim, self.action_dim, device=device)
        self.solver = SSAC(self.sac_cfg, self.state_dim, self.action_dim, self.con_dim, self.horizon, epochs,
                           self.steps_per_epoch, self.solver_updates_per_step, self.constraint_scale, env_factory,
                           self.model_ensemble, device=device)
        self.replay_buffer = self._create_buffer(self.buffer_max)
        self.virt_buffer = self._create_buffer(self.buffer_max)
        self.uniform_policy = UniformPolicy(self.real_env, device=device)
        self.register_buffer('episodes_sampled', torch.tensor(0, device=device))
        self.register_buffer('steps_sampled', torch.tensor(0, device=device))
        self.register_buffer('n_violations', torch.tensor(0, device=device))
        self.register_buffer('epochs_completed', torch.tensor(0, device=device))
        self.recent_critic_losses = []
        self.recent_cons_critic_losses = []
        self.noise = DeviceNoise(noise_seed)
        self._ws = {}
        self.stepper = None

    @property
    def eval_env(self):
        """ProductEnv of N_EVAL_TRAJ envs (1 in 'test' mode), built on first use
        (the reference builds it in __init__, src/smbpo.py:54-59)."""
        if self._eval_env is None:
            if self.mode == 'train':
                self._eval_env = ProductEnv([self.env_factory(id=i) for i in range(N_EVAL_TRAJ)])
            elif self.mode == 'test':
                self._eval_env = ProductEnv([self.env_factory(id=i) for i in range(1)])
            else:
                raise ValueError(f'Invalid SMBPO mode {self.mode!r}')
        return self._eval_env

    @property
    def actor(self):
        return self.solver.actor

    @property
    def constraint_critic(self):
        return self.solver.constraint_critic

    @property
    def actor_safe(self):
        return self.solver.actor_safe

    def _create_buffer(self, capacity):
        buf = ConstraintSafetySampleBuffer(self.state_dim, self.action_dim, capacity, con_dim=self.con_dim,
                                           device=self.device)
        return DummyModuleWrapper(buf)

    def _workspace(self, key, nbytes):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = t
        return t

    def _log_tabular(self, row):
        for k, v in row.items():
            self.data.append(k, v, verbose=True)
        if self.episode_log is not None:
            self.episode_log.row(row)

    # ------------------------------------------------------------------ constraint checks
    def check_constraints(self, states):
        """(done, violation, constraint_value) of a batch of states: the device constraint
        functions for known envs, else the env's numpy functions (src/smbpo.py:63-65)."""
        from . import ops
        if self.env_params is not None:
            return ops.env_constraints(self.env_params, states)
        from .torch_util import torchify
        s = states.detach().cpu().numpy()
        env = self.real_env
        return (torchify(env.check_done(s)), torchify(env.check_violation(s)),
                torchify(env.get_constraint_values(s)))

    def _shielded_action(self, state, noise):
        """actor.act1 + the real-env safety shield (src/smbpo.py:124-136); the shield's
        branch is a per-row select on the device."""
        from . import ops
        action = self.actor.act1(state, eval=False, noise=noise)
        if not self.safe_shield:
            return action
        sol = self.solver
        q = self.constraint_critic(state.unsqueeze(0), action.unsqueeze(0), uncertainty=sol.distributional_qc,
                                   noise=noise)
        a_safe = self.actor_safe.act(state.unsqueeze(0), eval=True)
        return ops.shield_select(q.reshape(1, -1), ops.SHIELD_THRESHOLD, self.safe_shield_threshold,
                                 action.unsqueeze(0), a_safe)[0]

    # ------------------------------------------------------------------ real-env collection
    def step_generator(self):
        """src/smbpo.py:111-212: one real-env step per next(); after buffer_min every
        step runs update_models (every model_update_period steps) and
        rollout_and_update() before acting."""
        max_episode_steps = get_max_episode_steps(self.real_env)
        episode = self._create_buffer(max_episode_steps)
        state = self.real_env.reset()
        while True:
            noise = self.noise.collection()   # identical on every data-parallel rank
            t = int(self.steps_sampled.item())
            if t >= self.buffer_min:
                if t % self.model_update_period == 0:
                    self.update_models(self.model_steps)
                self.rollout_and_update()
                action = self._shielded_action(state, noise)
            else:
                action = self.uniform_policy.act1(state, eval=False, noise=noise)
            next_state, reward, done, info = self.real_env.step(action)
            violation = info['violation']
            constraint_value = torch.tensor(info['constraint_value'], dtype=torch.float)
            d_chk, v_chk, h_chk = self.check_constraints(torch.as_tensor(next_state).unsqueeze(0))
            d_chk, v_chk, h_chk = bool(d_chk.reshape(-1)[0]), bool(v_chk.reshape(-1)[0]), h_chk.reshape(-1).cpu()
            assert done == d_chk, (done, d_chk, next_state)
            assert violation == v_chk, (violation, v_chk, next_state)
            assert torch.all(torch.isclose(constraint_value.reshape(-1), h_chk, atol=1e-03)), \
                (constraint_value, h_chk)
            for buffer in (episode, self.replay_buffer):
                buffer.append(states=state, actions=action, next_states=next_state, rewards=reward, dones=done,
                              violations=violation, constraint_values=constraint_value)
            self.steps_sampled += 1

            if done or len(episode) == max_episode_steps:
                episode_return = episode.get('rewards').sum().item()
                episode_length = len(episode)
                episode_safe = not episode.get('violations').any()
                self.episodes_sampled += 1
                if not episode_safe:
                    self.n_violations += episode.get('violations').sum()
                self._log_tabular({
                    'episodes sampled': self.episodes_sampled.item(),
                    'total violations': self.n_violations.item(),
                    'steps sampled': self.steps_sampled.item(),
                    'collect return': episode_return,
                    'collect return (+bonus)': episode_return + episode_length * self.alive_bonus,
                    'collect length': episode_length,
                    'collect safe': episode_safe,
                })
                if self.save_trajectories:
                    raise NotImplementedError('save_trajectories (h5py episode files) is outside the hot path; '
                                              'the reference writes them with src/sampling.py:202')
                episode = self._create_buffer(max_episode_steps)
                state = self.real_env.reset()
            else:
                if self.steps_sampled % max_episode_steps == 0:
                    self._log_tabular({
                        'episodes sampled': self.episodes_sampled.item(),
                        'total violations': self.n_violations.item(),
                        'steps sampled': self.steps_sampled.item(),
                        'collect return': None,
                        'collect return (+bonus)': None,
                        'collect length': None,
                        'collect safe': None,
                    })
                state = next_state
            yield t

    # ------------------------------------------------------------------ hot path
    _CONFIG = object()    # rollout(halt=)'s default: the config's rollout_halt_threshold

    def rollout(self, policy, initial_states=None, noise=None, timer=None, halt=_CONFIG):
        """src/smbpo.py:229-249 as one fused kernel for the whole horizon (device
        constraint fns), or per-step launches around the env's host fns otherwise.
        halt: None: off; a float: rows stop where the elites' disagreement is not <= it
        (ops.rollout); default: the config's rollout_halt_threshold (unset: off)."""
        from . import ops
        noise = self.noise if noise is None else noise
        if halt is self._CONFIG:
            halt = self.rollout_halt_threshold
            halt = None if isinstance(halt, Optional) else halt
        if self.env_params is None:
            ops._halt_request(self, noise, halt, True)    # (refuses any threshold: nothing is staged)
            return ops.rollout_host_env(self, policy, initial_states, noise)
        return ops.rollout(self, policy, initial_states, noise, timer, halt=halt)

    IMAGINE_SALT = 0x1A6E

    def imagine(self, states=None, policy=None, horizon=None, *, members=None, deterministic=False,
                model_noise=True, discount=None, noise=None, actions=None, shield=None,
                shield_uncertainty=None, uncertainty=None, halt=None, lookahead=None, proposals=None,
                particles=None):
        """What the model predicts happens from ``states`` under ``policy``: the rollout of
        src/smbpo.py:229-249 kept per trajectory (ops.ImaginedRollout: row i of every tensor
        is the trajectory from start state i), on the fused horizon kernel. Nothing of the
        training state changes: not the virtual buffer, its pointer or steps_sampled.

        states     None: rollout_batch_size start states drawn from the replay buffer as
                   ``rollout`` draws them; else one trajectory per given row.
        policy     default the actor; horizon default self.horizon (<= 128).
        members    None: one random elite per step, as ``rollout``; an int: that ensemble
                   member at every step; H ints; 'each': one launch per elite member with
                   common draws (same noise counter), stacked in _elite_inds order.
        particles  None: off. The trajectories under each of G ensemble members, a particle
                   each: 'elites' (every elite in _elite_inds order: members='each' bit for
                   bit) or 1..32 member indices, repeats allowed. A particle keeps its member
                   for the whole horizon and every particle sees the same draws (one noise
                   counter, as 'each'). The result has 'each''s shape, a leading axis G on
                   every tensor, and ``particle_launches``, the horizon launches that made it
                   (G: one per particle). Not with ``members`` or a recorded tape (ValueError).
        deterministic   the policy's mean action; model_noise=False: the member's mean
                   prediction. (Recorded-draw inputs of the kernel: zeros for the
                   switched-off draw, device-generated normals for the other.)
        discount   of ``returns``; default the solver's.
        noise      default a stream private to imagine, derived from the trainer's seed, so
                   the training stream is left alone. A given noise object is used the way
                   ``rollout`` uses it (imagine(noise=DeviceNoise(s)) is rollout(noise=
                   DeviceNoise(s)) row for row) and advances by one counter.
        actions    [B, K, A] (or [B, A]: K = 1), 1 <= K <= horizon: "from this state AND
                   this action". Steps 0 .. K-1 of row i take actions[i, t] as given
                   (post-tanh, as ImaginedRollout.actions holds them; not clamped); the
                   policy acts from step K on, with the draws it would have had anyway.
                   With K = horizon the policy is never evaluated. The result's
                   ``given_steps`` is K.
        proposals  ``actions``' shape, with ``shield`` in any of its spellings: "from this
                   state, if THIS is what the controller proposes". Steps 0 .. K-1 of row i
                   pass proposals[i, t] through the shield in place of the policy's sample,
                   as _shielded_action passes a proposed action through the certificate, and
                   execute what it lets through: the proposal, or actor_safe's mean action
                   (the linear shield: the first passing blend between the two, blend 0 the
                   proposal). The shielded policy acts from step K on. The result's
                   ``actions`` are the executed ones, ``certificate`` at a given step is the
                   proposal's, ``interventions`` / ``blend`` say where the shield stepped
                   in, ``given_steps`` is K. As draw-free as its parents: at threshold inf
                   the run is imagine(actions=)'s, and from the policy's own sample at
                   K = 1 it is imagine(shield=)'s. Not with ``actions``, without ``shield``
                   (that is ``actions``) or with a recorded tape (ValueError).
        shield     None / False: the policy alone. True: the controller that drives the real
                   environment, the policy behind the safety shield (_shielded_action,
                   src/smbpo.py:124-136) at self.safe_shield_threshold; a float: at that
                   threshold. Each step the constraint critic's certificate of the policy's
                   action (uncertainty=solver.distributional_qc) is compared with the
                   threshold, and actor_safe's mean action taken where it is exceeded, inside
                   the kernel. The shield makes and moves no draw: with the same noise and
                   members the shielded and the unshielded run share every draw. The result
                   carries ``interventions``, ``certificate`` and ``shield_threshold``. Not
                   with ``actions`` or a recorded tape (ValueError).
                   'linear', ('linear', thr) or ('linear', thr, K): the controller every
                   evaluation runs and every reported number comes from, the policy behind
                   the linear shield (sample_episodes_batched, src/sampling.py:430-437), at
                   self.safe_shield_threshold or thr, with K = 11 candidates or 2 <= K <= 32.
                   Of the K blends between the policy's action (j = 0) and actor_safe's mean
                   action (j = K-1) a step takes the one closest to the policy's whose
                   certificate is <= the threshold, the safe action if none is, inside the
                   kernel and as draw-free as the threshold shield. The result carries
                   ``blend`` (j per step; blend / (K-1) is the safe action's share) and
                   ``shield_candidates`` as well; ``certificate`` stays that of the policy's
                   action and ``interventions`` is blend != 0. The evaluation's controller is
                   imagine(shield='linear', deterministic=True): evaluate acts on the
                   policy's mean. Refused like the other shields; an unknown string or K
                   outside 2..32 is a ValueError.
        shield_uncertainty   whether the certificate is the critic's distributional bound
                   (needs a distributional critic). Default: solver.distributional_qc under
                   the threshold shield, False under the linear one, whose candidates the
                   evaluation scores by the critic's mean.
        uncertainty   None / False: nothing more. True: where the model does not know along
                   the trajectories, the ensemble's spread over the elites at every
                   (states[i, t], actions[i, t]) (model_ensemble.disagreement, one pass over
                   the B * H rows after the rollout): the result carries ``disagreement``,
                   ``epistemic``, ``aleatoric`` and ``max_disagreement``, and
                   first_uncertain(threshold) reads them. 'all': over every member. A
                   post-pass: it works with every other argument, makes no draw, moves no
                   counter and changes no other tensor of the result.
        halt       None: nothing more. A float: the trajectories as rollout(halt=) keeps them.
                   A row stops at the first step of its life whose disagreement (over the
                   elites; over every member with uncertainty='all') is not <= halt: that
                   step and the later ones do not exist, ``lengths`` is 0..H, and every
                   tensor is rewritten for the new lengths (drpo_rollout_trajectories_cut on
                   the staged horizon; the optional groups are masked). Implies
                   uncertainty=True. The result carries ``halted_at`` and
                   ``halt_threshold``. A post-pass like uncertainty=: every step kept is
                   bit-identical to the unhalted call's, and no draw or counter moves. Under
                   members='each' each run is cut on its own.
        lookahead  None / False: nothing more. True: what the two critics say about the
                   trajectories, which otherwise end at the horizon: ``step_q`` / ``step_qc``
                   (min over solver.critic's nets and solver.constraint_critic's mean at every
                   (states[i, t], actions[i, t])), ``terminal_q`` / ``terminal_qc`` (at the state a
                   row ends in, under the policy's and under actor_safe's mean action), and for
                   every k = 0..H ``value_lookahead[:, k]``, the k-step value expansion
                   sum_{t<k} discount^t r_t + discount^k min Q(s_k, a_k), and
                   ``certificate_lookahead[:, k]``, the constraint critic's own backup
                   (src/ssac.py:284-294) unrolled k steps and closed with Qc: "k steps of this
                   controller, then the safe actor: still certified?". Both in the critics'
                   training units (reward_scale, alive_bonus, constraint_scale and
                   constraint_offset applied, src/smbpo.py:260-270), with ``discount``.
                   [:, k] - [:, 0] is the k-step TD residual of the critic against the model;
                   value_lookahead[:, H] under actions= is the planning score with a terminal
                   value. 'bound': with the constraint critic's distributional bound mean +
                   std_ratio * std, what the shield compares (needs a distributional critic).
                   The result carries ``lookahead_kind`` ('mean' or 'bound'). A post-pass like
                   uncertainty= (ops.lookahead, drpo_rollout_lookahead): it works with every
                   other argument, runs after the cut of halt= on the cut trajectories, makes no
                   draw, moves no counter and changes no other tensor of the result. Anything
                   else is a ValueError."""
        from . import ops
        from .rng import _mix64
        if self.env_params is None:
            raise NotImplementedError('imagine needs the constraint functions on the device: give the env a '
                                      'ConstraintProgram (drpo_constraint_program, see INTEGRATION.md); the host '
                                      'round trip of such envs is not supported here')
        H = self.horizon if horizon is None else int(horizon)   # (its range: checked by ops)
        if not (uncertainty is None or isinstance(uncertainty, bool) or uncertainty == 'all'):
            raise ValueError(f"uncertainty: {uncertainty!r} (None, True or 'all')")
        halt_thr = ops._halt_request(self, noise, halt, False)
        look = ops._lookahead_request(self, lookahead)
        if halt_thr is not None and not uncertainty:
            uncertainty = True
        policy = self.actor if policy is None else policy
        if noise is None:
            if self.__dict__.get('_imagine_noise') is None:
                self._imagine_noise = DeviceNoise(_mix64(self.noise.base_seed ^ self.IMAGINE_SALT), rank=0, world=1)
            noise = self._imagine_noise
        gamma = float(self.solver.discount if discount is None else discount)
        weights = np.power(np.float64(gamma), np.arange(H, dtype=np.float64))
        if states is not None:
            states = torch.as_tensor(states, dtype=torch.float32).to(self.device).reshape(-1, self.state_dim)
        B = self.rollout_batch_size if states is None else len(states)
        if actions is not None:
            actions = torch.as_tensor(actions, dtype=torch.float32).to(self.device).contiguous()
        if proposals is not None:
            proposals = torch.as_tensor(proposals, dtype=torch.float32).to(self.device).contiguous()

        parts = ops._particles_request(self.model_ensemble, particles, members, noise)
        each = isinstance(members, str) or parts is not None
        if isinstance(members, str) and members != 'each':
            raise ValueError(f"members: {members!r} (None, an int, {H} ints or 'each')")
        # the shield's shorthand as ops' threshold and candidates; ops._shield_request refuses and defaults
        kw = {'actions': actions, 'shield_uncertainty': shield_uncertainty}
        if proposals is not None:     # (off: ops sees the call it saw before)
            kw['proposals'] = proposals
        if isinstance(shield, (str, tuple, list)):
            from .sampling import LINEAR_SHIELD_CANDIDATES
            kind, thr, K = (shield, None, None) if isinstance(shield, str) else (tuple(shield) + (None,) * 3)[:3]
            if kind != 'linear' or (not isinstance(shield, str) and not 1 <= len(shield) <= 3):
                raise ValueError(f"shield: {shield!r} (True, a threshold, 'linear', ('linear', threshold) or "
                                 "('linear', threshold, candidates))")
            kw['shield'] = float(self.safe_shield_threshold if thr is None else thr)
            kw['shield_candidates'] = LINEAR_SHIELD_CANDIDATES if K is None else K
        elif shield is not None and shield is not False:
            kw['shield'] = float(self.safe_shield_threshold if shield is True else shield)
        if each or deterministic or not model_noise:
            if noise.parity:
                raise ValueError("a recorded tape fixes the members and the draws: no 'each', deterministic or "
                                 'model_noise with it')
            kw['ctr'] = noise.next()
        if deterministic or not model_noise:
            # the kernel's recorded-draw inputs, indexed by original row
            gen = torch.Generator(device=self.device)
            gen.manual_seed(_mix64(noise.seed ^ _mix64(kw['ctr'])) & 0x7FFFFFFFFFFFFFFF)
            A, S1 = self.action_dim, self.state_dim + 1

            def draws(on, width):
                if not on:
                    return torch.zeros(H, B, width, device=self.device)
                return torch.randn(H, B, width, device=self.device, generator=gen)
            kw.update(eps_a=draws(not deterministic, A), eps_m=draws(model_noise, S1), eps_layout=1)

        def run(m):
            im = ops.rollout_trajectories(self, policy, states, noise, members=m, weights=weights, horizon=H, **kw)
            if halt_thr is not None:     # while the run's staging is still in the workspace
                self._imagined_uncertainty(im, None if uncertainty is True else 'all')
                ops._cut_trajectories(self, policy, im, im.disagreement, halt_thr)
            if look is not None:
                ops.lookahead(self, policy, im, look, gamma)
            return im
        if each:
            ms = self.model_ensemble._elite_inds if parts is None else parts
            im = ops.ImaginedRollout.stack([run(int(m)) for m in ms])
            if parts is not None:
                im.particle_launches = len(parts)
        else:
            im = run(members)
        if uncertainty and halt_thr is None:
            self._imagined_uncertainty(im, None if uncertainty is True else 'all')
        return im

    def _imagined_uncertainty(self, im, members, scale=None):
        """The ensemble's spread at every step of imagined trajectories (imagine(uncertainty=)):
        fills im.disagreement, epistemic, aleatoric and max_disagreement."""
        sp = self.model_ensemble.disagreement(im.states[..., :-1, :], im.actions, members=members, scale=scale)
        mask = im.mask
        vals = {k: getattr(sp, k).reshape(mask.shape) for k in ('disagreement', 'epistemic', 'aleatoric')}
        vals = {k: torch.where(mask, v, torch.zeros_like(v)) for k, v in vals.items()}
        # max_disagreement: >= 0, and 0 beyond a row's length
        im.set_group('uncertainty', max_disagreement=vals['disagreement'].max(dim=-1).values, **vals)

    def imagine_vjp(self, im, grad_states=None, grad_rewards=None):
        """The vector-Jacobian product of an imagined rollout: upstream gradients of its states
        (grad_states [B, H+1, S]) and rewards (grad_rewards [B, H]; None: zeros) backed along the
        stored trajectories to (grad_actions [B, H, A], grad_start [B, S]), for sensitivity
        analysis and objectives of one's own. ``im`` is one run (not stacked) of the
        deterministic model step, imagine(model_noise=False), whose ``members`` are H ints; the
        Jacobians are the members' at the stored (states, actions), so lengths, dones and
        constraint checks are constants and a row's steps at and beyond its length get zero.
        drpo_rollout_adjoint has the definition; one launch where its kernel takes the model's
        shapes, the per-step launches elsewhere (ops.rollout_vjp(path=) asks for either). Draws
        nothing and changes nothing of the trainer."""
        from . import ops
        return ops.rollout_vjp(self, im, grad_states, grad_rewards)

    GRADIENT_SALT = 0x6AD1

    def value_gradient(self, states, actions, horizon=None, members=0, discount=None, policy=None, *, noise=None,
                       model_noise=False, particles=None, shield=None, proposals=None, halt=None):
        """Which way should this action sequence move: the gradient of a rollout's value with
        respect to its actions and its start state (an ops.ValueGradient: grad_actions [B, H, A],
        grad_states [B, S], value [B], imagined, critic_index). The value is value_lookahead[:, H]
        of imagine(states, actions=actions, lookahead=True, deterministic=True,
        model_noise=False): the discounted rewards in the critics' units, closed with min Q at the
        state a row ends in, under the policy's mean action there, unless the row terminated.
        Value and gradients come from one run. The minimising critic, the lengths, dones and
        constraint checks are constants of the gradient; a terminated row gets no terminal term.

        actions    [B, H, A]: every step given (K == horizon; [B, A] at horizon 1).
        members    an int or H ints: a fixed model (default member 0).
        discount, policy   as imagine's.
        noise      default a stream private to value_gradient (the run draws nothing, but takes
                   one counter of the object it is given).
        The gradient is that of the deterministic run under given actions, so model_noise=True,
        particles=, shield=, proposals= and halt= are refused (ValueError), as are members=None /
        'each', fewer given steps than the horizon and a recorded tape. Nothing of the training
        state changes: not the trainer's stream, the buffers or steps_sampled."""
        from . import ops
        from .rng import _mix64
        for name, v in (('particles', particles), ('shield', shield), ('proposals', proposals), ('halt', halt)):
            if v is not None and v is not False:
                raise ValueError(f'{name}: value_gradient differentiates the deterministic run under given actions; '
                                 f'{name}= is not part of it')
        if model_noise:
            raise ValueError('model_noise: value_gradient is the gradient of the deterministic model step')
        if members is None or isinstance(members, str):
            raise ValueError(f'members: {members!r} (an int or one int per step: the gradient needs a fixed model)')
        if noise is not None and noise.parity:
            raise ValueError('noise: a recorded tape fixes the draws of a rollout; value_gradient draws nothing')
        H = self.horizon if horizon is None else int(horizon)
        actions = torch.as_tensor(actions, dtype=torch.float32)
        if actions.dim() == 2:
            actions = actions.unsqueeze(1)
        if actions.dim() != 3 or actions.shape[1] != H or actions.shape[2] != self.action_dim:
            raise ValueError(f'actions: shape {tuple(actions.shape)}; value_gradient needs every step given, '
                             f'[B, {H}, {self.action_dim}] for horizon {H}')
        policy = self.actor if policy is None else policy
        if noise is None:
            if self.__dict__.get('_gradient_noise') is None:
                self._gradient_noise = DeviceNoise(_mix64(self.noise.base_seed ^ self.GRADIENT_SALT), rank=0, world=1)
            noise = self._gradient_noise
        gamma = float(self.solver.discount if discount is None else discount)
        im = self.imagine(states, policy, H, members=members, deterministic=True, model_noise=False, discount=gamma,
                          noise=noise, actions=actions, lookahead=True)
        return ops.value_gradient(self, policy, im, gamma)

    PLAN_SALT = 0x91A7

    def plan(self, states, horizon=None, *, candidates=64, iterations=4, steps=None, elites=None,
             temperature=float('inf'), momentum=0.0, init=None, init_std=0.5, min_std=0.05, threshold=None,
             lookahead=True, policy=None, members=None, model_noise=False, discount=None, noise=None,
             safety_filter=None, warm_start=None, shift=1, reset=None, tail=None, warm_std=None, noise_beta=0.0,
             particles=None, risk='mean', cert_risk='max', refine=0, refine_trials=8, refine_step=0.5):
        """The best of sampled action sequences from each of the P ``states``, by the model and the
        two critics: an MPPI / CEM planner whose score is imagine(actions=, lookahead=)'s
        value_lookahead[:, H] and whose constraint is its certificate_lookahead[:, H] (the
        largest output) <= ``threshold``: "the best sequence whose unrolled certificate stays
        under the shield's threshold". Returns an ops.PlanResult. Per iteration: one launch
        that draws ``candidates`` sequences per state around the current mean (candidate 0 is
        the incumbent, the best so far), one imagine(actions=, deterministic=True) of
        P * candidates rows, the critics at the states the rows end in, and one launch that
        scores, ranks and refits (drpo_plan_sample, drpo_plan_refit have the definitions).
        Nothing syncs with the host inside the loop, and nothing of the training state changes:
        not the trainer's stream, the buffers, steps_sampled or imagine's private stream.

        horizon      H, default self.horizon (<= 128); steps: K, the planned steps, 1..H, default
                     H. From step K on the policy's mean action continues the row.
        candidates   N per state, 2..1024; iterations >= 1.
        elites       the rows a refit uses, 1..N; default max(1, N // 8). A refit takes the best
                     feasible rows (certificate <= threshold) by score; a state without a
                     feasible row the rows of the least certificate.
        temperature  > 0: an elite's weight is exp((score - best score) / temperature); the
                     default inf weighs the elites alike (CEM), small values approach the best
                     row alone (MPPI's exponential weights over the elites).
        momentum     in [0, 1): the share of the old mean and std a refit keeps.
        init         None: a zero mean; 'policy': the first K mean actions of the policy's own
                     deterministic trajectory (one more imagine run); or a [P, K, A] tensor.
                     The first incumbent is the initial mean. init_std > 0: the initial std of
                     every action; min_std >= 0: the floor of every refit.
        threshold    default self.safe_shield_threshold; -inf: no row is feasible and the result
                     is the least certificate; +inf: the argmax of the score.
        lookahead    True: the constraint critic's mean; 'bound': its distributional bound.
        policy, members, model_noise, discount   as imagine's. members=None draws one elite per
                     step anew in every iteration, so scores of different iterations are then
                     not comparable; an int or H ints fix the model. Not 'each': that is
                     ``particles``.
        particles    None: off, the candidates are scored under one model, as above. Else
                     planning over the ensemble: 'elites' or 1..32 member indices, as imagine's
                     ``particles``. Every iteration's run is imagine(particles=): each candidate
                     under each of the G members with common draws, a particle keeping its member
                     for the whole horizon; the critics close the G * P * N rows at once and one
                     launch (drpo_plan_refit_particles) aggregates the members' scores and
                     certificates per candidate, then orders and refits on the aggregate as
                     before. Not with ``members``. With fixed particles and model_noise=False
                     the aggregate is a function of the state and the candidate, so the
                     incumbent's key still never decreases. init='policy' takes the policy's
                     trajectory under the first particle. The result carries ``particles``,
                     ``risk``, ``cert_risk``, ``member_scores``, ``member_certificates`` and
                     ``score_spread``; its ``imagined`` has the leading axis G, and under
                     safety_filter so have ``executed_actions`` and ``interventions``
                     (``safe_action`` is the first group's: step 0 is the same in all of them).
        risk         of the score over the particles: 'mean' (every member counts alike), 'worst'
                     (the lowest member score) or ('cvar', alpha), 0 < alpha <= 1: the mean of
                     the max(1, ceil(alpha * G)) lowest member scores. cert_risk: 'max' (every
                     member must certify: the largest member certificate is compared with
                     ``threshold``) or 'mean'. Both need ``particles``.
        noise        default a stream private to plan, derived from the trainer's seed. Each
                     sample launch takes one noise.next(), and imagine runs on the same object.
        safety_filter   None / False: the candidates are executed as given, as above. Else the
                     shield of the real controller runs inside the planner, safe MPC: every
                     iteration's run is imagine(proposals=candidates, shield=...), so a
                     candidate is scored and ranked on the trajectory the shield would let it
                     run, and from step K on the shielded policy continues the row. True: the
                     threshold shield at self.safe_shield_threshold; a float: at that
                     threshold; 'linear', ('linear', thr) or ('linear', thr, K): the linear
                     shield, as imagine's ``shield``. The refit, ``mean`` / ``std`` and the
                     incumbent stay over the proposals (a trajectory is a function of the
                     state and the proposals once the model is fixed, so the incumbent's key
                     still never decreases), and ``actions`` / ``action`` of the result are
                     proposals. The result carries ``executed_actions``, ``safe_action``
                     (the filtered first action, the one to hand to the environment),
                     ``interventions`` and ``filter_threshold`` of the best row. Independent
                     of ``threshold``, the planner's constraint on the unrolled certificate.
        noise_beta   in [0, 1): the lag-1 correlation of a candidate's noise along its steps
                     (AR(1) at unit variance, drpo_plan_sample_ar, over the white launch's own
                     draws), in every sample launch of the call. 0: white noise through the
                     white launch. Correlated noise gives smoother candidates, which is what a
                     controller that re-plans at every step wants.
        warm_start   the previous control step's PlanResult (or any object with ``mean``,
                     ``std`` and ``actions`` [P, K, A]) over the same P states in order and the
                     same K; not with ``init``. The call starts from ops.plan_shift of the three
                     (drpo_plan_shift, one launch): the sequences moved ``shift`` steps (0..K,
                     default 1) towards the front, and the first incumbent is the shifted
                     ``actions``, not the mean. shift=0 re-plans at the same states. The fresh
                     steps at the end repeat the last kept step, or take ``tail`` [P, A], with
                     std init_std. warm_std: the floor of the kept steps' std, default min_std
                     (a converged plan's std sits at min_std, so a controller that should keep
                     exploring wants it larger, a fraction of init_std). reset [P] bool: the
                     states that start cold (a zero mean, or ``tail``, and init_std), as a new
                     episode does; all of them set is the cold call, bit for bit. reset, tail
                     and warm_std need a warm_start.
                     With a fixed member and model_noise=False, shift=0 and the same states, the
                     best key is never below warm_start's: candidate 0 is its best row, run
                     again from the same state. With shift >= 1 nothing of the kind holds: the
                     shifted sequence is scored from another state.
        refine       R >= 0 rounds of gradient refinement of the incumbent after the last sampling
                     iteration (0: none, the planner as it is, with the same launches). A round
                     takes the gradient of every state's incumbent (one value_gradient of P rows),
                     builds refine_trials = L sequences clamp(a + refine_step * 2^-j * g /
                     max|g|, -1, 1), j = 0..L-1 (a backtracking line along the gradient, the
                     largest step refine_step in action units), imagines the P * (L + 1) rows with
                     the incumbent as candidate 0, closes them with the terminal critics and ranks
                     them with drpo_plan_refit: the planner's own order, feasibility rule and
                     tie-break. The best row becomes the incumbent, so its key never decreases;
                     ``mean`` and ``std`` are not refit. A state without a feasible incumbent, or
                     whose gradient is zero or not finite, is carried through unchanged (its
                     trials repeat the incumbent). ``actions``, ``score``, ``certificate`` and
                     ``feasible`` of the result are the refined incumbent's; ``candidates``,
                     ``scores``, ``ranks``, ``n_feasible`` and ``imagined`` stay the last sampling
                     iteration's. The result carries ``refine_score`` [R + 1, P] (the incumbent's
                     score before and after each round), ``refine_accepted`` [R, P] (the j taken,
                     -1: the incumbent stayed) and ``refine_gradient`` [P, K, A] (the last
                     gradient). Needs a fixed deterministic model and every step planned: not
                     with steps < horizon, members=None, model_noise=True, particles= or
                     safety_filter= (ValueError). No host sync inside the rounds.
        Not with a recorded tape; NotImplementedError for an env without device constraint
        functions, as imagine. SMBPO.mpc wraps the warm start in a controller. halt= inside the
        planner is not built."""
        q = dict(locals())
        del q['self']
        q = self._plan_checks(**q)
        from . import ops
        from .rng import _mix64
        H, N, K, P, A = q['H'], q['N'], q['K'], q['P'], q['A']
        states, init, elites, threshold, look, filt = (q[k] for k in ('states', 'init', 'elites', 'threshold', 'look',
                                                                      'filt'))
        parts = q['parts']

        # the device work
        dev = self.device
        states = states.to(dev)
        policy = self.actor if policy is None else policy
        if noise is None:
            if self.__dict__.get('_plan_noise') is None:
                self._plan_noise = DeviceNoise(_mix64(self.noise.base_seed ^ self.PLAN_SALT), rank=0, world=1)
            noise = self._plan_noise
        gamma = float(self.solver.discount if discount is None else discount)
        run = dict(members=members, deterministic=True, model_noise=model_noise, discount=gamma, noise=noise)
        refit = {}
        if parts is not None:     # (off: imagine and plan_refit see the calls they saw before)
            first = dict(run, members=parts[0])
            run = dict(run, particles=parts)
            refit = dict(particles=len(parts), score_tail=q['score_tail'], cert_mode=q['cert_mode'])
        if warm_start is not None:
            def on_dev(x, dtype=torch.float32):
                return None if x is None else torch.as_tensor(x, dtype=dtype).to(dev).contiguous()
            mean, std, incumbent = ops.plan_shift(
                *(on_dev(getattr(warm_start, k)) for k in ('mean', 'std', 'actions')), shift=shift,
                fresh_std=init_std, std_floor=min_std if warm_std is None else warm_std,
                reset=on_dev(reset, torch.bool), tail=on_dev(tail))
        else:
            if init is None:
                mean = torch.zeros(P, K, A, device=dev)
            elif isinstance(init, str):
                mean = self.imagine(states, policy, H, **(run if parts is None else first)).actions[:, :K].contiguous()
            else:
                mean = init.to(dev).contiguous()
            std = torch.full((P, K, A), float(init_std), device=dev)
            incumbent = mean
        corr = {} if noise_beta == 0 else {'corr': float(noise_beta)}
        tiled = states.repeat_interleave(N, dim=0)
        history = []
        for _ in range(iterations):
            cand = ops.plan_sample(mean, std, incumbent, N, noise.seed, noise.next(), **corr)
            if filt is None:
                im = self.imagine(tiled, policy, H, actions=cand, **run)
            else:     # the candidates as proposals: scored on what the shield lets them run
                im = self.imagine(tiled, policy, H, proposals=cand, shield=filt, **run)
            rows = im if parts is None else im.flat_runs()      # the G * P * N rows, run-major
            terminal_q, terminal_qc = ops._terminal_critics(self, policy, rows, look)
            fit = ops.plan_refit(self, rows, terminal_q, terminal_qc, cand, mean, std, gamma, candidates=N,
                                 threshold=threshold, elites=elites, temperature=temperature, momentum=momentum,
                                 min_std=min_std, **refit)
            mean, std, incumbent = fit['mean'], fit['std'], fit['best_actions']
            history.append((fit['best_score'], fit['best_cert'], fit['best_feasible']))
        best = {k: fit[k] for k in ('best_score', 'best_cert', 'best_feasible')}
        filtered = {}
        if q['refine']:
            # gradient refinement of the incumbent (the refusals left: no particles, no filter, K == H)
            L, eta = q['refine_trials'], float(q['refine_step'])
            sizes = torch.as_tensor([eta * 2.0 ** -j for j in range(L)], dtype=torch.float32).to(dev).view(1, L, 1, 1)
            wide = states.repeat_interleave(L + 1, dim=0)
            scores, accepted = [best['best_score']], []
            for _ in range(q['refine']):
                vg = self.value_gradient(states, incumbent, H, members, gamma, policy, noise=noise)
                g = vg.grad_actions
                gmax = g.abs().amax(dim=(1, 2))
                ok = best['best_feasible'] & torch.isfinite(gmax) & (gmax > 0)
                unit = (g / gmax.view(P, 1, 1)).unsqueeze(1)
                trials = (incumbent.unsqueeze(1) + sizes * unit).clamp(-1.0, 1.0)
                trials = torch.where(ok.view(P, 1, 1, 1), trials, incumbent.unsqueeze(1))
                rcand = torch.cat([incumbent.unsqueeze(1), trials], dim=1).reshape(P * (L + 1), K, A)
                rim = self.imagine(wide, policy, H, actions=rcand, **run)
                tq, tqc = ops._terminal_critics(self, policy, rim, look)
                rfit = ops.plan_refit(self, rim, tq, tqc, rcand, mean, std, gamma, candidates=L + 1,
                                      threshold=threshold, elites=1, temperature=temperature, momentum=0.0,
                                      min_std=min_std)
                incumbent = rfit['best_actions']
                best = {k: rfit[k] for k in best}
                scores.append(best['best_score'])
                accepted.append(rfit['best'] - 1)
            filtered.update(refine_score=torch.stack(scores), refine_accepted=torch.stack(accepted), refine_gradient=g)
        if filt is not None:
            # the best row's filtered trajectory, gathered on the device (row p * N + best[p])
            rows = torch.arange(P, device=dev, dtype=torch.int64) * N + fit['best'].to(torch.int64)
            ax = 0 if parts is None else 1                      # (particles: the best row under each member)
            executed = im.actions.index_select(ax, rows)
            filtered = dict(executed_actions=executed,
                            safe_action=executed[:, 0] if parts is None else executed[0, :, 0],
                            interventions=im.interventions.index_select(ax, rows), filter_threshold=im.shield_threshold)
        if parts is not None:
            filtered.update(particles=parts, risk=risk, cert_risk=cert_risk, member_scores=fit['member_score'],
                            member_certificates=fit['member_cert'], score_spread=fit['score_spread'])
        return ops.PlanResult(
            **filtered, noise_beta=float(noise_beta), warm_started=warm_start is not None,
            shift=None if warm_start is None else shift,
            actions=incumbent, action=incumbent[:, 0], score=best['best_score'], certificate=best['best_cert'],
            feasible=best['best_feasible'], n_feasible=fit['n_feasible'], mean=mean, std=std,
            history_score=torch.stack([h[0] for h in history]),
            history_certificate=torch.stack([h[1] for h in history]),
            history_feasible=torch.stack([h[2] for h in history]),
            candidates=cand.reshape(P, N, K, A), scores=fit['score'], certificates=fit['cert'], ranks=fit['rank'],
            imagined=im, threshold=threshold, lookahead_kind=look)

    def _plan_checks(self, states, horizon, *, candidates, iterations, steps, elites, temperature, momentum, init,
                     init_std, min_std, threshold, lookahead, policy, members, model_noise, discount, noise,
                     safety_filter, warm_start, shift, reset, tail, warm_std, noise_beta, particles, risk, cert_risk,
                     refine=0, refine_trials=8, refine_step=0.5, controller=False):
        """Every refusal of plan's arguments, before any device work; returns what they resolve
        to. controller=True (SMBPO.mpc, which has no states yet): shift, tail and warm_std are
        checked as far as they can be without P and without a warm_start."""
        from . import ops
        if self.env_params is None:
            raise NotImplementedError('plan needs the constraint functions on the device, as imagine does: give the '
                                      'env a ConstraintProgram (drpo_constraint_program, see INTEGRATION.md)')

        def is_int(x):
            return isinstance(x, (int, np.integer)) and not isinstance(x, bool)

        def is_num(x):
            return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
        H = self.horizon if horizon is None else horizon
        if not (is_int(H) and 1 <= H <= ops.TRAJ_MAX_H):
            raise ValueError(f'horizon: {H!r} (an int, 1..{ops.TRAJ_MAX_H})')
        N, K = candidates, H if steps is None else steps
        if not (is_int(N) and 2 <= N <= ops.PLAN_MAX_CANDIDATES):
            raise ValueError(f'candidates: {N!r} (an int, 2..{ops.PLAN_MAX_CANDIDATES})')
        if not (is_int(iterations) and iterations >= 1):
            raise ValueError(f'iterations: {iterations!r} (an int >= 1)')
        if not (is_int(K) and 1 <= K <= H):
            raise ValueError(f'steps: {K!r} (an int, 1..horizon {H})')
        elites = max(1, N // 8) if elites is None else elites
        if not (is_int(elites) and 1 <= elites <= N):
            raise ValueError(f'elites: {elites!r} (an int, 1..candidates {N})')
        if not (is_num(temperature) and temperature > 0):
            raise ValueError(f'temperature: {temperature!r} (> 0; inf weighs the elites alike)')
        if not (is_num(momentum) and 0 <= momentum < 1):
            raise ValueError(f'momentum: {momentum!r} (in [0, 1))')
        if not (is_num(min_std) and 0 <= min_std < float('inf')):
            raise ValueError(f'min_std: {min_std!r} (finite, >= 0)')
        if not (is_num(init_std) and 0 < init_std < float('inf')):
            raise ValueError(f'init_std: {init_std!r} (finite, > 0)')
        threshold = self.safe_shield_threshold if threshold is None else threshold
        if not (is_num(threshold) and threshold == threshold):
            raise ValueError(f'threshold: {threshold!r} (a number; -inf and inf are allowed)')
        threshold = float(np.float32(threshold))
        look = ops._lookahead_request(self, lookahead)
        if look is None:
            raise ValueError(f"lookahead: {lookahead!r} (plan scores with the critics: True or 'bound')")
        if isinstance(members, str):
            raise ValueError(f"members: {members!r} (None, an int or {H} ints; 'each' is not for plan)")
        if noise is not None and noise.parity:
            raise ValueError('plan with a recorded tape: a tape fixes the draws of one rollout, not of a planner')
        # the particles as imagine's, and how their scores and certificates aggregate
        parts = ops._particles_request(self.model_ensemble, particles, members, noise)
        cvar = isinstance(risk, (tuple, list)) and len(risk) == 2 and risk[0] == 'cvar' and is_num(risk[1]) and \
            0 < risk[1] <= 1
        if not (cvar or isinstance(risk, str) and risk in ('mean', 'worst')):
            raise ValueError(f"risk: {risk!r} ('mean', 'worst' or ('cvar', alpha) with 0 < alpha <= 1)")
        if not (isinstance(cert_risk, str) and cert_risk in ('max', 'mean')):
            raise ValueError(f"cert_risk: {cert_risk!r} ('max' or 'mean')")
        if parts is None and (risk != 'mean' or cert_risk != 'max'):
            raise ValueError('risk / cert_risk without particles: they say how the particles aggregate')
        score_tail = None
        if parts is not None:
            G = len(parts)
            score_tail = G if risk == 'mean' else 1 if risk == 'worst' else max(1, int(np.ceil(float(risk[1]) * G)))
        # the filter as imagine's ``shield`` (None: off), every spelling checked here
        filt = None if safety_filter is None or safety_filter is False else safety_filter
        if isinstance(filt, (str, tuple, list)):
            kind, thr, cands = (filt, None, None) if isinstance(filt, str) else (tuple(filt) + (None,) * 3)[:3]
            if kind != 'linear' or (not isinstance(filt, str) and not 1 <= len(filt) <= 3) or \
                    not (thr is None or is_num(thr) and thr == thr) or \
                    not (cands is None or is_int(cands) and 2 <= cands <= 32):
                raise ValueError(f"safety_filter: {safety_filter!r} (None, True, a threshold, 'linear', ('linear', "
                                 "threshold) or ('linear', threshold, candidates 2..32))")
            filt = ('linear', float(self.safe_shield_threshold if thr is None else thr)) + \
                (() if cands is None else (int(cands),))
        elif filt is True:
            filt = float(self.safe_shield_threshold)
        elif filt is not None:
            if not (is_num(filt) and filt == filt):
                raise ValueError(f'safety_filter: {safety_filter!r} (None, True, a threshold (-inf and inf are '
                                 "allowed, NaN is not) or 'linear')")
            filt = float(filt)
        if not (is_num(noise_beta) and 0 <= noise_beta < 1):
            raise ValueError(f'noise_beta: {noise_beta!r} (a number in [0, 1))')
        if not (is_int(shift) and 0 <= shift <= K):
            raise ValueError(f'shift: {shift!r} (an int, 0..steps {K})')
        if not (warm_std is None or is_num(warm_std) and warm_std >= 0):
            raise ValueError(f'warm_std: {warm_std!r} (None or a number >= 0)')
        if not (is_int(refine) and refine >= 0):
            raise ValueError(f'refine: {refine!r} (an int >= 0: the rounds of gradient refinement)')
        if not (is_int(refine_trials) and 1 <= refine_trials < ops.PLAN_MAX_CANDIDATES):
            raise ValueError(f'refine_trials: {refine_trials!r} (an int, 1..{ops.PLAN_MAX_CANDIDATES - 1})')
        if not (is_num(refine_step) and 0 < refine_step < float('inf')):
            raise ValueError(f'refine_step: {refine_step!r} (finite, > 0)')
        if refine:
            # the gradient is that of one deterministic run under K = H given actions (value_gradient)
            for name, v, bad in (('steps', K, K != H), ('particles', particles, parts is not None),
                                 ('members', members, members is None),
                                 ('model_noise', model_noise, bool(model_noise)),
                                 ('safety_filter', safety_filter, filt is not None)):
                if bad:
                    raise ValueError(f'refine with {name}={v!r}: gradient refinement needs every step planned (steps '
                                     '== horizon) under a fixed deterministic model (members an int or H ints, '
                                     'model_noise=False) without particles= or safety_filter=')
        A = self.action_dim
        if controller:
            # mpc: no states, no P and no warm start yet (act() makes them)
            if tail is not None and not ((torch.is_tensor(tail) or isinstance(tail, np.ndarray)) and tail.ndim == 2
                                         and tail.shape[-1] == A):
                raise ValueError(f'tail: {tail!r} (None or a [P, {A}] tensor)')
            return None
        if states is None:
            raise ValueError('plan needs start states')
        states = torch.as_tensor(states, dtype=torch.float32).reshape(-1, self.state_dim)
        P = len(states)
        if isinstance(init, str) and init != 'policy' or not (init is None or isinstance(init, str) or
                                                                torch.is_tensor(init) or isinstance(init, np.ndarray)):
            raise ValueError(f"init: {init!r} (None, 'policy' or a [P, K, A] tensor)")
        if init is not None and not isinstance(init, str):
            init = torch.as_tensor(init, dtype=torch.float32)
            if tuple(init.shape) != (P, K, A):
                raise ValueError(f'init: shape {tuple(init.shape)} is not [{P}, {K}, {A}]')

        def is_array(x):
            return torch.is_tensor(x) or isinstance(x, np.ndarray)
        if warm_start is None:
            for name, v in (('reset', reset), ('tail', tail), ('warm_std', warm_std)):
                if v is not None:
                    raise ValueError(f'{name} without warm_start: it says how a warm start is made')
        else:
            if init is not None:
                raise ValueError('warm_start together with init: a call starts from one of them')
            for k in ('mean', 'std', 'actions'):
                v = getattr(warm_start, k, None)
                if not (is_array(v) and tuple(v.shape) == (P, K, A)):
                    raise ValueError(f'warm_start: its {k} is {"missing" if v is None else "not"} a [{P}, {K}, {A}] '
                                     'tensor (a PlanResult over the same states and steps)')
            if reset is not None and not (is_array(reset) and tuple(reset.shape) == (P,) and
                                          reset.dtype in (torch.bool, np.dtype(bool))):
                raise ValueError(f'reset: {reset!r} (None or a [{P}] bool tensor)')
            if tail is not None and not (is_array(tail) and tuple(tail.shape) == (P, A)):
                raise ValueError(f'tail: {tail!r} (None or a [{P}, {A}] tensor)')
        return dict(H=H, N=N, K=K, P=P, A=A, states=states, init=init, elites=elites, threshold=threshold, look=look,
                    filt=filt, parts=parts, score_tail=score_tail, cert_mode=0 if cert_risk == 'max' else 1,
                    refine=refine, refine_trials=refine_trials, refine_step=refine_step)

    def mpc(self, *, fallback='safe', shift=1, warm_std=None, **plan_kwargs):
        """A receding-horizon controller on plan (an ops.PlanController): ``act(states)`` plans
        once per control step and warm-starts each plan from the last one, moved ``shift`` steps.

        fallback     'safe': a state whose best row is not feasible takes the safe actor's mean
                     action, the fallback of the shielded policy; None: the planner's action
                     whatever its certificate.
        shift, warm_std   as plan's, of every warm start.
        plan_kwargs  plan's own (horizon, candidates, iterations, noise_beta, safety_filter,
                     noise, particles, risk, cert_risk, ...), checked here once by plan's checks; not states, init,
                     warm_start or reset, which act() supplies. A ``tail`` [P, A] also starts
                     the cold plans.
        sampling.sample_episodes_batched(controller=) and evaluate(controller=) run one on the
        real environment. Not built: the planner inside step_generator, halt= inside the
        planner, data-parallel sharding of the states."""
        import inspect
        from . import ops
        for k in ('states', 'init', 'warm_start', 'reset'):
            if k in plan_kwargs:
                raise ValueError(f'mpc: {k} is not a controller setting (act() supplies it)')
        if fallback is not None and fallback != 'safe':
            raise ValueError(f"fallback: {fallback!r} ('safe' or None)")
        bound = inspect.signature(self.plan).bind(None, shift=shift, warm_std=warm_std, **plan_kwargs)
        bound.apply_defaults()
        self._plan_checks(**bound.arguments, controller=True)
        return ops.PlanController(self, fallback, shift, warm_std, plan_kwargs)

    def update_models(self, model_steps, noise=None):
        """src/smbpo.py:214-227."""
        log.message(f'Fitting models @ t = {self.steps_sampled.item()}')
        losses = self.model_ensemble.fit(self.replay_buffer, steps=model_steps,
                                         noise=self.noise if noise is None else noise)
        if len(losses):
            log.message('Loss statistics:')
            log.message(f'\tFirst {LOSS_AVERAGE_WINDOW}: {np.mean(losses[:LOSS_AVERAGE_WINDOW])}')
            log.message(f'\tLast {LOSS_AVERAGE_WINDOW}: {np.mean(losses[-LOSS_AVERAGE_WINDOW:])}')
            log.message(f'\tDeciles: {deciles(losses)}')
        rewards = self.replay_buffer.get('rewards')
        bounds = torch.stack([rewards.min(), rewards.max()]).float()
        GradReducer().broadcast_(bounds)     # data parallel: rank 0's bounds on every replica
        r_min, r_max = bounds.tolist()
        self.solver.update_r_bounds(r_min + self.alive_bonus, r_max + self.alive_bonus)
        return losses

    def update_solver(self, update_actor=True, update_multiplier=False, noise=None):
        """src/smbpo.py:251-279: mixed real/virtual minibatch + critic/actor/multiplier updates."""
        eng = self.solver.engine
        noise = self.noise if noise is None else noise
        lq, lqc = eng.update_solver(self, update_actor, update_multiplier, noise)
        self.recent_critic_losses.append(lq)
        self.recent_cons_critic_losses.append(lqc)

    def rollout_and_update(self, noise=None):
        self.rollout(self.actor, noise=noise)
        for step in range(self.solver_updates_per_step):
            self.update_solver(update_actor=step % self.sac_cfg.actor_update_interval == 0,
                               update_multiplier=step % self.sac_cfg.multiplier_update_interval == 0,
                               noise=noise)

    # ------------------------------------------------------------------ driver surface
    def setup(self):
        """src/smbpo.py:293-319: collect buffer_min uniform-policy steps, then the
        initial model fit."""
        if self.save_trajectories:
            raise NotImplementedError('save_trajectories (h5py episode files) is outside the hot path')
        if self.episodes_sampled.item() > 0:
            raise NotImplementedError('reloading collected episodes needs the h5py episode files '
                                      '(src/smbpo.py:298-303, save_trajectories), which are outside the hot path')
        assert len(self.replay_buffer) == self.steps_sampled
        self.stepper = self.step_generator()
        if len(self.replay_buffer) < self.buffer_min:
            log.message('Collecting initial data')
            while len(self.replay_buffer) < self.buffer_min:
                next(self.stepper)
            log.message('Initial model training')
            self.update_models(self.model_initial_steps)
        log.message('Collecting initial virtual data')
        log.message('Setup done!')

    def epoch(self):
        """src/smbpo.py:321-325."""
        if self.stepper is None:
            self.stepper = self.step_generator()
        for _ in range(self.steps_per_epoch):
            next(self.stepper)
        self.log_statistics()
        self.epochs_completed += 1

    def evaluate(self, controller=None):
        """src/smbpo.py:421-440: N_EVAL_TRAJ shielded evaluation episodes. ``controller`` (an
        ops.PlanController of self.mpc): the episodes' actions are the controller's instead of
        the shielded policy's; the same keys come back."""
        from .sampling import sample_episodes_batched
        ctl = {} if controller is None else {'controller': controller}
        trajs = sample_episodes_batched(self.eval_env, self.solver, N_EVAL_TRAJ, eval=True,
                                        safe_shield_threshold=self.eval_shield_threshold,
                                        shield_type=self.eval_shield_type, **ctl)
        lengths = [len(t) for t in trajs]
        returns = [t.get('rewards').sum().item() for t in trajs]
        violations = [t.get('violations').sum().item() for t in trajs]
        return {
            'eval return mean': float(np.mean(returns)),
            'eval return std': float(np.std(returns)),
            'eval length mean': float(np.mean(lengths)),
            'eval length std': float(np.std(lengths)),
            'eval violation mean': float(np.mean(violations)),
        }

    # ------------------------------------------------------------------ diagnostics
    def evaluate_models(self):
        """src/smbpo.py:327-336: per-member normalised one-step error deciles over the
        real buffer (one all-member forward, member stride 0 for the shared rows)."""
        states, actions, next_states = self.replay_buffer.get('states', 'actions', 'next_states')
        state_std = states.std(dim=0)
        state_std[state_std < 1e-7] = 1.0
        with torch.no_grad():
            predicted = self.model_ensemble.means(states, actions)[0]
        for i in range(self.model_cfg.ensemble_size):
            errors = torch.norm((predicted[i] - next_states) / (state_std + 1e-7), dim=1)
            log.message(f'Model {i + 1} error deciles: {deciles(errors)}')

    def model_rollout_error(self, horizon, *, max_segments=None, members=None, model_noise=False, noise=None,
                            uncertainty=False):
        """The k-step open-loop model error on the real buffer (k = ``horizon``): the model
        rolled forward from the first state of a real episode segment under the actions
        the episode actually took, against the states it actually reached. One ``imagine``
        call (given actions at every step, so the policy never runs) over at most
        ``max_segments`` (default rollout_batch_size) of the buffer's k-step segments,
        evenly spaced over their chronological list (no RNG). Returns an
        ops.ModelRolloutError. Changes nothing of the training state and logs nothing.
        uncertainty=True adds the elites' ``disagreement`` and ``epistemic`` along the imagined
        segments in the units of ``state_error``: does disagreement predict the real error?"""
        from . import ops
        from .sampling import episode_segments
        k = int(horizon)
        s, a, s2, r, dn = self.replay_buffer.get('states', 'actions', 'next_states', 'rewards', 'dones',
                                                 device=self.device)
        starts = episode_segments(s, s2, dn, k)
        if len(starts) == 0:
            raise ValueError(f'the replay buffer ({len(s)} rows) holds no episode segment of {k} steps')
        cap = self.rollout_batch_size if max_segments is None else int(max_segments)
        if cap < 1:
            raise ValueError(f'max_segments {cap} must be >= 1')
        if len(starts) > cap:
            pick = (torch.arange(cap, device=starts.device) * len(starts)) // cap
            starts = starts[pick]
        rows = starts.unsqueeze(1) + torch.arange(k, device=starts.device)       # [n, k]
        im = self.imagine(states=s[starts], actions=a[rows].reshape(len(starts), k, self.action_dim), horizon=k,
                          model_noise=model_noise, members=members, noise=noise)
        state_std = s.std(dim=0)                   # as evaluate_models forms it
        state_std[state_std < 1e-7] = 1.0
        alive = im.mask
        nan = torch.full((), float('nan'), device=self.device)
        se = torch.norm((im.states[..., 1:, :] - s2[rows]) / (state_std + 1e-7), dim=-1)
        re = (im.rewards - r[rows].reshape(len(starts), k)).abs()
        out = ops.ModelRolloutError(starts, im, torch.where(alive, se, nan), torch.where(alive, re, nan), alive)
        if uncertainty:
            self._imagined_uncertainty(im, None, scale=1.0 / (state_std + 1e-7))
            out.disagreement = torch.where(alive, im.disagreement, nan)
            out.epistemic = torch.where(alive, im.epistemic, nan)
        return out

    def _consume_chunk_draws(self, n, noise):
        """The reference's constraint_critic(sample=True) draws one randn_like per
        batch_map chunk of 1000 rows (src/smbpo.py:376-378, src/ssac.py:80); a recorded
        tape keeps those draws in order (they do not affect the std it reports)."""
        C = self.con_dim
        for s0 in range(0, n, BATCH_MAP_ROWS):
            m = min(BATCH_MAP_ROWS, n - s0)
            noise.randn_like((m, C) if C > 1 else (m,), used=False)

    def log_statistics(self):
        """src/smbpo.py:338-419."""
        from .sampling import stat_forwards
        self.evaluate_models()
        avg = pythonic_mean(self.recent_critic_losses) if self.recent_critic_losses else None
        log.message(f'Average recent critic loss: {avg}')
        self.data.append('critic loss', avg)
        self.recent_critic_losses.clear()
        avg = pythonic_mean(self.recent_cons_critic_losses) if self.recent_cons_critic_losses else None
        log.message(f'Average recent constraint critic loss: {avg}')
        self.data.append('constraint critic loss', avg)
        self.recent_cons_critic_losses.clear()
        log.message('Buffer sizes:')
        log.message(f'\tReal: {len(self.replay_buffer)}')
        log.message(f'\tVirtual: {len(self.virt_buffer)}')

        noise = self.noise
        real_s, real_a, real_v = self.replay_buffer.get('states', 'actions', 'violations')
        virt_s, virt_v = self.virt_buffer.get('states', 'violations')
        virt_a = self.actor.act(virt_s, eval=True).detach()
        groups = {
            'real (violation)': (real_s[real_v], real_a[real_v]),
            'real (~violation)': (real_s[~real_v], real_a[~real_v]),
            'virtual (violation)': (virt_s[virt_v], virt_a[virt_v]),
            'virtual (~violation)': (virt_s[~virt_v], virt_a[~virt_v]),
        }
        cfg = self.sac_cfg
        for which, (states, actions) in groups.items():
            mean_q = mean_qc = mean_qc_std = mean_lam = None
            if len(states) > 0:
                if cfg.distributional_qc and noise.parity:
                    self._consume_chunk_draws(len(states), noise)
                st = stat_forwards(self.solver, states, actions, cfg.distributional_qc, cfg.mlp_multiplier)
                mean_q, mean_qc = st['q'].mean(), st['qc'].mean()
                if cfg.distributional_qc:
                    mean_qc_std = st['qc_std'].mean()
                if 'lam' in st:
                    mean_lam = st['lam'].mean()
            log.message(f'Average Q {which}: {mean_q}')
            self.data.append(f'Average Q {which}', mean_q)
            log.message(f'Average Qc {which}: {mean_qc}')
            self.data.append(f'Average Qc {which}', mean_qc)
            if cfg.distributional_qc:
                log.message(f'Average Qc std {which}: {mean_qc_std}')
                self.data.append(f'Average Qc std {which}', mean_qc_std)
            if cfg.mlp_multiplier:
                log.message(f'Average Lambda {which}: {mean_lam}')
                self.data.append(f'Average Lambda {which}', mean_lam)
        if not cfg.mlp_multiplier:
            mean_lam = self.solver.lam.item()
            log.message(f'Average Lambda: {mean_lam}')
            self.data.append('Average Lambda', mean_lam)
        if torch.cuda.is_available():
            t = torch.cuda.get_device_properties(0).total_memory
            r, a = torch.cuda.memory_reserved(0), torch.cuda.memory_allocated(0)
            log.message(f'GPU memory info: total {t}, reserved {r}, allocated {a}, '
                        f'reserved but unallocated {r - a}')

    def mean_recent_losses(self):
        return pythonic_mean(self.recent_critic_losses), pythonic_mean(self.recent_cons_critic_losses)
