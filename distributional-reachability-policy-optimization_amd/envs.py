"""Device environment registry: maps the reference's env classes to the batched
constraint functions implemented on the device (csrc/env_constraints.hpp).

The reference calls env.check_done / check_violation / get_constraint_values on
host numpy arrays (src/smbpo.py:63-65); the build evaluates the same functions
inside the fused rollout kernel. Envs are recognised by class name (the
reference's classes need gym / mujoco / safe_control_gym, which the build does not
import) or by an explicit ``drpo_env_id`` attribute."""
import numpy as np

from . import _abi

# the device environment ids (DRPO_ENV_*; tests/test_path_queries.py pins them to drpo_abi_const)
ENV_IDS = {'PointRobot': 0, 'QuadrotorWrapperEnv': 1, 'SafeInvertedPendulumEnv': 2,
           'SimuVeh3dofcontiSurrCstr': 3}
ENV_NAMES = {'point-robot': 0, 'quadrotor': 1, 'cartpole': 2, 'cartpole-move': 2, 'cartpole-upright': 2,
             'tracking': 3}
CON_DIM = {0: 1, 1: 2, 2: 4, 3: 1}
QUAD_X_THRESHOLD, QUAD_Z_THRESHOLD = 2.0, 3.0   # safe_control_gym defaults (unpinned)
CART_X_THRESHOLD, CART_TH_THRESHOLD = 0.9, 0.2   # SafeInvertedPendulumEnv defaults (inverted_pendulum.py:11-16)


ENV_PROGRAM = _abi.ENV_PROGRAM   # DRPO_ENV_PROGRAM: constraint functions described by a ConstraintProgram
PROGRAM_ATTR = 'drpo_constraint_program'


def _unwrap(env):
    """The first env of the wrapper chain with built-in device constraint functions;
    else the first that advertises a constraint program; else None."""
    seen, e = 0, env
    while e is not None and seen < 8:
        if hasattr(e, 'drpo_env_id') or type(e).__name__ in ENV_IDS:
            return e
        e = getattr(e, 'env', None)
        seen += 1
    seen, e = 0, env
    while e is not None and seen < 8:
        if getattr(e, PROGRAM_ATTR, None) is not None:
            return e
        e = getattr(e, 'env', None)
        seen += 1
    return None


def _program_of(e):
    """The ConstraintProgram an env advertises (attribute drpo_constraint_program: a
    program or a zero-argument callable returning one), or None."""
    if hasattr(e, 'drpo_env_id') or type(e).__name__ in ENV_IDS:
        return None   # the built-in ids take precedence
    prog = getattr(e, PROGRAM_ATTR, None)
    if prog is not None and not isinstance(prog, ConstraintProgram):
        prog = prog()
    if prog is not None and not isinstance(prog, ConstraintProgram):
        raise TypeError(f'{type(e).__name__}.{PROGRAM_ATTR} must be a ConstraintProgram or a callable returning one')
    return prog


class ConstraintProgram:
    """Declarative constraint functions of a user-defined environment, evaluated on the
    device by the rollout kernels (drpo_env_program_t, env id 4) instead of the host
    round trip through env.check_done / check_violation / get_constraint_values
    (src/smbpo.py:63-65).

    C constraint rows (1..8), each ``affine`` or ``balls``; violation = any(h_c > 0);
    done = OR of ``done_box``, ``done_ball`` (at most one) and ``done_on_violation``.

    Arithmetic: states are float32 promoted to double, every constant is a double, all
    arithmetic and comparisons are in double, h is rounded to float32 on output and the
    violation test is made before that rounding. Each builder method rounds its
    constants to ``dtype`` (default float64) before storing them as doubles: a float32
    state compared in double with a float32-rounded bound gives the float32 result,
    which reproduces numpy code that compares a float32 state with a float32 bound.

        prog = (ConstraintProgram()
                .balls((0, 1), [(0.4, -1.2), (-0.4, 1.2), (1.5, 0.0)], 0.8)
                .done_box((0, 1), -3.0, 3.0).done_ball((0, 1), (2.2, 2.2), 0.3))
    """

    MAX_ROWS, MAX_TERMS, MAX_CENTRES, MAX_BOX = (_abi.PROG_MAX_ROWS, _abi.PROG_MAX_TERMS, _abi.PROG_MAX_CENTRES,
                                                 _abi.PROG_MAX_BOX)

    def __init__(self):
        self.rows = []             # ('affine', dims, coefs, bias) | ('balls', dims, centres [n][nd], radius)
        self.box = None            # (dims, lo, hi)
        self.ball = None           # (dims, centre, radius)
        self.on_violation = False
        self._dev = {}

    # ------------------------------------------------------------------ builder
    @staticmethod
    def _dims(dims, what):
        d = np.atleast_1d(np.asarray(dims))
        if d.ndim != 1 or d.size == 0 or not np.issubdtype(d.dtype, np.integer):
            raise ValueError(f'{what}: dims must be a non-empty list of integers, got {dims!r}')
        if d.min() < 0 or d.max() > 255:
            raise ValueError(f'{what}: state index out of range 0..255 in {dims!r}')
        return tuple(int(x) for x in d)

    @staticmethod
    def _consts(x, dtype):
        c = np.asarray(x, dtype=dtype).astype(np.float64)
        if np.any(np.isnan(c)):
            raise ValueError('constants must not be NaN')
        return c

    def _new_row(self, row):
        if len(self.rows) >= self.MAX_ROWS:
            raise ValueError(f'a constraint program has at most {self.MAX_ROWS} constraint rows')
        self.rows.append(row)
        self._dev.clear()
        return self

    def affine(self, dims, coefs, bias, dtype=np.float64):
        """h = sum_k coefs[k] * s[dims[k]] + bias (terms added left to right), 1..8 terms."""
        dims = self._dims(dims, 'affine')
        coefs = np.atleast_1d(self._consts(coefs, dtype))
        if coefs.shape != (len(dims),):
            raise ValueError(f'affine: {len(dims)} dims but coefs of shape {coefs.shape}')
        if len(dims) > self.MAX_TERMS:
            raise ValueError(f'affine: {len(dims)} terms (at most {self.MAX_TERMS})')
        return self._new_row(('affine', dims, coefs, float(self._consts(bias, dtype))))

    def from_linear_constraint(self, A, b, active_dims, dtype=np.float64):
        """One affine row per row of A: h = A x - b with x = s[active_dims], the
        reference's LinearConstraint / BoundedConstraint
        (src/env/poles/constraints.py:159-247). Zero coefficients are dropped; a row
        with more than 8 non-zeros (or none) is refused."""
        A = np.atleast_2d(np.asarray(A, dtype=np.float64))
        b = np.atleast_1d(np.asarray(b, dtype=np.float64))
        active = self._dims(active_dims, 'from_linear_constraint')
        if A.shape != (len(b), len(active)):
            raise ValueError(f'from_linear_constraint: A {A.shape} does not match b {b.shape} / '
                             f'{len(active)} active dims')
        if len(self.rows) + len(b) > self.MAX_ROWS:
            raise ValueError(f'a constraint program has at most {self.MAX_ROWS} constraint rows')
        for r in range(len(b)):
            nz = np.flatnonzero(A[r])
            if len(nz) == 0 or len(nz) > self.MAX_TERMS:
                raise ValueError(f'from_linear_constraint: row {r} has {len(nz)} non-zero coefficients '
                                 f'(1..{self.MAX_TERMS})')
            self.affine([active[k] for k in nz], A[r, nz], -b[r], dtype=dtype)
        return self

    def balls(self, dims, centres, radius, dtype=np.float64):
        """h = radius - min_k ||s[dims] - centre_k||_2: 2 or 3 dims, 1..8 centres."""
        dims = self._dims(dims, 'balls')
        if len(dims) not in (2, 3):
            raise ValueError(f'balls: {len(dims)} dims (2 or 3)')
        centres = np.atleast_2d(self._consts(centres, dtype))
        if centres.ndim != 2 or centres.shape[1] != len(dims) or centres.shape[0] == 0:
            raise ValueError(f'balls: centres of shape {centres.shape} for {len(dims)} dims')
        if centres.shape[0] > self.MAX_CENTRES:
            raise ValueError(f'balls: {centres.shape[0]} centres (at most {self.MAX_CENTRES})')
        return self._new_row(('balls', dims, centres, float(self._consts(radius, dtype))))

    def done_box(self, dims, lo, hi, dtype=np.float64):
        """done when s[d] < lo or s[d] > hi for any of up to 8 dims (lo / hi scalar or per dim)."""
        dims = self._dims(dims, 'done_box')
        if self.box is not None:
            raise ValueError('done_box: a program has at most one box (give it every dim)')
        if len(dims) > self.MAX_BOX:
            raise ValueError(f'done_box: {len(dims)} dims (at most {self.MAX_BOX})')
        lo = np.broadcast_to(self._consts(lo, dtype), (len(dims),)).copy()
        hi = np.broadcast_to(self._consts(hi, dtype), (len(dims),)).copy()
        self.box = (dims, lo, hi)
        self._dev.clear()
        return self

    def done_ball(self, dims, centre, radius, dtype=np.float64):
        """done when ||s[dims] - centre||_2 <= radius (2 or 3 dims; at most one)."""
        dims = self._dims(dims, 'done_ball')
        if self.ball is not None:
            raise ValueError('done_ball: a program has at most one done ball')
        if len(dims) not in (2, 3):
            raise ValueError(f'done_ball: {len(dims)} dims (2 or 3)')
        centre = np.atleast_1d(self._consts(centre, dtype))
        if centre.shape != (len(dims),):
            raise ValueError(f'done_ball: centre of shape {centre.shape} for {len(dims)} dims')
        self.ball = (dims, centre, float(self._consts(radius, dtype)))
        self._dev.clear()
        return self

    def done_on_violation(self):
        self.on_violation = True
        self._dev.clear()
        return self

    # ------------------------------------------------------------------ properties
    @property
    def C(self):
        return len(self.rows)

    @property
    def min_state_dim(self):
        """Smallest state dimension this program can run on (1 + its largest index)."""
        idx = [d for r in self.rows for d in r[1]]
        idx += list(self.box[0]) if self.box else []
        idx += list(self.ball[0]) if self.ball else []
        return 1 + max(idx)

    def _require_complete(self):
        if not self.rows:
            raise ValueError('an empty constraint program: add at least one affine / balls row')
        if self.box is None and self.ball is None and not self.on_violation:
            raise ValueError('a constraint program needs a done rule (done_box / done_ball / done_on_violation)')

    def __eq__(self, other):
        return isinstance(other, ConstraintProgram) and self.pack() == other.pack()

    __hash__ = object.__hash__

    # ------------------------------------------------------------------ CPU oracle
    @staticmethod
    def _dist(s, dims, centre):
        q = None
        for k, d in enumerate(dims):
            t = s[:, d] - centre[k]
            q = t * t if q is None else q + t * t
        return np.sqrt(q)

    def evaluate_numpy(self, states, return_margin=False):
        """(done [n] bool, violation [n] bool, h [n, C] float32[, margin [n] float64]):
        the program in plain numpy, the arithmetic of the device interpreter. ``margin``
        is per state row the smallest absolute distance of any compared quantity from
        its threshold (|h_c|, |s[d] - lo|, |s[d] - hi|, |dist - radius|): a row with a
        tiny margin is one whose flags a differently rounded restatement may flip."""
        self._require_complete()
        s32 = np.asarray(states)
        if s32.ndim != 2 or s32.shape[1] < self.min_state_dim:
            raise ValueError(f'states of shape {s32.shape}: need [n, S >= {self.min_state_dim}]')
        s = s32.astype(np.float32).astype(np.float64)
        n = len(s)
        h = np.empty((n, self.C), np.float64)
        for c, row in enumerate(self.rows):
            if row[0] == 'affine':
                _, dims, coefs, bias = row
                acc = coefs[0] * s[:, dims[0]]
                for k in range(1, len(dims)):
                    acc = acc + coefs[k] * s[:, dims[k]]
                h[:, c] = acc + bias
            else:
                _, dims, centres, radius = row
                md = np.full(n, np.inf)
                for centre in centres:
                    md = np.minimum(self._dist(s, dims, centre), md)
                h[:, c] = radius - md
        viol = np.any(h > 0.0, axis=1)
        margin = np.min(np.abs(h), axis=1)
        done = viol.copy() if self.on_violation else np.zeros(n, bool)
        if self.box is not None:
            dims, lo, hi = self.box
            for k, d in enumerate(dims):
                done |= (s[:, d] < lo[k]) | (s[:, d] > hi[k])
                margin = np.minimum(margin, np.minimum(np.abs(s[:, d] - lo[k]), np.abs(s[:, d] - hi[k])))
        if self.ball is not None:
            dims, centre, radius = self.ball
            dist = self._dist(s, dims, centre)
            done |= dist <= radius
            margin = np.minimum(margin, np.abs(dist - radius))
        out = (done, viol, h.astype(np.float32))
        return out + (margin,) if return_margin else out

    # ------------------------------------------------------------------ packing / upload
    def _struct(self):
        self._require_complete()
        p = _abi.EnvProgram()
        p.C = self.C
        p.done_on_violation = int(self.on_violation)
        for c, row in enumerate(self.rows):
            r = p.rows[c]
            if row[0] == 'affine':
                _, dims, coefs, bias = row
                r.kind, r.n, r.nd, r.k0 = _abi.PROG_AFFINE, len(dims), 0, bias
                vals = coefs
            else:
                _, dims, centres, radius = row
                r.kind, r.n, r.nd, r.k0 = _abi.PROG_BALLS, len(centres), len(dims), radius
                vals = centres.reshape(-1)
            for k, d in enumerate(dims):
                r.dims[k] = d
            for k, x in enumerate(vals):
                r.v[k] = float(x)
        if self.box is not None:
            dims, lo, hi = self.box
            p.box_n = len(dims)
            for k, d in enumerate(dims):
                p.box_dims[k], p.box_lo[k], p.box_hi[k] = d, float(lo[k]), float(hi[k])
        if self.ball is not None:
            dims, centre, radius = self.ball
            p.ball_nd, p.ball_radius = len(dims), radius
            for k, d in enumerate(dims):
                p.ball_dims[k], p.ball_centre[k] = d, float(centre[k])
        return p

    def pack(self):
        """The bytes of drpo_env_program_t."""
        import ctypes
        p = self._struct()
        return ctypes.string_at(ctypes.byref(p), ctypes.sizeof(p))

    def check(self, state_dim):
        """The C-side validation (drpo_env_program_check) against a state dimension: the
        only check there is, since the kernels trust the uploaded program's indices."""
        import ctypes
        from . import _lib
        L = _lib.lib()
        p = self._struct()
        if L.drpo_env_program_check(ctypes.byref(p), int(state_dim)) != 0:
            raise ValueError(L.drpo_last_error().decode())
        return self

    def device(self, dev, state_dim=None):
        """Cached uint8 device tensor of pack(), uploaded once per (device, program
        state). Runs check() against ``state_dim`` (default: the program's own largest
        index + 1; callers that know the env's state dimension pass it)."""
        import torch
        S = self.min_state_dim if state_dim is None else int(state_dim)
        key = (str(torch.device(dev)), S)
        t = self._dev.get(key)
        if t is None:
            self.check(S)
            raw = np.frombuffer(self.pack(), dtype=np.uint8).copy()
            t = self._dev[key] = torch.from_numpy(raw).to(dev)
        return t


def verify_constraint_program(env, states, program=None):
    """Compare a constraint program with the env's own numpy check_done /
    check_violation / get_constraint_values on ``states`` ([n, S], e.g. replay states):
    h must agree to atol = rtol = 1e-5, the flags must be equal on every row whose
    margin (ConstraintProgram.evaluate_numpy) is >= 1e-5. Raises ValueError naming the
    function and the first offending row. Run it once before training with a program."""
    e = _unwrap(env)
    prog = program if program is not None else (getattr(e, PROGRAM_ATTR, None) if e is not None else None)
    if prog is not None and not isinstance(prog, ConstraintProgram):
        prog = prog()
    if not isinstance(prog, ConstraintProgram):
        raise ValueError(f'{type(env).__name__} advertises no constraint program ({PROGRAM_ATTR})')
    s = np.asarray(states, dtype=np.float32)
    done, viol, h, margin = prog.evaluate_numpy(s, return_margin=True)
    n = len(s)
    h_env = np.asarray(env.get_constraint_values(s), dtype=np.float64).reshape(n, -1)
    if h_env.shape[1] != prog.C:
        raise ValueError(f'get_constraint_values: the env has {h_env.shape[1]} constraints, the program {prog.C}')
    bad = ~np.isclose(h.astype(np.float64), h_env, rtol=1e-5, atol=1e-5).all(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f'get_constraint_values: row {i} (state {s[i]}): program {h[i]} != env {h_env[i]}')
    sure = margin >= 1e-5
    for name, got in (('check_violation', viol), ('check_done', done)):
        want = np.asarray(getattr(env, name)(s)).reshape(n).astype(bool)
        bad = (got != want) & sure
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f'{name}: row {i} (state {s[i]}): program {bool(got[i])} != env {bool(want[i])} '
                             f'(margin {margin[i]:.3g})')
    return int(sure.sum())


def device_env_params(env, required=False):
    """dict(env_id, con_dim, tracking_surr_start, tracking_n_surr, thr0, thr1) for an env
    with device constraint functions, or None for an unknown env: the trainer then
    keeps the reference's host numpy round trip (src/smbpo.py:63-65) for it. An env
    that is not one of the four built-ins but advertises a ConstraintProgram
    (attribute ``drpo_constraint_program``) gets env_id 4, con_dim = the program's row
    count and the extra key ``program``.

    thr0/thr1: quadrotor x/z_threshold (safe_control_gym attributes, unpinned
    defaults 2/3); cartpole x_threshold / th_threshold
    (src/env/poles/inverted_pendulum.py:11-17, kwarg ``threshold``)."""
    if isinstance(env, str):
        eid, e = ENV_NAMES[env], None
    else:
        e = _unwrap(env)
        if e is None:
            if required:
                raise NotImplementedError(f'no device constraint functions for env {type(env).__name__}; '
                                          f'known: {sorted(ENV_IDS)}')
            return None
        prog = _program_of(e)
        if prog is not None:
            # a user-defined env: its constraint functions run as a program on the
            # production kernels (env id 4); the other keys as for point-robot
            prog._require_complete()
            return dict(env_id=ENV_PROGRAM, con_dim=prog.C, tracking_surr_start=47, tracking_n_surr=1, thr0=0.0,
                        thr1=0.0, program=prog)
        eid = getattr(e, 'drpo_env_id', None)
        eid = ENV_IDS[type(e).__name__] if eid is None else int(eid)
    p = dict(env_id=eid, con_dim=CON_DIM[eid], tracking_surr_start=47, tracking_n_surr=1, thr0=0.0, thr1=0.0)
    if eid == 1:
        p['thr0'], p['thr1'] = QUAD_X_THRESHOLD, QUAD_Z_THRESHOLD
    if eid == 2:
        p['thr0'], p['thr1'] = CART_X_THRESHOLD, CART_TH_THRESHOLD
    if e is not None and eid == 3:
        p['tracking_surr_start'] = int(getattr(e, 'surr_vehs_start_dim', 47))
        p['tracking_n_surr'] = int(getattr(e, 'surr_veh_num', 1))
    if e is not None and eid == 1:
        inner = getattr(e, 'env', e)
        p['thr0'] = float(getattr(inner, 'x_threshold', QUAD_X_THRESHOLD))
        p['thr1'] = float(getattr(inner, 'z_threshold', QUAD_Z_THRESHOLD))
    if e is not None and eid == 2:
        p['thr0'] = float(getattr(e, 'x_threshold', CART_X_THRESHOLD))
        p['thr1'] = float(getattr(e, 'th_threshold', CART_TH_THRESHOLD))
    return p


class Box:
    """Minimal continuous space (gym.spaces.Box surface used by the trainer: shape,
    low, high) for dims-only and test environments."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        if shape is None:
            shape = np.shape(low)
        self.shape = tuple(shape)
        self.dtype = dtype
        self.low = np.broadcast_to(np.asarray(low, dtype), self.shape).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype), self.shape).copy()


_Space = Box


class ShapeEnv:
    """Dims-only stand-in for a reference env class (synthetic benchmarks and tests):
    the device constraint functions are selected by env id, so no simulator is needed."""

    DIMS = {0: (11, 2, 300), 1: (12, 2, 360), 2: (4, 1, 1000), 3: (51, 2, 200)}

    def __init__(self, name, id=None):
        self.drpo_env_id = ENV_NAMES[name]
        S, A, T = self.DIMS[self.drpo_env_id]
        self.observation_space = Box(-np.inf, np.inf, (S,))
        self.action_space = Box(-1.0, 1.0, (A,))
        self.con_dim = CON_DIM[self.drpo_env_id]
        self._max_episode_steps = T
        if self.drpo_env_id == 3:
            self.surr_vehs_start_dim, self.surr_veh_num = 47, 1
        if self.drpo_env_id == 1:
            self.x_threshold, self.z_threshold = QUAD_X_THRESHOLD, QUAD_Z_THRESHOLD
        if self.drpo_env_id == 2:
            self.x_threshold, self.th_threshold = CART_X_THRESHOLD, CART_TH_THRESHOLD


def get_max_episode_steps(env):
    """src/env/util.py:27-33."""
    if hasattr(env, '_max_episode_steps'):
        return env._max_episode_steps
    if hasattr(env, 'env'):
        return get_max_episode_steps(env.env)
    raise ValueError('env does not have _max_episode_steps')


def env_dims(env):
    """src/env/util.py:23-24 (Box spaces: prod(shape))."""
    import math
    return (int(math.prod(env.observation_space.shape)), int(math.prod(env.action_space.shape)), env.con_dim)


class ProductEnv:
    """Batch of independent host environments (src/env/batch.py:87-109) for evaluation.

    States live on the device (the envs' TorchWrapper returns device tensors); the
    actions of one step are copied to the host ONCE and each env steps on its row
    (the reference copies per env)."""

    def __init__(self, envs, max_episode_steps=None):
        self.envs = list(envs)
        self.proto_env = self.envs[0]
        self.n_envs = len(self.envs)
        self._max_episode_steps = max_episode_steps if max_episode_steps is not None else \
            get_max_episode_steps(self.proto_env)

    @property
    def observation_space(self):
        return self.proto_env.observation_space

    @property
    def action_space(self):
        return self.proto_env.action_space

    @property
    def con_dim(self):
        return self.proto_env.con_dim

    def partial_reset(self, indices):
        import torch
        return torch.stack([self.envs[int(i)].reset() for i in indices])

    def reset(self):
        return self.partial_reset(range(self.n_envs))

    def step(self, actions):
        import torch
        acts = actions.detach().cpu() if torch.is_tensor(actions) else actions
        next_states, rewards, dones, infos = [], [], [], []
        for env, a in zip(self.envs, acts):
            s2, r, d, info = env.step(a)
            next_states.append(s2)
            rewards.append(r)
            dones.append(d)
            infos.append(info)
        dev = next_states[0].device
        return (torch.stack(next_states), torch.tensor(rewards, device=dev), torch.tensor(dones, device=dev),
                infos)

    def __repr__(self):
        return f'Batch<{self.n_envs}x{self.proto_env}>'
