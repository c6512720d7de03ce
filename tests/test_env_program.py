"""Constraint programs on the host (no GPU): ConstraintProgram.evaluate_numpy against
the oracle's built-in constraint functions and an independent formula, the builder's
limits, the packed drpo_env_program_t and its C-side check, registration through
device_env_params, and verify_constraint_program.

The 513-row input sets have no row with margin < 1e-5 (asserted below), so flags are
compared on every row. h is compared as float32 to atol 1e-6: the values are O(1-10)
and the program's double arithmetic differs from the oracle's only in the order of
a few double operations, far below a float32 ulp (<= 9.5e-7 at |h| < 16)."""
import ctypes

import numpy as np
import pytest

import env_programs as EP
from drpo_amd import _abi, _lib
from drpo_amd import envs
from drpo_amd.envs import ConstraintProgram
from oracle import drpo_oracle as O


def _no_thin_margin(prog, s):
    margin = prog.evaluate_numpy(s, return_margin=True)[3]
    assert margin.shape == (len(s),) and margin.min() >= 1e-5


@pytest.mark.parametrize('name,oracle,n_done,n_viol', [('point-robot', O.constraints_point_robot, 129, 63),
                                                      ('quadrotor', O.constraints_quadrotor, 209, 148),
                                                      ('cartpole', O.constraints_cartpole, 150, 150)])
def test_builtin_programs_match_oracle(name, oracle, n_done, n_viol):
    make, states = EP.CASES[name]
    prog, s = make(), states()
    assert s.shape[0] == 513 and s.dtype == np.float32
    _no_thin_margin(prog, s)
    done, viol, h = prog.evaluate_numpy(s)
    rd, rv, rh = oracle(s)
    assert h.dtype == np.float32 and h.shape == (513, prog.C) == np.asarray(rh).shape
    np.testing.assert_array_equal(done, rd)
    np.testing.assert_array_equal(viol, rv)
    np.testing.assert_allclose(h, np.asarray(rh).astype(np.float32), rtol=0, atol=1e-6)
    assert int(done.sum()) == n_done and int(viol.sum()) == n_viol
    if name == 'quadrotor':
        assert int((done & ~viol).sum()) == 61
    if name == 'cartpole':
        assert ((h > 0).sum(0) > 0).all()     # every one of the 4 rows is active somewhere


def test_custom_program_matches_independent_formula():
    prog, s = EP.custom_program(), EP.custom_states()
    assert prog.C == 3 and prog.min_state_dim == 9
    _no_thin_margin(prog, s)
    rd, rv, rh, oob, goal = EP.custom_reference(s)
    assert int(rv.sum()) == 199 and [int(x) for x in (rh > 0).sum(0)] == [42, 80, 101]
    assert (int(oob.sum()), int(goal.sum()), int(rd.sum())) == (77, 9, 84)
    done, viol, h = prog.evaluate_numpy(s)
    np.testing.assert_array_equal(done, rd)
    np.testing.assert_array_equal(viol, rv)
    np.testing.assert_allclose(h, rh.astype(np.float32), rtol=0, atol=1e-6)


def test_float32_constants_reproduce_float32_comparisons():
    """A float32 state compared in double with a float32-rounded bound gives the float32 result."""
    th = np.float32(0.1)                       # 0.1f > 0.1
    s = np.array([[th], [np.nextafter(th, np.float32(1))]], np.float32)
    as32 = ConstraintProgram().affine([0], [1.0], 0.0).done_box([0], -th, th, dtype=np.float32)
    as64 = ConstraintProgram().affine([0], [1.0], 0.0).done_box([0], -0.1, 0.1)
    np.testing.assert_array_equal(as32.evaluate_numpy(s)[0], s[:, 0] > th)
    np.testing.assert_array_equal(as32.evaluate_numpy(s)[0], [False, True])
    np.testing.assert_array_equal(as64.evaluate_numpy(s)[0], [True, True])


def test_builder_limits():
    P = ConstraintProgram
    with pytest.raises(ValueError):
        P().affine(list(range(9)), [1.0] * 9, 0.0)
    with pytest.raises(ValueError):
        P().balls((0, 1), [(float(k), 0.0) for k in range(9)], 1.0)
    with pytest.raises(ValueError):
        P().balls((0, 1, 2, 3), [(0.0, 0.0, 0.0, 0.0)], 1.0)
    with pytest.raises(ValueError):
        P().done_ball((0, 1, 2, 3), (0.0, 0.0, 0.0, 0.0), 1.0)
    p = P()
    for _ in range(8):
        p.affine([0], [1.0], 0.0)
    with pytest.raises(ValueError):
        p.affine([0], [1.0], 0.0)                       # C = 9
    with pytest.raises(ValueError):
        P().affine([0], [1.0], 0.0).done_ball((0, 1), (0.0, 0.0), 1.0).done_ball((0, 1), (1.0, 1.0), 1.0)
    for empty in (P(), P().done_on_violation(), P().affine([0], [1.0], 0.0)):   # no rows / no done rule
        with pytest.raises(ValueError):
            empty.pack()
        with pytest.raises(ValueError):
            empty.evaluate_numpy(np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        P().from_linear_constraint(np.ones((1, 9)), [0.0], list(range(9)))
    with pytest.raises(ValueError):
        P().affine([-1], [1.0], 0.0)
    with pytest.raises(ValueError):
        P().affine([0, 1], [1.0], 0.0)
    with pytest.raises(ValueError):
        P().done_box(list(range(9)), -1.0, 1.0)


def test_from_linear_constraint_equals_hand_written_cartpole():
    """BoundedConstraint (src/env/poles/constraints.py:216-247): A = [-I; I], b = [-lb, ub]."""
    lb, ub = np.array([-0.9, -0.2]), np.array([0.9, 0.2])
    A = np.vstack((-np.eye(2), np.eye(2)))
    b = np.hstack((-lb, ub))
    prog = ConstraintProgram().from_linear_constraint(A, b, [0, 1]).done_on_violation()
    assert prog.C == 4
    assert prog.pack() == EP.cartpole_program().pack() and prog == EP.cartpole_program()


def test_pack_and_c_side_check():
    L = _lib.lib()
    prog = EP.custom_program()
    raw = prog.pack()
    assert len(raw) == L.drpo_abi_sizeof(b'drpo_env_program_t') == ctypes.sizeof(_abi.EnvProgram)
    assert L.drpo_abi_sizeof(b'drpo_env_program_row_t') == ctypes.sizeof(_abi.EnvProgramRow)
    host = _abi.EnvProgram.from_buffer_copy(raw)
    assert host.C == 3 and host.box_n == 3 and host.ball_nd == 2 and host.rows[0].n == 3
    assert L.drpo_env_program_check(ctypes.byref(host), 9) == 0
    assert L.drpo_env_program_check(ctypes.byref(host), 8) == 1          # DRPO_EINVAL: index 8 out of range
    assert b'state index 8' in L.drpo_last_error()
    prog.check(9)
    with pytest.raises(ValueError, match='state index 8'):
        prog.check(8)
    # the C side re-checks kinds and counts (a program not made by the builder)
    for field, value in (('C', 9), ('C', 0), ('box_n', 9), ('ball_nd', 4)):
        bad = _abi.EnvProgram.from_buffer_copy(raw)
        setattr(bad, field, value)
        assert L.drpo_env_program_check(ctypes.byref(bad), 9) == 1, field
    for field, value in (('kind', 2), ('n', 9), ('n', 0), ('nd', 4)):
        bad = _abi.EnvProgram.from_buffer_copy(raw)
        setattr(bad.rows[0], field, value)
        assert L.drpo_env_program_check(ctypes.byref(bad), 9) == 1, field


class _Space:
    def __init__(self, n):
        self.shape = (n,)


class MyThreeHazardRobot:            # a class name the build does not know
    drpo_constraint_program = staticmethod(lambda: EP.point_robot_program(
        hazards=((0.4, -1.2), (-0.4, 1.2), (1.5, 0.0))))

    def __init__(self):
        self.observation_space, self.action_space, self.con_dim = _Space(11), _Space(2), 1


class NoProgramEnv:
    def __init__(self):
        self.observation_space, self.action_space, self.con_dim = _Space(11), _Space(2), 1


class Wrapper:
    def __init__(self, env):
        self.env = env


def test_registration():
    p = envs.device_env_params(Wrapper(MyThreeHazardRobot()))
    assert p['env_id'] == 4 == envs.ENV_PROGRAM and p['con_dim'] == 1
    assert isinstance(p['program'], ConstraintProgram) and len(p['program'].rows[0][2]) == 3
    assert set(p) == {'env_id', 'con_dim', 'tracking_surr_start', 'tracking_n_surr', 'thr0', 'thr1', 'program'}
    assert envs.device_env_params(NoProgramEnv()) is None
    with pytest.raises(NotImplementedError):
        envs.device_env_params(NoProgramEnv(), required=True)

    # a program given as an instance; the built-ins' class names keep precedence
    class Direct(NoProgramEnv):
        drpo_constraint_program = EP.cartpole_program()

    assert envs.device_env_params(Direct())['con_dim'] == 4

    class PointRobot(NoProgramEnv):
        drpo_constraint_program = EP.cartpole_program()

    p = envs.device_env_params(PointRobot())
    assert p['env_id'] == 0 and 'program' not in p
    assert 'program' not in envs.device_env_params(envs.ShapeEnv('quadrotor'))


def test_verify_constraint_program():
    import pr_env
    s = EP.point_robot_states()

    class Robot(pr_env.PointRobot):
        drpo_constraint_program = EP.point_robot_program()

    assert envs.verify_constraint_program(Robot(), s) == 513
    assert envs.verify_constraint_program(pr_env.PointRobot(), s, program=EP.point_robot_program()) == 513

    class Moved(pr_env.PointRobot):
        drpo_constraint_program = EP.point_robot_program(hazards=((0.4, -1.2), (-0.4, 1.3)))

    with pytest.raises(ValueError, match=r'get_constraint_values: row \d+'):
        envs.verify_constraint_program(Moved(), s)

    class WrongDone(pr_env.PointRobot):
        drpo_constraint_program = (ConstraintProgram().balls((0, 1), pr_env.HAZARDS, 0.8)
                                   .done_box((0, 1), -3.0, 3.0))      # the goal disc is missing

    with pytest.raises(ValueError, match=r'check_done: row \d+'):
        envs.verify_constraint_program(WrongDone(), s)
    with pytest.raises(ValueError, match='advertises no constraint program'):
        envs.verify_constraint_program(pr_env.PointRobot(), s)
