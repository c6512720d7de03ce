"""Constraint programs (drpo_amd.envs.ConstraintProgram) and their inputs shared by
the CPU and GPU program tests: the three built-in environments that a program can
express, restated as programs, and a custom S = 9, C = 3 program with no built-in
equivalent."""
import math

import numpy as np

from drpo_amd.envs import ConstraintProgram

f32 = np.float32
N = 513   # rows per input set: two full 256-thread workgroups and one thread of a third


def point_robot_program(hazards=((0.4, -1.2), (-0.4, 1.2))):
    """src/env/point_robot.py:96-131."""
    return (ConstraintProgram().balls((0, 1), hazards, 0.8)
            .done_box((0, 1), -3.0, 3.0).done_ball((0, 1), (2.2, 2.2), 0.3))


def quadrotor_program():
    """src/env/quadrotor/quadrotor.py:83-158: BoundedConstraint z in [0.5, 1.5]; done out
    of the x / z thresholds 2 / 3, past the float32 pitch bound, or on violation."""
    th = f32(85 * math.pi / 180)
    return (ConstraintProgram().from_linear_constraint([[-1.0], [1.0]], [-0.5, 1.5], [2])
            .done_box((0, 2, 4), [-2.0, -3.0, -th], [2.0, 3.0, th], dtype=np.float32).done_on_violation())


def cartpole_program():
    """src/env/poles/inverted_pendulum.py:11-26,79-121, hand-written rows."""
    return (ConstraintProgram().affine([0], [-1.0], -0.9).affine([1], [-1.0], -0.2)
            .affine([0], [1.0], -0.9).affine([1], [1.0], -0.2).done_on_violation())


def custom_program():
    """S = 9, C = 3: three hazard discs, two half-spaces; done out of a box or in a goal disc."""
    return (ConstraintProgram()
            .balls((1, 4), [(0.5, -1.0), (-1.5, 0.7), (2.0, 2.0)], 0.6)
            .affine([0, 3, 6, 7, 8], [2.0, 0.7, -1.3, -0.5, 0.25], -4.0)
            .affine([5], [-1.0], -1.25)
            .done_box((0, 2, 8), [-3.0, -2.5, -4.0], [3.0, 2.5, 4.0])
            .done_ball((1, 4), (-2.2, 1.1), 0.4))


def point_robot_states():
    return np.random.RandomState(0).randn(N, 11).astype(f32) * 2


def quadrotor_states():
    s = np.random.RandomState(0).randn(N, 12).astype(f32)
    s[:, 2] = 1 + 0.5 * s[:, 2]
    return s


def cartpole_states():
    return np.random.RandomState(0).randn(N, 4).astype(f32) * np.array([0.6, 0.15, 1, 1], f32)


def custom_states():
    return np.random.RandomState(1).randn(N, 9).astype(f32) * 1.5


def custom_reference(s):
    """The custom program's functions written independently of ConstraintProgram
    (vectorised numpy on float64 copies): (done, violation, h [n, 3], oob, goal)."""
    x = s.astype(np.float64)
    p = x[:, [1, 4]]
    centres = np.array([[0.5, -1.0], [-1.5, 0.7], [2.0, 2.0]])
    dist = np.sqrt(((p[:, None, :] - centres[None]) ** 2).sum(-1))
    h0 = 0.6 - dist.min(1)
    h1 = x[:, [0, 3, 6, 7, 8]] @ np.array([2.0, 0.7, -1.3, -0.5, 0.25]) - 4.0
    h2 = -x[:, 5] - 1.25
    h = np.stack([h0, h1, h2], 1)
    oob = (np.abs(x[:, 0]) > 3.0) | (np.abs(x[:, 2]) > 2.5) | (np.abs(x[:, 8]) > 4.0)
    goal = np.hypot(x[:, 1] + 2.2, x[:, 4] - 1.1) <= 0.4
    return oob | goal, (h > 0).any(1), h, oob, goal


CASES = {'point-robot': (point_robot_program, point_robot_states), 'quadrotor': (quadrotor_program, quadrotor_states),
         'cartpole': (cartpole_program, cartpole_states), 'custom': (custom_program, custom_states)}
