"""numpy helpers the fp64 test oracles of the rows tools share (body_motion_oracle, fit_pose_oracle, contact_estimate_oracle, contact_force_oracle,
inverse_dynamics_oracle, push_oracle): test infrastructure.  Each replaced copies that were shown equal bit for bit on 1000 seeded inputs
(profiles/rows_call/helpers_equal.py); the copies that differ stayed where they were, with the difference named there."""
import numpy as np

from oracle.kpo import OracleSim


def f32(a):
    """the fp32 rounding of a, as fp64: device and reference then start from the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


def qmul(a, b):
    """Hamilton product of quaternions (w, x, y, z)"""
    w0, x0, y0, z0 = a; w1, x1, y1, z1 = b
    return np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1, w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])


def quat_matrix(q):
    """rotation matrix of a quaternion (w, x, y, z), normalised first"""
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def make_frame(n):
    """mju_makeFrame of a UNIT normal (the rule of contact_frame in kp_step_args.hpp): rows n, t1, t2; t1 = the y axis (the z axis when |n_y| >= 0.5) made
    orthogonal to n and normalised, t2 = n x t1"""
    n = np.asarray(n, float)
    y = np.array([0.0, 1.0, 0.0]) if abs(n[1]) < 0.5 else np.array([0.0, 0.0, 1.0])
    y = y - n.dot(y) * n
    y = y / np.linalg.norm(y)
    return np.stack([n, y, np.cross(n, y)])


def oracle(kpm_path):
    """the oracle for kinematics only: no contact rows, no limit rows"""
    return OracleSim(kpm=kpm_path, contact=False, limits=False)
