"""fp64 reference of an impulse push (kp_sim_apply_impulse), built from OracleSim's own kinematics and solve.

Every body's velocity Jacobian comes from the oracle in the oracle's convention: 75 calls of set_state_raw(qpos, e_k); forward();
get("cvel") give column k.  cvel[b] = [angular; linear], the linear part being the velocity of the point of body b that sits at the
root's subtree_com (kp_oracle.c: the c-frame of mj_comVel), so the velocity of a point r of body b is lin + ang x (r - subtree_com).
The push is dv = M^-1 J_b(r)^T [p; l] with M^-1 the oracle's solveM (armature included).
"""
import numpy as np

from np_rigid import quat_matrix as _rot

NV, NB = 75, 24


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def body_jacobians(oracle, qpos):
    """(J [24, 6, 75] = cvel of every body per unit dof velocity, subtree_com [3], xpos [24, 3], xquat [24, 4]) at qpos.
    Leaves the oracle at (qpos, 0) with forward() run, so that fullM / solveM belong to qpos."""
    qpos = np.asarray(qpos, np.float64)
    J = np.zeros((NB, 6, NV))
    for k in range(NV):
        e = np.zeros(NV); e[k] = 1.0
        oracle.set_state_raw(qpos, e); oracle.forward()
        J[:, :, k] = oracle.get("cvel").reshape(NB, 6)
    oracle.set_state_raw(qpos, np.zeros(NV)); oracle.forward()
    return J, oracle.get("subtree_com"), oracle.get("xpos").reshape(NB, 3), oracle.get("xquat").reshape(NB, 4)


def point_jacobian(oracle, qpos, body, offset):
    """J_b(r) [6, 75]: rows 0..2 the velocity of the point r = xpos_b + R_b offset, rows 3..5 the body's angular velocity; and r"""
    J, com, xpos, xquat = body_jacobians(oracle, qpos)
    r = xpos[body] + _rot(xquat[body]) @ np.asarray(offset, float)
    Jw, Jl = J[body, :3], J[body, 3:]
    return np.vstack([Jl - _skew(r - com) @ Jw, Jw]), r


def generalised_impulse(oracle, qpos, body, offset, impulse):
    Jp, _ = point_jacobian(oracle, qpos, body, offset)
    return Jp.T @ np.asarray(impulse, float)


def delta_qvel(oracle, qpos, entity, offset, impulse):
    """dv [75] of the humanoid for a push of body `entity` (0..23); zeros for every other entity (an object push leaves the humanoid alone)."""
    if not 0 <= int(entity) < NB:
        return np.zeros(NV)
    return oracle.solveM(generalised_impulse(oracle, qpos, int(entity), offset, impulse))


def com_velocity(oracle, qpos, qvel, eps=1e-3):
    """centre-of-mass velocity: the directional derivative of subtree_com along qvel (central difference on the configuration manifold)"""
    def moved(s):
        q = np.asarray(qpos, np.float64).copy(); v = np.asarray(qvel, float) * s
        q[:3] += v[:3]
        w = v[3:6]; a = np.linalg.norm(w)                   # root angular velocity is in the root frame: q <- q (x) exp(w / 2)
        dq = np.array([1.0, 0, 0, 0]) if a < 1e-300 else np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * w / a])
        w0, x0, y0, z0 = q[3:7]; w1, x1, y1, z1 = dq
        q[3:7] = [w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1, w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1]
        q[7:] += v[6:]
        oracle.set_state_raw(q, np.zeros(NV)); oracle.forward()
        return oracle.get("subtree_com")
    # steps relative to the largest dof velocity (a pushed hand turns at hundreds of rad/s), two of them extrapolated to fourth order
    h = eps / max(float(np.abs(qvel).max()), 1e-300)
    d1, d2 = (moved(h) - moved(-h)) / (2 * h), (moved(h / 2) - moved(-h / 2)) / h
    return (4 * d2 - d1) / 3


def object_delta_qvel(oracle, slot, obj_qpos7, offset, impulse):
    """M_obj^-1 g of the free object in `slot` (the oracle must hold it and have run forward()): dofs = 3 world translations of the body origin,
    3 rotations about the body axes (kpo_obj_forward); the push point is given from the body origin, in the body frame."""
    M, _ = oracle.object_dyn(slot)
    R = _rot(obj_qpos7[3:7])
    p, l = np.asarray(impulse[:3], float), np.asarray(impulse[3:], float)
    tq = l + np.cross(R @ np.asarray(offset, float), p)
    g = np.concatenate([p, R.T @ tq])
    return np.linalg.solve(M, g)
