"""fp64 reference of the body-motion read-out (kp_sim_body_motion): test infrastructure.

OracleSim is used for kinematics only (xpos, xquat, xipos of a pose) and, in the tests, for fullM.  Velocities and accelerations are finite differences
of that forward kinematics along the motion the row describes,
    q(t) = q (+) (t v + 1/2 t^2 a):   root position += t v_lin + 1/2 t^2 a_lin,  root quaternion = q (x) exp(t w + 1/2 t^2 alpha) (w, alpha in the
    root's own axes, as the free joint has them),  hinges += t v + 1/2 t^2 a,
which agrees with the true motion to O(t^3), the t^3 term being odd (it cancels in the symmetric second difference).  With x(t) a body point and
phi(t) = log(R(t) R(0)^T) the world rotation vector from the pose at 0:
    velocity      (x(e) - x(-e)) / 2e            angular velocity      (phi(e) - phi(-e)) / 2e
    acceleration  (x(e) - 2 x(0) + x(-e)) / e^2  angular acceleration  (phi(e) + phi(-e)) / e^2          (phi'' (0) = alpha + 1/2 w x w = alpha)
each O(e^2), and one Richardson step (4 D(e) - D(2e)) / 3 removes that term.  With s = max(1, |v|^2, |a|) (the rate at which the motion's time
derivatives grow: x^(n) ~ s^(n/2)) the second difference then carries a truncation error ~ s^3 e^4 and a rounding error ~ 1e-15 / e^2; they balance at
e = (1e-15 / s^3)^(1/6) = 3.2e-3 / sqrt(s), which auto_eps() returns: 6e-4 at 5 rad/s, 1.6e-4 at 20 rad/s, 3e-5 under the 1e4 rad/s^2 of a hard
contact, where both errors are ~1e-6 m/s^2 on accelerations of 1e3 m/s^2 (tests/test_body_motion_cpu.py shows the plateau).  Momentum and energy are plain sums over the
bodies with the blob's masses and inertias.  None of this shares anything with the spatial algebra of the kernel.
"""
import numpy as np

from np_rigid import f32, oracle, qmul  # noqa: F401  (the tests reach them through this module)

NB, NQ, NV = 24, 76, 75


def auto_eps(v, a):
    """the step at which truncation and rounding of the Richardson second difference balance (module docstring)"""
    s = max(1.0, float(np.abs(v).max()) ** 2, float(np.abs(a).max()))
    return 10.0 ** -2.5 / np.sqrt(s)


CENTROID = {"com": slice(0, 3), "com_vel": slice(3, 6), "L_com": slice(6, 9), "ke": 9, "pe": 10, "com_acc": slice(11, 14), "Ldot_com": slice(14, 17), "mass": 17}


def qexp(r):
    """unit quaternion of the rotation vector r"""
    th = np.linalg.norm(r)
    s = 0.5 if th < 1e-12 else np.sin(0.5 * th) / th
    return np.concatenate([[np.cos(0.5 * th)], s * np.asarray(r, float)])


def qmat(q):
    """not np_rigid.quat_matrix: 1 - 2 (y^2 + z^2) on the diagonal where that one has w^2 + x^2 - y^2 - z^2; equal to rounding, not bit
    for bit (profiles/rows_call/helpers_equal.log)"""
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rotvec(R):
    """log of a rotation matrix close to the identity (|angle| << pi)"""
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # sin(th) axis
    s = np.linalg.norm(w)
    return w if s < 1e-12 else (np.arcsin(min(s, 1.0)) / s) * w


def advance(q, v, a, t):
    """q (+) (t v + 1/2 t^2 a); the root quaternion is normalised first"""
    d = t * np.asarray(v, float) + 0.5 * t * t * np.asarray(a, float)
    out = np.array(q, float)
    out[3:7] /= np.linalg.norm(out[3:7])
    out[:3] += d[:3]
    out[3:7] = qmul(out[3:7], qexp(d[3:6]))
    out[7:] += d[6:]
    return out


def fk(o, q):
    """(xpos [24,3], R [24,3,3], xipos [24,3]) of the pose q on the oracle.  Not fit_pose_oracle.fk: that one returns (xpos, xquat) and normalises the
    root quaternion itself before a raw set_state + forward; this one resets the oracle with q as given"""
    o.reset(q, np.zeros(NV))
    xq = o.get("xquat").reshape(NB, 4)
    return o.get("xpos").reshape(NB, 3), np.stack([qmat(x) for x in xq]), o.get("xipos").reshape(NB, 3)


def _diffs(o, q, v, a, e, base):
    p0, R0, c0 = base
    pp, Rp, cp = fk(o, advance(q, v, a, e))
    pm, Rm, cm = fk(o, advance(q, v, a, -e))
    php = np.stack([rotvec(Rp[b] @ R0[b].T) for b in range(NB)]); phm = np.stack([rotvec(Rm[b] @ R0[b].T) for b in range(NB)])
    return dict(vel=(pp - pm) / (2 * e), acc=(pp - 2 * p0 + pm) / e ** 2, cvel=(cp - cm) / (2 * e), cacc=(cp - 2 * c0 + cm) / e ** 2,
                w=(php - phm) / (2 * e), alpha=(php + phm) / e ** 2)


def kinematics_fd(o, q, v, a, eps=None, richardson=True):
    """dict(xpos, R, xipos; vel, acc: of the body frame origins; cvel, cacc: of the bodies' centres of mass; w, alpha), each [24,3] (R [24,3,3]), world axes"""
    eps = auto_eps(v, a) if eps is None else eps
    base = fk(o, advance(q, v, a, 0.0))
    d1 = _diffs(o, q, v, a, eps, base)
    if richardson:
        d2 = _diffs(o, q, v, a, 2 * eps, base)
        d1 = {k: (4 * d1[k] - d2[k]) / 3 for k in d1}
    return dict(xpos=base[0], R=base[1], xipos=base[2], **d1)


def world_inertia(kpm, R):
    """[24,3,3] the bodies' inertia about their centres of mass, world axes (blob: xx yy zz xy xz yz in the body frame)"""
    I = np.asarray(kpm["body_inertia"], float).reshape(NB, 6)
    Ib = np.stack([np.array([[i[0], i[3], i[4]], [i[3], i[1], i[5]], [i[4], i[5], i[2]]]) for i in I])
    return np.einsum("bij,bjk,blk->bil", R, Ib, R)


def reference(o, kpm, q, v=None, a=None, eps=None, richardson=True):
    """The read-out of one row in fp64: dict(body_vel [24,6], body_acc [24,6], body_com_vel [24,3], centroid [18]) plus xpos, xquat-free extras
    (L_root: angular momentum about the root position; I_total: inertia of the whole figure about its centre of mass)."""
    v = np.zeros(NV) if v is None else np.asarray(v, float)
    a = np.zeros(NV) if a is None else np.asarray(a, float)
    k = kinematics_fd(o, q, v, a, eps, richardson)
    m = np.asarray(kpm["body_mass"], float)
    g = np.asarray(kpm["opt"][1:4], float)
    Iw = world_inertia(kpm, k["R"])
    M = m.sum()
    com = (m[:, None] * k["xipos"]).sum(0) / M
    p = (m[:, None] * k["cvel"]).sum(0)
    r = k["xipos"] - com
    Iwv = np.einsum("bij,bj->bi", Iw, k["w"])
    L = (np.cross(r, m[:, None] * k["cvel"]) + Iwv).sum(0)
    ke = 0.5 * (m * (k["cvel"] ** 2).sum(1)).sum() + 0.5 * (k["w"] * Iwv).sum() + 0.5 * (np.asarray(kpm["dof_armature"], float) * v * v).sum()
    Ld = (np.cross(r, m[:, None] * k["cacc"]) + np.einsum("bij,bj->bi", Iw, k["alpha"]) + np.cross(k["w"], Iwv)).sum(0)
    cen = np.zeros(18)
    cen[0:3], cen[3:6], cen[6:9], cen[9], cen[10] = com, p / M, L, ke, -M * (g @ com)
    cen[11:14], cen[14:17], cen[17] = (m[:, None] * k["cacc"]).sum(0) / M, Ld, M
    I_total = (Iw + m[:, None, None] * ((r * r).sum(1)[:, None, None] * np.eye(3) - np.einsum("bi,bj->bij", r, r))).sum(0)
    return dict(body_vel=np.concatenate([k["w"], k["vel"]], 1), body_acc=np.concatenate([k["alpha"], k["acc"]], 1), body_com_vel=k["cvel"], centroid=cen,
                xpos=k["xpos"], R=k["R"], xipos=k["xipos"], L_root=L + np.cross(com - k["xpos"][0], p), I_total=I_total)


def conservation_drift(kpm, c0, c1, t):
    """(dp - m g t [3], dL_com [3], d(ke + pe)) between two centroid rows a time t apart: what free flight keeps at zero"""
    m, g = float(np.asarray(kpm["body_mass"], float).sum()), np.asarray(kpm["opt"][1:4], float)
    return (m * (c1[CENTROID["com_vel"]] - c0[CENTROID["com_vel"]]) - m * g * t, c1[CENTROID["L_com"]] - c0[CENTROID["L_com"]],
            (c1[CENTROID["ke"]] + c1[CENTROID["pe"]]) - (c0[CENTROID["ke"]] + c0[CENTROID["pe"]]))


def edge_rows(std_qpos):
    """name -> (q, v) of the edge rows of the GPU parity test (fp32-representable): a non-unit root quaternion, joints at +-3 pi, heading at +-pi,
    20 rad/s on every joint, all-zero qvel"""
    rng = np.random.default_rng(16)
    base = np.array(std_qpos, float); base[7:] += rng.normal(size=69) * 0.2
    v0 = rng.uniform(-3.0, 3.0, NV)
    out = {}
    q = base.copy(); q[3:7] *= 1.7
    out["nonunit_quat"] = (q, v0)
    q = base.copy(); q[7::2] += 3 * np.pi; q[8::2] -= 3 * np.pi
    out["joints_3pi"] = (q, v0)
    for s in (1.0, -1.0):
        q = base.copy(); q[3:7] = qmul(qexp([0.0, 0.0, s * np.pi]), q[3:7] / np.linalg.norm(q[3:7]))
        out["heading_%spi" % ("+" if s > 0 else "-")] = (q, v0)
    v = v0.copy(); v[6:] = 20.0 * np.sign(rng.normal(size=69))
    out["fast_joints"] = (base.copy(), v)
    out["zero_qvel"] = (base.copy(), np.zeros(NV))
    return {k: (f32(q), f32(v)) for k, (q, v) in out.items()}
