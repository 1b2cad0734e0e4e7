"""numpy restatement of the UHC's extended controller (test infrastructure): HumanoidEnv.compute_torque (uhc/envs/humanoid_im.py:433-480) for
action_v 0 (base pose a_ref, no 2 pi unwrap) / 1 and meta_pd / meta_pd_joint, pinned to the reference by tests/golden/uhc_controller_variants.npz.
oracle/np_spd.compute_torque_np always unwraps and never scales the gains, so it is composed here rather than changed."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve


def gains(kpm, ctrl, meta, rfc, i_iter, sim_iter=15):
    jkp, jkd = np.array(kpm["kp"], float), np.array(kpm["kd"], float)
    m0 = 69 + 6 * rfc
    if meta == 1:
        return jkp * np.clip(ctrl[m0 + i_iter] + 1, 0, 10), jkd * np.clip(ctrl[m0 + i_iter + sim_iter] + 1, 0, 10)
    if meta == 2:
        return jkp * np.clip(ctrl[m0:m0 + 69] + 1, 0, 10), jkd * np.clip(ctrl[m0 + 69:m0 + 138] + 1, 0, 10)
    return jkp, jkd


def compute_torque_xc(qpos, qvel, M, C, ctrl, base_pos, kpm, action_v=1, meta=0, rfc=1, i_iter=0):
    dt = kpm["opt"][0]
    base = np.array(base_pos, float)
    if action_v == 1:
        while np.any(base - qpos[7:] > np.pi):
            base[base - qpos[7:] > np.pi] -= 2 * np.pi
        while np.any(base - qpos[7:] < -np.pi):
            base[base - qpos[7:] < -np.pi] += 2 * np.pi
    target = base + ctrl[:69] * kpm["a_scale"]
    jkp, jkd = gains(kpm, ctrl, meta, rfc, i_iter)
    k_p = np.zeros(75); k_d = np.zeros(75); k_p[6:] = jkp; k_d[6:] = jkd
    qpos_err = np.concatenate((np.zeros(6), qpos[7:] + qvel[6:] * dt - target))
    qvel_err = np.array(qvel, float)
    acc = cho_solve(cho_factor(M + np.diag(k_d) * dt), -C - k_p * qpos_err - k_d * qvel_err)
    qvel_err = qvel_err + acc * dt
    return -jkp * qpos_err[6:] - jkd * qvel_err[6:]


def oracle_control_step(o, kpm, ctrl, base_pos, action_v, meta, rfc, nsub=15):
    """do_simulation (humanoid_im.py:506-533) on OracleSim, composed per substep: fullM / qfrc_bias of the current data, the torque, clip, RFC, step."""
    from oracle import np_spd
    for i in range(nsub):
        q, v = o.get("qpos"), o.get("qvel")
        tau = compute_torque_xc(q, v, o.fullM(), o.get("qfrc_bias"), ctrl, base_pos, kpm, action_v, meta, rfc, i)
        tau = np.clip(tau, -kpm["torque_lim"], kpm["torque_lim"])
        applied = np_spd.rfc_implicit_np(q, ctrl[69:75], kpm) if rfc else np.zeros(6)
        o.set_ctrl(tau, applied)
        o.step()
