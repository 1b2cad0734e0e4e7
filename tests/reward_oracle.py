"""fp64 numpy restatements of the reward functions beside world_rfc_implicit / dynamic_supervision_v1.  Not a test module:
tests/test_reward_variants_cpu.py holds them to tests/golden/reward_variants.npz (the reference's own functions, tools/make_golden_rewards.py)
without a GPU, tests/test_gpu_uhc_rewards.py and tests/test_gpu_kin_reward_v2.py compare the HIP kernels with them.  Built on oracle/np_oracle.py
(pinned to the reference by tests/test_oracle_golden.py).  Quaternions are (w, x, y, z); one env per call.

    uhc/core/reward_function.py        world_rfc_implicit_v1_mul :56-102, local_rfc_implicit_reward :172-231, world_rfc_implicit_v2 :301-372,
                                       world_rfc_implicit_v3 :376-450
    kin_poly/core/reward_function.py   dynamic_supervision_v2 :999-1050
"""
import json
import math
import os

import numpy as np

from oracle import np_oracle as O

DT = 1.0 / 30.0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UHC_IDS = ("world_rfc_implicit_v1_mul", "local_rfc_implicit", "world_rfc_implicit_v2", "world_rfc_implicit_v3")
# every function's own `ws.get(key, default)` list, written out here from the reference (kinpoly_amd.uhc_config.REWARD_DEFAULTS is checked against it)
DEFAULTS = {
    "world_rfc_implicit_v1_mul": dict(k_p=2, k_v=0.005, k_e=20, k_c=1000, k_vf=1),
    "local_rfc_implicit": dict(w_p=0.5, w_v=0.0, w_e=0.2, w_rp=0.1, w_rv=0.1, w_vf=0.1, k_p=2, k_v=0.005, k_e=20, k_vf=1, k_rh=300, k_rq=300, k_rl=5.0, k_ra=0.5),
    "world_rfc_implicit_v2": dict(k_p=0.4, k_wp=0.4, k_v=0.005, k_j=100, k_c=100, k_vf=1),
    "world_rfc_implicit_v3": dict(w_p=0.4, w_wp=0.4, w_v=0.005, w_j=100, w_c=100, w_vf=1, k_p=0.4, k_wp=0.4, k_v=0.005, k_j=100, k_c=100, k_vf=1),
    "dynamic_supervision_v2": dict(w_hp=1.0, w_hq=1.0, w_p=0.6, w_v=0.1, w_e=0.2, k_hp=1.0, k_hq=1.0, k_p=2, k_v=0.005, k_e=20),
}


def full_ws(rid, ws):
    return {**DEFAULTS[rid], **{k: v for k, v in ws.items() if k in DEFAULTS[rid]}}


def _vf_r(action, vf_dim, k_vf):
    vf = action[-vf_dim:] if vf_dim > 0 else action             # action[-0:] is the whole action
    return math.exp(-k_vf * np.linalg.norm(vf) ** 2)


def _common(s, ex, ind, dt):
    bquat = O.get_body_quat(s["qpos"])
    return bquat, O.get_angvel_fd(s["prev_bquat"], bquat, dt), O.multi_quat_norm(O.multi_quat_diff(bquat, ex["bquat"][ind]))


def world_rfc_implicit_v1_mul(s, ex, ind, action, vf_dim, ws, b_diffw, jw=None, dt=DT):
    bquat, bangvel, pose_diff = _common(s, ex, ind, dt)
    pose_diff[1:] *= b_diffw
    cur_ee = np.concatenate([s["xpos"][b] for b in O.EE_BODIES])
    info = np.array([math.exp(-ws["k_p"] * np.linalg.norm(pose_diff) ** 2), math.exp(-ws["k_v"] * np.linalg.norm(bangvel - ex["bangvel"][ind]) ** 2),
                     math.exp(-ws["k_e"] * np.linalg.norm(cur_ee - ex["ee_wpos"][ind]) ** 2), math.exp(-ws["k_c"] * np.linalg.norm(s["com"] - ex["com"][ind]) ** 2),
                     _vf_r(action, vf_dim, ws["k_vf"])])
    return float(np.prod(info)), info


def local_rfc_implicit(s, ex, ind, action, vf_dim, ws, b_diffw, jw=None, dt=DT):
    bquat, bangvel, pose_diff = _common(s, ex, ind, dt)
    q, p = s["qpos"], s["prev_qpos"]
    qvel = O.get_qvel_fd_new(p.copy(), q.copy(), dt)
    rlinv_local = O.transform_vec(qvel[:3], p[3:7], "root")     # get_qvel_fd_new(prev, cur, dt, 'root'): the frame of ITS cur_qpos = prev_qpos (math.py:62-64)
    cur_ee = np.concatenate([O.transform_vec(s["xpos"][b] - q[:3], q[3:7], "root") for b in O.EE_BODIES])
    pose_r = math.exp(-ws["k_p"] * np.linalg.norm(pose_diff[1:] * b_diffw) ** 2)
    vel_r = math.exp(-ws["k_v"] * np.linalg.norm(bangvel[3:] - ex["bangvel"][ind][3:]) ** 2)
    ee_r = math.exp(-ws["k_e"] * np.linalg.norm(cur_ee - ex["ee_pos"][ind]) ** 2)
    rq = O.multi_quat_norm(O.multi_quat_diff(O.de_heading(q[3:7]), ex["rq_rmh"][ind]))[0]
    rp_r = math.exp(-ws["k_rh"] * (q[2] - ex["qpos"][ind][2]) ** 2 - ws["k_rq"] * rq ** 2)
    rv_r = math.exp(-ws["k_rl"] * np.linalg.norm(rlinv_local - ex["rlinv_local"][ind]) ** 2 - ws["k_ra"] * np.linalg.norm(qvel[3:6] - ex["rangv"][ind]) ** 2)
    vf_r = _vf_r(action, vf_dim, ws["k_vf"]) if ws["w_vf"] > 0.0 else 0.0
    r = ws["w_p"] * pose_r + ws["w_v"] * vel_r + ws["w_e"] * ee_r + ws["w_rp"] * rp_r + ws["w_rv"] * rv_r + ws["w_vf"] * vf_r
    return r / (ws["w_p"] + ws["w_v"] + ws["w_e"] + ws["w_rp"] + ws["w_rv"] + ws["w_vf"]), np.array([pose_r, vel_r, ee_r, rp_r, rv_r, vf_r])


def _v2_terms(s, ex, ind, action, vf_dim, ws, jw, dt):
    bquat, bangvel, pose_diff = _common(s, ex, ind, dt)
    wpose_diff = O.multi_quat_norm(O.multi_quat_diff(s["xquat"].reshape(-1), ex["wbquat"][ind]))
    bcom = np.linalg.norm((ex["body_com"][ind].reshape(-1, 3) - s["xipos"]) * jw[:, None], axis=1) ** 2
    jpos = np.linalg.norm((s["xpos"] - ex["wbpos"][ind].reshape(-1, 3)) * jw[:, None], axis=1) ** 2
    return np.array([math.exp(-ws["k_p"] * ((pose_diff * jw) ** 2).mean()), math.exp(-ws["k_wp"] * ((wpose_diff * jw) ** 2).mean()),
                     math.exp(-ws["k_c"] * bcom.mean()), math.exp(-ws["k_j"] * jpos.mean()),
                     math.exp(-ws["k_v"] * ((bangvel - ex["bangvel"][ind]) ** 2).mean()), _vf_r(action, vf_dim, ws["k_vf"])])


def world_rfc_implicit_v2(s, ex, ind, action, vf_dim, ws, b_diffw, jw, dt=DT):
    info = _v2_terms(s, ex, ind, action, vf_dim, ws, jw, dt)
    return float(np.prod(info)), info


def world_rfc_implicit_v3(s, ex, ind, action, vf_dim, ws, b_diffw, jw, dt=DT):
    info = _v2_terms(s, ex, ind, action, vf_dim, ws, jw, dt)
    return float(np.dot([ws["w_p"], ws["w_wp"], ws["w_c"], ws["w_j"], ws["w_v"], ws["w_vf"]], info)), info


UHC_FUNCS = {"world_rfc_implicit_v1_mul": world_rfc_implicit_v1_mul, "local_rfc_implicit": local_rfc_implicit, "world_rfc_implicit_v2": world_rfc_implicit_v2,
             "world_rfc_implicit_v3": world_rfc_implicit_v3}


def kin_rotation_from_quaternion(q):
    """kin_poly/utils/transformation.py:362-372, kin_poly's own copy: zero if |1 - w| < 1e-6 or |1 + w| < 1e-6, else the unit axis times 2 acos(w)"""
    if abs(1.0 - q[0]) < 1e-6 or abs(1 + q[0]) < 1e-6:
        return np.zeros(3)
    angle = 2 * math.acos(q[0])
    axis = q[1:4] / math.sin(angle / 2.0)
    return axis / np.linalg.norm(axis) * angle


def kin_angvel_fd(prev_bquat, cur_bquat, dt):       # kin_poly/utils/math_utils.py:47-53
    q_diff = O.multi_quat_diff(cur_bquat, prev_bquat)
    return np.concatenate([kin_rotation_from_quaternion(q_diff[4 * i:4 * i + 4]) / dt for i in range(24)])


def dynamic_supervision_v2(qpos, xpos, xquat, prev_bquat, head_pose_t, gt_bquat_t, gt_bquat_prev, gt_wbpos_t, ws, b_diffw, dt=DT):
    """head position / orientation as v1; pose, velocity and all 24 body positions against the ground truth; a weighted sum -> (reward, info [5]).
    The helpers are kin_poly's own: its multi_quat_norm takes acos(w) without the absolute value (math_utils.py:105-109)."""
    hp_r = math.exp(-ws["k_hp"] * np.linalg.norm(xpos[13] - head_pose_t[:3]) ** 2)
    hq = O.multi_quat_norm_v2(O.multi_quat_diff(xquat[13], head_pose_t[3:])).mean()
    hq_r = math.exp(-ws["k_hq"] * hq ** 2)
    bquat = O.get_body_quat(qpos)
    pose_diff = np.arccos(np.clip(O.multi_quat_diff(bquat, gt_bquat_t)[::4], -1.0, 1.0))
    pose_diff[1:] *= b_diffw
    pose_r = math.exp(-ws["k_p"] * np.linalg.norm(pose_diff) ** 2)
    vel_r = math.exp(-ws["k_v"] * np.linalg.norm(kin_angvel_fd(prev_bquat, bquat, dt) - kin_angvel_fd(gt_bquat_prev, gt_bquat_t, dt)) ** 2)
    ee_r = math.exp(-ws["k_e"] * np.linalg.norm(xpos - gt_wbpos_t.reshape(-1, 3)) ** 2)
    info = np.array([hp_r, hq_r, pose_r, vel_r, ee_r])
    return float(np.dot([ws["w_hp"], ws["w_hq"], ws["w_p"], ws["w_v"], ws["w_e"]], info)), info


# ------------------------------------------------------------------ torch forms, any dtype / device: the error rule's "fp32 torch path on the same inputs"
def torch_reward(rid, s, ex_row, action, vf_dim, ws, b_diffw24, jw, dt, dtype=None, device="cpu"):
    """the kinpoly_amd.uhc_env function of `rid` on batched rows: s and ex_row are dicts of [N, .] arrays or tensors (dtype None: float64)"""
    import torch
    from kinpoly_amd import uhc_env as U
    dtype = dtype or torch.float64
    t = lambda a: a.to(device, dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype, device=device)      # noqa: E731
    S, E = {k: t(v) for k, v in s.items()}, {k: t(v) for k, v in ex_row.items()}
    a, bw, tail = t(action), t(b_diffw24), (dt, ws, vf_dim)
    if rid in ("world_rfc_implicit", "world_rfc_implicit_v1_mul"):
        fn = U.world_rfc_implicit_reward_t if rid == "world_rfc_implicit" else U.world_rfc_implicit_v1_mul_reward_t
        return fn(S["xpos"], S["bquat"], S["prev_bquat"], S["com"], a, E["bquat"], E["bangvel"], E["ee_wpos"], E["com"], bw, *tail)
    if rid == "local_rfc_implicit":
        return U.local_rfc_implicit_reward_t(S["qpos"], S["prev_qpos"], S["xpos"], S["bquat"], S["prev_bquat"], a, E["qpos"], E["bquat"], E["bangvel"], E["ee_pos"],
                                             E["rq_rmh"], E["rlinv_local"], E["rangv"], bw, *tail)
    fn = U.world_rfc_implicit_v2_reward_t if rid == "world_rfc_implicit_v2" else U.world_rfc_implicit_v3_reward_t
    return fn(S["xpos"], S["xquat"], S["xipos"], S["bquat"], S["prev_bquat"], a, E["bquat"], E["wbquat"], E["bangvel"], E["wbpos"], E["body_com"], t(jw), *tail)


def dynamic_supervision_v2_t(bquat, xpos, xquat, prev_bquat, head_pose_t, gt_bquat_t, gt_bquat_prev, gt_wbpos_t, ws, b_diffw24, dt=DT):
    """dynamic_supervision_v2 on [N, .] tensors of one dtype -> (reward [N], info [N, 5]).  The package has no torch path of the kinematic reward, so the
    fp32 figure of the error rule comes from this one.  fp64: the reference's formulas (acos(w); zero velocity below 1e-6); fp32: the forms
    kinpoly_amd.context explains (atan2 of |xyz| and w, |xyz|^2 < eps (1 + |w|)), the ones the package's fp32 torch paths use."""
    import torch
    from kinpoly_amd.context import quat_inv, quat_mul
    N, f64 = bquat.shape[0], bquat.dtype == torch.float64

    def acos_w(q):
        return torch.acos(q[..., 0].clamp(-1.0, 1.0)) if f64 else torch.atan2(q[..., 1:].norm(dim=-1), q[..., 0])

    def angvel(prev, cur):
        q = quat_mul(cur.view(N, 24, 4), quat_inv(prev.view(N, 24, 4)))
        w, n = q[..., 0], q[..., 1:].norm(dim=-1)
        small = ((1 - w).abs() < 1e-6) | ((1 + w).abs() < 1e-6) if f64 else (n * n < 1e-6 * (1 + w.abs()))
        out = q[..., 1:] / n.clamp_min(1e-30)[..., None] * (2 * acos_w(q))[..., None] / dt
        return torch.where(small[..., None], torch.zeros_like(out), out).reshape(N, 72)

    hp_r = torch.exp(-ws["k_hp"] * ((xpos.view(N, 24, 3)[:, 13] - head_pose_t[:, :3]) ** 2).sum(1))
    hq = quat_mul(xquat.view(N, 24, 4)[:, 13], quat_inv(head_pose_t[:, 3:]))
    hq_r = torch.exp(-ws["k_hq"] * ((hq[:, 0].abs() - 1.0) ** 2 + (hq[:, 1:] ** 2).sum(1)))
    pose = acos_w(quat_mul(bquat.view(N, 24, 4), quat_inv(gt_bquat_t.view(N, 24, 4)))) * b_diffw24[None]
    pose_r = torch.exp(-ws["k_p"] * (pose ** 2).sum(1))
    vel_r = torch.exp(-ws["k_v"] * ((angvel(prev_bquat, bquat) - angvel(gt_bquat_prev, gt_bquat_t)) ** 2).sum(1))
    ee_r = torch.exp(-ws["k_e"] * ((xpos - gt_wbpos_t) ** 2).sum(1))
    info = torch.stack([hp_r, hq_r, pose_r, vel_r, ee_r], 1)
    return ws["w_hp"] * hp_r + ws["w_hq"] * hq_r + ws["w_p"] * pose_r + ws["w_v"] * vel_r + ws["w_e"] * ee_r, info


def rel_err(got, want):
    """max |got - want| / max(1, |want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ------------------------------------------------------------------ the fixture
def load_fixture():
    g = np.load(os.path.join(GOLD, "reward_variants.npz"))
    ex = {k[2:]: g[k] for k in g.files if k.startswith("e_")}
    ex["qpos"] = g["clip"]
    return g, ex


def uhc_case(g, ex, i):
    """case i of the fixture -> (rid, state, expert row, action, vf_dim, full weights, jw, reward, info); the functions' dt is g["dt"], env.dt"""
    rid = str(g["rid"][i])
    s = {"qpos": g["qpos"][i], "prev_qpos": g["prev_qpos"][i], "prev_bquat": g["prev_bquat"][i], "xpos": g["xpos"][i].reshape(24, 3),
         "xquat": g["xquat"][i].reshape(24, 4), "xipos": g["xipos"][i].reshape(24, 3), "com": g["com"][i]}
    ind = min(int(g["t"][i]), ex["qpos"].shape[0] - 1)                   # get_expert_index with start_ind 0
    nd = int(g["info_dim"][i])
    return (rid, s, ind, g["action"][i][:int(g["action_dim"][i])], int(g["vf_dim"][i]), full_ws(rid, json.loads(str(g["ws"][i]))), g["jpos_diffw"][i],
            float(g["reward"][i]), g["info"][i][:nd])


def kin_case(g, i):
    t = int(g["k_t"][i])
    ws = full_ws("dynamic_supervision_v2", json.loads(str(g["k_ws"][i])))
    args = (g["k_qpos"][i], g["k_xpos"][i].reshape(24, 3), g["k_xquat"][i].reshape(24, 4), g["k_prev_bquat"][i], g["k_head_pose"][i][t], g["k_gt_bquat"][i][t],
            g["k_gt_bquat"][i][t - 1], g["k_gt_wbpos"][i][t], ws, g["b_diffw"], float(g["dt"]))
    return args, float(g["k_reward"][i]), g["k_info"][i]
