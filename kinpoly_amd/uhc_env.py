"""The UHC training environment (`HumanoidEnv`, uhc/envs/humanoid_im.py) and its expert-feature precompute
(`get_expert`, uhc/utils/tools.py:20-85), batched over N environments on the device.

It runs on the same C-ABI entry points as the kinematic-policy env: `kp_sim_step_ctrl` is `do_simulation`, `kp_sim_obs_cc` is
`get_full_obs_v1` against the expert frame t + 1 (installed with `kp_sim_set_target`), `kp_sim_fk` does the clip's forward
kinematics.  Reward (`world_rfc_implicit_reward`, uhc/core/reward_function.py:4-53) and termination (`calc_body_diff`, the MEAN
form of humanoid_im.py:719-726, threshold 0.5) are a handful of [N, .] tensor ops.  SURVEY.md section 8(f) row 3.
The other functions of the reward registry (:453-460) are the `*_reward_t` functions below on this single-clip path and
`kp_sim_uhc_track_r` on a take library; `reward_id` comes from the UhcConfig (or the constructor).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import sim as kpsim
from .context import quat_acos_w, quat_inv, quat_mul, quat_rotate_t, quat_sin_half, quat_small
from .env import RunningState
from .model_compiler import read_kpm
from .nets import MLP, PolicyMCP, Value, gaussian_log_prob
from .ppo import optimizer_step, ppo_surrogate, value_step, value_targets

EE_BODIES = (4, 8, 17, 22, 13)          # L_Toe, R_Toe, L_Wrist, R_Wrist, Head (humanoid_im.py:329)
UHC_REWARD_WEIGHTS = dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=2.0, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0)   # uhc.yml:37-48


def rotation_from_quaternion_t(q):
    """uhc/khrylib/utils/transformation.py:348-356 on [..., 4]: axis * angle, no wrap; exactly 0 when 1 - |w| < 1e-8."""
    small = quat_small(q)
    s = quat_sin_half(q).clamp_min(1e-30)
    out = q[..., 1:] / s[..., None] * (2 * quat_acos_w(q))[..., None]
    return torch.where(small[..., None], torch.zeros_like(out), out)


def get_angvel_fd_t(prev_bquat, cur_bquat, dt):
    """math.py:68-74 on [..., 96] -> [..., 72]."""
    p, c = prev_bquat.reshape(*prev_bquat.shape[:-1], 24, 4), cur_bquat.reshape(*cur_bquat.shape[:-1], 24, 4)
    return (rotation_from_quaternion_t(quat_mul(c, quat_inv(p))) / dt).reshape(*prev_bquat.shape[:-1], 72)


def get_qvel_fd_new_t(cur_qpos, next_qpos, dt):
    """math.py:45-65 (transform=None) on [..., 76] -> [..., 75]: root angular velocity in the root frame, joint differences unwrapped."""
    v = (next_qpos[..., :3] - cur_qpos[..., :3]) / dt
    qrel = quat_mul(next_qpos[..., 3:7], quat_inv(cur_qpos[..., 3:7]))
    w = qrel[..., 0]
    small = quat_small(qrel)
    s = quat_sin_half(qrel).clamp_min(1e-30)
    angle = torch.where(small, torch.zeros_like(w), 2 * quat_acos_w(qrel))
    axis = torch.where(small[..., None], torch.tensor([1.0, 0.0, 0.0], device=w.device, dtype=w.dtype).expand_as(qrel[..., 1:]), qrel[..., 1:] / s[..., None])
    angle = torch.where(angle > math.pi, angle - 2 * math.pi, angle)
    rv = quat_rotate_t(cur_qpos[..., 3:7], axis * angle[..., None] / dt)
    diff = next_qpos[..., 7:] - cur_qpos[..., 7:]
    diff = diff - 2 * math.pi * torch.ceil((diff - math.pi) / (2 * math.pi))          # the two while-loops: into (-pi, pi]
    return torch.cat([v, rv, diff / dt], -1)


def get_expert_batch(sim: kpsim.KpSim, expert_qpos: torch.Tensor, body_mass: torch.Tensor, dt=1.0 / 30.0) -> dict:
    """get_expert for N clips at once: expert_qpos [N, T, 76] -> dict of [N, T, .] device tensors (same keys as the reference)."""
    N, T, _ = expert_qpos.shape
    q = expert_qpos.to(sim.device, torch.float32).contiguous()
    fk = sim.fk(q.reshape(-1, 76))
    wbpos, wbquat = fk["wbpos"].view(N, T, 24, 3), fk["wbquat"].view(N, T, 24, 4)
    body_com = fk["body_com"].view(N, T, 24, 3)
    bquat = fk["bquat"].view(N, T, 24, 4).clone()
    bquat[:, :, 0] = q[:, :, 3:7]                                   # env.get_body_quat() starts from the raw root quaternion
    ex = {"qpos": q, "wbpos": wbpos.reshape(N, T, 72), "wbquat": wbquat.reshape(N, T, 96), "bquat": bquat.reshape(N, T, 96),
          "body_com": body_com.reshape(N, T, 72), "com": (body_com * body_mass[None, None, :, None]).sum(2) / body_mass.sum(),
          "head_pose": torch.cat([wbpos[:, :, 13], wbquat[:, :, 13]], -1)}
    ee = wbpos[:, :, list(EE_BODIES)]
    ex["ee_wpos"] = ee.reshape(N, T, 15)
    rootq = q[:, :, None, 3:7].expand(N, T, 5, 4)
    ex["ee_pos"] = quat_rotate_t(rootq, ee - q[:, :, None, :3]).reshape(N, T, 15)
    h = torch.zeros_like(q[:, :, 3:7]); h[..., 0] = q[..., 3]; h[..., 3] = q[..., 6]
    h = h / h.norm(dim=-1, keepdim=True)
    ex["rq_rmh"] = quat_mul(quat_inv(h), q[:, :, 3:7])
    qvel = get_qvel_fd_new_t(q[:, :-1], q[:, 1:], dt).clamp(-10.0, 10.0)
    qvel = torch.cat([qvel[:, :1], qvel], 1)                        # frame 0 repeats frame 1's finite difference
    ex["qvel"], ex["rlinv"], ex["rangv"] = qvel, qvel[..., :3], qvel[..., 3:6]
    ex["rlinv_local"] = torch.cat([quat_rotate_t(q[:, 1:2, 3:7], qvel[:, :1, :3]), quat_rotate_t(q[:, 1:, 3:7], qvel[:, 1:, :3])], 1)
    bav = get_angvel_fd_t(ex["bquat"][:, :-1], ex["bquat"][:, 1:], dt)
    ex["bangvel"] = torch.cat([bav[:, :1], bav], 1)
    ex["len"] = T
    ex["height_lb"], ex["head_height_lb"] = q[:, :, 2].min(1).values, ex["head_pose"][:, :, 2].min(1).values
    return ex


def world_rfc_implicit_reward_t(xpos, bquat, prev_bquat, com, action, e_bquat, e_bangvel, e_ee_wpos, e_com, b_diffw, dt=1.0 / 30.0, ws=UHC_REWARD_WEIGHTS, vf_dim=6):
    """uhc/core/reward_function.py:4-53 on [N, .] tensors -> (reward [N], info [N, 5]).  The w_vf term reads action[-vf_dim:] (:44-46) as the reference
    does: with meta-PD those are meta entries, and with residual_force off (vf_dim 0) action[-0:] is the whole action."""
    N = xpos.shape[0]
    cur_ee = xpos.view(N, 24, 3)[:, list(EE_BODIES)].reshape(N, 15)
    cur_bangvel = get_angvel_fd_t(prev_bquat, bquat, dt)
    qd = quat_mul(bquat.view(N, 24, 4), quat_inv(e_bquat.view(N, 24, 4)))
    pose_diff = (torch.acos(qd[..., 0].abs().clamp(-1.0, 1.0)) if qd.dtype == torch.float64 else torch.atan2(quat_sin_half(qd), qd[..., 0].abs())) * b_diffw[None]   # acos(|w|)
    pose_r = torch.exp(-ws["k_p"] * (pose_diff ** 2).sum(1))
    vel_r = torch.exp(-ws["k_v"] * ((cur_bangvel - e_bangvel) ** 2).sum(1))
    ee_r = torch.exp(-ws["k_e"] * ((cur_ee - e_ee_wpos) ** 2).sum(1))
    com_r = torch.exp(-ws["k_c"] * ((com - e_com) ** 2).sum(1))
    vf = action[:, -vf_dim:] if vf_dim > 0 else action
    vf_r = torch.exp(-ws["k_vf"] * (vf ** 2).sum(1)) if ws["w_vf"] > 0 else torch.zeros_like(pose_r)
    r = ws["w_p"] * pose_r + ws["w_v"] * vel_r + ws["w_e"] * ee_r + ws["w_c"] * com_r + ws["w_vf"] * vf_r
    return r / (ws["w_p"] + ws["w_v"] + ws["w_e"] + ws["w_c"] + ws["w_vf"]), torch.stack([pose_r, vel_r, ee_r, com_r, vf_r], 1)


def quat_angle_t(q1, q0):
    """multi_quat_norm(multi_quat_diff(q1, q0)) (math.py:158-174) on [..., 4]: acos(|w|) of q1 (x) q0^-1, in fp32 as the angle of the point (|w|, |xyz|)."""
    qd = quat_mul(q1, quat_inv(q0))
    return torch.acos(qd[..., 0].abs().clamp(-1.0, 1.0)) if qd.dtype == torch.float64 else torch.atan2(quat_sin_half(qd), qd[..., 0].abs())


def _vf_term(action, ws, vf_dim):
    vf = action[:, -vf_dim:] if vf_dim > 0 else action                  # action[-env.vf_dim:]; [-0:] is the whole action
    return torch.exp(-ws["k_vf"] * (vf ** 2).sum(1))


def world_rfc_implicit_v1_mul_reward_t(xpos, bquat, prev_bquat, com, action, e_bquat, e_bangvel, e_ee_wpos, e_com, b_diffw, dt=1.0 / 30.0, ws=None, vf_dim=6):
    """uhc/core/reward_function.py:56-102 -> (reward [N], info [N, 5]): world_rfc_implicit's five terms multiplied, the vf term always on."""
    N = xpos.shape[0]
    cur_ee = xpos.view(N, 24, 3)[:, list(EE_BODIES)].reshape(N, 15)
    pose_diff = quat_angle_t(bquat.view(N, 24, 4), e_bquat.view(N, 24, 4)) * b_diffw[None]
    pose_r = torch.exp(-ws["k_p"] * (pose_diff ** 2).sum(1))
    vel_r = torch.exp(-ws["k_v"] * ((get_angvel_fd_t(prev_bquat, bquat, dt) - e_bangvel) ** 2).sum(1))
    ee_r = torch.exp(-ws["k_e"] * ((cur_ee - e_ee_wpos) ** 2).sum(1))
    com_r = torch.exp(-ws["k_c"] * ((com - e_com) ** 2).sum(1))
    vf_r = _vf_term(action, ws, vf_dim)
    return pose_r * vel_r * ee_r * com_r * vf_r, torch.stack([pose_r, vel_r, ee_r, com_r, vf_r], 1)


def local_rfc_implicit_reward_t(qpos, prev_qpos, xpos, bquat, prev_bquat, action, e_qpos, e_bquat, e_bangvel, e_ee_pos, e_rq_rmh, e_rlinv_local, e_rangv,
                                b_diffw, dt=1.0 / 30.0, ws=None, vf_dim=6):
    """uhc/core/reward_function.py:172-231 -> (reward [N], info [N, 6] = pose, vel, ee, root pose, root vel, vf).  b_diffw [24] as the world rewards take
    it (its root entry is not read: pose and velocity ignore the root).  The root velocities are get_qvel_fd_new(prev_qpos, qpos, dt, 'root')[:6]: both in
    the frame of prev_qpos' root, unclamped."""
    N = xpos.shape[0]
    rootq = qpos[:, 3:7]
    ee = xpos.view(N, 24, 3)[:, list(EE_BODIES)]
    cur_ee = quat_rotate_t(rootq[:, None].expand(N, 5, 4), ee - qpos[:, None, :3]).reshape(N, 15)
    pose_diff = quat_angle_t(bquat.view(N, 24, 4)[:, 1:], e_bquat.view(N, 24, 4)[:, 1:]) * b_diffw[None, 1:]
    pose_r = torch.exp(-ws["k_p"] * (pose_diff ** 2).sum(1))
    vel_r = torch.exp(-ws["k_v"] * ((get_angvel_fd_t(prev_bquat, bquat, dt) - e_bangvel)[:, 3:] ** 2).sum(1))
    ee_r = torch.exp(-ws["k_e"] * ((cur_ee - e_ee_pos) ** 2).sum(1))
    h = torch.zeros_like(rootq); h[:, 0] = rootq[:, 0]; h[:, 3] = rootq[:, 3]
    h = h / h.norm(dim=-1, keepdim=True)
    rq_dist = quat_angle_t(quat_mul(quat_inv(h), rootq), e_rq_rmh)       # de_heading(qpos[3:7]) against rq_rmh
    rp_r = torch.exp(-ws["k_rh"] * (qpos[:, 2] - e_qpos[:, 2]) ** 2 - ws["k_rq"] * rq_dist ** 2)
    qv = get_qvel_fd_new_t(prev_qpos, qpos, dt)
    linv = quat_rotate_t(prev_qpos[:, 3:7], qv[:, :3])
    rv_r = torch.exp(-ws["k_rl"] * ((linv - e_rlinv_local) ** 2).sum(1) - ws["k_ra"] * ((qv[:, 3:6] - e_rangv) ** 2).sum(1))
    vf_r = _vf_term(action, ws, vf_dim) if ws["w_vf"] > 0 else torch.zeros_like(pose_r)
    r = ws["w_p"] * pose_r + ws["w_v"] * vel_r + ws["w_e"] * ee_r + ws["w_rp"] * rp_r + ws["w_rv"] * rv_r + ws["w_vf"] * vf_r
    return r / (ws["w_p"] + ws["w_v"] + ws["w_e"] + ws["w_rp"] + ws["w_rv"] + ws["w_vf"]), torch.stack([pose_r, vel_r, ee_r, rp_r, rv_r, vf_r], 1)


def _world_v2_terms(xpos, xquat, xipos, bquat, prev_bquat, action, e_bquat, e_wbquat, e_bangvel, e_wbpos, e_body_com, jw, dt, ws, vf_dim):
    N = xpos.shape[0]
    pose_r = torch.exp(-ws["k_p"] * ((quat_angle_t(bquat.view(N, 24, 4), e_bquat.view(N, 24, 4)) * jw[None]) ** 2).mean(1))
    wpose_r = torch.exp(-ws["k_wp"] * ((quat_angle_t(xquat.view(N, 24, 4), e_wbquat.view(N, 24, 4)) * jw[None]) ** 2).mean(1))
    vel_r = torch.exp(-ws["k_v"] * ((get_angvel_fd_t(prev_bquat, bquat, dt) - e_bangvel) ** 2).mean(1))
    com_r = torch.exp(-ws["k_c"] * ((((e_body_com - xipos).view(N, 24, 3) * jw[None, :, None]) ** 2).sum(2)).mean(1))
    jpos_r = torch.exp(-ws["k_j"] * ((((xpos - e_wbpos).view(N, 24, 3) * jw[None, :, None]) ** 2).sum(2)).mean(1))
    return pose_r, wpose_r, com_r, jpos_r, vel_r, _vf_term(action, ws, vf_dim)


def world_rfc_implicit_v2_reward_t(xpos, xquat, xipos, bquat, prev_bquat, action, e_bquat, e_wbquat, e_bangvel, e_wbpos, e_body_com, jw, dt=1.0 / 30.0, ws=None, vf_dim=6):
    """uhc/core/reward_function.py:301-372 -> (reward [N], info [N, 6] = pose, wpose, com, jpos, vel, vf): every distance a mean of squares, the terms
    multiplied.  jw [24] is reward_weights.jpos_diffw."""
    terms = _world_v2_terms(xpos, xquat, xipos, bquat, prev_bquat, action, e_bquat, e_wbquat, e_bangvel, e_wbpos, e_body_com, jw, dt, ws, vf_dim)
    pose_r, wpose_r, com_r, jpos_r, vel_r, vf_r = terms
    return pose_r * wpose_r * com_r * jpos_r * vel_r * vf_r, torch.stack(terms, 1)


def world_rfc_implicit_v3_reward_t(xpos, xquat, xipos, bquat, prev_bquat, action, e_bquat, e_wbquat, e_bangvel, e_wbpos, e_body_com, jw, dt=1.0 / 30.0, ws=None, vf_dim=6):
    """uhc/core/reward_function.py:376-450: v2's terms in a weighted sum that is not normalised."""
    terms = _world_v2_terms(xpos, xquat, xipos, bquat, prev_bquat, action, e_bquat, e_wbquat, e_bangvel, e_wbpos, e_body_com, jw, dt, ws, vf_dim)
    pose_r, wpose_r, com_r, jpos_r, vel_r, vf_r = terms
    r = ws["w_p"] * pose_r + ws["w_wp"] * wpose_r + ws["w_c"] * com_r + ws["w_j"] * jpos_r + ws["w_v"] * vel_r + ws["w_vf"] * vf_r
    return r, torch.stack(terms, 1)


class BatchedHumanoidEnv:
    """HumanoidEnv (UHC imitation env) x N. `load_expert(qpos [N, T, 76])`, `reset(mask)`, `step(a [N, action_dim])`.

    cfg (a UhcConfig) selects the controller's observation (obs_v 0 / 1 / 2, obs_vel, obs_v 0's heading / de-heading / phase), the termination body
    and the episode / reward constants of its file; without it the env is uhc.yml's (784-d get_full_obs_v1, env_term_body 'body')."""

    def __init__(self, n_envs, device=0, kpm_path=None, env_episode_len=100000, env_init_noise=0.0, env_expert_trail_steps=0,
                 body_diff_thresh=0.5, reward_weights=None, model_options=None, seed=0, cfg=None, reward_id=None, push_schedule=None):
        self.n = int(n_envs)
        self.push_schedule = push_schedule       # kinpoly_amd.push.PushSchedule or None: pushes at the tail of step() (None: no launch is added)
        self.cfg = cfg
        if cfg is not None:
            env_episode_len, env_init_noise, env_expert_trail_steps = cfg.env_episode_len, cfg.env_init_noise, cfg.env_expert_trail_steps
            reward_weights = reward_weights or cfg.full_reward_weights()
            model_options = {**(model_options or {}), **cfg.model_options()}
            reward_id = reward_id or cfg.reward_id
        # the function of the reward registry (reward_function.py:453-460); without a cfg and a reward_id the env is uhc.yml's, world_rfc_implicit
        self.reward_id = reward_id or "world_rfc_implicit"
        if self.reward_id not in kpsim.UHC_REWARD_IDS:
            raise ValueError(f"reward_id {self.reward_id!r} (implemented: {', '.join(kpsim.UHC_REWARD_IDS)})")
        if self.reward_id != "world_rfc_implicit":
            from .uhc_config import REWARD_DEFAULTS
            reward_weights = {**REWARD_DEFAULTS[self.reward_id], **(reward_weights or {})}      # that function's own `ws.get` defaults
        self.info_dim = kpsim.uhc_reward_info_dim(self.reward_id)
        self.obs_v = cfg.obs_v if cfg is not None else 1
        self.vf_dim = cfg.vf_dim if cfg is not None else 6
        self.a_ref = None if cfg is None or cfg.action_v != 0 else cfg.a_ref
        self.term_body = cfg.env_term_body if cfg is not None else "body"
        kpm_path = kpm_path or kpsim.DEFAULT_KPM
        self.model = kpsim.KpModel(kpm_path, **(model_options or {}))
        self.sim = kpsim.KpSim(self.model, self.n, device)
        self.device = self.sim.device
        kpm = read_kpm(kpm_path)
        self.body_mass = torch.tensor(kpm["body_mass"], dtype=torch.float32, device=self.device)
        self.b_diffw = torch.tensor(kpm["uhc_b_diffw"], dtype=torch.float32, device=self.device)        # pose_diff[1:] *= cfg.b_diffw (root weight 1)
        self.jpos_diffw = torch.tensor(kpm["body_diffw"], dtype=torch.float32, device=self.device)
        self.env_episode_len, self.env_init_noise, self.trail = env_episode_len, env_init_noise, env_expert_trail_steps
        self.body_diff_thresh, self.ws = body_diff_thresh, dict(reward_weights or UHC_REWARD_WEIGHTS)
        # reward_weights.jpos_diffw of v2 / v3 (reward_function.py:307): 24 body weights of the reward alone, default all 1
        self.rw_jpos_diffw = torch.tensor(self.ws.get("jpos_diffw") or [1.0] * 24, dtype=torch.float32, device=self.device)
        self._prev_qpos = torch.zeros((self.n, 76), dtype=torch.float32, device=self.device) if self.reward_id == "local_rfc_implicit" else None
        self.frame_skip, self.dt = 15, self.model.get_option("timestep") * 15
        self.gen = torch.Generator(device=self.device); self.gen.manual_seed(seed)
        self.cur_t = torch.zeros(self.n, dtype=torch.long, device=self.device)
        self.expert = self.takes = None
        self.obs_dim, self.action_dim = self.sim.cc_obs_dim, self.sim.cc_action_dim
        self._obs = torch.empty((self.n, self.obs_dim), dtype=torch.float32, device=self.device)
        self._ar = torch.arange(self.n, device=self.device)
        if self.a_ref is not None:
            self.a_ref = torch.tensor(self.a_ref, dtype=torch.float32, device=self.device)

    def load_expert(self, expert_qpos: torch.Tensor):
        self.expert = get_expert_batch(self.sim, expert_qpos, self.body_mass, self.dt)
        if self.takes is not None:
            self.takes, self.cur_t = None, torch.zeros(self.n, dtype=torch.long, device=self.device)

    def load_takes(self, library: kpsim.KpTakes, take_ids=None):
        """Imitate takes of a device-resident library (kinpoly_amd.sim.KpTakes, built with this env's sim) instead of one rectangular clip: every env is
        on a take of its own length (take_ids [N], default env e -> take e mod K), `step` runs the fused tracking kernel and `reset(mask, take_ids,
        start)` moves envs between takes.  Call reset() before the first step.

        A library with objects (KpTakes(obj_rows=...), SmplObjDataset.to_library): reset() also places every reset env's objects from the library row its
        humanoid state comes from (reset_model's has_obj branch) and the handle simulates them from then on; fail_safe() leaves them where the physics put
        them.  Refused: a model blob without object geoms, threads_per_env other than 64.  A library WITHOUT objects loaded onto a handle that already
        runs objects parks all five objects of every env (the handle stays on the object layout; parked objects touch nothing)."""
        n, dev = self.n, self.device
        if library.has_objects:
            if int(self.model.get_option("n_obj_geoms")) == 0:
                raise ValueError("load_takes: the take library carries objects but the model blob has no object geoms")
            if int(self.model.get_option("threads_per_env")) != 64:
                raise ValueError(f"load_takes: a take library with objects needs threads_per_env = 64, the model has {int(self.model.get_option('threads_per_env'))}")
            self._objects_on = True
        elif getattr(self, "_objects_on", False):
            from .dataset import convert_obj_qpos_np
            self.sim.set_objects(torch.tensor(convert_obj_qpos_np(np.zeros((n, 7)), None), dtype=torch.float32, device=dev).contiguous())
        self.takes, self.expert = library, None
        self.take_id = torch.zeros(n, dtype=torch.int32, device=dev); self.start_ind = torch.zeros(n, dtype=torch.int32, device=dev)
        self.cur_t = torch.zeros(n, dtype=torch.int32, device=dev)
        self._base = torch.zeros((n, 76), dtype=torch.float32, device=dev)
        self._take_len = torch.as_tensor(library.lens, device=dev)
        self._st = kpsim.KpUhcState(self.take_id.data_ptr(), self.start_ind.data_ptr(), self.cur_t.data_ptr(), self._base.data_ptr())
        w = self.ws
        other = self.reward_id != "world_rfc_implicit"
        g = lambda k: float(w.get(k, 0.0)) if other else float(w[k])    # a key the env's reward function does not read is 0; world_rfc_implicit reads all ten
        self._tc = kpsim.KpUhcCfg(*[g(k) for k in ("w_p", "w_v", "w_e", "w_c", "w_vf", "k_p", "k_v", "k_e", "k_c", "k_vf")], float(self.dt), float(self.body_diff_thresh),
                                  int(self.term_body == "body"), int(self.env_episode_len), int(self.trail), int(self.obs_v), int(self.vf_dim), int(self.action_dim),
                                  None if self.a_ref is None else self.a_ref.data_ptr(), self.b_diffw.data_ptr())
        # the other functions of the registry go through kp_sim_uhc_track_r; world_rfc_implicit stays on kp_sim_uhc_track
        self._tcr = None
        if other:
            self._tcr = kpsim.KpUhcCfgR(self._tc, kpsim.UHC_REWARD_IDS.index(self.reward_id), *[g(k) for k in ("w_rp", "w_rv", "k_rh", "k_rq", "k_rl", "k_ra", "w_wp", "w_j", "k_wp", "k_j")],
                                        self.rw_jpos_diffw.data_ptr(), None if self._prev_qpos is None else self._prev_qpos.data_ptr())
        self._next_ids = np.arange(n, dtype=np.int32) % library.K if take_ids is None else np.ascontiguousarray(take_ids, np.int32)

    def _noise(self):
        return (torch.randn((self.n, 69), device=self.device, generator=self.gen) * self.env_init_noise).contiguous() if self.env_init_noise > 0 else None

    def _obs_takes(self):
        phase = (self.cur_t.float() / self._take_len[self.take_id.long()]).contiguous() if self.sim.cc_obs_phase else None
        return self.sim.obs_cc(self._obs, phase=phase)

    def _reset_takes(self, env_mask, take_ids, start):
        m8 = None if env_mask is None else env_mask.to(self.device, torch.uint8).contiguous()
        if take_ids is None and self._next_ids is not None:            # the first reset puts the envs on the takes load_takes was given
            take_ids, m8 = self._next_ids, None
        self._next_ids = None
        self.sim.uhc_assign(self.takes, self._st, self._tc, m8, take_ids, start, keep_t=False, noise=self._noise())
        return self._obs_takes()

    def fail_safe(self, env_mask: torch.Tensor | None = None):
        """HumanoidEnv.fail_safe (humanoid_im.py:235-238) for the masked envs: state := the expert's qpos / qvel at the current index; cur_t stays."""
        if self.takes is None:
            raise RuntimeError("fail_safe needs a take library (load_takes)")
        m8 = None if env_mask is None else env_mask.to(self.device, torch.uint8).contiguous()
        self.sim.uhc_assign(self.takes, self._st, self._tc, m8, None, None, keep_t=True, noise=None)
        return self._obs_takes()

    def get_obj_qpos(self):
        """data.qpos[76:111] of every env: a zero-copy [N, 35] view of KP_OBJ_QPOS (follows the simulator; clone to keep)"""
        return self.sim.view("obj_qpos")

    def get_obj_qvel(self):
        """data.qvel[75:105] of every env: a zero-copy [N, 30] view of KP_OBJ_QVEL"""
        return self.sim.view("obj_qvel")

    @property
    def has_objects(self):
        return self.takes is not None and self.takes.has_objects

    def render_rgb(self, envs=None, camera=None, width=320, height=240):
        """Frames of the envs (all, or the indices `envs`): figure 0 the simulated pose, figure 1 the expert frame the controller tracks, the take's
        objects -> uint8 [n, H, W, 4] on the device (kinpoly_amd.render.render_env; camera None follows every env's root)."""
        from .render import render_env
        return render_env(self.sim, self.get_obj_qpos().clone() if self.has_objects else None, envs, camera, width, height)

    def render_ego(self, envs=None, width=64, height=64, camera=None):
        """What every env's simulated figure sees from its head (all envs, or the indices `envs`), with the env's objects -> uint8 [n, H, W, 4] on the
        device (kinpoly_amd.render.render_env_ego; camera: a HeadCamera, None for the default one at the head hull's centroid, fovy 90)."""
        from .render import render_env_ego
        return render_env_ego(self.sim, self.get_obj_qpos().clone() if self.has_objects else None, envs, camera, width, height)

    def push(self, entity, impulse, offset=None, env_mask=None):
        """An impulse push of the current state (KpSim.apply_impulse): entity int32 [N] (0..23 body, 24 + k object slot, -1 none), impulse [N, 6] = (p, l),
        offset [N, 3] or None, env_mask bool / uint8 [N] or None.  Call it between two step()s; the observation step() returned is then one push old."""
        m8 = None if env_mask is None else env_mask.to(self.device, torch.uint8).contiguous()
        self.sim.apply_impulse(entity.to(self.device, torch.int32).contiguous(), impulse.to(self.device, torch.float32).contiguous(),
                               None if offset is None else offset.to(self.device, torch.float32).contiguous(), m8)

    def contact_forces(self, cc_action=None, **kw) -> dict:
        """Contact forces of the current state (KpSim.contact_forces: per-contact forces, per-entity wrenches about the world origin, qfrc_constraint, qacc,
        the controller's torque) as device tensors.  cc_action [N, action_dim]: the action the stable-PD torque is formed from, against the PD base pose the
        handle stores at the time of the call (after step(): the expert frame of the observation); None = the action of the last step() (the env keeps a
        reference to that buffer).  For an env that was reset inside or after that step the held action still belongs to the finished episode.
        kw: env_mask, want; torque=[N,75] replaces the controller by a given torque."""
        if "torque" in kw:
            if cc_action is not None:
                raise ValueError("contact_forces: cc_action and torque are mutually exclusive")
            return self.sim.contact_forces(**kw)
        if cc_action is None:
            cc_action = getattr(self, "_last_cc_action", None)
            if cc_action is None:
                raise RuntimeError("contact_forces(): no action yet -- call step() first, or pass cc_action")
        return self.sim.contact_forces(action=cc_action.to(self.device, torch.float32).contiguous(), **kw)

    def body_motion(self, qacc=None, outputs=("body_vel", "body_com_vel", "centroid")) -> dict:
        """KpSim.body_motion on the STORED qpos / qvel of every env (zero-copy views: no host round trip): body velocities, momentum and energy of the
        current state as device tensors [N, ...].  qacc [N, 75] or None: the accelerations body_acc, com_acc and Ldot_com are formed with."""
        return self.sim.body_motion(self.sim.view("qpos"), self.sim.view("qvel"), qacc, outputs=outputs)

    def centroidal(self, qacc=None) -> dict:
        """balance.centroidal of the stored state: com, com_vel, L_com, ke, pe, com_acc, Ldot_com, mass per env (device tensors)"""
        from . import balance
        return balance.centroidal(self.sim, self.sim.view("qpos"), self.sim.view("qvel"), qacc)

    def _scheduled_push(self, done):
        """the tail of step(): what the schedule draws for the episode clock the step just advanced, for the envs that go on.
        With a schedule installed a non-finite body_diff counts as a failure: a push far beyond what a body survives (1e4 N s at every step) drives the fp32
        state to inf / nan within a control step, and the reference's `body_diff > thresh` (humanoid_im.py:559) is False for a nan -- without pushes that rule
        stays as it is."""
        entity, impulse, offset = self.push_schedule.draw(self.cur_t, done == 0)
        self.sim.apply_impulse(entity, impulse, offset)

    def _step_takes(self, a):
        if self._next_ids is not None:
            raise RuntimeError("load_takes: call reset() before the first step (the envs are on no take yet)")
        sim, n, dev = self.sim, self.n, self.device
        f = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)      # fresh outputs every step (the caller keeps them): allocator only, no launch
        o = {"custom_reward": f(n), "custom_info": f(n, self.info_dim), "body_diff": f(n), "percent": f(n), "fail": f(n, dt=torch.uint8), "end": f(n, dt=torch.uint8),
             "done": f(n, dt=torch.uint8)}
        sim.step_begin()
        if self._prev_qpos is not None:                                # env.prev_qpos (humanoid_im.py:538): local_rfc_implicit's root velocities
            self._prev_qpos.copy_(sim.view("qpos"))
        sim.step_ctrl_base(a.contiguous(), self._base, self.frame_skip)
        self._last_cc_action = a
        track, tc = (sim.uhc_track, self._tc) if self._tcr is None else (sim.uhc_track_r, self._tcr)
        track(self.takes, self._st, tc, a, o["custom_reward"], o["custom_info"], o["body_diff"], o["fail"], o["end"], o["done"], o["percent"])
        if self.push_schedule is not None:
            bad = (~torch.isfinite(o["body_diff"])).to(torch.uint8)      # a diverged env fails (see _scheduled_push)
            o["fail"] |= bad; o["done"] |= bad
            self._scheduled_push(o["done"])
        obs = self._obs_takes()
        info = {k: (v.view(torch.bool) if v.dtype == torch.uint8 else v) for k, v in o.items()}
        return obs, torch.ones(self.n, device=self.device), info.pop("done"), info

    def _e(self, key, t):
        return self.expert[key][self._ar, t.clamp(max=self.expert["len"] - 1)].contiguous()

    def _obs_now(self):
        if self.obs_v == 0:                                             # get_full_obs: get_expert_kin_pose(delta_t=0), frame t (humanoid_im.py:132, 679)
            self.sim.set_target(self._e("qpos", self.cur_t))
        else:                                                           # get_full_obs_v1 / _v2 look at expert frame t + 1 (humanoid_im.py:158, 245)
            self.sim.set_target(self._e("qpos", self.cur_t + 1))
        phase = (self.cur_t.float() / self.expert["len"]).contiguous() if self.sim.cc_obs_phase else None      # get_phase: cur_t / expert len (:141-142)
        return self.sim.obs_cc(self._obs, phase=phase)

    def reset(self, env_mask: torch.Tensor | None = None, take_ids=None, start=None):
        """take_ids / start (host int arrays [N], library path only): the take and start frame the masked envs move to; None keeps each env's take"""
        if self.takes is not None:
            return self._reset_takes(env_mask, take_ids, start)
        if take_ids is not None or start is not None:
            raise RuntimeError("reset(take_ids=...) needs a take library (load_takes)")
        m8 = None if env_mask is None else env_mask.to(self.device, torch.uint8).contiguous()
        if env_mask is None:
            self.cur_t.zero_()
        else:
            self.cur_t.masked_fill_(env_mask.to(self.device, torch.bool), 0)
        q0 = self.expert["qpos"][:, 0].clone()
        if self.env_init_noise > 0:
            q0[:, 7:] += torch.randn((self.n, 69), device=self.device, generator=self.gen) * self.env_init_noise
        self.sim.set_state(q0.contiguous(), self.expert["qvel"][:, 0].contiguous(), m8)
        return self._obs_now()

    def _reward_clip(self, a, xpos, bquat, com, prev_qpos):
        """reward_func[reward_id] of the single-clip path: the torch functions above on the expert rows of cur_t"""
        sim, e, t = self.sim, self._e, self.cur_t
        prev_bquat, tail = sim.get("prev_bquat"), (self.dt, self.ws, self.vf_dim)
        if self.reward_id in ("world_rfc_implicit", "world_rfc_implicit_v1_mul"):
            fn = world_rfc_implicit_reward_t if self.reward_id == "world_rfc_implicit" else world_rfc_implicit_v1_mul_reward_t
            return fn(xpos, bquat, prev_bquat, com, a, e("bquat", t), e("bangvel", t), e("ee_wpos", t), e("com", t), self.b_diffw, *tail)
        if self.reward_id == "local_rfc_implicit":
            return local_rfc_implicit_reward_t(sim.get("qpos"), prev_qpos, xpos, bquat, prev_bquat, a, e("qpos", t), e("bquat", t), e("bangvel", t), e("ee_pos", t),
                                               e("rq_rmh", t), e("rlinv_local", t), e("rangv", t), self.b_diffw, *tail)
        fn = world_rfc_implicit_v2_reward_t if self.reward_id == "world_rfc_implicit_v2" else world_rfc_implicit_v3_reward_t
        return fn(xpos, sim.get("xquat"), sim.get("xipos"), bquat, prev_bquat, a, e("bquat", t), e("wbquat", t), e("bangvel", t), e("wbpos", t), e("body_com", t),
                  self.rw_jpos_diffw, *tail)

    def step(self, a: torch.Tensor):
        if self.takes is not None:
            return self._step_takes(a)
        sim = self.sim
        sim.step_begin()                                               # prev_bquat
        tq = self._e("qpos", self.cur_t)                               # compute_torque's base pose is get_expert_kin_pose(delta_t=0) (humanoid_im.py:441, 678)
        if self.a_ref is not None:                                     # action_v 0: cfg.a_ref (:451-452); the kernel skips the unwrap for it
            tq = tq.clone(); tq[:, 7:] = self.a_ref
        sim.set_target(tq)
        prev_qpos = sim.get("qpos") if self._prev_qpos is not None else None       # env.prev_qpos (humanoid_im.py:538)
        sim.step_ctrl(a.contiguous(), self.frame_skip)
        self._last_cc_action = a
        self.cur_t += 1
        xpos, bquat = sim.get("xpos"), sim.get("bquat")
        com = (sim.get("xipos").view(self.n, 24, 3) * self.body_mass[None, :, None]).sum(1) / self.body_mass.sum()
        e_wbpos = self._e("wbpos", self.cur_t)
        body_diff = (((xpos - e_wbpos).view(self.n, 24, 3) * self.jpos_diffw[None, :, None]).norm(dim=2)).mean(1)
        if self.term_body == "body":
            fail = body_diff > self.body_diff_thresh
        else:   # 'head': the reference's chain tests 'Head', 'root' and 'body' only (humanoid_im.py:554-561), so the default never fails an episode
            fail = torch.zeros_like(body_diff, dtype=torch.bool)
        end = (self.cur_t >= self.env_episode_len) | (self.cur_t >= self.expert["len"] + self.trail)
        reward, rinfo = self._reward_clip(a, xpos, bquat, com, prev_qpos)
        if self.push_schedule is not None:
            fail = fail | ~torch.isfinite(body_diff)                    # a diverged env fails (see _scheduled_push)
            self._scheduled_push(fail | end)
        obs = self._obs_now()
        return obs, torch.ones(self.n, device=self.device), fail | end, {"fail": fail, "end": end, "percent": self.cur_t.float() / self.expert["len"],
                                                                        "custom_reward": reward, "custom_info": rinfo, "body_diff": body_diff}


class RunningStateOnline(RunningState):
    """ZFilter with update=True (uhc/khrylib/utils/zfilter.py): RunningStat.push over a whole [B, dim] batch at once
    (Chan et al. pairwise merge == pushing the rows one by one, in exact arithmetic)."""

    def __init__(self, dim=784, clip=5.0, device="cuda"):
        super().__init__(np.zeros(dim), np.ones(dim), clip, device)
        self.count = 0
        self._mean64 = torch.zeros(dim, dtype=torch.float64, device=self.mean.device)
        self._m2 = torch.zeros(dim, dtype=torch.float64, device=self.mean.device)

    def update(self, x: torch.Tensor):
        x = x.double()
        b = x.shape[0]
        bm = x.mean(0); bm2 = ((x - bm) ** 2).sum(0)
        tot = self.count + b
        delta = bm - self._mean64
        self._m2 += bm2 + delta ** 2 * (self.count * b / tot)
        self._mean64 += delta * (b / tot)
        self.count = tot
        self.mean.copy_(self._mean64.float())
        std = torch.sqrt(self._m2 / (self.count - 1)) if self.count > 1 else self._mean64.abs()
        self.std.copy_(std.float())

    def __call__(self, x, update=True):
        if update:
            self.update(x)
        y = (x - self.mean) / (self.std + 1e-8)
        return y.clamp(-self.clip, self.clip) if self.clip else y


class CopycatAgent:
    """The UHC training iteration (uhc/agents/agent_copycat.py: sample with the running state updating, GAE, PPO on PolicyMCP)
    on the batched env: one process per GPU, built from the same steps as kinpoly_amd.ppo.PPOTrainer."""

    def __init__(self, env: BatchedHumanoidEnv, policy: PolicyMCP | None = None, value=None, gamma=0.95, tau=0.95, clip_epsilon=0.2,
                 policy_lr=5e-5, value_lr=3e-4, num_optim_epoch=10, group=None, dataset=None, seed=0, output_dir=None, push_schedule=None):
        self.env, self.group = env, group
        if push_schedule is not None:            # pushes while sampling and evaluating (kinpoly_amd.push.PushSchedule): the env applies them
            env.push_schedule = push_schedule
        cfg = getattr(env, "cfg", None)
        self.policy = (policy or (cfg.make_policy() if cfg is not None else PolicyMCP())).to(env.device).float()
        self.value = (value or (cfg.make_value() if cfg is not None else Value(MLP(env.obs_dim, (1024, 512), "relu")))).to(env.device).float()
        self.running_state = RunningStateOnline(env.obs_dim, 5.0, env.device)
        self.gamma, self.tau, self.clip_epsilon, self.num_optim_epoch = gamma, tau, clip_epsilon, num_optim_epoch
        self.opt_p = torch.optim.Adam([p for p in self.policy.parameters() if p.requires_grad], lr=policy_lr)
        self.opt_v = torch.optim.Adam(self.value.parameters(), lr=value_lr)
        # a library of takes (kinpoly_amd.dataset.AmassSingleDataset): every episode plays a newly drawn whole take (agent_copycat.py:144)
        self.dataset, self.output_dir, self.freq_dict, self.take_log = dataset, output_dir, None, []
        if dataset is not None:
            rank = 0
            if group is not None:
                import torch.distributed as dist
                rank = dist.get_rank(group)
            self.rng = np.random.default_rng([int(seed), rank])      # every rank draws its own takes
            path = None if output_dir is None else os.path.join(output_dir, "freq_dict.pt")
            if path is not None and os.path.exists(path):               # agent_copycat.py:27-28
                import joblib
                self.freq_dict = joblib.load(path)
            else:
                self.freq_dict = dataset.new_freq_dict()
            if env.takes is None:
                env.load_takes(dataset.to_library(env.sim), self._draw(1)[0])

    FREQ_CAP = 5000                                                      # agent_copycat.py:220

    def _draw(self, rows):
        """take ids [rows, N] drawn ahead on the host from the data set's draw_probs(freq_dict): as in the reference, the dict a sample() draws from is
        the one it started with (the workers hold a copy, agent_copycat.py:141-144, 210-220)"""
        p = self.dataset.draw_probs(self.freq_dict)
        return self.rng.choice(len(p), size=(rows, self.env.n), p=p).astype(np.int32)

    def record_episodes(self, episodes):
        """freq_dict[take] += [percent, fr_start] for every finished episode (agent_copycat.py:182, 210-220), the last FREQ_CAP kept per take"""
        for k, percent, fr_start in episodes:
            self.freq_dict[self.dataset.data_keys[k]].append([float(percent), int(fr_start)])
        self.freq_dict = {k: v if len(v) < self.FREQ_CAP else v[-self.FREQ_CAP:] for k, v in self.freq_dict.items()}

    def save_freq_dict(self, output_dir=None):
        import joblib
        d = output_dir or self.output_dir
        os.makedirs(d, exist_ok=True)
        joblib.dump(self.freq_dict, os.path.join(d, "freq_dict.pt"))

    def feed_eval(self, results: dict, data_mode="train", i_iter=0, output_dir=None):
        """eval_policy's bookkeeping (agent_copycat.py:72-85) for {take: {'percent': ...}}: a completed take enters freq_dict once, a failed one three
        times; eval_dict_<mode>.pt[i_iter] = {take: percent}.  Returns the coverage count."""
        coverage = 0
        for k, res in results.items():
            full = res["percent"] == 1
            coverage += int(full)
            if k in self.freq_dict:
                self.freq_dict[k] += [[res["percent"], 0] for _ in range(1 if full else 3)]
        d = output_dir or self.output_dir
        if d is not None:
            import joblib
            from collections import defaultdict
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, f"eval_dict_{data_mode}.pt")
            ev = joblib.load(path) if os.path.exists(path) else defaultdict(list)
            ev[i_iter] = {k: v["percent"] for k, v in results.items()}
            joblib.dump(ev, path)
        return coverage

    @torch.no_grad()
    def eval_policy(self, data_mode="train", i_iter=0, dataset=None, output_dir=None):
        """AgentCopycat.eval_policy (agent_copycat.py:46-85): every take of the data set (default: the training set) played whole with the mean action,
        the result fed back into freq_dict (feed_eval) and kept in eval_dict_<mode>.pt.  The env returns to the training library afterwards."""
        from .evaluate import eval_uhc_takes
        ds = dataset if dataset is not None else self.dataset
        train_lib = self.env.takes
        res = eval_uhc_takes(self.env, self.policy, self.running_state, ds, library=train_lib if ds is self.dataset else None)
        if train_lib is not None:
            self.env.load_takes(train_lib, self._draw(1)[0])
        coverage = self.feed_eval(res, data_mode, i_iter, output_dir)
        return f"Coverage {data_mode} of {coverage} out of {ds.get_len()}"

    @torch.no_grad()
    def sample(self, horizon):
        """`horizon` steps of every env with the running state updating -> S, A, R, M [N, horizon, .].  With a data set every episode plays a newly drawn
        take: the ids of the whole call are drawn ahead on the host, the finished episodes go to take_log / freq_dict after the call's one host read"""
        env, takes = self.env, self.dataset is not None
        S, A, R, M, D, P, K = [], [], [], [], [], [], []
        ids = self._draw(horizon) if takes else None
        first = env.reset(torch.ones(env.n, dtype=torch.bool, device=env.device), take_ids=self._draw(1)[0]) if takes else env.reset()
        obs = self.running_state(first, update=True)
        for t in range(horizon):
            a = self.policy.select_action(obs, False, env.gen).contiguous()
            if takes:
                K.append(env.take_id.clone())
            nobs, _, done, info = env.step(a)
            S.append(obs); A.append(a); R.append(info["custom_reward"]); M.append((~done).float())
            if takes:
                D.append(done); P.append(info["percent"])
            nobs = env.reset(done, take_ids=ids[t] if takes else None)
            obs = self.running_state(nobs, update=True)
        if takes:
            done, pct, take = torch.stack(D, 1).cpu().numpy(), torch.stack(P, 1).cpu().numpy(), torch.stack(K, 1).cpu().numpy()      # the one host read of the period
            eps = [(int(take[e, t]), float(pct[e, t]), 0) for t in range(horizon) for e in np.nonzero(done[:, t])[0]]
            if self.group is not None:                                   # ranks merge once per sample(), as the AR agent does
                import torch.distributed as dist
                allv = [None] * dist.get_world_size(self.group)
                dist.all_gather_object(allv, eps, group=self.group)
                eps = [x for v in allv for x in v]
            self.take_log.append(eps)
            self.record_episodes(eps)
        return torch.stack(S, 1), torch.stack(A, 1), torch.stack(R, 1), torch.stack(M, 1)

    def log_prob(self, states, actions):
        return gaussian_log_prob(*self.policy(states), actions)

    def optimize_policy(self, horizon=32):
        S, A, R, M = self.sample(horizon)
        N, T, _ = S.shape
        fs, fa = S.reshape(N * T, -1), A.reshape(N * T, -1)
        adv, ret = value_targets(self.value, fs, R, M, self.gamma, self.tau, self.group)
        with torch.no_grad():
            fixed = self.log_prob(fs, fa)
        stats = {}
        for _ in range(self.num_optim_epoch):        # per epoch one value step, then one policy step clipped to 40 (every step: the UHC agent's clip list is a list)
            vloss = value_step(self.value, self.opt_v, fs, ret, self.group)
            surr = ppo_surrogate(self.log_prob(fs, fa), fixed, adv, self.clip_epsilon)
            optimizer_step(self.opt_p, surr, self.group, max_norm=40.0)
            stats = {"value_loss": float(vloss.detach()), "surr_loss": float(surr.detach())}
        stats.update(avg_reward=float(R.mean()), fail_rate=float((1 - M).mean()), num_steps=N * T)
        return stats
