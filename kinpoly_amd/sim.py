"""ctypes binding of libkinpoly_sim.so (include/kinpoly_sim.h) for torch device tensors.

This is the thin host layer: tensors in, tensors out.  A `KpSim` enqueues on the torch stream that was current when it
was created; `KpSim.use_current_stream()` rebinds it (kp_sim_set_stream) when the caller moves to another stream -- the library
never guesses.  There is NO CPU fallback: if the extension or a HIP device is missing, construction
fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import build as _build

NQ, NV, NU, NBODY = 76, 75, 69, 24
CC_OBS_DIM, AR_OBS_DIM, KIN_ACTION_DIM, CC_ACTION_DIM = 784, 105, 80, 75
AR_OBS_DIM_NO_ACTION = 101      # get_ar_obs_v1 without the action one-hot (use_action: false): model option ar_obs_action = 0


def ar_obs_dim(use_vel=False, use_head=True, use_action=True) -> int:
    """Row width of get_ar_obs_v1 for a statear yml's switches (humanoid_ar_v1.py:183-201; model options ar_obs_vel / ar_obs_head / ar_obs_action):
    74 pose + 75 velocities (use_vel) + 7 head difference (use_head) + 7 object + 13 head targets (use_head) + 4 action one-hot (use_action)."""
    return 74 + 75 * bool(use_vel) + 7 * bool(use_head) + 7 + 13 * bool(use_head) + 4 * bool(use_action)


AR_OBS_DIMS = tuple(ar_obs_dim(v, h, a) for h in (True, False) for v in (False, True) for a in (True, False))      # 105, 101, 180, 176, 85, 81, 160, 156


def ar_obs_options(use_vel=False, use_head=True, use_action=True) -> dict:
    """The model options of an observation variant that differ from the defaults (KpModel(**options))."""
    return {k: int(v) for k, v, d in (("ar_obs_vel", use_vel, False), ("ar_obs_head", use_head, True), ("ar_obs_action", use_action, True)) if bool(v) != d}
DEFAULT_KPM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "smpl_humanoid.kpm")
STEP_KPM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "smpl_humanoid_step.kpm")

FIELDS = dict(qpos=0, qvel=1, xpos=2, xquat=3, xipos=4, bquat=5, head=6, target_qpos=7, target_wbpos=8,
              target_wbquat=9, target_bquat=10, target_com=11, qpos_d=12, qvel_d=13, prev_bquat=14, prev_hpos=15, obj_qpos=16, obj_qvel=17,
              M=18, bias=19)

_lib = None


class KpCtx(C.Structure):
    """mirror of kp_ctx (include/kinpoly_sim.h)"""
    _fields_ = [("T", C.c_int), ("head_pose", C.c_void_p), ("head_vels", C.c_void_p), ("obj_head_relative_poses", C.c_void_p),
                ("action_one_hot", C.c_void_p), ("gt_bquat", C.c_void_p), ("gt_wbpos", C.c_void_p), ("obj_qpos", C.c_void_p),
                ("cur_t", C.c_void_p), ("row", C.c_void_p)]


class KpObsExt(C.Structure):
    """mirror of kp_obs_ext (include/kinpoly_sim.h): the context and `of` tables of kp_sim_obs_ar_ex, strides in floats"""
    _fields_ = [("ctx_dim", C.c_int), ("ctx_feat", C.c_void_p), ("ctx_stride_row", C.c_long), ("ctx_stride_t", C.c_long),
                ("of_dim", C.c_int), ("of", C.c_void_p), ("of_stride_row", C.c_long), ("of_stride_t", C.c_long)]


class KpRecordPre(C.Structure):
    """mirror of kp_record_pre (include/kinpoly_sim.h)"""
    _fields_ = [(k, C.c_int) for k in ("n", "T", "t", "ctx_T")] + [(k, C.c_void_p) for k in (
        "obs", "fresh", "qpos", "ctx_qpos", "row", "cur_t", "row_len", "row_meta", "states", "episode_start", "curr_qpos", "gt_target_qpos", "meta")]


class KpRecordPost(C.Structure):
    """mirror of kp_record_post"""
    _fields_ = [("n", C.c_int), ("T", C.c_int), ("t", C.c_int), ("fr_num", C.c_float)] + [(k, C.c_void_p) for k in (
        "action", "reward", "fail", "done", "percent", "c_info", "obs", "qpos", "cc_action", "cc_state", "meta",
        "actions", "rewards", "fails", "dones", "percents", "c_infos", "next_states", "res_qpos", "cc_actions", "cc_states", "v_metas")]


class KpRewardCfg(C.Structure):
    """mirror of kp_reward_cfg; defaults = config/statear/kin_poly.yml:72-86, humanoid_ar_v1.py:53-54"""
    _fields_ = [(k, C.c_float) for k in ("w_hp", "w_hq", "w_p", "w_jp", "w_act_p", "w_act_v", "k_hp", "k_hq", "k_p", "k_jp", "k_act_p",
                                          "k_act_v", "dt", "body_diff_thresh", "body_diff_gt_thresh")] + [("use_gt_term", C.c_int)]

    @classmethod
    def default(cls, use_gt_term=True):
        return cls(0.15, 0.15, 0.2, 0.2, 0.2, 0.1, 45.0, 45.0, 50.0, 50.0, 5.0, 0.005, 1.0 / 30.0, 10.0, 12.0, int(use_gt_term))


class KpRewardCfgV2(C.Structure):
    """mirror of kp_reward_cfg_v2 (dynamic_supervision_v2); defaults = its `ws.get(key, default)` list (reward_function.py:1003-1004) and the v1 thresholds"""
    _fields_ = [(k, C.c_float) for k in ("w_hp", "w_hq", "w_p", "w_v", "w_e", "k_hp", "k_hq", "k_p", "k_v", "k_e", "dt", "body_diff_thresh",
                                          "body_diff_gt_thresh")] + [("use_gt_term", C.c_int), ("b_diffw", C.c_void_p)]

    @classmethod
    def default(cls, b_diffw, use_gt_term=True):
        """b_diffw: device float tensor [24] (root 1, then cc_cfg.b_diffw); the caller keeps it alive"""
        return cls(1.0, 1.0, 0.6, 0.1, 0.2, 1.0, 1.0, 2.0, 0.005, 20.0, 1.0 / 30.0, 10.0, 12.0, int(use_gt_term), b_diffw.data_ptr())


class KpUhcState(C.Structure):
    """mirror of kp_uhc_state"""
    _fields_ = [(k, C.c_void_p) for k in ("take_id", "start_ind", "cur_t", "base_qpos")]


class KpUhcCfg(C.Structure):
    """mirror of kp_uhc_cfg"""
    _fields_ = [(k, C.c_float) for k in ("w_p", "w_v", "w_e", "w_c", "w_vf", "k_p", "k_v", "k_e", "k_c", "k_vf")] + [("dt", C.c_double), ("body_diff_thresh", C.c_float)] + \
               [(k, C.c_int) for k in ("term_body", "env_episode_len", "trail", "obs_v", "vf_dim", "action_dim")] + [("a_ref", C.c_void_p), ("b_diffw", C.c_void_p)]


UHC_REWARD_IDS = ("world_rfc_implicit", "world_rfc_implicit_v1_mul", "local_rfc_implicit", "world_rfc_implicit_v2", "world_rfc_implicit_v3")      # KP_UHC_*, in order


def uhc_reward_info_dim(reward_id) -> int:
    """the width of a reward function's info row (kp_uhc_reward_info_dim): reward_id a name of UHC_REWARD_IDS or its index"""
    i = UHC_REWARD_IDS.index(reward_id) if isinstance(reward_id, str) else int(reward_id)
    return 5 if i in (0, 1) else 6


class KpUhcCfgR(C.Structure):
    """mirror of kp_uhc_cfg_r"""
    _fields_ = [("base", KpUhcCfg), ("reward_id", C.c_int)] + [(k, C.c_float) for k in ("w_rp", "w_rv", "k_rh", "k_rq", "k_rl", "k_ra", "w_wp", "w_j", "k_wp", "k_j")] + \
               [("jpos_diffw", C.c_void_p), ("prev_qpos", C.c_void_p)]


class KpRenderStyle(C.Structure):
    """mirror of kp_render_style: base colours (r, g, b in 0..1) of the figures, the objects, the floor checker's two cells and the sky; zfar in metres"""
    _fields_ = [("figure", C.c_float * 3 * 4), ("object", C.c_float * 3), ("floor", C.c_float * 3 * 2), ("sky", C.c_float * 3), ("zfar", C.c_float)]

    @classmethod
    def default(cls):
        st = cls()
        load_library().kp_render_style_default(C.byref(st))
        return st


class KpContactOut(C.Structure):
    """mirror of kp_contact_out: the device arrays kp_sim_contact_forces fills (each may be NULL, not all)"""
    _fields_ = [(k, C.c_void_p) for k in ("ncon", "contact", "wrench", "qfrc_constraint", "qacc", "torque", "obj_qacc")]


# outputs of KpSim.contact_forces: name -> (trailing shape, dtype)
CONTACT_OUTPUTS = {"ncon": ((), torch.int32), "contact": ((64, 12), torch.float32), "wrench": ((26, 6), torch.float32), "qfrc_constraint": ((75,), torch.float32),
                   "qacc": ((75,), torch.float32), "torque": ((75,), torch.float32), "obj_qacc": ((2, 6), torch.float32)}


class KpInvDynOut(C.Structure):
    """mirror of kp_invdyn_out: the device arrays kp_sim_inverse_dynamics fills (each may be NULL, not all)"""
    _fields_ = [(k, C.c_void_p) for k in ("qfrc_inverse", "qfrc_constraint", "qfrc_bias", "contact", "net_wrench", "ncon")]


# outputs of KpSim.inverse_dynamics: name -> (trailing shape, dtype), in kp_invdyn_out's order
INVDYN_OUTPUTS = {"qfrc_inverse": ((75,), torch.float32), "qfrc_constraint": ((75,), torch.float32), "qfrc_bias": ((75,), torch.float32),
                  "contact": ((64, 12), torch.float32), "net_wrench": ((6,), torch.float32), "ncon": ((), torch.int32)}


class KpMotionOut(C.Structure):
    """mirror of kp_motion_out: the device arrays kp_sim_body_motion fills (each may be NULL, not all)"""
    _fields_ = [(k, C.c_void_p) for k in ("body_vel", "body_acc", "body_com_vel", "centroid")]


# outputs of KpSim.body_motion: name -> (trailing shape, dtype), in kp_motion_out's order
MOTION_OUTPUTS = {"body_vel": ((24, 6), torch.float32), "body_acc": ((24, 6), torch.float32), "body_com_vel": ((24, 3), torch.float32),
                  "centroid": ((18,), torch.float32)}
# the fields of a centroid row: name -> slice
CENTROID_FIELDS = {"com": slice(0, 3), "com_vel": slice(3, 6), "L_com": slice(6, 9), "ke": 9, "pe": 10, "com_acc": slice(11, 14), "Ldot_com": slice(14, 17),
                   "mass": 17}


class KpFitIn(C.Structure):
    """mirror of kp_fit_in: the device rows kp_sim_fit_pose reads (qpos0 and tgt_pos required, the others may be NULL)"""
    _fields_ = [(k, C.c_void_p) for k in ("qpos0", "tgt_pos", "tgt_quat", "w_pos", "w_rot", "q_prior", "w_prior")]


class KpFitCfg(C.Structure):
    """mirror of kp_fit_cfg (host side): the Levenberg-Marquardt schedule of kp_sim_fit_pose"""
    _fields_ = [("n_iters", C.c_int)] + [(k, C.c_float) for k in ("mu0", "mu_min", "mu_max", "mu_up", "mu_down")] + [("damp", C.c_float * 75), ("clamp_limits", C.c_int)]

    @classmethod
    def default(cls):
        c = cls()
        load_library().kp_fit_cfg_default(C.byref(c))
        return c


class KpFitOut(C.Structure):
    """mirror of kp_fit_out: the device rows kp_sim_fit_pose fills (dq may be NULL)"""
    _fields_ = [(k, C.c_void_p) for k in ("qpos", "info", "dq")]


# the columns of KpSim.fit_pose's info rows: name -> index
FIT_INFO = {"cost0": 0, "cost": 1, "accepted": 2, "mu": 3, "max_epos": 4, "max_erot": 5, "dq_inf": 6, "status": 7}


class KpMarkerSet(C.Structure):
    """mirror of kp_marker_set (host side): n_points, pt_body int32 [K], pt_offset float [K, 3]"""
    _fields_ = [("n_points", C.c_int), ("pt_body", C.c_void_p), ("pt_offset", C.c_void_p)]


class KpFitPointsIn(C.Structure):
    """mirror of kp_fit_points_in: the device rows kp_sim_fit_points reads (qpos0 required, pt_tgt with K > 0, the others may be NULL)"""
    _fields_ = [(k, C.c_void_p) for k in ("qpos0", "pt_tgt", "pt_w", "tgt_pos", "tgt_quat", "w_pos", "w_rot", "q_prior", "w_prior")]


class KpFitPointsCfg(C.Structure):
    """mirror of kp_fit_points_cfg (host side): kp_sim_fit_pose's schedule (fit), the floor term's weight and height"""
    _fields_ = [("fit", KpFitCfg), ("w_floor", C.c_float), ("floor_z", C.c_float)]

    @classmethod
    def default(cls):
        c = cls()
        load_library().kp_fit_points_cfg_default(C.byref(c))
        return c


class KpFitPointsOut(C.Structure):
    """mirror of kp_fit_points_out: the device rows kp_sim_fit_points fills (dq and pt_err may be NULL)"""
    _fields_ = [(k, C.c_void_p) for k in ("qpos", "info", "dq", "pt_err")]


# the columns of KpSim.fit_points' info rows: FIT_INFO's, then the points' and the floor's figures at the result
FIT_POINTS_INFO = {**FIT_INFO, "max_ept": 8, "rms_ept": 9, "max_depth": 10, "n_below": 11}
MAX_POINTS = 1024


class KpFitSceneCfg(C.Structure):
    """mirror of kp_fit_scene_cfg (host side): kp_sim_fit_points' configuration (pts) and the object term's weight"""
    _fields_ = [("pts", KpFitPointsCfg), ("w_obj", C.c_float)]

    @classmethod
    def default(cls):
        c = cls()
        load_library().kp_fit_scene_cfg_default(C.byref(c))
        return c


# the columns of KpSim.fit_scene's info rows: FIT_POINTS_INFO's, then the object term's figures at the result (15 is a spare zero)
FIT_SCENE_INFO = {**FIT_POINTS_INFO, "max_obj_depth": 12, "n_obj_verts": 13, "n_obj_pairs": 14}


class KpFitImageCfg(C.Structure):
    """mirror of kp_fit_image_cfg (host side): kp_sim_fit_scene's configuration (scene) and the nearest camera depth a weighted observation may have"""
    _fields_ = [("scene", KpFitSceneCfg), ("z_near", C.c_float)]

    @classmethod
    def default(cls):
        c = cls()
        load_library().kp_fit_image_cfg_default(C.byref(c))
        return c


class KpFitImageObs(C.Structure):
    """mirror of kp_fit_image_obs: n_cams, camera_rows and the device arrays cam [camera_rows, C, 16], uv [R, C, K, 2], uv_w [R, C, K] (may be NULL)"""
    _fields_ = [("n_cams", C.c_int), ("camera_rows", C.c_int), ("cam", C.c_void_p), ("uv", C.c_void_p), ("uv_w", C.c_void_p)]


class KpFitImageOut(C.Structure):
    """mirror of kp_fit_image_out: the device rows kp_sim_fit_image fills (dq, pt_err and uv_err may be NULL)"""
    _fields_ = [(k, C.c_void_p) for k in ("qpos", "info", "dq", "pt_err", "uv_err")]


# the columns of KpSim.fit_image's info rows: FIT_SCENE_INFO's (status 2: a weighted observation behind z_near at the start), then the reprojection
# figures at the result over the weighted observations (pixels; their number; the smallest camera depth)
FIT_IMAGE_INFO = {**FIT_SCENE_INFO, "max_euv": 16, "rms_euv": 17, "n_uv": 18, "min_depth": 19}
MAX_CAMS = 8


class KpEstimateCfg(C.Structure):
    """mirror of kp_estimate_cfg (host side): the candidates' reach, the weights of the residual force / moment, the multiplier penalty, the friction
    coefficient (0: the model's) and the Newton iterations of kp_sim_estimate_contacts"""
    _fields_ = [(k, C.c_float) for k in ("reach", "w_f", "w_m", "rho", "mu")] + [("n_iters", C.c_int)]

    @classmethod
    def default(cls, model):
        """kp_estimate_cfg_default for a KpModel: reach 0.03 m, w_f = 1 / (m g)^2, w_m = 1 / (m g x 1 m)^2, rho = 1e-3 w_f, mu 0, n_iters 20"""
        c = cls()
        load_library().kp_estimate_cfg_default(model.h, C.byref(c))
        return c


class KpEstimateOut(C.Structure):
    """mirror of kp_estimate_out: the device arrays kp_sim_estimate_contacts fills (each may be NULL, not all)"""
    _fields_ = [(k, C.c_void_p) for k in ("qfrc_inverse", "qfrc_contact", "contact", "lambda", "resid", "net_wrench", "ncon", "info")]


# outputs of KpSim.estimate_contacts: name -> (trailing shape, dtype), in kp_estimate_out's order
ESTIMATE_OUTPUTS = {"qfrc_inverse": ((75,), torch.float32), "qfrc_contact": ((75,), torch.float32), "contact": ((64, 12), torch.float32),
                    "lambda": ((64, 4), torch.float32), "resid": ((6,), torch.float32), "net_wrench": ((6,), torch.float32), "ncon": ((), torch.int32),
                    "info": ((8,), torch.float32)}
# the columns of an info row: name -> index; status: 0 ok, 1 non-finite input (zero rows), bit 2 possibly truncated (64 candidates), bit 4 not converged
ESTIMATE_INFO = {"cost0": 0, "cost": 1, "iters": 2, "active": 3, "f_norm": 4, "searches": 5, "reserved": 6, "status": 7}


class KinPolyNativeError(RuntimeError):
    pass


_V, _I, _F, _D, _S = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_char_p      # handles and device / host arrays are all void*
_PI = C.POINTER(C.c_int)
_CTX, _RW, _PRE, _POST, _UST, _UCFG, _EXT, _STYLE = (C.POINTER(k) for k in (KpCtx, KpRewardCfg, KpRecordPre, KpRecordPost, KpUhcState, KpUhcCfg, KpObsExt, KpRenderStyle))
# every symbol include/kinpoly_sim.h declares: symbol -> (restype, argtypes).  load_library types them all from here, and tests check the header against it.
_SIGNATURES = {
    "kp_last_error": (_S, []), "kp_version": (_S, []),
    "kp_model_load": (_V, [_S]), "kp_model_compile": (_I, [_S, _S, _S]), "kp_model_load_xml": (_V, [_S, _S]), "kp_model_free": (None, [_V]),
    "kp_model_set_option": (_I, [_V, _S, _D]), "kp_model_get_option": (_D, [_V, _S]),
    "kp_sim_create": (_V, [_V, _I, _I, _V]), "kp_sim_destroy": (None, [_V]), "kp_sim_n_envs": (_I, [_V]), "kp_sim_set_stream": (_I, [_V, _V]),
    "kp_sim_status_device": (_V, [_V]), "kp_sim_contacts": (_I, [_V, _V]), "kp_sim_mass_matrix": (_I, [_V, _V, _V]),
    "kp_sim_set_state": (_I, [_V, _V, _V, _V]), "kp_sim_set_full_state": (_I, [_V, _V, _V, _V, _V, _V]), "kp_sim_set_target": (_I, [_V, _V, _V]),
    "kp_sim_set_objects": (_I, [_V, _V, _V]), "kp_sim_set_obj_state": (_I, [_V, _V, _V, _V]),
    "kp_sim_apply_impulse": (_I, [_V, _V, _V, _V, _V, _V]),
    "kp_sim_contact_forces": (_I, [_V, _I, _V, _V, _V]),      # handle, actuation, act, env_mask, kp_contact_out*
    "kp_sim_inverse_dynamics": (_I, [_V, _I, _V, _V, _V, _V, _V]),      # handle, n_rows, qpos, qvel, qacc, obj_qpos, kp_invdyn_out*
    "kp_sim_body_motion": (_I, [_V, _I, _V, _V, _V, _V]),      # handle, n_rows, qpos, qvel, qacc, kp_motion_out*
    "kp_sim_point_jacobian": (_I, [_V, _I, _V, _V, _V, _V]),      # handle, n_rows, qpos, body, offset, J
    "kp_fit_cfg_default": (None, [C.POINTER(KpFitCfg)]),
    "kp_sim_fit_pose": (_I, [_V, _I, _V, _V, _V]),      # handle, n_rows, kp_fit_in*, kp_fit_cfg*, kp_fit_out*
    "kp_fit_points_cfg_default": (None, [C.POINTER(KpFitPointsCfg)]),
    "kp_sim_fit_points": (_I, [_V, _I, _V, _V, _V, _V]),      # handle, n_rows, kp_marker_set*, kp_fit_points_in*, kp_fit_points_cfg*, kp_fit_points_out*
    "kp_fit_scene_cfg_default": (None, [C.POINTER(KpFitSceneCfg)]),
    "kp_sim_fit_scene": (_I, [_V, _I, _V, _V, _V, _V, _V]),      # handle, n_rows, kp_marker_set*, kp_fit_points_in*, obj_qpos, kp_fit_scene_cfg*, kp_fit_scene_out*
    "kp_fit_image_cfg_default": (None, [C.POINTER(KpFitImageCfg)]),
    # handle, n_rows, kp_marker_set*, kp_fit_points_in*, obj_qpos, kp_fit_image_obs*, kp_fit_image_cfg*, kp_fit_image_out*
    "kp_sim_fit_image": (_I, [_V, _I, _V, _V, _V, _V, _V, _V]),
    "kp_estimate_cfg_default": (None, [_V, C.POINTER(KpEstimateCfg)]),
    "kp_sim_estimate_contacts": (_I, [_V, _I, _V, _V, _V, _V, _V, _V]),      # handle, n_rows, qpos, qvel, qacc, obj_qpos, kp_estimate_cfg*, kp_estimate_out*
    "kp_sim_fk": (_I, [_V, _I, _V, _V, _V, _V, _V, _V]), "kp_sim_fk_backward": (_I, [_V, _I, _V, _V, _V, _V, _V]),
    "kp_sim_pose_contacts": (_I, [_V, _I, _V, _V, _V, _F, _V, _V, _V]),
    # the offscreen renderer (kp_render.hip); kp_model_hull_planes is host only
    "kp_model_hull_planes": (_I, [_V, _V, _V]), "kp_render_style_default": (None, [_STYLE]),
    "kp_sim_render": (_I, [_V, _I, _I, _V, _V, _V, _V, _I, _I, _I, _STYLE, _V, _V, _V]),
    # the egocentric renderer (kp_render_ego.hip): A side, B side, camera_rows, width, height, hide_body, style, grid, six outputs
    "kp_sim_render_ego": (_I, [_V, _I, _I, _V, _V, _V, _V, _V, _V, _V, _V, _I, _I, _I, _I, _STYLE, _I, _I, _V, _V, _V, _V, _V, _V]),
    "kp_sim_step_ctrl": (_I, [_V, _V, _I, _V]), "kp_sim_step_ctrl_base": (_I, [_V, _V, _I, _V, _V]), "kp_sim_step_kin": (_I, [_V, _V, _V]),
    "kp_sim_step_head": (_I, [_V, _V]), "kp_sim_step_begin": (_I, [_V]),
    "kp_sim_obs_cc": (_I, [_V, _V, _V, _V, _F]), "kp_sim_obs_cc_ex": (_I, [_V, _V, _V, _V, _F, _V]), "kp_sim_cc_obs_dim": (_I, [_V]),
    "kp_sim_obs_ar": (_I, [_V, _CTX, _V]), "kp_sim_ar_obs_dim": (_I, [_V]),
    "kp_field_dim": (_I, [_I]), "kp_sim_get": (_I, [_V, _I, _V]), "kp_sim_field_device": (_V, [_V, _I]),
    "kp_sim_term_reward": (_I, [_V, _CTX, _RW, _V, _V, _V, _V]),
    "kp_sim_post_step": (_I, [_V, _CTX, _RW, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "kp_sim_term_reward_v2": (_I, [_V, _CTX, C.POINTER(KpRewardCfgV2), _V, _V, _V, _V]),
    "kp_sim_post_step_v2": (_I, [_V, _CTX, C.POINTER(KpRewardCfgV2), _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "kp_sim_reset_rows": (_I,[_V, _V, _V, _V, _V, _V, _I, _V, _I, _V, _V, _V]),
    "kp_sim_diag": (_I, [_V, _V]), "kp_sim_lean_state": (_I, [_V, _V]), "kp_sim_launch_cost": (_I, [_V, _V]), "kp_job_schedule": (_I, [_I, _I, _I, _PI]),
    "kp_sim_last_step_seconds": (_D, [_V]), "kp_sim_timing_reset": (_I, [_V]), "kp_sim_timing_mean_seconds": (_D, [_V, _PI]),
    "kp_sim_phase_cycles": (_I, [_V, C.POINTER(_D)]), "kp_sim_phase_cycles_env": (_I, [_V, _V]),
    "kp_takes_create": (_V, [_V, _V, _I, _V, _I, _D]), "kp_takes_destroy": (None, [_V]),
    "kp_takes_create_obj": (_V, [_V, _V, _V, _I, _V, _I, _D]), "kp_takes_has_objects": (_I, [_V]),
    "kp_takes_table": (_I, [_V, _S, C.POINTER(_V), _PI, _PI]), "kp_takes_info": (_I, [_V, _PI, _PI, _V]),
    "kp_sim_uhc_track": (_I, [_V, _V, _UST, _UCFG, _V, _V, _V, _V, _V, _V, _V, _V]), "kp_sim_uhc_assign": (_I, [_V, _V, _UST, _UCFG, _V, _V, _V, _I, _V]),
    "kp_uhc_reward_info_dim": (_I, [_I]), "kp_sim_uhc_track_r": (_I, [_V, _V, _UST, C.POINTER(KpUhcCfgR), _V, _V, _V, _V, _V, _V, _V, _V]),
    # stand-alone kernels (no kp_sim): sizes, device arrays, ..., stream
    "kp_pool_advance": (_I, [_I, _I, _V, _V, _V, _V, _V]),
    "kp_rollout_record_pre": (_I, [_PRE, _V]), "kp_rollout_record_post": (_I, [_POST, _V]),
    "kp_rollout_record_pre_w": (_I, [_PRE, _I, _V]), "kp_rollout_record_post_w": (_I, [_POST, _I, _V]),
    "kp_mcp_compose": (_I, [_I, _I, _I, _V, _V, _V, _I, _V, _V, _V]),
    "kp_mcp_tail": (_I, [_I, _I, _I, _I, _V, _V, _V, _I, _V, _V, _V, _I, _V, _V, _V]),
    "kp_kin_advance": (_I, [_I, _V, _V, _F, _V, _V, _V]), "kp_gru_cell_step": (_I, [_I, _I, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "kp_gae": (_I, [_I, _I, _V, _V, _V, _F, _F, _V, _V, _V]), "kp_gae_bootstrap": (_I, [_I, _I, _V, _V, _V, _V, _F, _F, _V, _V, _V]),
    "kp_gru_gates_forward": (_I, [_I, _I, _V, _V, _V, _V, _V, _V, _V]), "kp_gru_gates_backward": (_I, [_I, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    # the backward side of the kinematic roll-out (kp_kin_tape.hip)
    "kp_kin_advance_backward": (_I, [_I, _V, _V, _F, _V, _V, _V, _V, _V]),
    "kp_sim_obs_ar_backward": (_I, [_V, _CTX, _I, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "kp_sim_fk_head_backward": (_I, [_V, _I, _V, _V, _V, _V, _V, _V, _V, _V]),
    # the observation with a context / `of` block (kp_obs_ctx.hip)
    "kp_sim_obs_ar_ex": (_I, [_V, _CTX, _EXT, _V]),
    "kp_sim_obs_ar_ex_backward": (_I, [_V, _CTX, _EXT, _I, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    # the sampler's records at a wide row, and the ring refill of the two wide context tables
    "kp_rollout_record_pre_x": (_I, [_PRE, _I, _I, _I, _V]), "kp_rollout_record_post_x": (_I, [_POST, _I, _I, _I, _V]),
    "kp_ctx_rows_write": (_I, [_I, _I, _I, _I, _I, _I, _V, _V, _V, _V, _V, _V, _V]),
}
ABI_SYMBOLS = list(_SIGNATURES)


def load_library(path: str | None = None):
    """dlopen the in-tree extension (never builds implicitly on a GPU box: the .so must be there)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("KP_SIM_LIBRARY") or _build.LIB      # KP_SIM_LIBRARY: another build of the same ABI (A/B measurements)
    if not os.path.exists(path):
        raise KinPolyNativeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(path)
    for sym, (restype, argtypes) in _SIGNATURES.items():
        f = getattr(L, sym)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise KinPolyNativeError(f"{what}: {load_library().kp_last_error().decode()}")


def compile_model_native(xml_path: str, uhc_yml: str | None, out_kpm: str):
    """kp_model_compile: the XML + STL + uhc.yml -> blob compiler behind the C ABI (kinpoly_amd/csrc/kp_compile.hpp; needs no GPU)."""
    L = load_library()
    _check(L.kp_model_compile(xml_path.encode(), None if uhc_yml is None else uhc_yml.encode(), out_kpm.encode()), "kp_model_compile")


class KpModel:
    def __init__(self, kpm_path: str = DEFAULT_KPM, xml: tuple | None = None, **options):
        """kpm_path: a compiled blob; or xml=(xml_path, uhc_yml_path or None): compile the reference's scene on the spot (kp_model_load_xml)."""
        self.L = load_library()
        self.kpm_path = None if xml is not None else kpm_path      # the blob's tables for host-side consumers (read_kpm)
        if xml is not None:
            self.h = self.L.kp_model_load_xml(xml[0].encode(), None if xml[1] is None else xml[1].encode())
        else:
            self.h = self.L.kp_model_load(kpm_path.encode())
        if not self.h:
            raise KinPolyNativeError(f"kp_model_load: {self.L.kp_last_error().decode()}")
        for k, v in options.items():
            self.set_option(k, v)

    def hull_planes(self):
        """The face planes of the 24 hulls (kp_model_hull_planes; host only, no device needed): (planes [n, 4] float32 = unit outward normal and d
        in the body frame, n.x <= d inside; adr [25] int32 = first plane of every body)."""
        n = self.L.kp_model_hull_planes(self.h, None, None)
        if n < 0:
            raise KinPolyNativeError(f"kp_model_hull_planes: {self.L.kp_last_error().decode()}")
        planes, adr = np.empty((n, 4), np.float32), np.empty(NBODY + 1, np.int32)
        self.L.kp_model_hull_planes(self.h, planes.ctypes.data_as(C.c_void_p), adr.ctypes.data_as(C.c_void_p))
        return planes, adr

    def set_option(self, name, value):
        _check(self.L.kp_model_set_option(self.h, name.encode(), float(value)), "kp_model_set_option")

    def get_option(self, name):
        return self.L.kp_model_get_option(self.h, name.encode())

    def __del__(self):
        try:
            self.L.kp_model_free(self.h)
        except Exception:
            pass


def _dev(name, t: torch.Tensor | None, shape, dtype=torch.float32):
    """Device pointer of t (None -> NULL) after THE check every entry point's arrays pass: a contiguous `dtype` device tensor of `shape`, where a None
    in `shape` stands for any size (the row count of a table) and shape = None for any shape.  The kernels index with fixed row widths: anything else would be read out of bounds."""
    if t is None:
        return None
    fits = shape is None or (t.dim() == len(shape) and all(w is None or w == d for w, d in zip(shape, t.shape)))
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and fits):
        want = "any shape" if shape is None else "shape (" + ", ".join("*" if w is None else str(w) for w in shape) + ")"
        raise ValueError(f"{name}: expected a contiguous {dtype} device tensor of {want}, got {t.dtype} {tuple(t.shape)} "
                         f"{'contiguous' if t.is_contiguous() else 'strided'} on {t.device}")
    return C.c_void_p(t.data_ptr())


def _ptr(t, n, dim):
    return _dev("tensor", t, (n, dim))


def _mask_ptr(m, n):
    return _dev("env_mask", m, (n,), torch.uint8)


def _device_view(ptr, shape, device, typestr="<f4") -> torch.Tensor:
    """zero-copy tensor over device memory the library owns (valid for the life of the handle that returned ptr)"""
    iface = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3, "strides": None}
    return torch.as_tensor(type("_KpDeviceView", (), {"__cuda_array_interface__": iface})(), device=device)


# ---- the rows tools (inverse_dynamics, estimate_contacts, body_motion, point_jacobian, fit_pose; contact_forces for its outputs): what their bindings
# share.  Plain functions on tensors of any device (tests/test_rows_binding_cpu.py runs them without the library); the methods add _dev's device check.
_JAC_OUTPUTS = {"J": ((6, NV), torch.float32)}
_FIT_OUTPUTS = {"qpos": ((NQ,), torch.float32), "info": ((8,), torch.float32), "dq": ((NV,), torch.float32)}      # in kp_fit_out's order


def fit_points_outputs(K: int) -> dict:
    """outputs of KpSim.fit_points for K points: name -> (trailing shape, dtype), in kp_fit_points_out's order"""
    return {"qpos": ((NQ,), torch.float32), "info": ((12,), torch.float32), "dq": ((NV,), torch.float32), "pt_err": ((int(K),), torch.float32)}


def fit_scene_outputs(K: int) -> dict:
    """outputs of KpSim.fit_scene for K points: fit_points_outputs' with info [16] (FIT_SCENE_INFO)"""
    return {**fit_points_outputs(K), "info": ((16,), torch.float32)}


def fit_image_outputs(K: int, n_cams: int) -> dict:
    """outputs of KpSim.fit_image for K points and n_cams cameras: fit_scene_outputs' with info [20] (FIT_IMAGE_INFO) and uv_err, in kp_fit_image_out's order"""
    return {**fit_scene_outputs(K), "info": ((20,), torch.float32), "uv_err": ((int(n_cams), int(K)), torch.float32)}


def marker_arrays(who, pt_body, pt_offset):
    """The marker set of a fit_points call as the host arrays kp_marker_set points at: body int32 [K], offset float32 [K, 3], after the entry point's
    own checks (K 0 .. 1024, bodies 0..23, finite offsets), so that a bad set is a ValueError before anything native runs."""
    body = np.asarray(pt_body)
    if body.ndim != 1 or (body.size and not np.issubdtype(body.dtype, np.integer)):
        raise ValueError(f"{who}: pt_body must be a 1-d integer array, got {body.dtype} {body.shape}")
    K = body.shape[0]
    off = np.asarray(pt_offset, np.float64)
    if K == 0:
        off = off.reshape(0, 3)
    if off.shape != (K, 3):
        raise ValueError(f"{who}: pt_offset must be ({K}, 3), got {off.shape}")
    if K > MAX_POINTS:
        raise ValueError(f"{who}: at most {MAX_POINTS} points, got {K}")
    if K and (body.min() < 0 or body.max() >= 24):
        raise ValueError(f"{who}: pt_body must lie in 0..23")
    off = np.ascontiguousarray(off, np.float32)
    if not np.all(np.isfinite(off)):
        raise ValueError(f"{who}: pt_offset must be finite")
    return np.ascontiguousarray(body, np.int32), off


def _motion_spec(qpos, qvel, qacc, obj_qpos=None):
    """the inputs of the tools that take a motion: _rows_inputs' list"""
    f32 = torch.float32
    return [("qpos", qpos, (NQ,), f32, True), ("qvel", qvel, (NV,), f32, False), ("qacc", qacc, (NV,), f32, False), ("obj_qpos", obj_qpos, (35,), f32, False)]


def _rows_want(who, want, table, arg="want") -> tuple:
    """the wanted output names as a tuple, after the check that they are some of `table`'s"""
    want = tuple(want)
    if not want or any(k not in table for k in want):
        raise ValueError(f"{who}: {arg} must name some of {tuple(table)}, got {want}")
    return want


def _rows_inputs(who, spec):
    """The inputs of a rows call, spec = [(name, tensor or None, tail shape, dtype, required)]: the first, qpos [..., 76], sets the leading shape, which the
    others must have too.  Returns lead, R = prod(lead) and the inputs flattened to [R, *tail] (None for an optional one that was not given)."""
    name0, qpos = spec[0][:2]
    if qpos.dim() < 1 or qpos.shape[-1] != NQ:
        raise ValueError(f"{who}: {name0} must be [..., {NQ}], got {tuple(qpos.shape)}")
    lead = tuple(qpos.shape[:-1])
    R = int(np.prod(lead, dtype=np.int64))
    flat = []
    for name, t, tail, _, required in spec:
        if t is None and required:
            raise ValueError(f"{who}: {name} is required")
        if t is not None and tuple(t.shape) != lead + tail:
            raise ValueError(f"{who}: {name} must be {lead + tail}, got {tuple(t.shape)}")
        flat.append(None if t is None else t.reshape((R,) + tail))
    return lead, R, flat


def _rows_ptrs(who, spec, flat) -> list:
    """the device pointers of _rows_inputs' rows: _dev's check of device, dtype and contiguity (the shapes are checked already; they go into its message)"""
    return [_dev(f"{who}: {name}", t, None if t is None else tuple(t.shape), dtype) for (name, _, _, dtype, _), t in zip(spec, flat)]


def _rows_outputs(R, table, want, device) -> dict:
    """the [R, *shape] outputs of `table` (name -> (trailing shape, dtype)) for the wanted names"""
    return {k: torch.empty((R, *table[k][0]), dtype=table[k][1], device=device) for k in want}


def _rows_struct(cls, table, out):
    """the C struct of output pointers, in the table's order: NULL for what was not wanted"""
    return cls(*[C.c_void_p(out[k].data_ptr()) if k in out else None for k in table])


def _rows_view(out, lead) -> dict:
    """the outputs of _rows_outputs with the leading shape of the inputs"""
    return {k: v.view(lead + tuple(v.shape[1:])) for k, v in out.items()}


class KpSim:
    """N batched environments on one GPU (one kp_sim handle)."""

    def __init__(self, model: KpModel, n_envs: int, device: int | torch.device = 0):
        if not torch.cuda.is_available():
            raise KinPolyNativeError("no HIP device visible: the simulator has no CPU fallback")
        self.model = model
        self.L = model.L
        self.n = int(n_envs)
        self.device = torch.device("cuda", device if isinstance(device, int) else (device.index or 0))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.h = self.L.kp_sim_create(model.h, self.n, self.device.index, C.c_void_p(stream))
        if not self.h:
            raise KinPolyNativeError(f"kp_sim_create: {self.L.kp_last_error().decode()}")
        self._stream = stream
        self.obs_ar_dim = int(self.L.kp_sim_ar_obs_dim(self.h))      # AR_OBS_DIM, or the width of the model's ar_obs_vel / ar_obs_head / ar_obs_action (ar_obs_dim)
        self.obs_ar_vel, self.obs_ar_head, self.obs_ar_action = (bool(model.get_option(k)) for k in ("ar_obs_vel", "ar_obs_head", "ar_obs_action"))
        self.cc_obs_dim = int(self.L.kp_sim_cc_obs_dim(self.h))      # CC_OBS_DIM, or the width of the model's cc_obs_* options (UhcConfig.obs_dim)
        self.cc_obs_phase = bool(model.get_option("cc_obs_phase")) and int(model.get_option("cc_obs_v")) == 0
        self.cc_action_dim = int(model.get_option("cc_action_dim"))

    def use_current_stream(self):
        """Enqueue all later calls on torch's current stream of this device (the caller orders the old and the new stream)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if stream != self._stream:
            _check(self.L.kp_sim_set_stream(self.h, C.c_void_p(stream)), "kp_sim_set_stream")
            self._stream = stream

    def status_tensor(self) -> torch.Tensor:
        """int32 [4] device view of the launch status words (kp_sim_status_device): [2] != 0 = a queue launch stalled."""
        if getattr(self, "_status", None) is None:
            self._status = _device_view(self.L.kp_sim_status_device(self.h), (4,), self.device, "<i4")
        return self._status

    def queue_counters(self) -> dict:
        """Counters of the last job-queue launch (host read): jobs claimed / published, jobs a wave kept instead of queueing, and the jobs the lean
        layout handed to kp_step_overflow_kernel (more contacts than EnvLdsLean::MAXCON)."""
        if getattr(self, "_qctr", None) is None:
            self._qctr = _device_view(self.L.kp_sim_status_device(self.h), (128,), self.device, "<i4")
        c = self._qctr.cpu().numpy()
        st = (C.c_int32 * 3)()
        _check(self.L.kp_sim_lean_state(self.h, C.cast(st, C.c_void_p)), "kp_sim_lean_state")
        return {"claimed": int(c[0]), "published": int(c[1]), "stalled": int(c[2]), "kept_by_their_wave": int(c[16]), "lean_overflow_jobs": int(c[64]),
                "lean_layout_next_launch": bool(st[0]), "fallbacks_to_full_layout": int(st[1]), "control_step_launches": int(st[2])}

    def record_contacts(self):
        """Arm the contact read-out (kp_sim_contacts): later step_ctrl launches keep the contact set of their last collision pass."""
        _check(self.L.kp_sim_contacts(self.h, None), "kp_sim_contacts")

    def contacts(self):
        """List over envs of dict(body, b2, dist [n], pos [n,3], normal [n,3]) of the last collision pass (after record_contacts())."""
        buf = np.zeros((self.n, 1 + 64 * 9), np.float32)
        _check(self.L.kp_sim_contacts(self.h, buf.ctypes.data_as(C.c_void_p)), "kp_sim_contacts")
        out = []
        for e in range(self.n):
            n = int(buf[e, 0]); r = buf[e, 1:1 + 9 * n].reshape(n, 9).astype(np.float64)
            out.append(dict(body=r[:, 0].astype(int), b2=r[:, 1].astype(int), dist=r[:, 2], pos=r[:, 3:6], normal=r[:, 6:9]))
        return out

    def mass_matrix(self):
        """(M [N,75,75], qfrc_bias [N,75]) of the state the derived quantities belong to (mj_fullM / data.qfrc_bias)."""
        M = torch.empty((self.n, 75, 75), dtype=torch.float32, device=self.device); b = self._new(75)
        _check(self.L.kp_sim_mass_matrix(self.h, C.c_void_p(M.data_ptr()), C.c_void_p(b.data_ptr())), "kp_sim_mass_matrix")
        return M, b

    def __del__(self):
        try:
            self.L.kp_sim_destroy(self.h)
        except Exception:
            pass

    def _new(self, dim):
        return torch.empty((self.n, dim), dtype=torch.float32, device=self.device)

    def set_state(self, qpos, qvel, env_mask=None):
        _check(self.L.kp_sim_set_state(self.h, _ptr(qpos, self.n, NQ), _ptr(qvel, self.n, NV), _mask_ptr(env_mask, self.n)), "kp_sim_set_state")

    def set_objects(self, obj_qpos, env_mask=None):
        _check(self.L.kp_sim_set_objects(self.h, _ptr(obj_qpos, self.n, 35), _mask_ptr(env_mask, self.n)), "kp_sim_set_objects")

    def set_obj_state(self, obj_qpos, obj_qvel, env_mask=None):
        _check(self.L.kp_sim_set_obj_state(self.h, _ptr(obj_qpos, self.n, 35), _ptr(obj_qvel, self.n, 30), _mask_ptr(env_mask, self.n)), "kp_sim_set_obj_state")

    def set_target(self, target_qpos, env_mask=None):
        _check(self.L.kp_sim_set_target(self.h, _ptr(target_qpos, self.n, NQ), _mask_ptr(env_mask, self.n)), "kp_sim_set_target")

    def step_ctrl(self, cc_action, n_substeps=15, env_mask=None):
        _check(self.L.kp_sim_step_ctrl(self.h, _ptr(cc_action, self.n, self.cc_action_dim), int(n_substeps), _mask_ptr(env_mask, self.n)), "kp_sim_step_ctrl")

    def step_ctrl_base(self, cc_action, base_qpos, n_substeps=15, env_mask=None):
        """step_ctrl with compute_torque's base pose read from base_qpos [N,76] (kp_sim_step_ctrl_base); the stored target is left alone"""
        _check(self.L.kp_sim_step_ctrl_base(self.h, _ptr(cc_action, self.n, self.cc_action_dim), int(n_substeps), _mask_ptr(env_mask, self.n),
                                            _ptr(base_qpos, self.n, NQ)), "kp_sim_step_ctrl_base")

    def uhc_track(self, takes, st, cfg, cc_action, reward, info, body_diff, fail, end, done, percent):
        """the tail of HumanoidEnv.step in one launch (kp_sim_uhc_track); st: KpUhcState, cfg: KpUhcCfg; outputs are caller-owned device tensors"""
        _check(self.L.kp_sim_uhc_track(self.h, takes.h, C.byref(st), C.byref(cfg), _ptr(cc_action, self.n, self.cc_action_dim), C.c_void_p(reward.data_ptr()),
                                       _ptr(info, self.n, 5), C.c_void_p(body_diff.data_ptr()), _mask_ptr(fail, self.n), _mask_ptr(end, self.n), _mask_ptr(done, self.n),
                                       C.c_void_p(percent.data_ptr())), "kp_sim_uhc_track")

    def uhc_track_r(self, takes, st, cfg, cc_action, reward, info, body_diff, fail, end, done, percent):
        """uhc_track with the reward function cfg.reward_id names (kp_sim_uhc_track_r); cfg: KpUhcCfgR; info [N, uhc_reward_info_dim(cfg.reward_id)]"""
        _check(self.L.kp_sim_uhc_track_r(self.h, takes.h, C.byref(st), C.byref(cfg), _ptr(cc_action, self.n, self.cc_action_dim), C.c_void_p(reward.data_ptr()),
                                         _ptr(info, self.n, uhc_reward_info_dim(cfg.reward_id)), C.c_void_p(body_diff.data_ptr()), _mask_ptr(fail, self.n),
                                         _mask_ptr(end, self.n), _mask_ptr(done, self.n), C.c_void_p(percent.data_ptr())), "kp_sim_uhc_track_r")

    def uhc_assign(self, takes, st, cfg, env_mask=None, take_ids=None, start=None, keep_t=False, noise=None):
        """reset_model / fail_safe for the masked envs (kp_sim_uhc_assign); take_ids / start: host int32 arrays [N] or None"""
        ids = None if take_ids is None else np.ascontiguousarray(take_ids, np.int32)
        st0 = None if start is None else np.ascontiguousarray(start, np.int32)
        for a in (ids, st0):
            if a is not None and a.shape != (self.n,):
                raise ValueError(f"uhc_assign: take_ids / start must have shape ({self.n},)")
        _check(self.L.kp_sim_uhc_assign(self.h, takes.h, C.byref(st), C.byref(cfg), _mask_ptr(env_mask, self.n), None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                        None if st0 is None else st0.ctypes.data_as(C.c_void_p), int(bool(keep_t)), _ptr(noise, self.n, NU)), "kp_sim_uhc_assign")

    def step_head(self, kin_action):
        """step_begin + step_kin + set_target(step_kin's result) in one launch (kp_sim_step_head)"""
        _check(self.L.kp_sim_step_head(self.h, _ptr(kin_action, self.n, KIN_ACTION_DIM)), "kp_sim_step_head")

    def step_kin(self, kin_action, out=None):
        out = self._new(NQ) if out is None else out
        _check(self.L.kp_sim_step_kin(self.h, _ptr(kin_action, self.n, KIN_ACTION_DIM), _ptr(out, self.n, NQ)), "kp_sim_step_kin")
        return out

    def obs_cc(self, out=None, zf_mean=None, zf_std=None, clip=0.0, phase=None):
        """The UHC observation of the handle's layout (kp_sim_obs_cc_ex): [N, cc_obs_dim]; 784 = get_full_obs_v1 for a default model.
        phase: float [N] device tensor cur_t / expert len, required exactly when the layout has obs_v 0's phase slot."""
        out = self._new(self.cc_obs_dim) if out is None else out
        zm, zs = (_dev("ZFilter mean / std", z if z is None or not z.is_contiguous() else z.view(-1), (self.cc_obs_dim,)) for z in (zf_mean, zf_std))
        ph = None if phase is None else _ptr(phase.view(self.n, 1), self.n, 1)
        _check(self.L.kp_sim_obs_cc_ex(self.h, _ptr(out, self.n, self.cc_obs_dim), zm, zs, float(clip), ph), "kp_sim_obs_cc_ex")
        return out

    def get(self, field: str, out=None):
        fid = FIELDS[field]
        dim = self.L.kp_field_dim(fid)
        out = self._new(dim) if out is None else out
        _check(self.L.kp_sim_get(self.h, fid, _ptr(out, self.n, dim)), "kp_sim_get")
        return out

    def view(self, field: str) -> torch.Tensor:
        """Zero-copy [N, dim] device view of a STORED field (kp_sim_field_device: qpos, qvel, xpos, ..., obj_qpos; not the derived read-outs).  The
        view follows the simulator: it shows the state as of the work enqueued before the reader on the same stream, and is overwritten by the next step --
        for a consumer that copies the rows it needs in its own launch (the sampler's record kernel), not for keeping."""
        cache = self.__dict__.setdefault("_views", {})
        if field not in cache:
            fid = FIELDS[field]
            ptr = self.L.kp_sim_field_device(self.h, fid)
            if not ptr:
                raise KinPolyNativeError(f"kp_sim_field_device: '{field}' is not a stored field")
            cache[field] = _device_view(ptr, (self.n, self.L.kp_field_dim(fid)), self.device)
        return cache[field]

    def set_full_state(self, qpos, qvel, qpos_d, qvel_d, env_mask=None):
        _check(self.L.kp_sim_set_full_state(self.h, _ptr(qpos, self.n, NQ), _ptr(qvel, self.n, NV), _ptr(qpos_d, self.n, NQ),
                                            _ptr(qvel_d, self.n, NV), _mask_ptr(env_mask, self.n)), "kp_sim_set_full_state")

    def apply_impulse(self, entity, impulse, offset=None, env_mask=None, want_dqvel=False):
        """An impulse push between two control steps (kp_sim_apply_impulse): qvel += M(qpos)^-1 J^T [p; l] per env.  entity: int32 [N] device tensor
        (0..23 body, 24 + k object slot, anything else: no push); impulse [N,6] = (p in N s, l in N m s), world axes; offset [N,3] or None: the
        point on the entity, in its own frame; env_mask uint8 [N] or None.  want_dqvel: return the humanoid's velocity jump [N,75]."""
        dq = self._new(NV) if want_dqvel else None
        _check(self.L.kp_sim_apply_impulse(self.h, _dev("entity", entity, (self.n,), torch.int32), _dev("offset", offset, (self.n, 3)),
                                           _dev("impulse", impulse, (self.n, 6)), _mask_ptr(env_mask, self.n), _ptr(dq, self.n, NV)), "kp_sim_apply_impulse")
        return dq

    def contact_forces(self, action=None, torque=None, env_mask=None, want=tuple(CONTACT_OUTPUTS)) -> dict:
        """Contact forces of the STORED state (kp_sim_contact_forces): the mj_forward of substep 0 of the control step step_ctrl would run next, without
        the integration; nothing the handle stores changes.  action [N, cc_action_dim]: the controller's torque for that cc_action (mode 2); torque
        [N,75] = qfrc_applied[0:6] ++ ctrl[69], as given (mode 1); neither: no actuation (mode 0).  want: names of CONTACT_OUTPUTS.  Returns a dict of
        device tensors: ncon int32 [N]; contact [N,64,12] = A, B, dist, pos[3], normal[3] (into A), force[3] (on A); wrench [N,26,6] = force, torque about
        the world origin per entity (24 bodies, 2 object slots); qfrc_constraint, qacc, torque [N,75]; obj_qacc [N,2,6]."""
        if action is not None and torque is not None:
            raise ValueError("contact_forces: action and torque are mutually exclusive")
        want = _rows_want("contact_forces", want, CONTACT_OUTPUTS)
        mode, act = (2, _dev("action", action, (self.n, self.cc_action_dim))) if action is not None else (1, _dev("torque", torque, (self.n, NV))) if torque is not None else (0, None)
        out = _rows_outputs(self.n, CONTACT_OUTPUTS, want, self.device)
        _check(self.L.kp_sim_contact_forces(self.h, mode, act, _mask_ptr(env_mask, self.n), C.byref(_rows_struct(KpContactOut, CONTACT_OUTPUTS, out))), "kp_sim_contact_forces")
        return out

    def inverse_dynamics(self, qpos, qvel=None, qacc=None, obj_qpos=None, want=("qfrc_inverse",)) -> dict:
        """Inverse dynamics of motion rows (kp_sim_inverse_dynamics, mj_inverse's data.qfrc_inverse): qpos [..., 76], qvel / qacc [..., 75] or None
        (zeros), obj_qpos [..., 35] or None (objects within 50 m are static obstacles), any leading shape, the same on every input.  Nothing the
        handle stores is read or changed.  want: names of INVDYN_OUTPUTS.  Returns a dict of device tensors with that leading shape: qfrc_inverse,
        qfrc_constraint, qfrc_bias [..., 75] (qfrc_applied[0:6] ++ ctrl[69] coordinates); contact [..., 64, 12] = A, B (-1), dist, pos[3], normal[3],
        force[3]; net_wrench [..., 6] = contact force on the humanoid, torque about the world origin; ncon int32 [...]."""
        want = _rows_want("inverse_dynamics", want, INVDYN_OUTPUTS)
        spec = _motion_spec(qpos, qvel, qacc, obj_qpos)
        lead, R, rows = _rows_inputs("inverse_dynamics", spec)
        ins = _rows_ptrs("inverse_dynamics", spec, rows)
        out = _rows_outputs(R, INVDYN_OUTPUTS, want, self.device)
        if R > 0:                # no rows: nothing to launch (and an empty tensor has no address to hand over)
            _check(self.L.kp_sim_inverse_dynamics(self.h, R, *ins, C.byref(_rows_struct(KpInvDynOut, INVDYN_OUTPUTS, out))), "kp_sim_inverse_dynamics")
        return _rows_view(out, lead)

    def estimate_contacts(self, qpos, qvel=None, qacc=None, obj_qpos=None, cfg: KpEstimateCfg | None = None, want=("qfrc_inverse",)) -> dict:
        """Contact forces estimated from kinematics (kp_sim_estimate_contacts): the forces inside the friction pyramids of the points within cfg.reach of
        a surface that best explain the rows' root residual.  Inputs as inverse_dynamics: qpos [..., 76], qvel / qacc [..., 75] or None (zeros), obj_qpos
        [..., 35] or None, any leading shape.  cfg: a KpEstimateCfg (None: KpEstimateCfg.default(self.model)).  want: names of ESTIMATE_OUTPUTS.
        Returns a dict of device tensors with that leading shape: qfrc_inverse, qfrc_contact [..., 75]; contact [..., 64, 12] (contact_forces' rows,
        B = -1, the estimated force); lambda [..., 64, 4]; resid [..., 6] (force, moment about the root position, world axes); net_wrench [..., 6] (about
        the world origin); ncon int32 [...]; info [..., 8] (ESTIMATE_INFO).  Nothing the handle stores is read or changed."""
        want = _rows_want("estimate_contacts", want, ESTIMATE_OUTPUTS)
        spec = _motion_spec(qpos, qvel, qacc, obj_qpos)
        lead, R, rows = _rows_inputs("estimate_contacts", spec)
        ins = _rows_ptrs("estimate_contacts", spec, rows)
        cfg = KpEstimateCfg.default(self.model) if cfg is None else cfg
        out = _rows_outputs(R, ESTIMATE_OUTPUTS, want, self.device)
        if R > 0:
            _check(self.L.kp_sim_estimate_contacts(self.h, R, *ins, C.byref(cfg), C.byref(_rows_struct(KpEstimateOut, ESTIMATE_OUTPUTS, out))), "kp_sim_estimate_contacts")
        return _rows_view(out, lead)

    def body_motion(self, qpos, qvel=None, qacc=None, outputs=tuple(MOTION_OUTPUTS)) -> dict:
        """Body velocities and accelerations, momentum and energy of motion rows (kp_sim_body_motion): qpos [..., 76], qvel / qacc [..., 75] or None
        (zeros), any leading shape, the same on every input.  Nothing the handle stores is read or changed.  outputs: names of MOTION_OUTPUTS.  Returns
        a dict of device tensors with that leading shape, world axes: body_vel [..., 24, 6] = angular, linear velocity of the body frame origin;
        body_acc [..., 24, 6] = angular, classical linear acceleration of it; body_com_vel [..., 24, 3]; centroid [..., 18] (CENTROID_FIELDS: com,
        com_vel, L_com, ke, pe, com_acc, Ldot_com, mass)."""
        want = _rows_want("body_motion", outputs, MOTION_OUTPUTS, "outputs")
        spec = _motion_spec(qpos, qvel, qacc)[:3]
        lead, R, rows = _rows_inputs("body_motion", spec)
        ins = _rows_ptrs("body_motion", spec, rows)
        out = _rows_outputs(R, MOTION_OUTPUTS, want, self.device)
        if R > 0:
            _check(self.L.kp_sim_body_motion(self.h, R, *ins, C.byref(_rows_struct(KpMotionOut, MOTION_OUTPUTS, out))), "kp_sim_body_motion")
        return _rows_view(out, lead)

    def point_jacobian(self, qpos, body, offset=None) -> torch.Tensor:
        """mj_jac on rows (kp_sim_point_jacobian): qpos [..., 76], body int32 [...] (0..23; anything else: a zero row), offset [..., 3] in the body's
        frame or None (the body origin), any leading shape.  Returns J [..., 6, 75]: rows 0..2 the world velocity of the point, rows 3..5 the body's
        world angular velocity, per unit dof velocity (qvel order).  Nothing the handle stores is read or changed."""
        spec = [("qpos", qpos, (NQ,), torch.float32, True), ("body", body, (), torch.int32, True), ("offset", offset, (3,), torch.float32, False)]
        lead, R, rows = _rows_inputs("point_jacobian", spec)
        ins = _rows_ptrs("point_jacobian", spec, rows)
        out = _rows_outputs(R, _JAC_OUTPUTS, ("J",), self.device)
        if R > 0:
            _check(self.L.kp_sim_point_jacobian(self.h, R, *ins, C.c_void_p(out["J"].data_ptr())), "kp_sim_point_jacobian")
        return _rows_view(out, lead)["J"]

    def fit_pose(self, qpos0, tgt_pos, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None, cfg: KpFitCfg | None = None, want_dq=False) -> dict:
        """Pose fitting on rows (kp_sim_fit_pose): Levenberg-Marquardt from qpos0 [..., 76] towards the body positions tgt_pos [..., 24, 3] and, where
        given, orientations tgt_quat [..., 24, 4], weighted by w_pos / w_rot [..., 24] (None: ones / zeros), with the hinge prior q_prior / w_prior
        [..., 69] (both or neither); any leading shape, the same on every input.  cfg: a KpFitCfg (None: KpFitCfg.default()).  Returns a dict of device
        tensors: qpos [..., 76], info [..., 8] (FIT_INFO: cost0, cost, accepted, mu, max_epos, max_erot, dq_inf, status) and, with want_dq, dq
        [..., 75] of the last solve.  Nothing the handle stores is read or changed."""
        if (q_prior is None) != (w_prior is None):
            raise ValueError("fit_pose: q_prior and w_prior go together")
        f32 = torch.float32
        spec = [("qpos0", qpos0, (NQ,), f32, True), ("tgt_pos", tgt_pos, (24, 3), f32, True), ("tgt_quat", tgt_quat, (24, 4), f32, False), ("w_pos", w_pos, (24,), f32, False),
                ("w_rot", w_rot, (24,), f32, False), ("q_prior", q_prior, (69,), f32, False), ("w_prior", w_prior, (69,), f32, False)]
        lead, R, rows = _rows_inputs("fit_pose", spec)
        ins = _rows_ptrs("fit_pose", spec, rows)
        cfg = KpFitCfg.default() if cfg is None else cfg
        out = _rows_outputs(R, _FIT_OUTPUTS, ("qpos", "info", "dq") if want_dq else ("qpos", "info"), self.device)
        if R > 0:
            _check(self.L.kp_sim_fit_pose(self.h, R, C.byref(KpFitIn(*ins)), C.byref(cfg), C.byref(_rows_struct(KpFitOut, _FIT_OUTPUTS, out))), "kp_sim_fit_pose")
        return _rows_view(out, lead)

    def fit_points(self, qpos0, pt_body, pt_offset, pt_tgt=None, pt_w=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None,
                   cfg: KpFitPointsCfg | None = None, want=("qpos", "info")) -> dict:
        """Pose fitting to points at body offsets, with a floor term (kp_sim_fit_points): Levenberg-Marquardt from qpos0 [..., 76].  The marker set
        is HOST data shared by all rows: pt_body [K] integers 0..23, pt_offset [K, 3] in the body frames (K 0 .. 1024).  Device rows of any leading
        shape, the same on every input: pt_tgt [..., K, 3] (required when K > 0), pt_w [..., K] or None (ones; a point with w <= 0 is skipped and its
        target may be NaN), tgt_pos [..., 24, 3] or None (no origin term), tgt_quat, w_pos, w_rot, q_prior, w_prior as in fit_pose.  At least one of
        K > 0 and tgt_pos.  cfg: a KpFitPointsCfg (None: its default, the floor term off).  want: names of fit_points_outputs(K).  Returns a dict of
        device tensors: qpos [..., 76], info [..., 12] (FIT_POINTS_INFO), dq [..., 75], pt_err [..., K] (the caller's point order).  Nothing the
        handle stores is read or changed."""
        body, off = marker_arrays("fit_points", pt_body, pt_offset)
        K = body.shape[0]
        table = fit_points_outputs(K)
        want = _rows_want("fit_points", want, table)
        if (q_prior is None) != (w_prior is None):
            raise ValueError("fit_points: q_prior and w_prior go together")
        if K == 0 and tgt_pos is None:
            raise ValueError("fit_points: nothing to fit (no points and no tgt_pos)")
        f32 = torch.float32
        spec = [("qpos0", qpos0, (NQ,), f32, True), ("pt_tgt", pt_tgt, (K, 3), f32, K > 0), ("pt_w", pt_w, (K,), f32, False), ("tgt_pos", tgt_pos, (24, 3), f32, False),
                ("tgt_quat", tgt_quat, (24, 4), f32, False), ("w_pos", w_pos, (24,), f32, False), ("w_rot", w_rot, (24,), f32, False),
                ("q_prior", q_prior, (69,), f32, False), ("w_prior", w_prior, (69,), f32, False)]
        lead, R, rows = _rows_inputs("fit_points", spec)
        ins = _rows_ptrs("fit_points", spec, rows)
        cfg = KpFitPointsCfg.default() if cfg is None else cfg
        out = _rows_outputs(R, table, want, self.device)
        if R > 0:
            need = {k: out[k] if k in out else torch.empty((R, *table[k][0]), dtype=f32, device=self.device) for k in ("qpos", "info")}      # the two the entry point requires
            ms = KpMarkerSet(K, body.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
            _check(self.L.kp_sim_fit_points(self.h, R, C.byref(ms), C.byref(KpFitPointsIn(*ins)), C.byref(cfg), C.byref(_rows_struct(KpFitPointsOut, table, {**need, **out}))),
                   "kp_sim_fit_points")
        return _rows_view(out, lead)

    def fit_scene(self, qpos0, pt_body, pt_offset, pt_tgt=None, pt_w=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None,
                  obj_qpos=None, cfg: KpFitSceneCfg | None = None, want=("qpos", "info")) -> dict:
        """fit_points with the scene's static objects as obstacles (kp_sim_fit_scene): the same inputs, and obj_qpos [..., 35] or None (every row is the
        floor scene) -- the rows' object poses, placed as for inverse_dynamics (objects farther than 50 m are parked).  cfg: a KpFitSceneCfg (None: its
        default, the object and the floor term off).  want: names of fit_scene_outputs(K).  Returns fit_points' dict with info [..., 16]
        (FIT_SCENE_INFO: the deepest counted vertex, the counted vertices and the pairs with a term at the result in 12..14).  Needs a handle on a
        blob with object geoms when obj_qpos is given.  Nothing the handle stores is read or changed."""
        body, off = marker_arrays("fit_scene", pt_body, pt_offset)
        K = body.shape[0]
        table = fit_scene_outputs(K)
        want = _rows_want("fit_scene", want, table)
        if (q_prior is None) != (w_prior is None):
            raise ValueError("fit_scene: q_prior and w_prior go together")
        if K == 0 and tgt_pos is None:
            raise ValueError("fit_scene: nothing to fit (no points and no tgt_pos)")
        f32 = torch.float32
        spec = [("qpos0", qpos0, (NQ,), f32, True), ("pt_tgt", pt_tgt, (K, 3), f32, K > 0), ("pt_w", pt_w, (K,), f32, False), ("tgt_pos", tgt_pos, (24, 3), f32, False),
                ("tgt_quat", tgt_quat, (24, 4), f32, False), ("w_pos", w_pos, (24,), f32, False), ("w_rot", w_rot, (24,), f32, False),
                ("q_prior", q_prior, (69,), f32, False), ("w_prior", w_prior, (69,), f32, False), ("obj_qpos", obj_qpos, (35,), f32, False)]
        lead, R, rows = _rows_inputs("fit_scene", spec)
        ins = _rows_ptrs("fit_scene", spec, rows)
        cfg = KpFitSceneCfg.default() if cfg is None else cfg
        if not (cfg.w_obj >= 0.0 and np.isfinite(cfg.w_obj)):
            raise ValueError("fit_scene: w_obj must be >= 0 and finite")
        out = _rows_outputs(R, table, want, self.device)
        if R > 0:
            need = {k: out[k] if k in out else torch.empty((R, *table[k][0]), dtype=f32, device=self.device) for k in ("qpos", "info")}      # the two the entry point requires
            ms = KpMarkerSet(K, body.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
            _check(self.L.kp_sim_fit_scene(self.h, R, C.byref(ms), C.byref(KpFitPointsIn(*ins[:9])), ins[9], C.byref(cfg),
                                           C.byref(_rows_struct(KpFitPointsOut, table, {**need, **out}))), "kp_sim_fit_scene")
        return _rows_view(out, lead)

    def fit_image(self, qpos0, pt_body, pt_offset, cam=None, uv=None, uv_w=None, pt_tgt=None, pt_w=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None,
                  q_prior=None, w_prior=None, obj_qpos=None, cfg: KpFitImageCfg | None = None, want=("qpos", "info")) -> dict:
        """fit_scene with 2D key points seen by calibrated cameras (kp_sim_fit_image): the same inputs (pt_tgt may be None with K > 0: no 3D term), and
        cam [C, 16] (one set of cameras for all rows) or [..., C, 16] (one per row), uv [..., C, K, 2] in pixels, uv_w [..., C, K] or None (ones; an
        observation with w <= 0 is skipped and its uv may be NaN).  C 0 .. 8; a record is R_cw (9, row-major), t, fx, fy, cx, cy (fit.Pinhole.pack).
        cam None: no image term.  cfg: a KpFitImageCfg (None: its default).  want: names of fit_image_outputs(K, C).  Returns fit_scene's dict with
        info [..., 20] (FIT_IMAGE_INFO) and uv_err [..., C, K].  Nothing the handle stores is read or changed."""
        body, off = marker_arrays("fit_image", pt_body, pt_offset)
        K = body.shape[0]
        if (cam is None) != (uv is None):
            raise ValueError("fit_image: cam and uv go together")
        if cam is not None and (cam.dim() < 2 or cam.shape[-1] != 16):
            raise ValueError(f"fit_image: cam must be [C, 16] or [..., C, 16], got {tuple(cam.shape)}")
        Cn = 0 if cam is None else int(cam.shape[-2])
        if Cn > MAX_CAMS:
            raise ValueError(f"fit_image: at most {MAX_CAMS} cameras, got {Cn}")
        table = fit_image_outputs(K, Cn)
        want = _rows_want("fit_image", want, table)
        if (q_prior is None) != (w_prior is None):
            raise ValueError("fit_image: q_prior and w_prior go together")
        if not (K > 0 and pt_tgt is not None) and tgt_pos is None and not (K > 0 and Cn > 0):
            raise ValueError("fit_image: nothing to fit (no 3D targets, no tgt_pos and no observations)")
        f32 = torch.float32
        shared = cam is not None and cam.dim() == 2
        spec = [("qpos0", qpos0, (NQ,), f32, True), ("pt_tgt", pt_tgt, (K, 3), f32, False), ("pt_w", pt_w, (K,), f32, False), ("tgt_pos", tgt_pos, (24, 3), f32, False),
                ("tgt_quat", tgt_quat, (24, 4), f32, False), ("w_pos", w_pos, (24,), f32, False), ("w_rot", w_rot, (24,), f32, False),
                ("q_prior", q_prior, (69,), f32, False), ("w_prior", w_prior, (69,), f32, False), ("obj_qpos", obj_qpos, (35,), f32, False),
                ("cam", None if shared else cam, (Cn, 16), f32, False), ("uv", uv, (Cn, K, 2), f32, False), ("uv_w", uv_w, (Cn, K), f32, False)]
        lead, R, rows = _rows_inputs("fit_image", spec)
        ins = _rows_ptrs("fit_image", spec, rows)
        if shared:
            ins[10] = _dev("fit_image: cam", cam, (Cn, 16), f32)
        cfg = KpFitImageCfg.default() if cfg is None else cfg
        if not (cfg.scene.w_obj >= 0.0 and np.isfinite(cfg.scene.w_obj)):
            raise ValueError("fit_image: w_obj must be >= 0 and finite")
        if not (cfg.z_near > 0.0 and np.isfinite(cfg.z_near)):
            raise ValueError("fit_image: z_near must be > 0 and finite")
        out = _rows_outputs(R, table, want, self.device)
        if R > 0:
            need = {k: out[k] if k in out else torch.empty((R, *table[k][0]), dtype=f32, device=self.device) for k in ("qpos", "info")}      # the two the entry point requires
            ms = KpMarkerSet(K, body.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
            obs = KpFitImageObs(Cn, 1 if shared else R, ins[10], ins[11], ins[12])
            _check(self.L.kp_sim_fit_image(self.h, R, C.byref(ms), C.byref(KpFitPointsIn(*ins[:9])), ins[9], C.byref(obs), C.byref(cfg),
                                           C.byref(_rows_struct(KpFitImageOut, table, {**need, **out}))), "kp_sim_fit_image")
        return _rows_view(out, lead)

    def fk(self, qpos_rows: torch.Tensor):
        """qpos_fk_batch on [R,76] rows -> dict(qpos, wbpos, wbquat, bquat, body_com) of device tensors."""
        rows = _dev("fk: qpos_rows", qpos_rows, (None, NQ))
        R = qpos_rows.shape[0]
        out = {k: torch.empty((R, d), dtype=torch.float32, device=self.device) for k, d in
               (("qpos", 76), ("wbpos", 72), ("wbquat", 96), ("bquat", 96), ("body_com", 72))}
        _check(self.L.kp_sim_fk(self.h, R, rows, *[C.c_void_p(o.data_ptr()) for o in out.values()]), "kp_sim_fk")
        return out

    def fk_backward(self, qpos_rows, wbpos, wbquat, grad_wbpos):
        """(d wbpos / d qpos)^T grad_wbpos for the rows of an fk() call -> [R,76]."""
        R = qpos_rows.shape[0]
        ins = [_dev("fk_backward: " + k, t, (R, d)) for k, t, d in (("qpos_rows", qpos_rows, NQ), ("wbpos", wbpos, 72), ("wbquat", wbquat, 96), ("grad_wbpos", grad_wbpos, 72))]
        out = torch.empty((R, NQ), dtype=torch.float32, device=self.device)
        _check(self.L.kp_sim_fk_backward(self.h, R, *ins, C.c_void_p(out.data_ptr())), "kp_sim_fk_backward")
        return out

    def _obs_ar_backward(self, name, ctx, ext, qpos_rows, wbpos, wbquat, grad_obs, grad_obj_2_head):
        """kp_sim_<name> for obs_ar_backward (ext None) and obs_ar_ex_backward: the shape checks, the outputs (grad_ctx for a wide row with a context
        block) and the call -> the outputs in the ABI's order, None for the ones the row does not have"""
        _dev(f"{name}: grad_obs", grad_obs, (None, None))
        R, W = grad_obs.shape
        ins = [_dev(f"{name}: {k}", t, (R, d)) for k, t, d in (("qpos_rows", qpos_rows, NQ), ("wbpos", wbpos, 72), ("wbquat", wbquat, 96), ("grad_obs", grad_obs, W),
                                                              ("grad_obj_2_head", grad_obj_2_head, 7))]
        new = lambda d: torch.empty((R, d), dtype=torch.float32, device=self.device)      # noqa: E731
        outs = [new(NQ), (new(NV) if self.obs_ar_vel else None), new(3), new(4)]
        if ext is not None:
            outs.append(new(ext.ctx_dim) if ext.ctx_dim > 0 else None)
        _check(getattr(self.L, "kp_sim_" + name)(self.h, C.byref(ctx), *([] if ext is None else [C.byref(ext)]), R, W, *ins,
                                                 *[None if o is None else C.c_void_p(o.data_ptr()) for o in outs]), "kp_sim_" + name)
        return tuple(outs)

    def obs_ar_backward(self, ctx: "KpCtx", qpos_rows, wbpos, wbquat, grad_obs, grad_obj_2_head=None):
        """(d obs_ar)^T grad_obs for the first R <= N rows (kp_sim_obs_ar_backward; wbpos / wbquat: fk() of qpos_rows) -> (grad_qpos [R,76], the local
        pose block's part; grad_qvel [R,75] or None without use_vel; grad_hpos [R,3]; grad_hquat [R,4]).  grad_obj_2_head [R,7]: cotangent of the
        object block read as a feature, added to that block's."""
        return self._obs_ar_backward("obs_ar_backward", ctx, None, qpos_rows, wbpos, wbquat, grad_obs, grad_obj_2_head)

    def fk_head_backward(self, qpos_rows, wbpos, wbquat, grad_wbpos=None, grad_hpos=None, grad_hquat=None, grad_qpos_add=None):
        """fk_backward plus the head's world quaternion (kp_sim_fk_head_backward): (d wbpos / d qpos)^T (grad_wbpos, grad_hpos added to the head's slot)
        + (d head quaternion / d qpos)^T grad_hquat + grad_qpos_add -> [R,76]; a None cotangent is zero."""
        R = qpos_rows.shape[0]
        ins = [_dev("fk_head_backward: " + k, t, (R, d)) for k, t, d in (("qpos_rows", qpos_rows, NQ), ("wbpos", wbpos, 72), ("wbquat", wbquat, 96), ("grad_wbpos", grad_wbpos, 72),
                                                                           ("grad_hpos", grad_hpos, 3), ("grad_hquat", grad_hquat, 4), ("grad_qpos_add", grad_qpos_add, NQ))]
        out = torch.empty((R, NQ), dtype=torch.float32, device=self.device)
        _check(self.L.kp_sim_fk_head_backward(self.h, R, *ins, C.c_void_p(out.data_ptr())), "kp_sim_fk_head_backward")
        return out

    def pose_contacts(self, qpos_rows: torch.Tensor, obj_qpos: torch.Tensor | None = None, pen_margin: float = 0.005) -> dict:
        """compute_physcis_metris' per-frame contact walk (kp_sim_pose_contacts) on [R,76] rows (+ their [R,35] object blocks, or None: floor
        only) -> dict of device tensors: pen [R] (sum of max(0, -dist - pen_margin) over the hull - floor / hull - object contacts), ncon [R]
        int32, hits [R, n_obj_geoms] uint32 (bit b = hull b touches object geom g), xpos [R,72], xquat [R,96] (the rows' body poses, fk())."""
        _dev("pose_contacts: qpos_rows", qpos_rows, (None, NQ))
        R = qpos_rows.shape[0]
        op = _dev("pose_contacts: obj_qpos", obj_qpos, (R, 35))
        n_og = int(self.model.get_option("n_obj_geoms"))
        out = {"pen": torch.empty(R, dtype=torch.float32, device=self.device), "ncon": torch.empty(R, dtype=torch.int32, device=self.device),
               "hits": torch.empty((R, n_og), dtype=torch.int32, device=self.device).view(torch.uint32)}
        if R == 0:
            out["xpos"] = torch.empty((0, 72), dtype=torch.float32, device=self.device)
            out["xquat"] = torch.empty((0, 96), dtype=torch.float32, device=self.device)
            return out
        f = self.fk(qpos_rows)
        out["xpos"], out["xquat"] = f["wbpos"], f["wbquat"]
        _check(self.L.kp_sim_pose_contacts(self.h, R, C.c_void_p(out["xpos"].data_ptr()), C.c_void_p(out["xquat"].data_ptr()), op, float(pen_margin),
                                           *[C.c_void_p(out[k].data_ptr()) for k in ("pen", "ncon", "hits")]), "kp_sim_pose_contacts")
        return out

    RENDER_OUTPUTS = {"rgba": (torch.uint8, (4,)), "geom": (torch.int32, ()), "depth": (torch.float32, ())}

    def render_poses(self, xpos: torch.Tensor, xquat: torch.Tensor, obj_qpos: torch.Tensor | None = None, camera=None, width: int = 320, height: int = 240,
                     want=("rgba",), style: "KpRenderStyle | None" = None) -> dict:
        """kp_sim_render on body poses: xpos [R,K,72] / xquat [R,K,96] (K = 1..4 figures per row, fk()'s wbpos / wbquat), obj_qpos [R,35] or None
        (floor and figures only), camera = a kinpoly_amd.render.Camera, a [7] / [1,7] / [R,7] tensor (lookat[3], distance, azimuth, elevation, fovy;
        degrees) or None (the reference viewer's default) -> dict of device tensors for the names in `want`: rgba uint8 [R,H,W,4], geom int32 [R,H,W]
        (-1 nothing, 0 floor, 100 k + 1 + b body b of figure k, 25 + g object geom g), depth float32 [R,H,W] (+inf where nothing is hit)."""
        _dev("render: xpos", xpos, (None, None, 72))
        R, K = xpos.shape[:2]
        xq = _dev("render: xquat", xquat, (R, K, 96))
        op = _dev("render: obj_qpos", obj_qpos, (R, 35))
        if camera is None or hasattr(camera, "tensor"):
            from .render import Camera
            camera = (camera or Camera()).tensor(self.device)
        cam = camera.reshape(1, 7) if camera.dim() == 1 else camera
        if cam.dim() != 2 or cam.shape[0] not in (1, R):
            raise ValueError(f"render: camera must be [7], [1,7] or [{R},7], got {tuple(camera.shape)}")
        cp = _dev("render: camera", cam, (cam.shape[0], 7))
        unknown = [k for k in want if k not in self.RENDER_OUTPUTS]
        if unknown or not want:
            raise ValueError(f"render: want must name some of {sorted(self.RENDER_OUTPUTS)}, got {tuple(want)}")
        out = {k: torch.empty((R, int(height), int(width)) + self.RENDER_OUTPUTS[k][1], dtype=self.RENDER_OUTPUTS[k][0], device=self.device) for k in want}
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None      # noqa: E731
        _check(self.L.kp_sim_render(self.h, R, K, C.c_void_p(xpos.data_ptr()), xq, op, cp, cam.shape[0], int(width), int(height),
                                    None if style is None else C.byref(style), ptr("geom"), ptr("depth"), ptr("rgba")), "kp_sim_render")
        return out

    def render(self, qpos_rows: torch.Tensor, obj_qpos: torch.Tensor | None = None, camera=None, width: int = 320, height: int = 240, want=("rgba",),
               style: "KpRenderStyle | None" = None) -> dict:
        """Frames of qpos rows [R,76], or [R,K,76] for K figures per row (e.g. simulated and expert): fk() of every figure, then render_poses."""
        if qpos_rows.dim() == 2:
            qpos_rows = qpos_rows[:, None]
        _dev("render: qpos_rows", qpos_rows, (None, None, NQ))
        R, K = qpos_rows.shape[:2]
        f = self.fk(qpos_rows.reshape(R * K, NQ)) if R else {"wbpos": qpos_rows.new_empty((0, 72)), "wbquat": qpos_rows.new_empty((0, 96))}
        return self.render_poses(f["wbpos"].view(R, K, 72), f["wbquat"].view(R, K, 96), obj_qpos, camera, width, height, want, style)

    EGO_OUTPUTS = {**RENDER_OUTPUTS, "flow": (torch.float32, (2,)), "ok": (torch.uint8, ()), "cells": (torch.float32, (2,))}

    def _pose_camera(self, camera, R, what):
        """a HeadCamera-free camera argument of the ego renderer: a [8] / [1,8] / [R,8] device tensor (eye[3], quaternion[4] w x y z, fovy) -> [1 or R, 8]"""
        cam = camera.reshape(1, 8) if camera.dim() == 1 else camera
        if cam.dim() != 2 or cam.shape[0] not in (1, R) or cam.shape[1] != 8:
            raise ValueError(f"render_ego: {what} must be [8], [1,8] or [{R},8], got {tuple(camera.shape)}")
        _dev("render_ego: " + what, cam, (cam.shape[0], 8))
        return cam

    def render_ego_poses(self, xpos: torch.Tensor, xquat: torch.Tensor, obj_qpos: torch.Tensor | None, camera: torch.Tensor, xpos_b: torch.Tensor | None = None,
                         xquat_b: torch.Tensor | None = None, obj_qpos_b: torch.Tensor | None = None, camera_b: torch.Tensor | None = None, width: int = 64,
                         height: int = 64, want=("rgba",), grid=None, hide_body: int = -1, style: "KpRenderStyle | None" = None) -> dict:
        """kp_sim_render_ego on body poses: the A side as render_poses takes it but with pose cameras [R,8] / [1,8] / [8] (eye[3], quaternion[4] w x y z
        world from camera, fovy in degrees; the head body's axes: +z forward, +y up, +x left), and optionally the same rows one frame later as the B
        side (xpos_b, xquat_b, camera_b; obj_qpos_b exactly when obj_qpos is given) -> dict of device tensors for the names in `want`: rgba, geom,
        depth as render_poses; flow float32 [R,H,W,2] (pixels, A -> B), ok uint8 [R,H,W], cells float32 [R,Gy,Gx,2] (grid = (Gy, Gx) or one int: the
        mean flow of the ok pixels of every cell).  hide_body: a body 0..23 of figure 0 that is not drawn, -1 for none."""
        _dev("render_ego: xpos", xpos, (None, None, 72))
        R, K = xpos.shape[:2]
        xq = _dev("render_ego: xquat", xquat, (R, K, 96))
        op = _dev("render_ego: obj_qpos", obj_qpos, (R, 35))
        cam = self._pose_camera(camera, R, "camera")
        b = [_dev("render_ego: xpos_b", xpos_b, (R, K, 72)), _dev("render_ego: xquat_b", xquat_b, (R, K, 96)), _dev("render_ego: obj_qpos_b", obj_qpos_b, (R, 35)), None]
        if camera_b is not None:
            cam_b = self._pose_camera(camera_b, R, "camera_b")
            if cam_b.shape[0] != cam.shape[0]:
                raise ValueError(f"render_ego: camera and camera_b must have the same number of rows, got {cam.shape[0]} and {cam_b.shape[0]}")
            b[3] = C.c_void_p(cam_b.data_ptr())
        unknown = [k for k in want if k not in self.EGO_OUTPUTS]
        if unknown or not want:
            raise ValueError(f"render_ego: want must name some of {sorted(self.EGO_OUTPUTS)}, got {tuple(want)}")
        gy, gx = (0, 0) if grid is None else ((int(grid), int(grid)) if isinstance(grid, int) else (int(grid[0]), int(grid[1])))
        if "cells" in want and grid is None:
            raise ValueError("render_ego: want names cells but no grid is given")
        out = {k: torch.empty(((R, gy, gx) if k == "cells" else (R, int(height), int(width))) + self.EGO_OUTPUTS[k][1], dtype=self.EGO_OUTPUTS[k][0], device=self.device)
               for k in want}
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None      # noqa: E731
        _check(self.L.kp_sim_render_ego(self.h, R, K, C.c_void_p(xpos.data_ptr()), xq, op, C.c_void_p(cam.data_ptr()), *b, cam.shape[0], int(width), int(height),
                                        int(hide_body), None if style is None else C.byref(style), gx, gy,
                                        *[ptr(k) for k in ("geom", "depth", "rgba", "flow", "ok", "cells")]), "kp_sim_render_ego")
        return out

    def render_ego(self, qpos_a: torch.Tensor, obj_a: torch.Tensor | None, cam_a, qpos_b: torch.Tensor | None = None, obj_b: torch.Tensor | None = None, cam_b=None,
                   width: int = 64, height: int = 64, want=("rgba",), grid=None, hide_body: int = -1, style: "KpRenderStyle | None" = None) -> dict:
        """Egocentric frames of qpos rows [R,76] or [R,K,76]: fk() of every figure, then render_ego_poses.  cam_a / cam_b: pose-camera tensors, or a
        kinpoly_amd.render.HeadCamera (the camera rides on figure 0's head in that frame; its hide_head sets hide_body).  qpos_b (+ obj_b, cam_b): the rows
        one frame later."""
        def poses(q, what):
            if q.dim() == 2:
                q = q[:, None]
            _dev("render_ego: " + what, q, (None, None, NQ))
            R, K = q.shape[:2]
            f = self.fk(q.reshape(R * K, NQ)) if R else {"wbpos": q.new_empty((0, 72)), "wbquat": q.new_empty((0, 96))}
            return f["wbpos"].view(R, K, 72), f["wbquat"].view(R, K, 96)

        def cam(c, xp, xq):
            return c.rows(xp[:, 0], xq[:, 0]) if hasattr(c, "rows") else c

        if hide_body < 0 and getattr(cam_a, "hide_head", False):
            hide_body = cam_a.hide_body
        xp, xq = poses(qpos_a, "qpos_a")
        if qpos_b is None:
            return self.render_ego_poses(xp, xq, obj_a, cam(cam_a, xp, xq), None, None, obj_b, cam_b, width, height, want, grid, hide_body, style)
        xpb, xqb = poses(qpos_b, "qpos_b")
        return self.render_ego_poses(xp, xq, obj_a, cam(cam_a, xp, xq), xpb, xqb, obj_b, None if cam_b is None else cam(cam_b, xpb, xqb), width, height, want,
                                     grid, hide_body, style)

    def step_begin(self):
        _check(self.L.kp_sim_step_begin(self.h), "kp_sim_step_begin")

    def make_ctx(self, T, head_pose, head_vels, obj_rel, action_one_hot, gt_bquat, gt_wbpos, cur_t, obj_qpos=None, row=None) -> "KpCtx":
        n = self.n
        R = head_pose.shape[0] if row is not None else n        # context rows (>= n_envs with the row indirection)
        _dev("row", row, (n,), torch.int32)
        for k, t, shp in (("head_pose", head_pose, (R, T, 7)), ("head_vels", head_vels, (R, T, 6)), ("obj_rel", obj_rel, (R, T, 7)),
                          ("action_one_hot", action_one_hot, (R, 4)), ("gt_bquat", gt_bquat, (R, T, 96)), ("gt_wbpos", gt_wbpos, (R, T, 72))):
            _dev("context tensor " + k, t, shp)
        _dev("cur_t", cur_t, (n,), torch.int32)
        ctx = KpCtx(int(T), head_pose.data_ptr(), head_vels.data_ptr(), obj_rel.data_ptr(), action_one_hot.data_ptr(), gt_bquat.data_ptr(),
                    gt_wbpos.data_ptr(), None if obj_qpos is None else obj_qpos.data_ptr(), cur_t.data_ptr(), None if row is None else row.data_ptr())
        ctx._keep = (head_pose, head_vels, obj_rel, action_one_hot, gt_bquat, gt_wbpos, obj_qpos, cur_t, row)
        return ctx

    def obs_ar(self, ctx: "KpCtx", out=None):
        out = self._new(self.obs_ar_dim) if out is None else out
        _check(self.L.kp_sim_obs_ar(self.h, C.byref(ctx), _ptr(out, self.n, self.obs_ar_dim)), "kp_sim_obs_ar")
        return out

    def make_obs_ext(self, T, rows, ctx_dim=0, ctx_feat=None, of=None, ctx_time_major=True, of_time_major=False) -> "KpObsExt":
        """kp_obs_ext for a kp_ctx of `rows` context rows and T frames: ctx_feat [T, rows, ctx_dim] (time-major, what get_context_feat keeps) or
        [rows, T, ctx_dim], None = the zero block; of [rows, T, F] (the data set's) or [T, rows, F], None = no `of` block."""
        def table(name, t, time_major, dim):
            _dev("obs_ext: " + name, t, (T, rows, dim) if time_major else (rows, T, dim))
            return (dim, rows * dim) if time_major else (T * dim, dim)          # (stride_row, stride_t)
        x = KpObsExt(int(ctx_dim), None, 0, 0, 0, None, 0, 0)
        if ctx_feat is not None:
            x.ctx_feat = ctx_feat.data_ptr()
            x.ctx_stride_row, x.ctx_stride_t = table("ctx_feat", ctx_feat, ctx_time_major, int(ctx_dim))
        if of is not None:
            _dev("obs_ext: of", of, (None, None, None))
            x.of_dim, x.of = int(of.shape[2]), of.data_ptr()
            x.of_stride_row, x.of_stride_t = table("of", of, of_time_major, int(of.shape[2]))
        x._keep = (ctx_feat, of)
        return x

    def obs_ar_ex(self, ctx: "KpCtx", ext: "KpObsExt", out=None):
        """[context block | obs_ar's row | of block] in one launch (kp_sim_obs_ar_ex) -> [N, ext.ctx_dim + obs_ar_dim + ext.of_dim]"""
        W = ext.ctx_dim + self.obs_ar_dim + ext.of_dim
        out = self._new(W) if out is None else out
        _check(self.L.kp_sim_obs_ar_ex(self.h, C.byref(ctx), C.byref(ext), _ptr(out, self.n, W)), "kp_sim_obs_ar_ex")
        return out

    def obs_ar_ex_backward(self, ctx: "KpCtx", ext: "KpObsExt", qpos_rows, wbpos, wbquat, grad_obs, grad_obj_2_head=None):
        """obs_ar_backward for the wide row (kp_sim_obs_ar_ex_backward): -> (grad_qpos, grad_qvel or None, grad_hpos, grad_hquat, grad_ctx [R, ctx_dim] --
        the context block's cotangent, None when ctx_dim is 0)."""
        return self._obs_ar_backward("obs_ar_ex_backward", ctx, ext, qpos_rows, wbpos, wbquat, grad_obs, grad_obj_2_head)

    def term_reward(self, ctx: "KpCtx", cfg: "KpRewardCfg | KpRewardCfgV2", reward=None, info=None, fail=None, diffs=None):
        """termination + reward; the cfg's type names the reward: KpRewardCfg dynamic_supervision_v1, KpRewardCfgV2 dynamic_supervision_v2"""
        v2 = isinstance(cfg, KpRewardCfgV2)
        reward = torch.empty(self.n, device=self.device) if reward is None else reward
        info = self._new(6) if info is None else info
        fail = torch.empty(self.n, dtype=torch.uint8, device=self.device) if fail is None else fail
        diffs = self._new(2) if diffs is None else diffs
        fn = self.L.kp_sim_term_reward_v2 if v2 else self.L.kp_sim_term_reward
        _check(fn(self.h, C.byref(ctx), C.byref(cfg), C.c_void_p(reward.data_ptr()), _ptr(info, self.n, 6), C.c_void_p(fail.data_ptr()), _ptr(diffs, self.n, 2)),
               "kp_sim_term_reward_v2" if v2 else "kp_sim_term_reward")
        return reward, info, fail, diffs

    def post_step(self, ctx: "KpCtx", cfg: "KpRewardCfg | KpRewardCfgV2", cur_t, row_len, episode_len, reward, info, fail, diffs, done, end, percent, done_count=None, obj7=None):
        """cur_t += 1; termination + reward; end / done / percent -- the tail of HumanoidAREnv.step in one launch (kp_sim_post_step).
        obj7 [N,7]: refreshed with the simulated pose of every env's action object (get_obj_qpos(action_one_hot)).  A KpRewardCfgV2 runs
        kp_sim_post_step_v2 (dynamic_supervision_v2)."""
        v2 = isinstance(cfg, KpRewardCfgV2)
        fn = self.L.kp_sim_post_step_v2 if v2 else self.L.kp_sim_post_step
        _check(fn(self.h, C.byref(ctx), C.byref(cfg), C.c_void_p(cur_t.data_ptr()), C.c_void_p(row_len.data_ptr()), int(episode_len),
                  C.c_void_p(reward.data_ptr()), _ptr(info, self.n, 6), C.c_void_p(fail.data_ptr()), _ptr(diffs, self.n, 2),
                  C.c_void_p(done.data_ptr()), C.c_void_p(end.data_ptr()), C.c_void_p(percent.data_ptr()),
                  None if done_count is None else C.c_void_p(done_count.data_ptr()), _ptr(obj7, self.n, 7)), "kp_sim_post_step_v2" if v2 else "kp_sim_post_step")

    def reset_rows(self, init_qpos, init_qvel, row=None, env_mask=None, cur_t=None, set_target=True, aux_rows=None, row_obj_qpos=None, row_one_hot=None, obj7=None):
        """masked reset from context rows: state <- init rows, cur_t = 0, sim.forward(), target = FK(init) (kp_sim_reset_rows).
        aux_rows [N, C]: caller-owned per-env rows zeroed for the same envs (the policy's GRU state).  row_obj_qpos [R, 35] (+ row_one_hot [R, 4],
        obj7 [N, 7]): the object block of reset_model from the env's context row, and get_obj_qpos(action_one_hot) of it."""
        R = init_qpos.shape[0]
        _check(self.L.kp_sim_reset_rows(self.h, _dev("init_qpos", init_qpos, (None, NQ)), _dev("init_qvel", init_qvel, (None, NV)), None if row is None else C.c_void_p(row.data_ptr()),
                                        _mask_ptr(env_mask, self.n), None if cur_t is None else C.c_void_p(cur_t.data_ptr()), int(bool(set_target)),
                                        _dev("aux_rows", aux_rows, (self.n, None)), 0 if aux_rows is None else int(aux_rows.shape[1]),
                                        _dev("row_obj_qpos", row_obj_qpos, (R, 35)), _dev("row_one_hot", row_one_hot, (R, 4)), _ptr(obj7, self.n, 7)), "kp_sim_reset_rows")

    def diag(self) -> np.ndarray:
        out = np.zeros((self.n, 4), np.int32)
        _check(self.L.kp_sim_diag(self.h, out.ctypes.data_as(C.c_void_p)), "kp_sim_diag")
        return out

    def timing_reset(self):
        _check(self.L.kp_sim_timing_reset(self.h), "kp_sim_timing_reset")

    def timing_mean_seconds(self):
        n = C.c_int(0)
        t = self.L.kp_sim_timing_mean_seconds(self.h, C.byref(n))
        return t, n.value

    def phase_cycles(self):
        out = (C.c_double * 8)()
        _check(self.L.kp_sim_phase_cycles(self.h, out), "kp_sim_phase_cycles")
        return dict(zip(("spd", "kin_bias", "collide", "constraint", "smooth", "contact", "integrate", "total"), list(out)))

    def phase_cycles_env(self):
        """per-env shader-clock cycles of the last control step's phases, numpy [N, 8] (KP_PROFILE=1)."""
        out = np.zeros((self.n, 8), np.float64)
        _check(self.L.kp_sim_phase_cycles_env(self.h, out.ctypes.data_as(C.c_void_p)), "kp_sim_phase_cycles_env")
        return out

    def launch_cost(self):
        """shader-clock cycles every env took in the last control-step launch (numpy uint64 [N])."""
        out = np.zeros(self.n, np.uint32)
        _check(self.L.kp_sim_launch_cost(self.h, out.ctypes.data_as(C.c_void_p)), "kp_sim_launch_cost")
        return out.astype(np.uint64) << 10

    def last_step_seconds(self) -> float:
        return self.L.kp_sim_last_step_seconds(self.h)


# the names kp_takes_table answers (kp_sim.hip; tests/test_gpu_uhc_takes.py asks the library for each of them)
TAKE_TABLES = ("qpos", "qpos_fk", "wbpos", "wbquat", "bquat", "body_com", "com", "head_pose", "ee_wpos", "ee_pos", "rq_rmh", "qvel", "rlinv", "rangv",
               "rlinv_local", "bangvel", "height_lb", "head_height_lb")


def _take_rows(what, rows, width):
    """(keep-alive, on_device, pointer) of a library's row array [R, width]: a device tensor stays where it is, anything else becomes a host fp32 array"""
    if torch.is_tensor(rows) and rows.is_cuda:
        rows = rows.to(torch.float32).contiguous()
        on_dev, ptr, shape = 1, rows.data_ptr(), tuple(rows.shape)
    else:
        rows = np.ascontiguousarray(rows.cpu().numpy() if torch.is_tensor(rows) else rows, np.float32)
        on_dev, ptr, shape = 0, rows.ctypes.data, rows.shape
    if len(shape) != 2 or shape[1] != width:
        raise ValueError(f"KpTakes: {what} must be [R, {width}], got {tuple(shape)}")
    return rows, on_dev, ptr


class KpTakes:
    """The device-resident take library (kp_takes): the expert tables of K takes of different lengths, concatenated row-wise.  Built once with a
    KpSim's forward kinematics and model tables; independent of the number of envs.  `table(name)` is a zero-copy [R, width] view ([K, 1] for the
    per-take minima); `take(k)` slices every per-row table to take k.

    obj_rows [R, 35] (kp_takes_create_obj): the object block data.qpos[76:111] of every row, on the same side (host / device) as qpos_rows.  Such a
    library `has_objects`, answers table("obj_pose") and take(k)["obj_pose"], and KpSim.uhc_assign places every reset env's objects from it."""

    def __init__(self, sim: KpSim, qpos_rows, take_off, dt: float = 1.0 / 30.0, obj_rows=None):
        self.sim, self.L, self.device = sim, sim.L, sim.device
        off = np.ascontiguousarray(np.asarray(take_off, np.int32).reshape(-1))
        K = len(off) - 1
        rows, on_dev, ptr = _take_rows("qpos_rows", qpos_rows, NQ)
        if K >= 1 and int(off[-1]) != rows.shape[0]:
            raise ValueError(f"KpTakes: take_off ends at {int(off[-1])}, qpos_rows has {rows.shape[0]} rows")
        if obj_rows is not None:
            orows, obj_on_dev, optr = _take_rows("obj_rows", obj_rows, 35)
            if orows.shape[0] != rows.shape[0]:
                raise ValueError(f"KpTakes: obj_rows has {orows.shape[0]} rows, qpos_rows has {rows.shape[0]}")
            if obj_on_dev != on_dev:
                raise ValueError("KpTakes: qpos_rows and obj_rows must both be device tensors or both be host arrays")
        with torch.cuda.device(self.device):
            if obj_rows is None:
                self.h = self.L.kp_takes_create(sim.h, C.c_void_p(ptr), on_dev, off.ctypes.data_as(C.c_void_p), K, float(dt))
            else:
                self.h = self.L.kp_takes_create_obj(sim.h, C.c_void_p(ptr), C.c_void_p(optr), on_dev, off.ctypes.data_as(C.c_void_p), K, float(dt))
        if not self.h:
            raise KinPolyNativeError(f"kp_takes_create{'' if obj_rows is None else '_obj'}: {self.L.kp_last_error().decode()}")
        k, r = C.c_int(0), C.c_int(0)
        lens = np.zeros(K, np.int32)
        _check(self.L.kp_takes_info(self.h, C.byref(k), C.byref(r), lens.ctypes.data_as(C.c_void_p)), "kp_takes_info")
        self.K, self.R, self.lens, self.take_off = k.value, r.value, lens, off.copy()
        self.has_objects = bool(self.L.kp_takes_has_objects(self.h))
        self._tabs = {}

    def table(self, name: str) -> torch.Tensor:
        if name not in self._tabs:
            p, rows, w = C.c_void_p(0), C.c_int(0), C.c_int(0)
            _check(self.L.kp_takes_table(self.h, name.encode(), C.byref(p), C.byref(rows), C.byref(w)), "kp_takes_table")
            self._tabs[name] = _device_view(p.value, (rows.value, w.value), self.device)
        return self._tabs[name]

    def take(self, k: int) -> dict:
        a, b = int(self.take_off[k]), int(self.take_off[k + 1])
        out = {n: self.table(n)[a:b] for n in TAKE_TABLES[:-2]}
        if self.has_objects:
            out["obj_pose"] = self.table("obj_pose")[a:b]
        out["len"] = b - a
        out["height_lb"], out["head_height_lb"] = self.table("height_lb")[k, 0], self.table("head_height_lb")[k, 0]
        return out

    def __del__(self):
        try:
            self._tabs.clear()
            self.L.kp_takes_destroy(self.h)
        except Exception:
            pass


def job_schedule(n_substeps: int, substeps_per_job: int = 4, taper: int = 1) -> list:
    """Job sizes of the queue-scheduled control step (kp_job_schedule; host arithmetic only)."""
    L = load_library()
    out = (C.c_int * 16)()
    n = L.kp_job_schedule(int(n_substeps), int(substeps_per_job), int(taper), out)
    if n < 0:
        raise KinPolyNativeError(f"kp_job_schedule: {L.kp_last_error().decode()}")
    return list(out[:n])


def _obs_width(obs_dim, ctx_dim=0, of_dim=0):
    """The row width the record kernels are launched with: one of the eight layout widths, between a context block and an `of` block when given."""
    if ctx_dim < 0 or of_dim < 0 or obs_dim - ctx_dim - of_dim not in AR_OBS_DIMS:
        wide = f" between a {ctx_dim}-d context block and a {of_dim}-d `of` block" if (ctx_dim or of_dim) else ""
        raise ValueError(f"obs_dim must be one of {AR_OBS_DIMS} (ar_obs_dim of use_vel / use_head / use_action){wide}, got {obs_dim}")
    return int(obs_dim)


def _u8(t):
    """bool tensors are passed as their uint8 storage"""
    return t.view(torch.uint8) if t is not None and t.dtype == torch.bool else t


def record_pre(t: int, T: int, obs=None, fresh=None, qpos=None, ctx_qpos=None, row=None, cur_t=None, row_len=None, row_meta=None,
               states=None, episode_start=None, curr_qpos=None, gt_target_qpos=None, meta=None, obs_dim=AR_OBS_DIM, ctx_dim=0, of_dim=0):
    """kp_rollout_record_pre: the before-the-step half of the sampler's per-step record, one launch (see include/kinpoly_sim.h).
    obs_dim: the width of obs / states (the env's obs_dim); ctx_dim / of_dim: the context and `of` blocks around the KpSim.obs_ar_dim columns in it
    (kp_rollout_record_pre_x; both 0: kp_rollout_record_pre_w)."""
    L = load_library()
    w = _obs_width(obs_dim, ctx_dim, of_dim)
    first = next(x for x in (obs, qpos, fresh) if x is not None)
    i32, u8 = torch.int32, torch.uint8
    n = first.shape[0]
    r = KpRecordPre(n, int(T), int(t), 0 if ctx_qpos is None else int(ctx_qpos.shape[1]),
                    _dev("obs", obs, (n, w)), _dev("fresh", _u8(fresh), (n,), u8), _dev("qpos", qpos, (n, 76)), _dev("ctx_qpos", ctx_qpos, (None, None, 76)),
                    _dev("row", row, (n,), i32), _dev("cur_t", cur_t, (n,), i32), _dev("row_len", row_len, None, i32), _dev("row_meta", row_meta, None),
                    _dev("states", states, (n, T, w)), _dev("episode_start", _u8(episode_start), (n, T), u8), _dev("curr_qpos", curr_qpos, (n, T, 76)),
                    _dev("gt_target_qpos", gt_target_qpos, (n, T, 76)), _dev("meta", meta, (n, T, 2)))
    stream = C.c_void_p(torch.cuda.current_stream(first.device).cuda_stream)
    if ctx_dim or of_dim:
        _check(L.kp_rollout_record_pre_x(C.byref(r), w, int(ctx_dim), int(of_dim), stream), "kp_rollout_record_pre_x")
    else:
        _check(L.kp_rollout_record_pre_w(C.byref(r), w, stream), "kp_rollout_record_pre")


def record_post(t: int, T: int, fr_num=0.0, action=None, reward=None, fail=None, done=None, percent=None, c_info=None, obs=None, qpos=None, cc_action=None, cc_state=None, meta=None,
                actions=None, rewards=None, fails=None, dones=None, percents=None, c_infos=None, next_states=None, res_qpos=None, cc_actions=None, cc_states=None, v_metas=None,
                obs_dim=AR_OBS_DIM, ctx_dim=0, of_dim=0):
    """kp_rollout_record_post: the after-the-step half (one launch); obs_dim: the width of obs / next_states, ctx_dim / of_dim as in record_pre."""
    L = load_library()
    w = _obs_width(obs_dim, ctx_dim, of_dim)
    first = next(x for x in (action, reward, done) if x is not None)
    u8 = torch.uint8
    n = first.shape[0]
    r = KpRecordPost(n, int(T), int(t), float(fr_num), _dev("action", action, (n, 80)), _dev("reward", reward, (n,)), _dev("fail", _u8(fail), (n,), u8),
                     _dev("done", _u8(done), (n,), u8), _dev("percent", percent, (n,)), _dev("c_info", c_info, (n, 6)), _dev("obs", obs, (n, w)), _dev("qpos", qpos, (n, 76)),
                     _dev("cc_action", cc_action, (n, CC_ACTION_DIM)), _dev("cc_state", cc_state, (n, CC_OBS_DIM)), _dev("meta", meta, (n, T, 2)),
                     _dev("actions", actions, (n, T, 80)), _dev("rewards", rewards, (n, T)), _dev("fails", _u8(fails), (n, T), u8), _dev("dones", _u8(dones), (n, T), u8),
                     _dev("percents", percents, (n, T)), _dev("c_infos", c_infos, (n, T, 6)), _dev("next_states", next_states, (n, T, w)), _dev("res_qpos", res_qpos, (n, T, 76)),
                     _dev("cc_actions", cc_actions, (n, T, CC_ACTION_DIM)), _dev("cc_states", cc_states, (n, T, CC_OBS_DIM)), _dev("v_metas", v_metas, (n, T, 3)))
    stream = C.c_void_p(torch.cuda.current_stream(first.device).cuda_stream)
    if ctx_dim or of_dim:
        _check(L.kp_rollout_record_post_x(C.byref(r), w, int(ctx_dim), int(of_dim), stream), "kp_rollout_record_post_x")
    else:
        _check(L.kp_rollout_record_post_w(C.byref(r), w, stream), "kp_rollout_record_post")


def ctx_rows_write(rows, seq: torch.Tensor | None, of: torch.Tensor | None, ctx_table: torch.Tensor | None, of_table: torch.Tensor | None):
    """The ring refill of the two wide context tables in one launch (kp_ctx_rows_write): ctx_table [R, T, H] rows `rows` <- seq [T', m, H] (time-major,
    TrajARNet.context_sequence), of_table [R, T, F] rows `rows` <- of [m, T', F]; clips of T' < T frames are padded with their last frame.  Either table
    (with its source) may be None.  rows: int64 [m], a host tensor / array (checked as it is, uploaded) or a device tensor (one host read for the
    check); no row twice.  Refused before any launch: a row outside [0, R), T' < 1 or T' > T, shapes that do not fit, host tensors."""
    L = load_library()
    tab = ctx_table if ctx_table is not None else of_table
    if tab is None:
        return
    _dev("ctx_rows_write: a table", tab, (None, None, None))
    R, T = tab.shape[:2]
    src = seq if ctx_table is not None else of
    if src is None:
        raise ValueError("ctx_rows_write: a table without its source")
    _dev("ctx_rows_write: a source", src, (None, None, None))
    m, Tp = (src.shape[1], src.shape[0]) if ctx_table is not None else (src.shape[0], src.shape[1])
    H = 0 if ctx_table is None else int(ctx_table.shape[2])
    F = 0 if of_table is None else int(of_table.shape[2])
    ptrs = [_dev("ctx_rows_write: " + k, t, shp) for k, t, shp in (("seq", seq if H else None, (Tp, m, H)), ("of", of if F else None, (m, Tp, F)),
                                                                   ("ctx_table", ctx_table, (R, T, H)), ("of_table", of_table, (R, T, F)))]
    if torch.is_tensor(rows) and rows.is_cuda:
        rows_dev = rows.to(torch.int64).contiguous()
        rows_host = rows_dev.cpu()
    else:
        rows_host = torch.as_tensor(np.asarray(rows) if not torch.is_tensor(rows) else rows).to(torch.int64).contiguous()
        rows_dev = rows_host.to(tab.device)
    if rows_host.dim() != 1 or rows_host.numel() != m:
        raise ValueError(f"ctx_rows_write: rows must be int64 [{m}] (one per clip), got {tuple(rows_host.shape)}")
    stream = C.c_void_p(torch.cuda.current_stream(tab.device).cuda_stream)
    _check(L.kp_ctx_rows_write(int(m), int(R), int(T), int(Tp), H, F, C.c_void_p(rows_dev.data_ptr()), C.c_void_p(rows_host.data_ptr()), *ptrs, stream), "kp_ctx_rows_write")


def pool_advance(done: torch.Tensor, head: torch.Tensor, ahead: torch.Tensor, row: torch.Tensor, n_slots: int):
    """Episode turnover on a ring of n_slots context rows per env (kp_pool_advance): done uint8 / bool [N]; head, ahead, row int32 [N], in place."""
    L = load_library()
    n = done.shape[0]
    stream = torch.cuda.current_stream(done.device).cuda_stream
    _check(L.kp_pool_advance(n, int(n_slots), _dev("pool_advance: done", _u8(done), None, torch.uint8),
                             *(_dev("pool_advance: " + k, t, (n,), torch.int32) for k, t in (("head", head), ("ahead", ahead), ("row", row))), C.c_void_p(stream)), "kp_pool_advance")


def _noise(who, noise, std, n, A):
    """(pointer, row stride) of the exploration noise [N, A], which may be a column slice of a wider buffer; it needs std [A]"""
    if noise is None:
        return None, 0
    if not (noise.is_cuda and noise.dtype == torch.float32 and tuple(noise.shape) == (n, A) and noise.stride(1) == 1 and std is not None and std.is_contiguous() and std.numel() == A):
        raise ValueError(f"{who}: noise [N, A] (unit column stride) needs std [A]")
    return C.c_void_p(noise.data_ptr()), int(noise.stride(0))


def mcp_compose(logits: torch.Tensor, prim: torch.Tensor, noise: torch.Tensor | None = None, std: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """sum_k softmax(logits)_k * prim[k] (+ std * noise): PolicyMCP's mixing stage in one launch (kp_mcp_compose).  logits [N, K], prim [K, N, A]
    contiguous float32 device tensors; noise [N, A] may be a column slice of a wider buffer (row stride = noise.stride(0))."""
    L = load_library()
    K, n, A = prim.shape
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and tuple(logits.shape) == (n, K) and prim.dtype == torch.float32 and prim.is_contiguous()):
        raise ValueError("mcp_compose: logits [N, K] and prim [K, N, A] must be contiguous float32 device tensors")
    nz, stride = _noise("mcp_compose", noise, std, n, A)
    out = torch.empty((n, A), device=prim.device, dtype=torch.float32) if out is None else out
    stream = torch.cuda.current_stream(prim.device).cuda_stream
    _check(L.kp_mcp_compose(n, K, A, C.c_void_p(logits.data_ptr()), C.c_void_p(prim.data_ptr()), nz, stride, None if std is None else C.c_void_p(std.data_ptr()),
                            C.c_void_p(out.data_ptr()), C.c_void_p(stream)), "kp_mcp_compose")
    return out


def mcp_tail(h2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, logits: torch.Tensor, noise: torch.Tensor | None = None,
             std: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """PolicyMCP's last layer + mixing stage (kp_mcp_tail, fp32 MFMA): h2 [K, N, J] raw second-GEMM output, b2 [K, J], w3 [K, J, A] or its
    rows zero-padded to [K, J, 80] (16-byte operand loads), b3 [K, A], logits [N, K] (composer output before the softmax); noise [N, A] may
    be a column slice of a wider buffer."""
    L = load_library()
    K, n, J = h2.shape
    A, ldw = b3.shape[1], w3.shape[2]
    if ldw < A:
        raise ValueError(f"mcp_tail: w3 [K, J, {ldw}] is narrower than b3 [K, {A}]")
    ins = [_dev("mcp_tail: " + k, t, s) for k, t, s in (("h2", h2, (K, n, J)), ("b2", b2, (K, J)), ("w3", w3, (K, J, ldw)), ("b3", b3, (K, A)), ("logits", logits, (n, K)))]
    nz, stride = _noise("mcp_tail", noise, std, n, A)
    out = torch.empty((n, A), device=h2.device, dtype=torch.float32) if out is None else out
    stream = torch.cuda.current_stream(h2.device).cuda_stream
    _check(L.kp_mcp_tail(n, K, J, A, ins[0], ins[1], ins[2], int(ldw), ins[3], ins[4], nz, stride,
                         None if std is None else C.c_void_p(std.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(stream)), "kp_mcp_tail")
    return out


def kin_advance(qpos: torch.Tensor, action: torch.Tensor, dt: float = 1.0 / 30.0, next_qpos: torch.Tensor | None = None, qvel: torch.Tensor | None = None):
    """One frame of TrajARNet's kinematic roll-out (kp_kin_advance): (next_qpos [N,76] with a unit root quaternion, finite-difference qvel [N,75])."""
    L = load_library()
    n = qpos.shape[0]
    qp, ap = _dev("kin_advance: qpos", qpos, (n, NQ)), _dev("kin_advance: action", action, (n, 80))
    next_qpos = torch.empty((n, NQ), device=qpos.device) if next_qpos is None else next_qpos
    qvel = torch.empty((n, NV), device=qpos.device) if qvel is None else qvel
    if not (next_qpos.is_contiguous() and qvel.is_contiguous()):
        raise ValueError("kin_advance: outputs must be contiguous")
    stream = torch.cuda.current_stream(qpos.device).cuda_stream
    _check(L.kp_kin_advance(n, qp, ap, float(dt), C.c_void_p(next_qpos.data_ptr()), C.c_void_p(qvel.data_ptr()),
                            C.c_void_p(stream)), "kp_kin_advance")
    return next_qpos, qvel


def kin_advance_backward(qpos: torch.Tensor, action: torch.Tensor, dt: float, grad_next_qpos: torch.Tensor | None, grad_qvel: torch.Tensor | None):
    """(d kin_advance)^T (kp_kin_advance_backward): cotangents of next_qpos [N,76] / qvel [N,75] (None: zero) -> (grad_qpos [N,76], grad_action [N,80])."""
    L = load_library()
    n = qpos.shape[0]
    ins = [_dev("kin_advance_backward: " + k, t, (n, d)) for k, t, d in (("qpos", qpos, NQ), ("action", action, 80))]
    gs = [_dev("kin_advance_backward: " + k, t, (n, d)) for k, t, d in (("grad_next_qpos", grad_next_qpos, NQ), ("grad_qvel", grad_qvel, NV))]
    gq, ga = torch.empty((n, NQ), device=qpos.device), torch.empty((n, 80), device=qpos.device)
    stream = torch.cuda.current_stream(qpos.device).cuda_stream
    _check(L.kp_kin_advance_backward(n, *ins, float(dt), *gs, C.c_void_p(gq.data_ptr()), C.c_void_p(ga.data_ptr()), C.c_void_p(stream)), "kp_kin_advance_backward")
    return gq, ga


def gru_cell_step(gi: torch.Tensor, gh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor, h: torch.Tensor, state: torch.Tensor | None = None,
                  h_out: torch.Tensor | None = None, xcat: torch.Tensor | None = None):
    """GRUCell gate math after the two bias-free gate GEMMs (kp_gru_cell_step): returns h' [N, H]; xcat [N, D + H] <- [state | h'] when given."""
    L = load_library()
    n, H = h.shape
    ok = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (gi, gh, b_ih, b_hh, h))
    if not (ok and tuple(gi.shape) == (n, 3 * H) and tuple(gh.shape) == (n, 3 * H) and b_ih.numel() == 3 * H and b_hh.numel() == 3 * H):
        raise ValueError("gru_cell_step: gi / gh [N, 3H], b_ih / b_hh [3H], h [N, H] must be contiguous float32 device tensors")
    D = 0
    if xcat is not None:
        D = state.shape[1]
        if not (state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and xcat.is_contiguous() and xcat.dtype == torch.float32 and tuple(xcat.shape) == (n, D + H)):
            raise ValueError("gru_cell_step: xcat must be a contiguous float32 [N, D + H] device tensor next to state [N, D]")
    h_out = torch.empty_like(h) if h_out is None else h_out
    stream = torch.cuda.current_stream(h.device).cuda_stream
    _check(L.kp_gru_cell_step(n, H, D, *(C.c_void_p(t.data_ptr()) for t in (gi, gh, b_ih, b_hh, h)), None if xcat is None else C.c_void_p(state.data_ptr()),
                              C.c_void_p(h_out.data_ptr()), None if xcat is None else C.c_void_p(xcat.data_ptr()), C.c_void_p(stream)), "kp_gru_cell_step")
    return h_out


def gae(rewards: torch.Tensor, masks: torch.Tensor, values: torch.Tensor, gamma: float, tau: float, last_values: torch.Tensor | None = None):
    """estimate_advantages before normalisation on env-major [N, T] float32 device tensors (k_gae); last_values [N] bootstraps
    episodes the horizon cut (kp_gae_bootstrap)."""
    L = load_library()
    n, T = rewards.shape
    ins = [_dev("gae: " + k, t, (n, T)) for k, t in (("rewards", rewards), ("masks", masks), ("values", values))]
    adv = torch.empty_like(rewards); ret = torch.empty_like(rewards)
    stream = torch.cuda.current_stream(rewards.device).cuda_stream
    _check(L.kp_gae_bootstrap(n, T, *ins, _dev("gae: last_values", last_values, (n,)), float(gamma), float(tau),
                              C.c_void_p(adv.data_ptr()), C.c_void_p(ret.data_ptr()), C.c_void_p(stream)), "kp_gae_bootstrap")
    return adv, ret
