"""The UHC `config/uhc/<id>.yml` reader: the part of uhc/utils/config_utils/copycat_config.py (`Config`, :12-146) that the batched imitation env,
its controller and scripts/train_uhc.py read, with the reference's defaults where a key is missing (:16-112).

    cfg = UhcConfig("uhc", config_root="/path/to/KinPoly")       # finds config/**/uhc.yml as the reference does (base_config.py:18-21)
    cfg = UhcConfig("/path/to/my_controller.yml")                # or a file
    env = BatchedHumanoidEnv(n_envs, cfg=cfg)

What the engine runs of the file: the observation switches obs_v (0 get_full_obs, 1 get_full_obs_v1, 2 get_full_obs_v2), obs_vel ('full' / 'root'),
and obs_v 0's obs_heading / root_deheading / obs_phase (the HIP kernel k_obs_cc); actor_type 'gauss' (PolicyGaussian) or 'mcp' (PolicyMCP);
env_term_body 'body' (calc_body_diff > 0.5) or the default 'head', which the reference's if / elif chain never matches (humanoid_im.py:554-561), so
such an episode never fails; the PPO constants; reward_id (the five implicit-RFC functions of the reward registry, REWARD_DEFAULTS; the two explicit
ones and the default 'quat' are refused, REFUSED_REWARDS) and reward_weights with that function's own defaults; the controller's action_v (1: PD target about the expert's kinematic pose, 0: about
a_ref = deg2rad of joint_params column 3, without the 2 pi unwrap), residual_force (implicit, or off) and meta_pd / meta_pd_joint (the step kernel's
extended controller, cc_action_v / cc_rfc / cc_meta_pd).  Any other value of a key the engine reads is refused with a ConfigError that names the key,
the value and what is implemented, instead of running as if the file were uhc.yml.  Nothing here needs a GPU.
"""
from __future__ import annotations

import glob
import math
import os

import yaml

from .config import ConfigError

NDOF = 69                   # actuated joint angles (model.actuator_ctrlrange.shape[0])


# the reward registry (uhc/core/reward_function.py:453-460): every function's own `ws.get(key, default)` list -- the same key has different defaults
# in different functions (k_p 2 / 0.4, k_c 1000 / 100, w_vf 0 / 0.1 / 1)
REWARD_DEFAULTS = {
    "world_rfc_implicit": dict(w_p=0.6, w_v=0.1, w_e=0.2, w_c=0.1, w_vf=0.0, k_p=2.0, k_v=0.005, k_e=20.0, k_c=1000.0, k_vf=1.0),                      # :7-9
    "world_rfc_implicit_v1_mul": dict(k_p=2.0, k_v=0.005, k_e=20.0, k_c=1000.0, k_vf=1.0),                                                             # :60
    "local_rfc_implicit": dict(w_p=0.5, w_v=0.0, w_e=0.2, w_rp=0.1, w_rv=0.1, w_vf=0.1, k_p=2.0, k_v=0.005, k_e=20.0, k_vf=1.0,
                               k_rh=300.0, k_rq=300.0, k_rl=5.0, k_ra=0.5),                                                                            # :176-178
    "world_rfc_implicit_v2": dict(k_p=0.4, k_wp=0.4, k_v=0.005, k_j=100.0, k_c=100.0, k_vf=1.0),                                                       # :305-307
    "world_rfc_implicit_v3": dict(w_p=0.4, w_wp=0.4, w_v=0.005, w_j=100.0, w_c=100.0, w_vf=1.0, k_p=0.4, k_wp=0.4, k_v=0.005, k_j=100.0, k_c=100.0,
                                  k_vf=1.0),                                                                                                           # :380-385
}
_EXPLICIT_WHY = ("it reads env.vf_bodies / env.body_vf_dim, which only residual_force_mode 'explicit' sets (humanoid_im.py:76-82), and that mode "
                 "cannot run in the reference")
REFUSED_REWARDS = {"world_rfc_explicit": _EXPLICIT_WHY, "local_rfc_explicit": _EXPLICIT_WHY,
                   "quat": "the reference's default names no function of its registry (reward_function.py:453-460)"}


def uhc_obs_dim(obs_v: int, obs_vel: str = "full", obs_heading: bool = False, obs_phase: bool = True) -> int:
    """Width of HumanoidEnv.get_obs() (humanoid_im.py:105-318): obs_v 1 = 784 / 715 (obs_vel full / root), obs_v 2 = v1 without the two COM blocks,
    obs_v 0 = obs_heading + qpos[2:] (74) + qvel (75) or qvel[:6] + kin pose (69) + obs_phase."""
    lv = 75 if obs_vel == "full" else 6
    if obs_v == 0:
        return int(bool(obs_heading)) + 74 + lv + NDOF + int(bool(obs_phase))
    return 229 + lv + (4 if obs_v == 1 else 2) * 72 + 2 * 96


def uhc_action_dim(residual_force: bool = True, residual_force_mode: str = "implicit", meta_pd: bool = False, meta_pd_joint: bool = False) -> int:
    """HumanoidEnv.set_spaces (humanoid_im.py:68-89): ndof + vf_dim (6 for implicit RFC) + meta_pd_dim (2 x 15 substeps, or 2 x 69 joints)."""
    vf = 6 if residual_force and residual_force_mode == "implicit" else 0
    meta = 30 if meta_pd else (2 * NDOF if meta_pd_joint else 0)
    return NDOF + vf + meta


class UhcConfig:
    def __init__(self, path_or_id: str, config_root: str | None = None, check: bool = True):
        """check=False reads the file without refusing what the engine does not run (for tools that only inspect it)."""
        if os.path.isfile(path_or_id):
            path, cfg_id = path_or_id, os.path.splitext(os.path.basename(path_or_id))[0]
        else:
            root = config_root or os.getcwd()
            files = glob.glob(os.path.join(root, "config", "**", f"{path_or_id}.yml"), recursive=True)
            if len(files) != 1:
                raise ConfigError(f"expected exactly one config/**/{path_or_id}.yml under {root}, found {len(files)}")
            path, cfg_id = files[0], path_or_id
        with open(path) as f:
            self.yaml_data = y = yaml.safe_load(f) or {}
        self.id, self.path = cfg_id, path
        self.data_specs = dict(y.get("data_specs", None) or {})          # DatasetAMASSSingle's settings (read here, used by kinpoly_amd.dataset.AmassSingleDataset)
        g = y.get
        # ---- training constants (copycat_config.py:16-44)
        self.gamma, self.tau = g("gamma", 0.95), g("tau", 0.95)
        self.policy_htype, self.policy_hsize = g("policy_htype", "relu"), list(g("policy_hsize", [300, 200]))
        self.policy_optimizer, self.policy_lr = g("policy_optimizer", "Adam"), g("policy_lr", 5e-5)
        self.value_htype, self.value_hsize = g("value_htype", "relu"), list(g("value_hsize", [300, 200]))
        self.value_optimizer, self.value_lr = g("value_optimizer", "Adam"), g("value_lr", 3e-4)
        self.clip_epsilon, self.log_std, self.fix_std = g("clip_epsilon", 0.2), g("log_std", -2.3), g("fix_std", False)
        self.num_optim_epoch, self.min_batch_size = g("num_optim_epoch", 10), g("min_batch_size", 50000)
        self.mini_batch_size = g("mini_batch_size", self.min_batch_size)
        self.max_iter_num, self.seed, self.save_model_interval = g("max_iter_num", 1000), g("seed", 1), g("save_model_interval", 100)
        self.reward_id, self.reward_weights, self.end_reward = g("reward_id", "quat"), dict(g("reward_weights", None) or {}), g("end_reward", False)
        self.actor_type = g("actor_type", "gauss")
        self.num_primitive = g("num_primitive", 8) if self.actor_type == "mcp" else None
        self.composer_dim = list(g("composer_dim", [300, 200]))          # PolicyMCP's composer MLP (policy_mcp.py:26)
        # ---- env (:64-97)
        self.env_init_noise, self.env_episode_len = g("env_init_noise", 0.0), g("env_episode_len", 200)
        self.env_term_body, self.env_expert_trail_steps = g("env_term_body", "head"), g("env_expert_trail_steps", 0)
        self.obs_v, self.obs_type, self.obs_coord = g("obs_v", 0), g("obs_type", "full"), g("obs_coord", "root")
        self.obs_phase, self.obs_heading, self.obs_vel = g("obs_phase", True), g("obs_heading", False), g("obs_vel", "full")
        self.root_deheading = g("root_deheading", False)
        self.action_type, self.action_v = g("action_type", "position"), g("action_v", 0)
        # ---- residual force, meta-PD (:100-110)
        self.residual_force, self.residual_force_scale = g("residual_force", False), g("residual_force_scale", 200.0)
        self.residual_force_lim, self.residual_force_mode = g("residual_force_lim", 100.0), g("residual_force_mode", "implicit")
        self.meta_pd, self.meta_pd_joint = g("meta_pd", False), g("meta_pd_joint", False)
        # ---- joint parameter multipliers (:123-130)
        self.jkp_multiplier = g("jkp_multiplier", 1.0)
        self.jkd_multiplier = g("jkd_multiplier", self.jkp_multiplier)
        self.torque_limit_multiplier = g("torque_limit_multiplier", 1.0)
        # a_ref: the PD base pose of action_v 0 (copycat_config.py:126-127: np.deg2rad of joint_params column 3)
        jp = y.get("joint_params")
        self.a_ref = [math.radians(float(r[3])) for r in jp] if jp else None
        if check:
            self._check_supported()

    # ------------------------------------------------------------------ what the engine refuses
    def _check_supported(self):
        bad = []

        def need(key, value, ok, implemented):
            if not ok:
                bad.append(f"{key}: {value!r} (implemented: {implemented})")

        need("obs_type", self.obs_type, self.obs_type == "full", "'full'")
        need("obs_coord", self.obs_coord, self.obs_coord == "root", "'root'")
        need("obs_v", self.obs_v, self.obs_v in (0, 1, 2), "0, 1 or 2")
        need("obs_vel", self.obs_vel, self.obs_vel in ("full", "root"), "'full' or 'root'")
        for k in ("obs_heading", "root_deheading", "obs_phase"):
            need(k, getattr(self, k), isinstance(getattr(self, k), bool), "true or false")
        need("action_type", self.action_type, self.action_type == "position",
             "'position' (the stable-PD controller of the step kernel)")
        need("action_v", self.action_v, self.action_v in (0, 1), "0 (PD target about a_ref) or 1 (about the expert's kinematic pose)")
        need("residual_force", self.residual_force, isinstance(self.residual_force, bool), "true or false")
        if self.action_v == 0 and (self.a_ref is None or len(self.a_ref) != NDOF):
            bad.append(f"joint_params: {'missing' if self.a_ref is None else len(self.a_ref)} rows (action_v 0 takes its base pose a_ref from {NDOF} rows)")
        need("residual_force_mode", self.residual_force_mode, self.residual_force_mode == "implicit",
             "'implicit' (the reference's rfc_explicit calls pos_body2world / vec_body2world, which it does not define)")
        need("meta_pd", self.meta_pd, isinstance(self.meta_pd, bool), "true or false")
        need("meta_pd_joint", self.meta_pd_joint, isinstance(self.meta_pd_joint, bool), "true or false")
        need("actor_type", self.actor_type, self.actor_type in ("gauss", "mcp"), "'gauss' (PolicyGaussian) or 'mcp' (PolicyMCP)")
        need("env_term_body", self.env_term_body, self.env_term_body in ("head", "body"),
             "'body' (calc_body_diff) or 'head' (never fails, as in the reference)")
        if self.reward_id in REFUSED_REWARDS:
            bad.append(f"reward_id: {self.reward_id!r} (implemented: {', '.join(map(repr, REWARD_DEFAULTS))}; {REFUSED_REWARDS[self.reward_id]})")
        else:
            need("reward_id", self.reward_id, self.reward_id in REWARD_DEFAULTS, ", ".join(map(repr, REWARD_DEFAULTS)))
        jw = self.reward_weights.get("jpos_diffw")
        if jw is not None and (not isinstance(jw, (list, tuple)) or len(jw) != 24):
            bad.append(f"reward_weights.jpos_diffw: {jw!r} (implemented: 24 numbers, one per body)")
        for k, v in (("residual_force_scale", 100.0), ("residual_force_lim", 100.0)):
            need(k, getattr(self, k), float(getattr(self, k)) == v, f"{v:g} (the compiled model blob carries uhc.yml's)")
        for k in ("jkp_multiplier", "jkd_multiplier", "torque_limit_multiplier"):
            need(k, getattr(self, k), float(getattr(self, k)) == 1.0, "1 (the compiled gains and torque limits do not carry a multiplier)")
        if int(self.reward_weights.get("v_ord", 2)) != 2:
            bad.append(f"reward_weights.v_ord: {self.reward_weights['v_ord']!r} (implemented: 2)")
        if bad:
            raise ConfigError(f"{self.path}: not supported by the batched engine -- " + "; ".join(bad))

    # ------------------------------------------------------------------ what the engine is built from
    @property
    def obs_dim(self) -> int:
        return uhc_obs_dim(self.obs_v, self.obs_vel, self.obs_heading, self.obs_phase)

    @property
    def action_dim(self) -> int:
        return uhc_action_dim(self.residual_force, self.residual_force_mode, self.meta_pd, self.meta_pd_joint)

    @property
    def vf_dim(self) -> int:
        return 6 if self.residual_force and self.residual_force_mode == "implicit" else 0

    @property
    def is_default_controller(self) -> bool:
        """True for uhc.yml's observation and controller (obs_v 1, full velocities, action_v 1, residual force, no meta-PD): what the kinematic-policy env runs."""
        return self.obs_v == 1 and self.obs_vel == "full" and self.action_v == 1 and self.vf_dim == 6 and self.meta_pd_mode == 0

    @property
    def meta_pd_mode(self) -> int:
        """0 none, 1 meta_pd (by substep), 2 meta_pd_joint (by joint); meta_pd wins when both are set (humanoid_im.py:84-89, 453-466)"""
        return 1 if self.meta_pd else (2 if self.meta_pd_joint else 0)

    def model_options(self) -> dict:
        """KpModel(**options) for this controller (kp_model_set_option's cc_obs_* and cc_action_v / cc_rfc / cc_meta_pd)."""
        v0 = self.obs_v == 0
        return {"cc_action_v": int(self.action_v), "cc_rfc": int(self.vf_dim > 0), "cc_meta_pd": self.meta_pd_mode,"cc_obs_v": int(self.obs_v), "cc_obs_vel_root": int(self.obs_vel == "root"), "cc_obs_heading": int(v0 and self.obs_heading),
                "cc_obs_deheading": int(v0 and self.root_deheading), "cc_obs_phase": int(v0 and self.obs_phase)}

    def make_value(self):
        """The critic of scripts/train_uhc.py:154: Value(MLP(state_dim, value_hsize, value_htype))."""
        from .nets import MLP, Value
        return Value(MLP(self.obs_dim, tuple(self.value_hsize), self.value_htype))

    def full_reward_weights(self) -> dict:
        """reward_func[reward_id]'s `ws.get(key, default)` with that function's own defaults (REWARD_DEFAULTS); for v2 / v3 also `jpos_diffw`, the
        24 numbers of reward_weights.jpos_diffw (default all 1; not cfg.jpos_diffw)."""
        d = dict(REWARD_DEFAULTS.get(self.reward_id, REWARD_DEFAULTS["world_rfc_implicit"]))
        d.update({k: float(v) for k, v in self.reward_weights.items() if k in d})
        if self.reward_id in ("world_rfc_implicit_v2", "world_rfc_implicit_v3"):
            d["jpos_diffw"] = [float(v) for v in self.reward_weights.get("jpos_diffw", [1.0] * 24)]
        return d

    def ppo_kwargs(self) -> dict:
        """CopycatAgent(...) keyword arguments (the PPO constants of agent_copycat / train_uhc.py)."""
        return dict(gamma=self.gamma, tau=self.tau, clip_epsilon=self.clip_epsilon, policy_lr=self.policy_lr, value_lr=self.value_lr,
                    num_optim_epoch=self.num_optim_epoch)

    def make_policy(self):
        """The actor actor_type names at this config's widths (PolicyGaussian: policy_gaussian.py:7-28; PolicyMCP: policy_mcp.py)."""
        from .nets import PolicyGaussian, PolicyMCP
        if self.actor_type == "mcp":
            return PolicyMCP(self.obs_dim, self.action_dim, tuple(self.policy_hsize), self.policy_htype, self.num_primitive, tuple(self.composer_dim),
                             log_std=self.log_std, fix_std=bool(self.fix_std))
        return PolicyGaussian(self.obs_dim, self.action_dim, tuple(self.policy_hsize), self.policy_htype, log_std=self.log_std, fix_std=bool(self.fix_std))


def require_uhc_yml_controller(cc_cfg) -> None:
    """The kinematic-policy env (HumanoidAREnv) drives uhc.yml's controller: the 784-d get_full_obs_v1 and PolicyMCP.  A cc config of another variant
    raises a ConfigError naming the key instead of loading a policy of the wrong shapes.  Duck-typed: attributes the object lacks are not checked."""
    want = (("obs_v", 1), ("obs_vel", "full"), ("actor_type", "mcp"), ("action_v", 1), ("residual_force", True), ("residual_force_mode", "implicit"),
            ("meta_pd", False), ("meta_pd_joint", False), ("action_type", "position"))
    bad = [f"{k}: {getattr(cc_cfg, k)!r} (the kinematic-policy env runs {v!r})" for k, v in want if hasattr(cc_cfg, k) and getattr(cc_cfg, k) != v]
    if bad:
        raise ConfigError(f"{getattr(cc_cfg, 'path', 'cc_cfg')}: not uhc.yml's controller -- " + "; ".join(bad))
