"""The `config/statear/<id>.yml` reader: the part of kin_poly/utils/statear_smpl_config.py (`Config`, :14-128) the rollout / PPO path reads.

    cfg = Config("kin_poly", config_root="/path/to/KinPoly")        # finds config/**/kin_poly.yml as the reference does (:26-29)
    cfg = Config("/path/to/my_run.yml")                              # or a file
    agent = AgentAR(n_envs, dataset=ds, **cfg.agent_kwargs())
    cfg.apply_reward_weights(agent.env)

Same directory layout as the reference (`results/all/statear/<id>/{models,models_policy,results,log}`, :33-41), same keys, same defaults where
the reference gives one (`.get(key, default)` in Config / AgentAR).  What the engine does not take from the file, because the HIP path fixes it:
`use_action` may be true (kin_poly.yml) or false (kin_poly_wo_action.yml: the 101-d observation without the action one-hot); `use_vel` (the 75
velocities in the observation) and `use_head` (false: no head-tracking blocks) may be either too, except `use_head: false` with `use_action: false`.
`mujoco_model` (the compiled blobs of kinpoly_amd/assets are humanoid_smpl_neutral_mesh_all[_step].xml, agent_ar.py:165-169), `model_specs`
of another architecture than TrajARNet's (checked: a mismatch raises), `policy_optimizer` other than Adam (checked), `obs_*` switches other than the
kin_poly.yml values (checked).  `use_of` / `use_context` (kin_only.yml, use_of.yml) are refused by the default entry and taken by
`Config(..., entry="kin_model")`, the supervised kinematic model of scripts/exp_arnet_all.py, with the file's net sizes (`model_kwargs()`), and by
`Config(..., entry="policy_ctx")`, the roll-out / PPO scripts with the video-conditioned policy (every other check of the default entry holds there:
`policy_v: 2` and `reward_id: dynamic_supervision_v3`, which kin_only.yml and use_of.yml declare, stay refused by name).  `policy_specs.reward_id` may be
`dynamic_supervision_v1` or `dynamic_supervision_v2` (REWARD_DEFAULTS; v3 .. v6 are refused).  Nothing here needs a GPU.
"""
from __future__ import annotations

import glob
import os

import yaml

ALL_ACTIONS = ("sit", "push", "avoid", "step")

# what the kernels implement (kin_poly.yml); a config that asks for something else is refused instead of silently run differently
# key: (what the kernels implement, the reference's default when the file omits the key -- statear_smpl_config.py:118-143)
_FIXED = {"use_of": (False, True), "use_context": (False, True),
          "obs_coord": ("heading", "heading"), "root_deheading": (True, False), "obs_global": (True, False), "obs_quat": (True, False), "has_z": (True, True)}
_FIXED_MODEL = {"model_v": 1, "rnn_hdim": 1024, "mlp_hsize": [1024, 512, 256], "mlp_htype": "relu", "rnn_type": "gru"}
_FIXED_POLICY = {"policy_v": 1, "fix_std": True, "policy_htype": "relu", "policy_hsize": [512, 256], "value_htype": "relu", "value_hsize": [512, 256],
                 "policy_optimizer": "Adam", "value_optimizer": "Adam", "reward_id": "dynamic_supervision_v1", "end_reward": False}
# what Config(entry="kin_model") takes from the file instead: the supervised kinematic model runs with a context / `of` block and any net sizes
_KIN_MODEL_FREE = ("use_of", "use_context", "rnn_hdim", "mlp_hsize", "cnn_fdim")
ENTRIES = ("policy", "kin_model", "policy_ctx")
# the policy entries' reward functions and each one's own `ws.get(key, default)` list (kin_poly/core/reward_function.py:935-940, 1003-1004)
REWARD_DEFAULTS = {
    "dynamic_supervision_v1": {"w_hp": 1.0, "w_hq": 1.0, "w_p": 1.0, "w_jp": 1.0, "w_act_p": 1.0, "w_act_v": 1.0,
                               "k_hp": 1.0, "k_hq": 1.0, "k_p": 1.0, "k_jp": 0.1, "k_act_p": 0.1, "k_act_v": 0.1},
    "dynamic_supervision_v2": {"w_hp": 1.0, "w_hq": 1.0, "w_p": 0.6, "w_v": 0.1, "w_e": 0.2, "k_hp": 1.0, "k_hq": 1.0, "k_p": 2.0, "k_v": 0.005, "k_e": 20.0},
}
# why a policy entry refuses them (the error text and INTEGRATION.md say it): in the reference that path cannot run
_REFUSED_WHY = {"policy_v": "policy_v 2: PolicyAR.step_lr reads a scheduler that only policy_v == 1 creates, policy_ar.py:33-37, 88-89",
                "reward_id": "dynamic_supervision_v3 reads env.cc_cfg.policy_specs, which the UHC config does not have, reward_function.py:1055-1056"}


class ConfigError(ValueError):
    pass


class Config:
    def __init__(self, cfg_id: str, action: str = "all", wild: bool = False, base_dir: str = "results", config_root: str | None = None, create_dirs: bool = False,
                 entry: str = "policy"):
        """entry: "policy" (the rollout / PPO scripts: every check below) or "kin_model" (scripts/exp_arnet_all.py, the supervised kinematic model: `use_of`
        / `use_context` may be true and model_specs' rnn_hdim / mlp_hsize / cnn_fdim are the file's -- config/statear/kin_only.yml, use_of.yml; the reference's
        exp_arnet_all.py never reads policy_specs, so they are not checked) or "policy_ctx" (scripts/train_ar_policy.py, eval_ar_policy.py: "policy" in every
        check, except that `use_of` / `use_context` may be true and the three net sizes are the file's, as under "kin_model")."""
        if entry not in ENTRIES:
            raise ConfigError(f"Config: entry must be 'policy', 'kin_model' or 'policy_ctx', got {entry!r}")
        self.entry = entry
        if os.path.isfile(cfg_id):
            path, cfg_id = cfg_id, os.path.splitext(os.path.basename(cfg_id))[0]
        else:
            files = glob.glob(os.path.join(config_root or os.getcwd(), "config", "**", f"{cfg_id}.yml"), recursive=True)
            if len(files) != 1:
                raise ConfigError(f"expected exactly one config/**/{cfg_id}.yml under {config_root or os.getcwd()}, found {len(files)}")
            path = files[0]
        with open(path) as f:
            self.yaml_data = y = yaml.safe_load(f)
        self.id, self.path, self.action, self.wild, self.all_actions = cfg_id, path, action, bool(wild), list(ALL_ACTIONS)
        # ---- directories (:33-41)
        self.base_dir = base_dir
        self.data_dir = y.get("dataset_path", "datasets")
        self.cfg_dir = os.path.join(base_dir, "all", "statear", cfg_id)
        self.model_dir, self.policy_model_dir = os.path.join(self.cfg_dir, "models"), os.path.join(self.cfg_dir, "models_policy")
        self.result_dir, self.log_dir = os.path.join(self.cfg_dir, "results"), os.path.join(self.cfg_dir, "log")
        if create_dirs:
            for d in (self.model_dir, self.policy_model_dir, self.result_dir, self.log_dir):
                os.makedirs(d, exist_ok=True)
        # ---- data (:47-54); the meta file with the take lists is read when it is there (:58-71)
        self.data_file = y["data_wild_file"] if wild else y["data_file"]
        self.meta_id = y["meta_wild_id"] if wild else y["meta_id"]
        self.of_file = y.get("of_file_wild", "of_feat_wild_all") if wild else y.get("of_file", "of_feat_smpl_all")
        self.meta, self.takes, self.take_actions = None, {"train": [], "test": []}, {}
        meta_path = os.path.join(self.data_dir, "meta", self.meta_id + ".yml")
        if os.path.exists(meta_path):
            with open(meta_path) as f:
                self.meta = yaml.safe_load(f)
            self.take_actions = self.meta.get("action_type", {})
            for mode in ("train", "test"):
                self.takes[mode] = [t for t in self.meta.get(mode, []) if action == "all" or self.take_actions.get(t) == action]
        # ---- scalars (:74-128, with the reference's defaults)
        g = y.get
        try:            # keys the reference indexes without a default (:82-93)
            self.seed, self.fr_num, self.lr, self.num_epoch, self.save_model_interval = y["seed"], y["fr_num"], y["lr"], y["num_epoch"], y["save_model_interval"]
        except KeyError as e:
            raise ConfigError(f"{path}: required key {e} is missing") from None
        self.smooth, self.weightdecay, self.num_epoch_fix = g("smooth", False), g("weightdecay", 0.0), g("num_epoch_fix", 100)
        self.batch_size, self.noise_std, self.add_noise = g("batch_size", 128), g("noise_std", 0.0), g("add_noise", False)
        self.model_specs, self.policy_specs = dict(g("model_specs", {})), dict(g("policy_specs", {}))
        self.joint_controller = self.policy_specs.get("joint_controller", False)       # :149-150
        self.reward_weights = dict(self.policy_specs.get("reward_weights", {}))
        self.reward_id = self.policy_specs.get("reward_id", _FIXED_POLICY["reward_id"])      # a file without the key has always run dynamic_supervision_v1
        self.use_action = y.get("use_action", True)          # statear_smpl_config.py:141
        self.use_vel, self.use_head = y.get("use_vel", False), y.get("use_head", True)      # :139-140
        self.use_of, self.use_context = y.get("use_of", True), y.get("use_context", True)  # :137-138 (refused by the default entry)
        self._check_supported()

    def _check_supported(self):
        y = self.yaml_data
        kin = self.entry == "kin_model"
        free = self.entry in ("kin_model", "policy_ctx")          # the context / `of` block and the file's net sizes
        bad = [f"{k}: {y.get(k, ref)!r} (the HIP observation / step kernels implement {v!r})" for k, (v, ref) in _FIXED.items()
               if y.get(k, ref) != v and not (free and k in _KIN_MODEL_FREE)]
        for k in ("use_action", "use_vel", "use_head") + (("use_of", "use_context") if free else ()):
            if not isinstance(getattr(self, k), bool):
                bad.append(f"{k}: {getattr(self, k)!r} (true or false)")
        if self.use_head is False and self.use_action is False:
            bad.append("use_head: False with use_action: False (the context GRU would have no input: get_context_dim is 0)")
        bad += [f"model_specs.{k}: {self.model_specs[k]!r} (TrajARNet here is {v!r})" for k, v in _FIXED_MODEL.items()
                if k in self.model_specs and self.model_specs[k] != v and not (free and k in _KIN_MODEL_FREE)]
        if free:
            hs = self.model_specs.get("mlp_hsize", [1024, 512, 256])
            if not (isinstance(self.model_specs.get("rnn_hdim", 1024), int) and self.model_specs.get("rnn_hdim", 1024) > 0):
                bad.append(f"model_specs.rnn_hdim: {self.model_specs.get('rnn_hdim')!r} (a positive integer)")
            if not (isinstance(hs, list) and hs and all(isinstance(h, int) and h > 0 for h in hs)):
                bad.append(f"model_specs.mlp_hsize: {hs!r} (a list of positive integers)")
            cf = self.model_specs.get("cnn_fdim", 128)
            if not (isinstance(cf, int) and not isinstance(cf, bool) and cf > 0):
                bad.append(f"model_specs.cnn_fdim: {cf!r} (a positive integer)")
        if not kin:
            bad += [f"policy_specs.{k}: {self.policy_specs[k]!r} (implemented: {v!r}" + (f"; {_REFUSED_WHY[k]}" if k in _REFUSED_WHY else "") + ")"
                    for k, v in _FIXED_POLICY.items() if k in self.policy_specs and self.policy_specs[k] != v and k != "reward_id"]
            if self.reward_id not in REWARD_DEFAULTS:
                bad.append(f"policy_specs.reward_id: {self.reward_id!r} (implemented: {', '.join(map(repr, REWARD_DEFAULTS))}; {_REFUSED_WHY['reward_id']})")
        if bad:
            raise ConfigError(f"{self.path}: not supported by the batched engine -- " + "; ".join(bad))

    # ------------------------------------------------------------------ what the engine is built from
    def feature_path(self, data_file: str | None = None) -> str:
        """<dataset_path>/features/<data_file>.p (DatasetAMASSBatch / StateARDataset, statear_smpl_dataset.py:38-39)"""
        return os.path.join(self.data_dir, "features", (data_file or self.data_file) + ".p")

    def model_kwargs(self) -> dict:
        """What scripts/exp_arnet_all.py passes on from model_specs: the net sizes (exp_arnet.build_net) and compute_loss's weights (the reference's
        defaults where the file omits one, traj_ar_smpl_net.py:40-41, 391-399); kin_poly.yml gives the engine's own defaults."""
        ms = self.model_specs
        w = {k: float(ms.get(k, d)) for k, d in (("w_rp", 50), ("w_rr", 50), ("w_p", 1), ("w_v", 1), ("w_ee", 1), ("w_op", 1), ("w_or", 1))}
        return dict(rnn_hdim=int(ms.get("rnn_hdim", 512)), mlp_hsize=tuple(ms.get("mlp_hsize", [1024, 512])), **w)

    def of_feature_path(self) -> str:
        """<dataset_path>/features/<of_file>.p: the image features of `use_of` (of_file / of_file_wild; statear_smpl_dataset.py:40-41)"""
        return os.path.join(self.data_dir, "features", self.of_file + ".p")

    def context_kwargs(self, of_dim: int | None = None) -> dict:
        """The video-conditioned part of AgentAR's arguments under entry "policy_ctx": use_context, of_dim (the feature file's width when the caller
        has read it, else model_specs.cnn_fdim) and the net sizes the file names, read through model_kwargs(); a size the file omits stays the
        engine's (AgentAR's default, what the default entry has always run such a file with).  Empty under another entry."""
        if self.entry != "policy_ctx":
            return {}
        mk = self.model_kwargs()
        of = (int(of_dim) if of_dim is not None else int(self.model_specs.get("cnn_fdim", 128))) if self.use_of else 0
        return dict(use_context=bool(self.use_context), of_dim=of, **{k: mk[k] for k in ("rnn_hdim", "mlp_hsize") if k in self.model_specs})

    def agent_kwargs(self, of_dim: int | None = None) -> dict:
        """AgentAR(...) keyword arguments for this file (agent_ar.py:60-99, 184-225: the optimisers, schedules, PPO and sampling constants); under entry
        "policy_ctx" also context_kwargs(of_dim)."""
        ps = self.policy_specs
        missing = [k for k in ("num_optim_epoch", "gamma", "tau", "clip_epsilon", "policy_lr", "value_lr", "log_std") if k not in ps]     # indexed without a default (:88-91, 190, 204)
        if missing:
            raise ConfigError(f"{self.path}: policy_specs lacks {missing}")
        return dict(seed=self.seed, wild=self.wild, policy_lr=ps.get("policy_lr", 1e-5), value_lr=ps.get("value_lr", 3e-4), supervised_lr=self.lr,
                    num_optim_epoch=ps.get("num_optim_epoch", 10), num_step_update=ps.get("num_step_update", 10), gamma=ps.get("gamma", 0.95), tau=ps.get("tau", 0.95),
                    clip_epsilon=ps.get("clip_epsilon", 0.2), rl_update=ps.get("rl_update", False), step_update=ps.get("step_update", False),
                    sampling_temp=ps.get("sampling_temp", 0.5), sampling_freq=ps.get("sampling_freq", 0.9), num_epoch_fix=self.num_epoch_fix, num_epoch=self.num_epoch,
                    joint_controller=bool(self.joint_controller), grad_joint=ps.get("grad_joint", False), grad_alternate=ps.get("grad_alternate", False),
                    log_std=ps.get("log_std", -3.2), policy_weightdecay=ps.get("policy_weightdecay", 0.0), value_weightdecay=ps.get("value_weightdecay", 0.0),
                    smooth=bool(self.smooth), init_update=ps.get("init_update", False), num_init_update=int(ps.get("num_init_update", 5)),
                    step_update_dyna=ps.get("step_update_dyna", False), num_step_dyna_update=int(ps.get("num_step_dyna_update", 10)), full_update=ps.get("full_update", False),
                    num_sample=int(self.yaml_data.get("num_sample", 20000)), batch_size=int(self.batch_size),
                    noise_std=float(self.noise_std) if self.add_noise else 0.0, use_action=self.use_action, use_vel=self.use_vel, use_head=self.use_head,
                    **self.context_kwargs(of_dim))

    def horizon(self, n_envs: int, world_size: int = 1, floor: int = 1) -> int:
        """Steps per env and iteration so that the job collects at least `min_batch_size` samples (agent_ar.py:277: `self.sample(min_batch_size)`;
        the forked workers stop at min_batch_size / num_threads each, :516, 600)."""
        need = int(self.policy_specs.get("min_batch_size", 10000))
        return max(floor, -(-need // (n_envs * world_size)))

    def apply_reward_weights(self, env):
        """policy_specs.reward_id / reward_weights -> the reward kernel and its constants: dynamic_supervision_v1's or _v2's own `ws.get(key, default)`
        list (REWARD_DEFAULTS).  An env that knows one reward only (no set_reward) keeps it: v1."""
        if hasattr(env, "set_reward"):
            env.set_reward(self.reward_id)
        for k, d in REWARD_DEFAULTS[self.reward_id].items():
            setattr(env.reward_cfg, k, float(self.reward_weights.get(k, d)))
        if int(self.reward_weights.get("v_ord", 2)) != 2:
            raise ConfigError("reward_weights.v_ord must be 2 (the angular-velocity term of the reward kernel is the L2 norm)")
        return env.reward_cfg

    def cc_checkpoint_path(self, cc_iter: int | None = None, proj_name: str = "motion_im"):
        """The UHC checkpoint the env loads (humanoid_ar_v1.py:69-76): results/<proj_name>/<cc_cfg>/models/iter_%04d.p, cc_iter -1 = the latest in that
        directory.  None when there is none."""
        d = os.path.join(self.base_dir, proj_name, self.policy_specs.get("cc_cfg", "uhc"), "models")
        it = self.policy_specs.get("cc_iter", -1) if cc_iter is None else cc_iter
        if it == -1:
            have = [int(f.split("_")[-1].split(".")[0]) for f in (os.listdir(d) if os.path.isdir(d) else []) if f.startswith("iter_") and f.endswith(".p")]
            if not have:
                return None
            it = max(have)
        p = os.path.join(d, "iter_%04d.p" % it)
        return p if os.path.exists(p) else None

    def checkpoint_path(self, i_iter: int) -> str:
        """'%s/iter_%04d.p' % (policy_model_dir, epoch + 1)   (agent_ar.py:363)"""
        return os.path.join(self.policy_model_dir, "iter_%04d.p" % i_iter)
