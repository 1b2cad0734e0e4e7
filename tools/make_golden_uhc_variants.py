"""Generate the fixtures of the UHC config's observation / actor variants by IMPORTING the reference's Python, as tools/make_golden.py does (where a
reference checkout can be imported; only data is written, no reference source):

    tests/golden/uhc_obs_variants.npz      HumanoidEnv.get_full_obs / _v1 / _v2 (uhc/envs/humanoid_im.py:112-318) on oracle states for every obs_v,
                                           obs_vel 'full' / 'root' and obs_v 0's obs_heading / root_deheading / obs_phase on and off
    tests/golden/uhc_controller_variants.npz  HumanoidEnv.compute_torque (humanoid_im.py:433-480) for action_v 0 / 1 x meta_pd / meta_pd_joint / none x
                                           residual force on / off at several substep indices, with the fullM / qfrc_bias it was given
    tests/golden/uhc_policy_gaussian.npz   PolicyGaussian (uhc/khrylib/rl/core/policy_gaussian.py) in fp64: state_dict, inputs, action mean
    tests/golden/uhc_variants/*.yml        settings-only variant files (uhc.yml with a few keys changed or dropped)
    tests/golden/uhc_variants_config.json  the reference copycat_config.Config attributes of each of those files

make_golden.py is imported for its stubs and helpers (its own generation runs only under __main__).  MuJoCo-side inputs (body_xpos, xquat, xipos)
come from this repository's fp64 oracle at the state itself (no stale substep), so a simulator handle set to the same qpos computes the same arrays.

    python tools/make_golden_uhc_variants.py [reference checkout]      (from an empty working directory)
"""
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs the reference's absent dependencies, puts the reference and this repository on sys.path)

OUT = G.OUT
VDIR = os.path.join(OUT, "uhc_variants")

# (obs_v, obs_vel, obs_heading, root_deheading, obs_phase): every combination the kernel instantiates
OBS_VARIANTS = [(1, "full", 0, 0, 0), (1, "root", 0, 0, 0), (2, "full", 0, 0, 0), (2, "root", 0, 0, 0)] + \
    [(0, vel, h, d, p) for vel in ("full", "root") for h in (0, 1) for d in (0, 1) for p in (0, 1)]

# variant files: uhc.yml with these top-level keys replaced (None: key dropped, so the reference default applies)
YML_VARIANTS = {
    "uhc_v0_gauss": {"obs_v": 0, "obs_heading": True, "root_deheading": True, "obs_phase": True, "actor_type": "gauss", "env_term_body": None},
    "uhc_v2_root": {"obs_v": 2, "obs_vel": "root"},
    "uhc_v1_root_gauss": {"obs_vel": "root", "actor_type": "gauss", "policy_hsize": [256, 128]},
    "uhc_v0_plain": {"obs_v": 0, "obs_phase": None, "env_episode_len": 60},
    "uhc_meta_pd": {"meta_pd": True},
    "uhc_ctrl_defaults": {"obs_v": None, "action_v": None, "residual_force": None, "actor_type": None, "obs_phase": None, "env_term_body": None},
    "uhc_meta_joint_v0": {"meta_pd_joint": True, "action_v": 0, "residual_force": False, "obs_v": 2},
    "uhc_defaults": {"obs_v": None, "action_v": None, "residual_force": None, "actor_type": None, "reward_id": None, "obs_phase": None, "env_term_body": None},
}
CONFIG_ATTRS = ["obs_v", "obs_type", "obs_coord", "obs_phase", "obs_heading", "obs_vel", "root_deheading", "action_type", "action_v", "residual_force",
                "residual_force_scale", "residual_force_lim", "residual_force_mode", "meta_pd", "meta_pd_joint", "actor_type", "env_term_body",
                "env_episode_len", "env_init_noise", "env_expert_trail_steps", "gamma", "tau", "policy_hsize", "policy_htype", "policy_lr", "value_lr",
                "clip_epsilon", "log_std", "fix_std", "num_optim_epoch", "min_batch_size", "reward_id", "reward_weights"]


def gen_obs_variants(hum):
    rng = np.random.default_rng(707)
    n, T = 12, 6
    clip = np.stack([G.rand_qpos(rng, 0.2) for _ in range(T)])
    fk = [hum.qpos_fk(q.copy()) for q in clip]
    expert = {"qpos": clip, "wbpos": np.stack([f["wbpos"].reshape(-1) for f in fk]), "wbquat": np.stack([f["wbquat"].reshape(-1) for f in fk]),
              "body_com": np.stack([f["body_com"].reshape(-1) for f in fk]), "len": T, "meta": {"cyclic": False}}
    env = G.make_env(G.him.HumanoidEnv)
    env.expert, env.start_ind = expert, 0
    env.cc_cfg.obs_type = "full"
    rec = {k: [] for k in ("qpos", "qvel", "t")}
    obs = {v: [] for v in OBS_VARIANTS}
    for i in range(n):
        q0 = G.rand_qpos(rng, 0.2); v0 = rng.normal(size=75) * 0.4
        if i == 3:
            q0[3:7] = [1.0, 0.0, 0.0, 0.0]          # heading 0
        env.data = G.oracle_data(q0, v0, stale_steps=0)
        env.cur_t = i % (T - 1)
        for v in OBS_VARIANTS:
            cc = env.cc_cfg
            cc.obs_v, cc.obs_vel, cc.obs_heading, cc.root_deheading, cc.obs_phase = v[0], v[1], bool(v[2]), bool(v[3]), bool(v[4])
            obs[v].append(env.get_obs())
        rec["qpos"].append(q0); rec["qvel"].append(v0); rec["t"].append(env.cur_t)
    out = {k: np.stack(x) for k, x in rec.items()}
    out["clip"], out["len"] = clip, T
    out["variants"] = np.array([[v[0], v[1] == "root", v[2], v[3], v[4]] for v in OBS_VARIANTS], dtype=np.int64)
    for j, v in enumerate(OBS_VARIANTS):
        out[f"obs_{j}"] = np.stack(obs[v])
    np.savez_compressed(os.path.join(OUT, "uhc_obs_variants.npz"), **out)


# (action_v, meta: 0 none / 1 meta_pd / 2 meta_pd_joint, residual force 0 / 1)
CTRL_VARIANTS = [(0, 0, 1), (1, 1, 1), (1, 2, 0), (0, 1, 0), (1, 0, 0), (0, 2, 1)]


def gen_controller_variants(ref):
    import yaml
    rng = np.random.default_rng(808)
    with open(os.path.join(ref, "config", "uhc", "uhc.yml")) as f:
        a_ref = np.deg2rad(np.array([r[3] for r in yaml.safe_load(f)["joint_params"]], float))
    env = G.make_env(G.him.HumanoidEnv)
    G.patch_fullM()
    env.cc_cfg.a_ref = a_ref
    env.start_ind, env.cur_t = 0, 0
    rec = {k: [] for k in ("variant", "state", "ctrl", "i_iter", "torque")}
    st = {k: [] for k in ("qpos", "qvel", "M", "bias", "expert_qpos")}
    for i in range(6):
        q0 = G.rand_qpos(rng, 0.3); v0 = rng.normal(size=75) * 0.5
        d = G.oracle_data(q0, v0)
        d.qfrc_bias = d.qfrc_bias[:75]
        env.data = d; env.model.nv = 75
        G.patch_fullM.M = d._M
        eq = G.rand_qpos(rng, 0.3)
        if i % 2 == 0:
            eq[7:] += 2 * np.pi * rng.integers(-1, 2, size=69)      # the 2 pi unwrap of action_v 1 (and its absence for action_v 0's a_ref)
        env.expert = {"qpos": eq[None].copy(), "len": 1, "meta": {"cyclic": False}}
        for k, v in (("qpos", d.qpos[:76].copy()), ("qvel", d.qvel[:75].copy()), ("M", d._M), ("bias", d.qfrc_bias[:75].copy()), ("expert_qpos", eq)):
            st[k].append(v)
        for vi, (av, meta, rfc) in enumerate(CTRL_VARIANTS):
            cc = env.cc_cfg
            cc.action_v, cc.meta_pd, cc.meta_pd_joint = av, meta == 1, meta == 2
            env.vf_dim = 6 if rfc else 0
            env.meta_pd_dim = 30 if meta == 1 else (138 if meta == 2 else 0)
            A = 69 + env.vf_dim + env.meta_pd_dim
            for it in (0, 7, 14):
                ctrl = np.zeros(213)
                ctrl[:A] = rng.normal(size=A) * 0.5
                if meta:
                    ctrl[69 + env.vf_dim:A] = rng.uniform(-1.5, 10.5, A - 69 - env.vf_dim)      # both clip bounds of clip(m + 1, 0, 10)
                tau = env.compute_torque(ctrl[:A].copy(), i_iter=it)
                for k, v in (("variant", vi), ("state", i), ("ctrl", ctrl), ("i_iter", it), ("torque", tau)):
                    rec[k].append(v)
    out = {k: np.array(v) for k, v in rec.items()}
    out.update({k: np.stack(v) for k, v in st.items()})
    out["variants"], out["a_ref"] = np.array(CTRL_VARIANTS), a_ref
    np.savez_compressed(os.path.join(OUT, "uhc_controller_variants.npz"), **out)


def gen_policy_gaussian():
    import types
    import torch
    from uhc.khrylib.rl.core.policy_gaussian import PolicyGaussian
    torch.manual_seed(9)
    cfg = types.SimpleNamespace(policy_hsize=[64, 48], policy_htype="tanh", fix_std=True, log_std=-2.3)
    pol = PolicyGaussian(cfg, action_dim=75, state_dim=219).double()
    with torch.no_grad():                         # the 0.1-scaled head would hide the hidden layers' digits: give it full-size weights
        pol.action_mean.weight.normal_(0, 0.3); pol.action_mean.bias.normal_(0, 0.1)
    x = torch.randn(16, 219, dtype=torch.float64)
    dist = pol(x)
    out = {"x": x.numpy(), "mean": dist.loc.detach().numpy(), "std": dist.scale.detach().numpy(), "hsize": np.array(cfg.policy_hsize), "htype": cfg.policy_htype}
    for k, v in pol.state_dict().items():
        out["sd__" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "uhc_policy_gaussian.npz"), **out)


def gen_variant_configs(ref):
    import yaml
    from uhc.utils.config_utils.copycat_config import Config
    with open(os.path.join(ref, "config", "uhc", "uhc.yml")) as f:
        base = yaml.safe_load(f)
    os.makedirs(VDIR, exist_ok=True)
    attrs = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.symlink(os.path.join(ref, "assets"), os.path.join(tmp, "assets"))
        for name, change in YML_VARIANTS.items():
            y = dict(base)
            for k, v in change.items():
                if v is None:
                    y.pop(k, None)
                else:
                    y[k] = v
            with open(os.path.join(VDIR, name + ".yml"), "w") as f:
                f.write(f"# uhc.yml with {', '.join(sorted(change))} changed or dropped (tools/make_golden_uhc_variants.py)\n")
                yaml.safe_dump(y, f, sort_keys=False, default_flow_style=None, width=200)
            c = Config(cfg_id=name, base_dir=tmp, cfg_dict=y)
            attrs[name] = {a: (getattr(c, a).tolist() if isinstance(getattr(c, a), np.ndarray) else getattr(c, a)) for a in CONFIG_ATTRS}
    with open(os.path.join(OUT, "uhc_variants_config.json"), "w") as f:
        json.dump(attrs, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else G.REF
    gen_obs_variants(G.make_humanoid())
    gen_controller_variants(ref)
    gen_policy_gaussian()
    gen_variant_configs(ref)
    for f in ("uhc_obs_variants.npz", "uhc_controller_variants.npz", "uhc_policy_gaussian.npz", "uhc_variants_config.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)))
