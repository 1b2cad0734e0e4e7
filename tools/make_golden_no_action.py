"""Generate the fixtures of the no-action-label ablation (config/statear/kin_poly_wo_action.yml, `use_action: false`) by IMPORTING the reference's
Python, as tools/make_golden.py does (where a reference checkout can be imported; only data is written, no reference source):

    tests/golden/ar_obs_no_action.npz       HumanoidAREnv.get_ar_obs_v1 with use_action off (humanoid_ar_v1.py:133-214): 101 floats per row
    tests/golden/traj_ar_net_no_action.npz  TrajARNet(use_action=False): seeded init_states, context features, whole-clip forward (gen_traj_ar_net's)
    tests/golden/pretrain_no_action.npz     the supervised forward, compute_loss / compute_loss_init and their gradients (gen_pretrain's)

make_golden.py is imported for its stubs and helpers (its own generation runs only under __main__).  The TrajARNet fixtures are gen_traj_ar_net /
gen_pretrain themselves, run with every config namespace they build switched to use_action=False and their output redirected.

    python tools/make_golden_no_action.py        (from an empty working directory: the reference's Config classes create directories under it)

tests/golden/kin_poly_wo_action.yml, read by tests/test_no_action_cpu.py, is the reference's config/statear/kin_poly_wo_action.yml copied as it is.
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs the reference's absent dependencies, puts the reference and this repository on sys.path)

OUT = G.OUT


def gen_ar_obs_no_action(hum):
    """get_ar_obs_v1 on gen_ar_obs_reward's kind of inputs, with the derived arrays taken at the state itself (no stale substep), so that a simulator
    handle whose state is set to the same qpos computes the same xpos / xquat and its rows can be compared directly.  Every other row carries an
    action one-hot and its object somewhere near the humanoid: the "predicted object relative to head" block (:171-179) still follows the label."""
    rng = np.random.default_rng(303)
    n, T = 16, 6
    env = G.make_env(G.har.HumanoidAREnv)
    env.smpl_humanoid = hum
    env.kin_cfg = types.SimpleNamespace(use_context=False, use_of=False, use_head=True, use_vel=False, use_obj=True, use_action=False)
    env.ar_model_v = 1
    env.policy_v = 1
    env.action_index_map = [0, 7, 21, 28]; env.action_len = [7, 14, 7, 7]
    rec = {k: [] for k in ("qpos", "qvel", "xpos", "xquat", "t", "head_pose", "head_vels", "obj_rel", "action_one_hot", "obj_qpos7", "obs_ar")}
    for i in range(n):
        q0 = G.rand_qpos(rng, 0.2); v0 = rng.normal(size=75) * 0.3
        d = G.oracle_data(q0, v0, stale_steps=0)
        assert np.abs(d.body_xpos[1:25] - hum.qpos_fk(q0.copy())["wbpos"].reshape(24, 3)).max() < 1e-9      # derived arrays at q0 itself
        one_hot = np.zeros(4)
        obj7 = np.array([0, 0, 0, 1, 0, 0, 0.0])
        if i % 2 == 1:
            a = (i // 2) % 4
            one_hot[a] = 1.0
            s = env.action_index_map[a]
            obj7 = np.concatenate([d.qpos[:3] + rng.normal(size=3) * 0.5, G.rand_quat(rng)])
            d.qpos[76 + s:76 + s + 7] = obj7
        env.data = d
        t = int(rng.integers(0, T))
        env.cur_t = t
        ctx = dict(action_one_hot=np.tile(one_hot, (T, 1)), head_pose=np.concatenate([rng.normal(size=(T, 3)), np.stack([G.rand_quat(rng) for _ in range(T)])], 1),
                   head_vels=rng.normal(size=(T, 6)), obj_head_relative_poses=rng.normal(size=(T, 7)))
        env.ar_context = ctx
        obs = env.get_ar_obs_v1()
        assert obs.shape == (101,)
        assert np.allclose(env.get_obj_qpos(action_one_hot=one_hot)[:7], obj7)
        rec["qpos"].append(d.qpos[:76].copy()); rec["qvel"].append(d.qvel[:75].copy())
        rec["xpos"].append(d.body_xpos[1:25].copy()); rec["xquat"].append(d.body_xquat[1:25].copy())
        rec["t"].append(t); rec["head_pose"].append(ctx["head_pose"][t]); rec["head_vels"].append(ctx["head_vels"][t])
        rec["obj_rel"].append(ctx["obj_head_relative_poses"][t]); rec["action_one_hot"].append(one_hot); rec["obj_qpos7"].append(obj7)
        rec["obs_ar"].append(obs)
    np.savez(os.path.join(OUT, "ar_obs_no_action.npz"), **{k: np.stack(v) for k, v in rec.items()})


class _NoActionTypes(types.ModuleType):
    """`types` as make_golden's generators see it: a config namespace that names use_action gets use_action=False."""

    def __init__(self):
        super().__init__("types")
        self.__dict__.update({k: getattr(types, k) for k in dir(types) if not k.startswith("__") and k != "SimpleNamespace"})

    @staticmethod
    def SimpleNamespace(**kw):
        if "use_action" in kw:
            kw["use_action"] = False
        return types.SimpleNamespace(**kw)


def run_without_action(gen, hum, produced, target):
    """Run make_golden's generator `gen` with use_action=False into a temporary directory and keep its file `produced` as tests/golden/<target>."""
    tmp = tempfile.mkdtemp()
    saved = G.types, G.OUT
    G.types, G.OUT = _NoActionTypes(), tmp
    try:
        gen(hum)
    finally:
        G.types, G.OUT = saved
    g = np.load(os.path.join(tmp, produced))
    assert (int(g["state_dim"]), int(g["context_dim"])) == (101, 13), (g["state_dim"], g["context_dim"])
    shutil.copy(os.path.join(tmp, produced), os.path.join(OUT, target))
    shutil.rmtree(tmp)


def check_dims_without_action():
    """state_dim / context_dim of the reference's TrajARNet with use_action=False, as a policy and as the plain network: 101 / 13 both."""
    import torch
    import kin_poly.models.traj_ar_smpl_net as tn
    import kin_poly.utils.torch_smpl_humanoid as tsh
    tsh.load_model_from_path = lambda f: G.fake_mj_model()
    cfg = types.SimpleNamespace(model_specs=dict(model_v=1, rnn_hdim=1024, mlp_hsize=[1024, 512, 256], mlp_htype="relu", rnn_type="gru"),
                                mujoco_model_file="unused.xml", use_of=False, use_head=True, use_action=False, use_vel=False, use_context=False,
                                add_noise=False, noise_std=0.01, has_z=True, data_dir=os.path.join(G.REF, "sample_data"))
    B, T = 1, 2
    data = {k: torch.zeros(B, T, d) for k, d in (("qpos", 76), ("qvel", 75), ("head_pose", 7), ("head_vels", 6), ("obj_head_relative_poses", 7),
                                                  ("obj_pose", 7), ("action_one_hot", 4), ("target", 80))}
    for as_policy in (True, False):
        net = tn.TrajARNet(cfg, data_sample=data, device=torch.device("cpu"), dtype=torch.float64, mode="test", as_policy=as_policy)
        assert (net.state_dim, net.context_dim) == (101, 13), (as_policy, net.state_dim, net.context_dim)


if __name__ == "__main__":
    hum = G.make_humanoid()
    check_dims_without_action()
    gen_ar_obs_no_action(hum)
    run_without_action(G.gen_traj_ar_net, hum, "traj_ar_net.npz", "traj_ar_net_no_action.npz")
    run_without_action(G.gen_pretrain, hum, "pretrain.npz", "pretrain_no_action.npz")
    for f in ("ar_obs_no_action.npz", "traj_ar_net_no_action.npz", "pretrain_no_action.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)))
