"""Generate tests/golden/ar_obs_variants.npz: the kinematic observation under the statear switches use_vel / use_head / use_action, by IMPORTING
the reference's Python as tools/make_golden.py does (where a reference checkout can be imported; only data is written, no reference source).

For every (use_vel, use_head, use_action) the file holds, under the key suffix v<vel>h<head>a<action>:

    env_obs_*        HumanoidAREnv.get_ar_obs_v1 (humanoid_ar_v1.py:133-214) on the 16 rows of tests/golden/ar_obs_no_action.npz (same state, derived
                     arrays, context row, action label and object pose: the inputs are read from that fixture and stored again here)
    net_obs_*        TrajARNet.get_obs (traj_ar_smpl_net.py:203-290) at every frame t of the clips of tests/golden/traj_ar_net_no_action.npz, the
                     simulated state set to the clip's (qpos, qvel) of that frame
    net_dims_*       (state_dim, context_dim) of the reference's TrajARNet (get_obs's width, get_context_dim)
    net_ctx_*        the first 64 channels of get_context_feat with weights seeded as gen_traj_ar_net seeds them (keys / shapes stored per variant)

The two head-less, action-less layouts (81 / 156 floats) have env_obs_* only: the reference's network has no context input there (get_context_dim 0).

    python tools/make_golden_obs_variants.py        (from an empty working directory: the reference's Config classes create directories under it)

tests/golden/kin_poly_use_vel.yml, kin_poly_no_head.yml, kin_poly_use_vel_no_head.yml and kin_poly_no_head_no_action.yml, read by
tests/test_obs_variants_cpu.py, are the reference's config/statear/kin_poly.yml with those one or two keys flipped (settings only).
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs the reference's absent dependencies, puts the reference and this repository on sys.path)

OUT = G.OUT
VARIANTS = [(v, h, a) for h in (True, False) for v in (False, True) for a in (True, False)]
CTX_CHANNELS = 64


def key(v, h, a):
    return f"v{int(v)}h{int(h)}a{int(a)}"


def width(v, h, a):
    return 74 + 75 * v + 7 * h + 7 + 13 * h + 4 * a


def gen_env_rows(hum, out):
    g = np.load(os.path.join(OUT, "ar_obs_no_action.npz"))
    n, T = len(g["qpos"]), 6
    env = G.make_env(G.har.HumanoidAREnv)
    env.smpl_humanoid = hum
    env.ar_model_v = 1
    env.policy_v = 1
    env.action_index_map = [0, 7, 21, 28]; env.action_len = [7, 14, 7, 7]
    for k in ("qpos", "qvel", "xpos", "xquat", "t", "head_pose", "head_vels", "obj_rel", "action_one_hot", "obj_qpos7"):
        out["env_" + k] = g[k]
    rows = {s: [] for s in VARIANTS}
    for i in range(n):
        d = G.FakeData()
        d.qpos = np.concatenate([g["qpos"][i], np.zeros(35)])
        d.qvel = np.concatenate([g["qvel"][i], np.zeros(30)])
        d.body_xpos = np.vstack([np.zeros((1, 3)), g["xpos"][i], np.zeros((5, 3))])
        d.body_xquat = np.vstack([[[1, 0, 0, 0]], g["xquat"][i], np.tile([1., 0, 0, 0], (5, 1))])
        one_hot = g["action_one_hot"][i]
        if one_hot.sum() > 0:
            s = env.action_index_map[int(np.argmax(one_hot))]
            d.qpos[76 + s:76 + s + 7] = g["obj_qpos7"][i]
        env.data = d
        t = int(g["t"][i])
        env.cur_t = t
        ctx = dict(action_one_hot=np.tile(one_hot, (T, 1)), head_pose=np.zeros((T, 7)), head_vels=np.zeros((T, 6)), obj_head_relative_poses=np.zeros((T, 7)))
        ctx["head_pose"][t], ctx["head_vels"][t], ctx["obj_head_relative_poses"][t] = g["head_pose"][i], g["head_vels"][i], g["obj_rel"][i]
        env.ar_context = ctx
        for (v, h, a) in VARIANTS:
            env.kin_cfg = types.SimpleNamespace(use_context=False, use_of=False, use_head=h, use_vel=v, use_obj=True, use_action=a)
            obs = env.get_ar_obs_v1()
            assert obs.shape == (width(v, h, a),), (v, h, a, obs.shape)
            rows[(v, h, a)].append(obs)
        assert np.array_equal(rows[(False, True, False)][-1], g["obs_ar"][i])          # the no-action fixture's own row, from its stored inputs
    for s, r in rows.items():
        out["env_obs_" + key(*s)] = np.stack(r)


def gen_net_rows(out):
    import torch
    import kin_poly.models.traj_ar_smpl_net as tn
    import kin_poly.utils.torch_smpl_humanoid as tsh
    tsh.load_model_from_path = lambda f: G.fake_mj_model()
    g = np.load(os.path.join(OUT, "traj_ar_net_no_action.npz"))
    data = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    for k, v in data.items():
        out["net_in_" + k] = v
    out["net_seed"] = 9
    B, T = data["qpos"].shape[:2]
    for (v, h, a) in VARIANTS:
        if not (h or a):
            continue
        cfg = types.SimpleNamespace(model_specs=dict(model_v=1, rnn_hdim=1024, mlp_hsize=[1024, 512, 256], mlp_htype="relu", rnn_type="gru"),
                                    mujoco_model_file="unused.xml", use_of=False, use_head=h, use_action=a, use_vel=v, use_context=False,
                                    add_noise=False, noise_std=0.01, has_z=True, data_dir=os.path.join(G.REF, "sample_data"))
        data_t = {k: torch.tensor(x) for k, x in data.items()}
        net = tn.TrajARNet(cfg, data_sample=data_t, device=torch.device("cpu"), dtype=torch.float64, mode="test", as_policy=True)
        assert net.state_dim == width(v, h, a) and net.context_dim == net.get_context_dim(data_t) == 13 * h + 4 * a
        sd = G.seeded_state_dict(net, 9)
        for k in sd:
            if k.startswith(("action_fc", "context_fc")):
                sd[k] = sd[k] * 0.05
        net.load_state_dict(sd)
        obs = []
        with torch.no_grad():
            for t in range(T):
                net.set_sim(data_t["qpos"][:, t].clone(), data_t["qvel"][:, t].clone())
                obs.append(net.get_obs({k: x.clone() for k, x in data_t.items()}, t)[0].numpy())
            ctx = net.get_context_feat({k: x.clone() for k, x in data_t.items()}).numpy()
        s = key(v, h, a)
        out["net_obs_" + s] = np.stack(obs, 1)                                   # [B, T, state_dim]
        out["net_dims_" + s] = np.array([net.state_dim, net.context_dim])
        out["net_ctx_" + s] = ctx[:, :, :CTX_CHANNELS]
        out["net_keys_" + s] = np.array(list(net.state_dict().keys()))
        out["net_shapes_" + s] = np.array([list(x.shape) + [0] * (2 - x.dim()) for x in net.state_dict().values()])


if __name__ == "__main__":
    out = {}
    gen_env_rows(G.make_humanoid(), out)
    gen_net_rows(out)
    path = os.path.join(OUT, "ar_obs_variants.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
