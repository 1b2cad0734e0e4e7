"""Generate tests/golden/policy_ctx.npz: the reference's env observation and PolicyAR under `use_context` / `use_of` (kin_poly.yml with the two switches
on: tests/golden/kin_poly_of.yml), by IMPORTING the reference's Python as tools/make_golden.py and tools/make_golden_context_obs.py do (where a
reference checkout can be imported; only data is written, no reference source).

In fp64 with rnn_hdim 16, mlp_hsize [16, 8, 8], `of` 12 wide, weights seeded as ar_obs_context.npz's (seed 9, action_fc / context_fc x 0.05), for the
two cases a policy entry runs -- context only (key suffix c1o0) and context + of (c1o1), as_policy True in both:

    (a) env_*            HumanoidAREnv.get_ar_obs_v1 on 12 states with ar_context['context_feat_rnn'] / ['of'] set: tools/make_golden.py::gen_ar_obs_reward's
                         construction (oracle states, derived arrays one substep stale), rows with and without an action object, frames that include the
                         clip's first and last.  env_obs_c1o0 [12, 16 + 105], env_obs_c1o1 [12, 16 + 105 + 12]; the inputs are shared by the two cases
    (b) ic_*_<case>      PolicyAR(policy_v=1).init_context(fix_height=False, cfg.smooth) on 3 clips of 5 frames, one clip at a time as the reference's
                         sampler calls it: context_feat_rnn [3, 5, 16], init_qpos, init_qvel, ar_qpos.  Clips: those of traj_ar_net_no_action.npz and
                         ar_obs_context.npz's seeded `of` (in_*)
    (c) fw_*_<case>      PolicyAR.forward in train mode after initialize_rnn on 12 recorded wide states that hold two episodes of 5 and 7 rows:
                         action means [12, 80] and get_log_prob of seeded actions [12, 1] (log_std -3.2)

    python tools/make_golden_policy_ctx.py        (from an empty working directory: the reference's Config classes create directories under it)

tests/golden/kin_poly_of.yml is the reference's config/statear/kin_poly.yml with use_of / use_context true, of_file / of_file_wild named and
model_specs.rnn_hdim 256 (cnn_fdim is 512 there already); settings only.
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs the reference's absent dependencies, puts the reference and this repository on sys.path)

OUT = G.OUT
CASES = [(1, 0), (1, 1)]
H, MLP, F, SEED = 16, [16, 8, 8], 12, 9


def key(c, o):
    return f"c{c}o{o}"


def gen_env_obs(out):
    """(a): gen_ar_obs_reward's states, with the two wide blocks in the context"""
    har, hum = G.har, G.make_humanoid()
    rng = np.random.default_rng(503)
    n, T = 12, 6
    env = G.make_env(har.HumanoidAREnv)
    env.smpl_humanoid = hum
    env.ar_model_v, env.policy_v = 1, 1
    env.action_index_map, env.action_len = [0, 7, 21, 28], [7, 14, 7, 7]
    frames = [0, T - 1, 1, 4, 0, T - 1] + [int(rng.integers(1, T - 1)) for _ in range(n - 6)]
    rec = {k: [] for k in ("qpos", "qvel", "xpos", "xquat", "t", "head_pose", "head_vels", "obj_rel", "action_one_hot", "obj_qpos", "obj7", "ctx_feat", "of")}
    obs = {key(c, o): [] for c, o in CASES}
    for i in range(n):
        d = G.oracle_data(G.rand_qpos(rng, 0.2), rng.normal(size=75) * 0.3)
        one_hot = np.zeros(4)
        if i % 4 == 1:                                   # sit: the object's slot 0
            one_hot[0] = 1.0
            d.qpos[76:83] = np.concatenate([rng.normal(size=3), G.rand_quat(rng)])
        elif i % 4 == 3:                                 # avoid: slot 21
            one_hot[2] = 1.0
            d.qpos[76 + 21:76 + 28] = np.concatenate([rng.normal(size=3), G.rand_quat(rng)])
        env.data = d
        env.cur_t = frames[i]
        ctx = dict(action_one_hot=np.tile(one_hot, (T, 1)), head_pose=np.concatenate([rng.normal(size=(T, 3)), np.stack([G.rand_quat(rng) for _ in range(T)])], 1),
                   head_vels=rng.normal(size=(T, 6)), obj_head_relative_poses=rng.normal(size=(T, 7)),
                   context_feat_rnn=rng.normal(size=(T, H)), of=rng.normal(size=(T, F)) * 0.5)
        env.ar_context = ctx
        for c, o in CASES:
            env.kin_cfg = types.SimpleNamespace(use_context=bool(c), use_of=bool(o), use_head=True, use_vel=False, use_obj=True, use_action=True)
            obs[key(c, o)].append(env.get_ar_obs_v1())
        rec["qpos"].append(d.qpos[:76].copy()); rec["qvel"].append(d.qvel[:75].copy()); rec["obj_qpos"].append(d.qpos[76:111].copy())
        rec["obj7"].append(np.asarray(env.get_obj_qpos(action_one_hot=one_hot), np.float64))
        rec["xpos"].append(d.body_xpos[1:25].copy()); rec["xquat"].append(d.body_xquat[1:25].copy())
        rec["t"].append(frames[i]); rec["action_one_hot"].append(one_hot)
        rec["head_pose"].append(ctx["head_pose"]); rec["head_vels"].append(ctx["head_vels"]); rec["obj_rel"].append(ctx["obj_head_relative_poses"])
        rec["ctx_feat"].append(ctx["context_feat_rnn"]); rec["of"].append(ctx["of"])
    out.update({"env_" + k: np.stack(v) for k, v in rec.items()})
    for k, v in obs.items():
        out["env_obs_" + k] = np.stack(v)
        assert out["env_obs_" + k].shape == (n, H + 105 + (F if k.endswith("o1") else 0))


def gen_policy(out):
    """(b) and (c)"""
    import torch
    import kin_poly.models.policy_ar as par
    import kin_poly.models.traj_ar_smpl_net as tn
    import kin_poly.utils.torch_smpl_humanoid as tsh
    tsh.load_model_from_path = lambda f: G.fake_mj_model()
    g = np.load(os.path.join(OUT, "traj_ar_net_no_action.npz"))
    data = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    B, T = data["qpos"].shape[:2]
    data["of"] = np.random.default_rng(411).normal(size=(B, T, F)) * 0.5          # ar_obs_context.npz's
    out.update({"in_" + k: v for k, v in data.items()})
    out["seed"] = SEED
    rng = np.random.default_rng(504)
    nb = 12
    masks = torch.ones(nb); masks[[4, 11]] = 0                                       # episodes of 5 and 7 rows
    out["fw_masks"] = masks.numpy()
    for c, o in CASES:
        s = key(c, o)
        cfg = types.SimpleNamespace(model_specs=dict(model_v=1, rnn_hdim=H, mlp_hsize=MLP, mlp_htype="relu", rnn_type="gru"), mujoco_model_file="unused.xml",
                                    use_of=bool(o), use_head=True, use_action=True, use_vel=False, use_context=bool(c), add_noise=False, noise_std=0.01, has_z=True,
                                    data_dir=os.path.join(G.REF, "sample_data"), smooth=True)
        one = lambda b: {k: torch.tensor(x[b:b + 1]) for k, x in data.items()}      # noqa: E731  (init_states writes into the dict it is given)
        net = tn.TrajARNet(cfg, data_sample=one(0), device=torch.device("cpu"), dtype=torch.float64, mode="test", as_policy=True)
        assert net.state_dim == H + 105 + F * o and net.context_dim == F * o + 17, (s, net.state_dim, net.context_dim)
        sd = G.seeded_state_dict(net, SEED)
        for k in sd:
            if k.startswith(("action_fc", "context_fc")):
                sd[k] = sd[k] * 0.05
        net.load_state_dict(sd)
        net.set_schedule_sampling(0.0)
        out["keys_" + s] = np.array(list(net.state_dict().keys()))
        out["shapes_" + s] = np.array([list(x.shape) + [0] * (2 - x.dim()) for x in net.state_dict().values()])
        stub = types.SimpleNamespace(traj_ar_net=net, old_arnet=[net], cfg=cfg, state_dim=net.state_dim, action_dim=80, policy_v=1, mode="test",
                                     action_log_std=torch.ones(1, 80) * -3.2)
        stub.get_action = lambda st: par.PolicyAR.get_action(stub, st)
        stub.forward = lambda st: par.PolicyAR.forward(stub, st)
        rows = {k: [] for k in ("context_feat_rnn", "init_qpos", "init_qvel", "ar_qpos")}
        for b in range(B):                               # the reference's sampler: one clip per init_context call
            ctx = par.PolicyAR.init_context(stub, one(b), fix_height=False)
            for k in rows:
                rows[k].append(ctx[k][0].numpy().copy())
        for k, v in rows.items():
            out[f"ic_{k}_{s}"] = np.stack(v)
        assert out[f"ic_context_feat_rnn_{s}"].shape == (B, T, H)
        # (c) the padded re-unroll over two episodes of unequal length, on recorded wide states
        states = torch.tensor(rng.normal(size=(nb, net.state_dim)) * 0.5)
        actions = torch.tensor(rng.normal(size=(nb, 80)) * 0.1)
        stub.mode = "train"
        par.PolicyAR.initialize_rnn(stub, (masks, torch.zeros((nb, 3))))
        assert (stub.num_episode, stub.max_episode_len) == (2, 7)
        with torch.no_grad():
            _, mean, _ = par.PolicyAR.forward(stub, states)
            logp = par.PolicyAR.get_log_prob(stub, states, actions)
        out["fw_states_" + s], out["fw_actions_" + s] = states.numpy(), actions.numpy()
        out["fw_mean_" + s], out["fw_logp_" + s] = mean.numpy(), logp.numpy()


def main():
    out = {}
    gen_env_obs(out)
    gen_policy(out)
    path = os.path.join(OUT, "policy_ctx.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
