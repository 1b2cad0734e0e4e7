"""Generate tests/golden/ar_obs_context.npz: the reference's TrajARNet under `use_context` / `use_of` (config/statear/kin_only.yml, use_of.yml), by
IMPORTING the reference's Python as tools/make_golden.py does (where a reference checkout can be imported; only data is written, no reference source).

For every case (use_context, use_of, as_policy) in CASES, under the key suffix c<ctx>o<of>p<policy>, from a reference TrajARNet in fp64 with
rnn_hdim 16, mlp_hsize [16, 8, 8] and weights seeded as gen_traj_ar_net seeds them (use_head, use_action on, use_vel off):

    dims_*      (state_dim, context_dim);  keys_* / shapes_*  the state dict's
    ctx_*       get_context_feat [B, T, 16]
    obs_*       get_obs at every frame with the sequence set, the simulated state set to the clip's (qpos, qvel) of that frame   [B, T, state_dim]
    obs0_*      get_obs at frame 0 before init_states (the zero block)
    qpos_* qvel_*                      the test-mode forward
    loss_* loss_idv_* grad_*:<param>   train mode, gt_rate 0, no noise: compute_loss, its components and the gradients of the parameters pretrain.npz
                                       names, and of context_rnn.rnn_f.weight_ih (reached through the observation's context block alone, beside the mean)

Inputs: the clips of tests/golden/traj_ar_net_no_action.npz (B = 3, T = 5), a seeded `of` [3, 5, 12] and a seeded `wbpos` [3, 5, 72] for the loss;
stored as in_*.  With F = 12 and H = 16 the state is wider than the hidden state.

    python tools/make_golden_context_obs.py        (from an empty working directory: the reference's Config classes create directories under it)

tests/golden/kin_only.yml and use_of.yml, read by tests/test_context_obs_cpu.py, are the reference's config/statear files copied as they are.
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs the reference's absent dependencies, puts the reference and this repository on sys.path)

OUT = G.OUT
CASES = [(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 1, 0)]
H, MLP, F, SEED = 16, [16, 8, 8], 12, 9
WATCH = ("action_fc.bias", "context_fc.bias", "action_mlp.affine_layers.2.bias", "context_mlp.affine_layers.0.bias", "context_rnn.rnn_f.weight_ih")
LOSS_W = dict(w_rp=50.0, w_rr=50.0, w_p=1.0, w_v=1.0, w_ee=10.0, w_op=1.0, w_or=10.0)


def key(c, o, p):
    return f"c{c}o{o}p{p}"


def main():
    import torch
    import kin_poly.models.traj_ar_smpl_net as tn
    import kin_poly.utils.torch_smpl_humanoid as tsh
    tsh.load_model_from_path = lambda f: G.fake_mj_model()
    g = np.load(os.path.join(OUT, "traj_ar_net_no_action.npz"))
    data = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    B, T = data["qpos"].shape[:2]
    rng = np.random.default_rng(411)
    data["of"] = rng.normal(size=(B, T, F)) * 0.5
    data["wbpos"] = rng.normal(size=(B, T, 72))
    out = {"in_" + k: v for k, v in data.items()}
    out["seed"] = SEED
    fresh = lambda: {k: torch.tensor(x) for k, x in data.items()}      # noqa: E731  (init_states writes into the dict it is given)
    for (c, o, p) in CASES:
        cfg = types.SimpleNamespace(model_specs=dict(model_v=1, rnn_hdim=H, mlp_hsize=MLP, mlp_htype="relu", rnn_type="gru", **LOSS_W),
                                    mujoco_model_file="unused.xml", use_of=bool(o), use_head=True, use_action=True, use_vel=False, use_context=bool(c),
                                    add_noise=False, noise_std=0.01, has_z=True, data_dir=os.path.join(G.REF, "sample_data"))
        net = tn.TrajARNet(cfg, data_sample=fresh(), device=torch.device("cpu"), dtype=torch.float64, mode="test", as_policy=bool(p))
        assert net.state_dim == H + 101 + 4 * p + F * o * p and net.context_dim == F * o + 17, (c, o, p, net.state_dim, net.context_dim)
        sd = G.seeded_state_dict(net, SEED)
        for k in sd:
            if k.startswith(("action_fc", "context_fc")):
                sd[k] = sd[k] * 0.05
        net.load_state_dict(sd)
        net.set_schedule_sampling(0.0)
        s = key(c, o, p)
        with torch.no_grad():
            d = fresh()
            net.set_sim(d["qpos"][:, 0].clone(), d["qvel"][:, 0].clone())
            out["obs0_" + s] = net.get_obs(d, 0)[0].numpy()
            assert np.all(out["obs0_" + s][:, :H] == 0)
            ctx = net.get_context_feat(fresh())
            d = fresh(); d["context_feat_rnn"] = ctx
            obs = []
            for t in range(T):
                net.set_sim(d["qpos"][:, t].clone(), d["qvel"][:, t].clone())
                obs.append(net.get_obs(d, t)[0].numpy())
            fp = net.forward(fresh())
        out["ctx_" + s], out["obs_" + s] = ctx.numpy(), np.stack(obs, 1)
        out["qpos_" + s], out["qvel_" + s] = fp["qpos"].numpy(), fp["qvel"].numpy()
        out["dims_" + s] = np.array([net.state_dim, net.context_dim])
        out["keys_" + s] = np.array(list(net.state_dict().keys()))
        out["shapes_" + s] = np.array([list(x.shape) + [0] * (2 - x.dim()) for x in net.state_dict().values()])
        net.mode = "train"
        net.zero_grad()
        d = fresh()
        fp = net.forward(d)
        loss, idv = net.compute_loss(fp, d)
        loss.backward()
        out["loss_" + s], out["loss_idv_" + s] = float(loss.detach()), np.array(idv)
        params = dict(net.named_parameters())
        for w in WATCH:
            out[f"grad_{s}:{w}"] = params[w].grad.numpy().copy()
    path = os.path.join(OUT, "ar_obs_context.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
