"""CPU: the kinematic policy under `use_context` / `use_of` on the roll-out side -- Config's "policy_ctx" entry (tests/golden/kin_poly_of.yml: kin_poly.yml
with the two switches on and rnn_hdim 256) and, in fp64 against tests/golden/policy_ctx.npz (tools/make_golden_policy_ctx.py: the reference's PolicyAR with
rnn_hdim 16, mlp_hsize [16, 8, 8], `of` 12 wide), PolicyAR.init_context and the train-mode forward over recorded wide states.

Tolerance: 1e-10 absolute, what the other fp64 reference fixtures are held to (tests/test_context_obs_cpu.py, tests/test_context_cpu.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YML = os.path.join(GOLDEN, "kin_poly_of.yml")
CASES = [(1, 0), (1, 1)]
IDS = [f"c{c}o{o}" for c, o in CASES]
H, F = 16, 12


def build(g, case, dtype=torch.float64, device="cpu"):
    """the case's policy network with the fixture's seeded weights, and the fixture's clips"""
    from kinpoly_amd.context import TrajARNet
    c, o = case
    k = f"c{c}o{o}"
    net = TrajARNet(rnn_hdim=H, mlp_hsize=(16, 8, 8), use_context=bool(c), of_dim=F * o, of_in_state=bool(o)).to(dtype)
    shapes = [tuple(int(x) for x in row if x > 0) for row in g["shapes_" + k]]
    assert {n: tuple(v.shape) for n, v in net.state_dict().items() if n != "action_log_std"} == dict(zip([str(x) for x in g["keys_" + k]], shapes))
    sd = O.seeded_state_dict(list(zip([str(x) for x in g["keys_" + k]], shapes)), int(g["seed"]))
    for name in sd:
        if name.startswith(("action_fc", "context_fc")):
            sd[name] = sd[name] * 0.05
    missing = net.load_state_dict({name: torch.tensor(v, dtype=dtype) for name, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"action_log_std"}
    net.refresh_log_std()
    data = {name[3:]: torch.tensor(g[name], dtype=dtype, device=device) for name in g.files if name.startswith("in_")}
    return net.to(device), data, k


# ------------------------------------------------------------------ Config
def test_policy_ctx_entry_loads_the_video_conditioned_yml(tmp_path):
    from kinpoly_amd.config import Config
    cfg = Config(YML, base_dir=str(tmp_path), entry="policy_ctx")
    assert cfg.use_of is True and cfg.use_context is True and cfg.of_file == "mocap_img_feats"
    assert Config(YML, wild=True, base_dir=str(tmp_path), entry="policy_ctx").of_file == "real_img_feats"
    mk = cfg.model_kwargs()
    assert (mk["rnn_hdim"], mk["mlp_hsize"]) == (256, (1024, 512, 256))
    kw = cfg.agent_kwargs()
    assert (kw["use_context"], kw["of_dim"], kw["rnn_hdim"], kw["mlp_hsize"]) == (True, 512, 256, (1024, 512, 256))      # of_dim: cnn_fdim without a feature file
    assert cfg.agent_kwargs(of_dim=40)["of_dim"] == 40                                                                    # the feature file's width when known
    assert (kw["use_action"], kw["use_vel"], kw["use_head"], kw["log_std"], kw["policy_lr"]) == (True, False, True, -3.2, 1e-5)
    assert cfg.of_feature_path().endswith(os.path.join("features", "mocap_img_feats.p"))


def test_policy_ctx_entry_on_a_plain_yml_builds_todays_agent(tmp_path):
    """both switches off: the new entry hands AgentAR the sizes it has always had, and the default entry hands it no new argument at all"""
    import yaml
    from kinpoly_amd.config import Config
    y = yaml.safe_load(open(YML))
    p = tmp_path / "plain.yml"
    p.write_text(yaml.safe_dump(dict(y, use_of=False, use_context=False, model_specs=dict(y["model_specs"], rnn_hdim=1024))))
    new, old = Config(str(p), base_dir=str(tmp_path), entry="policy_ctx").agent_kwargs(), Config(str(p), base_dir=str(tmp_path)).agent_kwargs()
    assert {k: new[k] for k in set(new) - set(old)} == dict(use_context=False, of_dim=0, rnn_hdim=1024, mlp_hsize=(1024, 512, 256))
    assert {k: new[k] for k in old} == old
    # a file that names no net size (or no model_specs at all) leaves the sizes to the engine, as the default entry does
    q = tmp_path / "bare.yml"
    q.write_text(yaml.safe_dump({k: v for k, v in dict(y, use_of=False, use_context=False).items() if k != "model_specs"}))
    bare = Config(str(q), base_dir=str(tmp_path), entry="policy_ctx").agent_kwargs()
    assert "rnn_hdim" not in bare and "mlp_hsize" not in bare and (bare["use_context"], bare["of_dim"]) == (False, 0)


def test_default_entry_still_refuses_the_switches(tmp_path):
    from kinpoly_amd.config import Config, ConfigError
    for entry in ({}, {"entry": "policy"}):
        with pytest.raises(ConfigError, match="use_of") as e:
            Config(YML, base_dir=str(tmp_path), **entry)
        assert "use_context" in str(e.value) and "rnn_hdim" in str(e.value)


@pytest.mark.parametrize("name", ["kin_only", "use_of"])
def test_policy_v2_and_reward_v3_stay_refused_by_name(name, tmp_path):
    """the two shipped files declare policy_v 2 and dynamic_supervision_v3, which cannot run in the reference either: refused under the new entry for
    that reason, no longer for their switches"""
    from kinpoly_amd.config import Config, ConfigError
    with pytest.raises(ConfigError, match="policy_v") as e:
        Config(os.path.join(GOLDEN, name + ".yml"), base_dir=str(tmp_path), entry="policy_ctx")
    msg = str(e.value)
    assert "reward_id" in msg and "dynamic_supervision_v3" in msg and "policy_ar.py:33-37" in msg and "reward_function.py:1055-1056" in msg
    items = msg.split(" -- ", 1)[1]                      # the refused keys (the message starts with the file's path, which is use_of.yml for one of them)
    assert "use_of" not in items and "use_context" not in items and "rnn_hdim" not in items


def test_unknown_entry_and_bad_sizes_raise(tmp_path):
    import yaml
    from kinpoly_amd.config import Config, ConfigError
    with pytest.raises(ConfigError, match="entry"):
        Config(YML, base_dir=str(tmp_path), entry="policy_of")
    y = yaml.safe_load(open(YML))
    for where, key, val in (("model_specs", "rnn_hdim", 0), ("model_specs", "mlp_hsize", []), ("model_specs", "cnn_fdim", -1), (None, "use_of", "yes"),
                            ("model_specs", "rnn_type", "lstm"), (None, "obs_quat", False), ("policy_specs", "fix_std", False)):
        z = {k: (dict(v) if isinstance(v, dict) else v) for k, v in y.items()}
        (z[where] if where else z)[key] = val
        p = tmp_path / f"bad_{key}.yml"
        p.write_text(yaml.safe_dump(z))
        with pytest.raises(ConfigError, match=key):
            Config(str(p), base_dir=str(tmp_path), entry="policy_ctx")


# ------------------------------------------------------------------ fixture (b): PolicyAR.init_context
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_init_context_matches_reference(golden, case):
    from kinpoly_amd.context import PolicyARContext
    from kinpoly_amd.pretrain import forward_supervised
    from test_context_obs_cpu import torch_fk
    g = golden("policy_ctx")
    net, data, k = build(g, case)
    assert (net.state_dim, net.ctx_block, net.base_dim) == (H + 105 + F * case[1], H, 105)
    ctx = PolicyARContext(net, None, smooth=True, need_rollout=False, keep_context_feat=True).init_context(data, fix_height=False)
    for name in ("context_feat_rnn", "init_qpos", "init_qvel"):
        err = float(np.abs(ctx[name].numpy() - g[f"ic_{name}_{k}"]).max())
        print(f"MEASURED init_context {k} {name}: max |error| {err:.3e}")
        np.testing.assert_allclose(ctx[name].numpy(), g[f"ic_{name}_{k}"], rtol=0, atol=1e-10)
    assert ctx["context_feat_rnn"].transpose(0, 1).is_contiguous()          # the env-major view of the time-major sequence: what the refill kernel reads
    # the kinematic roll-out of init_context (the fp64 torch path; on the device it is TrajARNet.rollout on the HIP kernels)
    with torch.no_grad():
        q = forward_supervised(net, torch_fk(), data)["qpos"].numpy()
    err = float(np.abs(q - g[f"ic_ar_qpos_{k}"]).max())
    print(f"MEASURED init_context {k} ar_qpos: max |error| {err:.3e}")
    np.testing.assert_allclose(q, g[f"ic_ar_qpos_{k}"], rtol=0, atol=1e-10)


# ------------------------------------------------------------------ fixture (c): PolicyAR.forward in train mode on recorded wide states
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_train_mode_forward_over_two_episodes_matches_reference(golden, case):
    g = golden("policy_ctx")
    net, _, k = build(g, case)
    states, actions, masks = torch.tensor(g["fw_states_" + k]), torch.tensor(g["fw_actions_" + k]), g["fw_masks"]
    assert states.shape == (12, net.state_dim) and list(np.nonzero(masks == 0)[0]) == [4, 11]
    start = torch.zeros((1, 12), dtype=torch.bool)
    start[0, 0] = start[0, 5] = True                                        # a row after a mask of 0 starts an episode
    with torch.no_grad():
        mean = net.unroll_reference(states[None], start)[0]
        assert torch.equal(net.unroll(states[None], start)[0], mean)        # fp64 on the CPU: unroll is that loop
        logp = net.log_prob(mean, actions)
    for name, got in (("mean", mean), ("logp", logp)):
        err = float(np.abs(got.numpy() - g[f"fw_{name}_{k}"]).max())
        print(f"MEASURED train-mode forward {k} {name}: max |error| {err:.3e} (max |reference| {float(np.abs(g[f'fw_{name}_{k}']).max()):.3e})")
    np.testing.assert_allclose(mean.numpy(), g["fw_mean_" + k], rtol=0, atol=1e-10)
    np.testing.assert_allclose(logp.numpy(), g["fw_logp_" + k], rtol=0, atol=1e-10)
    # the context block of the recorded states is data: no gradient reaches the context network through the re-unroll
    net.zero_grad()
    net.log_prob(net.unroll_reference(states[None], start)[0], actions).sum().backward()
    assert all(p.grad is None for n, p in net.named_parameters() if n.startswith(("context_rnn", "context_mlp", "context_fc")))
    assert net.action_rnn.rnn_f.weight_ih.grad is not None


# ------------------------------------------------------------------ refusals that need no device
def test_cache_init_context_is_refused_with_a_context_block():
    from kinpoly_amd.context import PolicyARContext, TrajARNet
    from kinpoly_amd.rollout import EpisodeSource
    wide = PolicyARContext(TrajARNet(rnn_hdim=H, mlp_hsize=(16, 8, 8), use_context=True), None, need_rollout=False)
    with pytest.raises(ValueError, match="cache_init_context"):
        EpisodeSource(context_fn=lambda n: {}, ctx_builder=wide, cache_init_context=True)
    EpisodeSource(context_fn=lambda n: {}, ctx_builder=wide)
    plain = PolicyARContext(TrajARNet(rnn_hdim=H, mlp_hsize=(16, 8, 8)), None, need_rollout=False)
    EpisodeSource(context_fn=lambda n: {}, ctx_builder=plain, cache_init_context=True)


def test_record_width_rule():
    """obs_dim = ctx_dim + one of the eight layout widths + of_dim; the default arguments keep refusing every other width"""
    from kinpoly_amd import sim as kpsim
    assert kpsim._obs_width(105) == 105 and kpsim._obs_width(256 + 105 + 512, 256, 512) == 873 and kpsim._obs_width(16 + 81, 16, 0) == 97
    for args in ((873,), (873, 256, 0), (873, 0, 512), (106, 0, 0), (105, 1, 0), (105 + 16, -16, 0)):
        with pytest.raises(ValueError, match="obs_dim"):
            kpsim._obs_width(*args)


def test_checkpoint_of_other_sizes_names_both_shapes():
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd.context import TrajARNet
    a = TrajARNet(rnn_hdim=16, mlp_hsize=(16, 8, 8), use_context=True, of_dim=12, of_in_state=True)
    sd = {k: v for k, v in a.state_dict().items()}
    ck.load_state_strict(TrajARNet(rnn_hdim=16, mlp_hsize=(16, 8, 8), use_context=True, of_dim=12, of_in_state=True), sd)
    with pytest.raises(ck.CheckpointWidthError, match="133-d") as e:          # another context width: the policy's input width differs
        ck.load_state_strict(TrajARNet(rnn_hdim=32, mlp_hsize=(16, 8, 8), use_context=True, of_dim=12, of_in_state=True), sd)
    assert "149-d" in str(e.value)
    with pytest.raises(ck.CheckpointWidthError, match=r"action_mlp.affine_layers.0.bias is \(16,\) in the checkpoint and \(24,\)"):
        ck.load_state_strict(TrajARNet(rnn_hdim=16, mlp_hsize=(24, 8, 8), use_context=True, of_dim=12, of_in_state=True), sd)
