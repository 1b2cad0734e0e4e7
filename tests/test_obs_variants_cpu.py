"""CPU: the kinematic policy's observation variants (a statear yml's `use_vel` and `use_head` next to `use_action`).

The fp64 restatement (tests/ar_obs_variants_oracle.py) is held to rows the reference's own get_ar_obs_v1 wrote (tests/golden/ar_obs_variants.npz,
tools/make_golden_obs_variants.py); Config accepts the ymls and refuses the head-less no-action one; TrajARNet's widths, its context GRU input and the
differentiable observation of the supervised roll-out equal the reference's; a checkpoint of another width is named; the C ABI's option table answers
the eight widths without a GPU."""
import os

import numpy as np
import pytest
import torch

import ar_obs_variants_oracle as V
from oracle import np_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
YMLS = {"kin_poly_use_vel": (True, True, True), "kin_poly_no_head": (False, False, True), "kin_poly_use_vel_no_head": (True, False, True)}      # (vel, head, action)
NET_VARIANTS = [s for s in V.VARIANTS if s[1] or s[2]]          # the reference's network has no context input without head and action


def _row(g, i, s):
    return V.obs_ar_variant(g["env_qpos"][i], g["env_qvel"][i], g["env_xpos"][i], g["env_xquat"][i], g["env_head_pose"][i], g["env_head_vels"][i], g["env_obj_rel"][i],
                            g["env_action_one_hot"][i], g["env_obj_qpos7"][i], *s)


@pytest.mark.parametrize("s", V.VARIANTS, ids=[V.key(*s) for s in V.VARIANTS])
def test_restatement_equals_the_reference_rows(golden, s):
    g = golden("ar_obs_variants")
    want = g["env_obs_" + V.key(*s)]
    assert want.shape == (16, V.width(*s)) and V.offsets(*s)["end"] == V.width(*s)
    for i in range(len(want)):
        np.testing.assert_allclose(_row(g, i, s), want[i], rtol=0, atol=1e-10)      # the bound tests/test_oracle_golden.py holds the oracle to
    if s[0]:
        o = V.offsets(*s)
        assert np.array_equal(want[:, o["vel"]:o["vel"] + 75], g["env_qvel"])          # data.qvel[:75], copied


def test_restatement_at_105_and_101_is_the_oracle(golden):
    g = golden("ar_obs_variants")
    assert [V.width(*s) for s in V.VARIANTS] == [105, 101, 180, 176, 85, 81, 160, 156]
    for i in range(16):
        want = O.obs_ar(g["env_qpos"][i], g["env_xpos"][i], g["env_xquat"][i], g["env_head_pose"][i], g["env_head_vels"][i], g["env_obj_rel"][i],
                        g["env_action_one_hot"][i], g["env_obj_qpos7"][i])
        assert np.array_equal(_row(g, i, (False, True, True)), want) and np.array_equal(_row(g, i, (False, True, False)), want[:101])
    assert np.array_equal(g["env_obs_v0h1a0"], golden("ar_obs_no_action")["obs_ar"])      # the same rows as the no-action fixture


def _cfg(tmp_path, name, text=None):
    d = tmp_path / "config" / "statear"
    d.mkdir(parents=True, exist_ok=True)
    p = d / f"{name}.yml"
    p.write_text(open(os.path.join(GOLDEN, f"{name}.yml")).read() if text is None else text)
    return str(p)


@pytest.mark.parametrize("name", sorted(YMLS))
def test_config_accepts_the_variant_ymls(tmp_path, name):
    from kinpoly_amd.config import Config
    vel, head, action = YMLS[name]
    _cfg(tmp_path, name)
    cfg = Config(name, config_root=str(tmp_path), base_dir=str(tmp_path / "results"))
    assert (cfg.use_vel, cfg.use_head, cfg.use_action) == (vel, head, action) and cfg.seed == 4
    kw = cfg.agent_kwargs()
    assert (kw["use_vel"], kw["use_head"], kw["use_action"]) == (vel, head, action)


def test_config_refusals(tmp_path):
    from kinpoly_amd.config import Config, ConfigError
    with pytest.raises(ConfigError, match="use_head.*use_action"):
        Config(_cfg(tmp_path, "kin_poly_no_head_no_action"))
    text = open(os.path.join(GOLDEN, "kin_poly_use_vel.yml")).read()
    with pytest.raises(ConfigError, match="use_of"):
        Config(_cfg(tmp_path, "with_of", text.replace("use_of: false", "use_of: true")))
    with pytest.raises(ConfigError, match="use_context"):
        Config(_cfg(tmp_path, "with_context", text.replace("use_context: false", "use_context: true")))
    with pytest.raises(ConfigError, match="use_vel"):
        Config(_cfg(tmp_path, "bad_vel", text.replace("use_vel: true", "use_vel: 3")))
    with pytest.raises(ConfigError, match="use_head"):
        Config(_cfg(tmp_path, "bad_head", text.replace("use_head: true", "use_head: maybe")))
    # without the keys the reference's defaults hold (statear_smpl_config.py:139-142): head on, velocities off
    kw = Config(_cfg(tmp_path, "no_keys", text.replace("use_vel: true\n", "").replace("use_head: true\n", ""))).agent_kwargs()
    assert (kw["use_vel"], kw["use_head"], kw["use_action"]) == (False, True, True)


def _seeded_net(g, s, dtype=torch.float64):
    from kinpoly_amd.context import TrajARNet
    vel, head, action = s
    net = TrajARNet(use_vel=vel, use_head=head, use_action=action).to(dtype)
    k = V.key(*s)
    shapes = [tuple(int(x) for x in row if x > 0) for row in g["net_shapes_" + k]]
    sd = O.seeded_state_dict(list(zip([str(x) for x in g["net_keys_" + k]], shapes)), int(g["net_seed"]))
    for name in sd:
        if name.startswith(("action_fc", "context_fc")):
            sd[name] = sd[name] * 0.05
    missing = net.load_state_dict({name: torch.tensor(v, dtype=dtype) for name, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"action_log_std"}, missing
    return net


@pytest.mark.parametrize("s", NET_VARIANTS, ids=[V.key(*s) for s in NET_VARIANTS])
def test_traj_ar_net_dims_context_and_observation_match_reference(golden, s):
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    from kinpoly_amd.pretrain import observe
    from kinpoly_amd.sim import ar_obs_dim
    from kinpoly_amd.supervised import TorchFK
    g = golden("ar_obs_variants")
    k = V.key(*s)
    net = _seeded_net(g, s)
    assert [net.state_dim, net.context_dim] == list(g["net_dims_" + k]) and net.state_dim == ar_obs_dim(*s) == V.width(*s)
    assert tuple(net.action_rnn.rnn_f.weight_ih.shape) == (3 * 1024, net.state_dim) and tuple(net.context_rnn.rnn_f.weight_ih.shape) == (3 * 1024, net.context_dim)
    data = {key[7:]: torch.tensor(g[key], dtype=torch.float64) for key in g.files if key.startswith("net_in_")}
    with torch.no_grad():
        ctx = net.get_context_feat(data)
    np.testing.assert_allclose(ctx[:, :, :64].numpy(), g["net_ctx_" + k], rtol=1e-9, atol=1e-11)          # test_no_action_cpu.py's bound on the same quantity
    kpm = read_kpm(DEFAULT_KPM)
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], "cpu", dtype=torch.float64)
    want = g["net_obs_" + k]
    for t in range(want.shape[1]):
        obs, _, _ = observe(fk, data["qpos"][:, t], data, t, use_action=s[2], use_vel=s[0], use_head=s[1], qvel=data["qvel"][:, t])
        np.testing.assert_allclose(obs.numpy(), want[:, t], rtol=1e-8, atol=1e-10)                         # test_pretrain_cpu.py's bound on the roll-out's rows


def test_traj_ar_net_refuses_no_head_no_action_and_defaults_are_unchanged():
    from kinpoly_amd.context import TrajARNet
    with pytest.raises(ValueError, match="use_head.*use_action"):
        TrajARNet(rnn_hdim=8, mlp_hsize=(8, 8), use_head=False, use_action=False)
    net = TrajARNet(rnn_hdim=8, mlp_hsize=(8, 8))
    assert (net.state_dim, net.context_dim, net.use_vel, net.use_head, net.use_action) == (105, 17, False, True, True)


def test_supervised_forward_runs_at_every_width():
    """forward_supervised carries the roll-out's own velocity into the use_vel observation and back-propagates through it."""
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    from kinpoly_amd.pretrain import forward_supervised
    from kinpoly_amd.supervised import TorchFK
    kpm = read_kpm(DEFAULT_KPM)
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], "cpu", dtype=torch.float64)
    g = np.load(os.path.join(GOLDEN, "ar_obs_variants.npz"))
    data = {key[7:]: torch.tensor(g[key], dtype=torch.float64) for key in g.files if key.startswith("net_in_")}
    torch.manual_seed(0)
    for s in ((True, True, True), (False, False, True), (True, False, True)):
        net = TrajARNet(rnn_hdim=16, mlp_hsize=(16, 16), use_vel=s[0], use_head=s[1], use_action=s[2]).double()
        pred = forward_supervised(net, fk, data)
        assert tuple(pred["qpos"].shape) == (3, 5, 76) and torch.isfinite(pred["action"]).all()
        pred["action"].sum().backward()
        assert torch.isfinite(net.action_rnn.rnn_f.weight_ih.grad).all() and tuple(net.action_rnn.rnn_f.weight_ih.shape) == (48, V.width(*s))


def test_checkpoint_width_mismatch_names_both_variants(tmp_path):
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.nets import MLP, Value
    torch.manual_seed(0)
    small = dict(rnn_hdim=8, mlp_hsize=(8, 8))
    paths = {}
    for s in ((True, True, True), (False, False, True), (False, True, True)):
        net = TrajARNet(**small, use_vel=s[0], use_head=s[1], use_action=s[2])
        paths[s] = str(tmp_path / f"{V.key(*s)}.p")
        ck.save_checkpoint(paths[s], net, Value(MLP(net.state_dim, (8, 8), "relu")))
        sd = ck.split_policy_dict(ck.load_checkpoint(paths[s])["policy_dict"])
        assert ck.policy_obs_dim(sd) == V.width(*s) and ck.obs_switches(V.width(*s)) == dict(use_vel=s[0], use_head=s[1], use_action=s[2])
        back = ck.load_state_strict(TrajARNet(**small, use_vel=s[0], use_head=s[1], use_action=s[2]), sd, what=paths[s])
        for k, v in net.state_dict().items():
            assert torch.equal(back.state_dict()[k], v), k
    vel = ck.split_policy_dict(ck.load_checkpoint(paths[(True, True, True)])["policy_dict"])
    nohead = ck.split_policy_dict(ck.load_checkpoint(paths[(False, False, True)])["policy_dict"])
    with pytest.raises(ck.CheckpointWidthError, match=r"180-d, use_vel: true, use_head: true, use_action: true.*105-d, use_action: true"):
        ck.load_state_strict(TrajARNet(**small), vel, what="vel.p")
    with pytest.raises(ck.CheckpointWidthError, match=r"85-d, use_vel: false, use_head: false, use_action: true.*180-d, use_vel: true"):
        ck.load_state_strict(TrajARNet(**small, use_vel=True), nohead, what="nohead.p")
    with pytest.raises(ck.CheckpointWidthError, match=r"105-d, use_action: true.*85-d, use_vel: false, use_head: false"):
        ck.load_state_strict(TrajARNet(**small, use_head=False), ck.split_policy_dict(ck.load_checkpoint(paths[(False, True, True)])["policy_dict"]), what="wide.p")
    assert all(ck.obs_switches(d) is None for d in (0, 100, 104, 106, 179))


def test_model_options_answer_the_eight_widths():
    """kp_model_set_option / kp_model_get_option (host code: no GPU): ar_obs_vel / ar_obs_head next to ar_obs_action; defaults unchanged; anything but 0 / 1 refused."""
    from kinpoly_amd import sim as kpsim
    m = kpsim.KpModel()
    assert [m.get_option(k) for k in ("ar_obs_vel", "ar_obs_head", "ar_obs_action", "ar_obs_dim")] == [0, 1, 1, 105]
    for s in V.VARIANTS:
        m = kpsim.KpModel(**kpsim.ar_obs_options(*s))
        assert m.get_option("ar_obs_dim") == V.width(*s) == kpsim.ar_obs_dim(*s)
        assert [bool(m.get_option(k)) for k in ("ar_obs_vel", "ar_obs_head", "ar_obs_action")] == list(s)
    assert kpsim.ar_obs_options() == {} and sorted(kpsim.AR_OBS_DIMS) == sorted(V.width(*s) for s in V.VARIANTS)
    for name in ("ar_obs_vel", "ar_obs_head"):
        for bad in (2, -1, 0.5):
            with pytest.raises(kpsim.KinPolyNativeError, match=name):
                kpsim.KpModel(**{name: bad})
