"""CPU tests of the UHC config reader (kinpoly_amd/uhc_config.py) and the Gaussian UHC actor: the reference copycat_config.Config attributes of the
variant files, the refusals, the widths, PolicyGaussian against the reference forward (tests/golden/uhc_*, tools/make_golden_uhc_variants.py)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from kinpoly_amd.config import ConfigError
from kinpoly_amd.uhc_config import UhcConfig, require_uhc_yml_controller, uhc_action_dim, uhc_obs_dim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VDIR = os.path.join(GOLD, "uhc_variants")
REF_ATTRS = json.load(open(os.path.join(GOLD, "uhc_variants_config.json")))
ACCEPTED = ["uhc_v0_gauss", "uhc_v2_root", "uhc_v1_root_gauss", "uhc_v0_plain", "uhc_meta_pd", "uhc_ctrl_defaults", "uhc_meta_joint_v0"]


def _yml(name):
    return os.path.join(VDIR, name + ".yml")


@pytest.mark.parametrize("name", sorted(REF_ATTRS))
def test_attributes_match_reference_config(name):
    c = UhcConfig(_yml(name), check=False)
    for k, want in REF_ATTRS[name].items():
        got = getattr(c, k)
        assert got == want, f"{name}.{k}: {got!r} != reference {want!r}"


@pytest.mark.parametrize("name", ACCEPTED)
def test_accepted_variants_and_their_widths(name):
    c = UhcConfig(_yml(name))
    r = REF_ATTRS[name]
    assert c.obs_dim == uhc_obs_dim(r["obs_v"], r["obs_vel"], r["obs_heading"], r["obs_phase"])
    assert c.action_dim == uhc_action_dim(r["residual_force"], r["residual_force_mode"], r["meta_pd"], r["meta_pd_joint"])
    assert c.vf_dim == (6 if r["residual_force"] else 0)
    o = c.model_options()
    assert o["cc_action_v"] == r["action_v"] and o["cc_rfc"] == int(r["residual_force"])
    assert o["cc_meta_pd"] == (1 if r["meta_pd"] else 2 if r["meta_pd_joint"] else 0)
    assert o["cc_obs_v"] == r["obs_v"] and o["cc_obs_vel_root"] == (r["obs_vel"] == "root")
    assert o["cc_obs_phase"] == int(r["obs_v"] == 0 and r["obs_phase"])


def test_id_lookup_under_config_root(tmp_path):
    d = tmp_path / "config" / "uhc"
    d.mkdir(parents=True)
    (d / "ctl.yml").write_text(open(_yml("uhc_v2_root")).read())
    c = UhcConfig("ctl", config_root=str(tmp_path))
    assert c.id == "ctl" and c.obs_dim == 571
    with pytest.raises(ConfigError, match="found 0"):
        UhcConfig("nope", config_root=str(tmp_path))


def test_widths_formula():
    assert [uhc_obs_dim(1, "full"), uhc_obs_dim(1, "root"), uhc_obs_dim(2, "full"), uhc_obs_dim(2, "root")] == [784, 715, 640, 571]
    assert uhc_obs_dim(0) == 219                                   # the reference defaults: obs_vel full, obs_phase on, no heading
    assert uhc_obs_dim(0, "root", True, False) == 1 + 74 + 6 + 69
    assert uhc_obs_dim(0, "full", True, True) == 220
    assert uhc_action_dim(True) == 75 and uhc_action_dim(False) == 69
    assert uhc_action_dim(True, meta_pd=True) == 105 and uhc_action_dim(True, meta_pd_joint=True) == 213
    assert uhc_action_dim(True, meta_pd=True, meta_pd_joint=True) == 105       # meta_pd wins (humanoid_im.py:84-89)
    g = np.load(os.path.join(GOLD, "uhc_obs_variants.npz"))
    for j, (v, root, h, _, p) in enumerate(g["variants"]):
        assert g[f"obs_{j}"].shape[1] == uhc_obs_dim(int(v), "root" if root else "full", bool(h), bool(p))


@pytest.mark.parametrize("name,keys", [("uhc_defaults", ["reward_id"])])
def test_refused_variant_files(name, keys):
    with pytest.raises(ConfigError) as e:
        UhcConfig(_yml(name))
    for k in keys:
        assert f"{k}:" in str(e.value)


@pytest.mark.parametrize("key,value", [("residual_force_mode", "explicit"), ("action_type", "torque"), ("obs_type", "partial"), ("obs_coord", "heading"),
                                       ("env_term_body", "Head"), ("env_term_body", "root"), ("reward_id", "quat"), ("jkp_multiplier", 2.0),
                                       ("jkd_multiplier", 0.5), ("torque_limit_multiplier", 1.5), ("action_v", 2), ("residual_force", "yes"),
                                       ("meta_pd_joint", 1), ("obs_v", 3), ("obs_vel", "none"), ("actor_type", "vae"), ("residual_force_scale", 200.0)])
def test_each_refused_value_names_its_key(tmp_path, key, value):
    y = yaml.safe_load(open(_yml("uhc_v2_root")))
    y[key] = value
    p = tmp_path / "v.yml"
    p.write_text(yaml.safe_dump(y))
    with pytest.raises(ConfigError) as e:
        UhcConfig(str(p))
    msg = str(e.value)
    assert f"{key}: {value!r}" in msg and "implemented" in msg


def test_kin_poly_env_refuses_variant_controllers():
    for name, key in (("uhc_v2_root", "obs_v"), ("uhc_v1_root_gauss", "obs_vel"), ("uhc_v0_gauss", "obs_v"), ("uhc_meta_pd", "meta_pd"),
                      ("uhc_ctrl_defaults", "action_v"), ("uhc_ctrl_defaults", "residual_force"), ("uhc_meta_joint_v0", "meta_pd_joint")):
        with pytest.raises(ConfigError, match=key):
            require_uhc_yml_controller(UhcConfig(_yml(name)))
    ok = UhcConfig(_yml("uhc_v2_root"))
    ok.obs_v = 1; ok.obs_vel = "full"
    require_uhc_yml_controller(ok)                                 # uhc.yml's controller passes


def test_policy_gaussian_matches_reference():
    from kinpoly_amd.nets import PolicyGaussian
    g = np.load(os.path.join(GOLD, "uhc_policy_gaussian.npz"))
    sd = {k[4:]: torch.tensor(g[k]) for k in g.files if k.startswith("sd__")}
    pol = PolicyGaussian(g["x"].shape[1], g["mean"].shape[1], tuple(int(h) for h in g["hsize"]), str(g["htype"])).double()
    assert set(pol.state_dict()) == set(sd)
    pol.load_state_dict(sd)
    with torch.no_grad():
        mean, log_std = pol(torch.tensor(g["x"]))
    np.testing.assert_allclose(mean.numpy(), g["mean"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(torch.exp(log_std).numpy(), g["std"], atol=1e-12, rtol=0)


def test_policy_gaussian_init_follows_reference():
    from kinpoly_amd.nets import PolicyGaussian
    torch.manual_seed(0)
    pol = PolicyGaussian(219, 75, (300, 200), "relu", log_std=-2.3, fix_std=True)
    assert float(pol.action_mean.bias.detach().abs().max()) == 0.0
    assert float(pol.action_mean.weight.detach().abs().max()) <= 0.1 / np.sqrt(200) + 1e-7       # Linear's U(-1/sqrt(fan_in), ..) x 0.1
    assert not pol.action_log_std.requires_grad and torch.all(pol.action_log_std == -2.3)
    c = UhcConfig(_yml("uhc_v0_gauss"))
    p = c.make_policy()
    assert isinstance(p, PolicyGaussian) and p.action_mean.in_features == 256 and p.net.affine_layers[0].in_features == c.obs_dim
    m = UhcConfig(_yml("uhc_v2_root")).make_policy()
    assert m.nets[0][0].affine_layers[0].in_features == 571 and m.action_log_std.shape == (1, 75)


def test_controller_restatement_matches_reference():
    """tests/uhc_ctrl_oracle.compute_torque_xc (the GPU tests' oracle) against the reference's compute_torque: action_v 0 / 1, meta_pd, meta_pd_joint,
    residual force on / off (the meta block's offset), substeps 0 / 7 / 14, with both clip bounds of the meta scale hit."""
    from kinpoly_amd.model_compiler import read_kpm
    from uhc_ctrl_oracle import compute_torque_xc
    g = np.load(os.path.join(GOLD, "uhc_controller_variants.npz"))
    kpm = read_kpm(os.path.join(ROOT, "kinpoly_amd", "assets", "smpl_humanoid.kpm"))
    for r in range(len(g["torque"])):
        av, meta, rfc = g["variants"][g["variant"][r]]
        i = g["state"][r]
        base = g["expert_qpos"][i][7:] if av == 1 else g["a_ref"]
        tau = compute_torque_xc(g["qpos"][i], g["qvel"][i], g["M"][i], g["bias"][i], g["ctrl"][r], base, kpm, av, meta, rfc, int(g["i_iter"][r]))
        np.testing.assert_allclose(tau, g["torque"][r], rtol=1e-9, atol=1e-9, err_msg=str((av, meta, rfc)))


def test_a_ref_is_read_from_joint_params():
    g = np.load(os.path.join(GOLD, "uhc_controller_variants.npz"))
    c = UhcConfig(_yml("uhc_ctrl_defaults"))
    assert c.action_v == 0 and c.residual_force is False and c.action_dim == 69
    np.testing.assert_allclose(c.a_ref, g["a_ref"], rtol=0, atol=1e-15)


def test_reward_vf_term_takes_the_last_vf_dim_entries():
    """world_rfc_implicit_reward's w_vf term reads action[-env.vf_dim:] (reward_function.py:44-46): the meta entries with meta-PD, and the whole action
    (action[-0:]) with residual_force off."""
    from kinpoly_amd.uhc_env import UHC_REWARD_WEIGHTS, world_rfc_implicit_reward_t
    torch.manual_seed(0)
    n = 5
    bq = torch.nn.functional.normalize(torch.randn(n, 24, 4, dtype=torch.float64), dim=-1).reshape(n, 96)
    args = (torch.randn(n, 72, dtype=torch.float64), bq, bq, torch.randn(n, 3, dtype=torch.float64))
    ex = (bq, torch.zeros(n, 72, dtype=torch.float64), torch.zeros(n, 15, dtype=torch.float64), torch.zeros(n, 3, dtype=torch.float64), torch.ones(24, dtype=torch.float64))
    for A, vf_dim in ((75, 6), (105, 6), (69, 0), (207, 0)):
        a = torch.randn(n, A, dtype=torch.float64) * 0.3
        _, info = world_rfc_implicit_reward_t(*args, a, *ex, 1.0 / 30.0, UHC_REWARD_WEIGHTS, vf_dim)
        want = np.exp(-UHC_REWARD_WEIGHTS["k_vf"] * ((a.numpy()[:, -vf_dim:] if vf_dim else a.numpy()) ** 2).sum(1))
        np.testing.assert_allclose(info[:, 4].numpy(), want, rtol=1e-12)
