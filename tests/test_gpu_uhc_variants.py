"""GPU tests of the UHC config's observation variants (kp_sim_obs_cc_ex / the k_obs_cc template against the reference's get_full_obs / _v1 / _v2 fixture),
the default handle's bit equality with kp_sim_obs_cc and kp_sim_obs_cc's 784-wide row on a handle of another layout, the option checks, the env's 'head' termination rule, and train_uhc.py --cfg end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VDIR = os.path.join(GOLD, "uhc_variants")
ACCEPTED = ["uhc_v0_gauss", "uhc_v2_root", "uhc_v1_root_gauss", "uhc_v0_plain", "uhc_meta_pd", "uhc_ctrl_defaults", "uhc_meta_joint_v0"]


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def _opts(v, root, h, d, p):
    return dict(cc_obs_v=int(v), cc_obs_vel_root=int(root), cc_obs_heading=int(h), cc_obs_deheading=int(d), cc_obs_phase=int(p))


def test_every_obs_variant_matches_reference(kp):
    g = np.load(os.path.join(GOLD, "uhc_obs_variants.npz"))
    n, T = len(g["qpos"]), int(g["len"])
    t = g["t"]
    for j, var in enumerate(g["variants"]):
        sim = kp.KpSim(kp.KpModel(**_opts(*var)), n)
        want = g[f"obs_{j}"]
        assert sim.cc_obs_dim == want.shape[1], (var, sim.cc_obs_dim)
        sim.set_state(dev(g["qpos"]), dev(g["qvel"]))
        sim.set_target(dev(g["clip"][t if var[0] == 0 else t + 1]))     # obs_v 0: expert frame t; v1 / v2: t + 1
        phase = dev(t / T) if (var[0] == 0 and var[4]) else None
        got = sim.obs_cc(phase=phase).cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(got, want, atol=5e-6, rtol=0, err_msg=str(var))       # the existing obs tests' bound


def test_zfilter_on_a_narrow_variant(kp):
    g = np.load(os.path.join(GOLD, "uhc_obs_variants.npz"))
    n = len(g["qpos"])
    sim = kp.KpSim(kp.KpModel(**_opts(2, 1, 0, 0, 0)), n)
    sim.set_state(dev(g["qpos"]), dev(g["qvel"])); sim.set_target(dev(g["clip"][g["t"] + 1]))
    raw = sim.obs_cc().cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(3)
    m, s = rng.normal(size=571), rng.uniform(0.1, 2.0, 571)
    z = sim.obs_cc(zf_mean=dev(m), zf_std=dev(s), clip=2.0).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(z, np.clip((raw - m) / (s + 1e-8), -2, 2), atol=1e-5, rtol=1e-6)
    with pytest.raises(ValueError, match="571"):
        sim.obs_cc(zf_mean=dev(np.zeros(784)), zf_std=dev(np.ones(784)))


def test_default_handle_is_bit_identical_to_obs_cc(kp):
    import ctypes as C
    g = np.load(os.path.join(GOLD, "uhc_obs_variants.npz"))
    n = len(g["qpos"])
    model = kp.KpModel()
    assert model.get_option("cc_obs_dim") == 784 and model.get_option("cc_action_dim") == 75
    sim = kp.KpSim(model, n)
    assert sim.cc_obs_dim == 784 and sim.cc_action_dim == 75
    sim.set_state(dev(g["qpos"]), dev(g["qvel"])); sim.set_target(dev(g["clip"][g["t"] + 1]))
    rng = np.random.default_rng(4)
    zm, zs = dev(rng.normal(size=784)), dev(rng.uniform(0.5, 2.0, 784))
    for args in ((None, None, 0.0), (zm, zs, 5.0)):
        ex = sim.obs_cc(zf_mean=args[0], zf_std=args[1], clip=args[2])
        old = torch.empty_like(ex)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
        assert sim.L.kp_sim_obs_cc(sim.h, p(old), p(args[0]), p(args[1]), C.c_float(args[2])) == 0
        torch.cuda.synchronize()
        assert torch.equal(ex, old)
    # kp_sim_obs_cc is the 784-wide get_full_obs_v1 row whatever the handle's layout: a cc_obs_v = 2 handle (640-wide rows of its own) on the same state
    n = 5
    assert len(g["qpos"]) >= n
    rows = []
    for opts in ({}, _opts(2, 0, 0, 0, 0)):
        sim = kp.KpSim(kp.KpModel(**opts), n)
        sim.set_state(dev(g["qpos"][:n]), dev(g["qvel"][:n])); sim.set_target(dev(g["clip"][g["t"][:n] + 1]))
        for args in ((None, None, 0.0), (zm, zs, 5.0)):
            out = torch.full((n, 784), float("nan"), device="cuda")
            assert sim.L.kp_sim_obs_cc(sim.h, p(out), p(args[0]), p(args[1]), C.c_float(args[2])) == 0
            torch.cuda.synchronize()
            rows.append(out)
    assert sim.cc_obs_dim == 640 and torch.isfinite(rows[0]).all()
    assert torch.equal(rows[0], rows[2]) and torch.equal(rows[1], rows[3])


def test_options_and_phase_are_checked(kp):
    m = kp.KpModel()
    for k, v in (("cc_obs_v", 3), ("cc_obs_vel_root", 2), ("cc_obs_heading", -1), ("cc_obs_deheading", 0.5), ("cc_obs_phase", 7)):
        with pytest.raises(kp.KinPolyNativeError, match=k):
            m.set_option(k, v)
    m.set_option("cc_obs_v", 0)
    assert m.get_option("cc_obs_dim") == 74 + 75 + 69
    m.set_option("cc_obs_phase", 1); m.set_option("cc_obs_heading", 1); m.set_option("cc_obs_vel_root", 1)
    assert m.get_option("cc_obs_dim") == 1 + 74 + 6 + 69 + 1
    sim = kp.KpSim(m, 4)
    m.set_option("cc_obs_v", 1)                                    # a handle keeps the widths it was created with
    assert sim.cc_obs_dim == 151 and kp.KpSim(m, 4).cc_obs_dim == 715
    with pytest.raises(kp.KinPolyNativeError, match="phase"):
        sim.obs_cc()
    with pytest.raises(kp.KinPolyNativeError, match="phase"):
        kp.KpSim(kp.KpModel(), 4).obs_cc(phase=torch.zeros(4, device="cuda"))


def test_env_follows_the_config(kp):
    from kinpoly_amd.uhc_config import UhcConfig
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv
    std = np.load(os.path.join(GOLD, "standing_neutral.npz"))
    n, T = 64, 12
    clips = np.tile(std["qpos"], (n, T, 1))
    clips[:, 1:, 0] += 3.0                                               # the expert steps 3 m away: body_diff > 0.5 from the first step on
    clips = torch.tensor(clips, dtype=torch.float32)
    cfg = UhcConfig(os.path.join(VDIR, "uhc_v0_gauss.yml"))           # obs_v 0 with heading, de-heading, phase; env_term_body dropped: 'head'
    env = BatchedHumanoidEnv(n, 0, cfg=cfg, seed=0)
    env.load_expert(clips)
    assert env.obs_dim == 220 and env.action_dim == 75 and env.env_episode_len == 100000
    obs = env.reset()
    assert obs.shape == (n, 220) and torch.all(obs[:, -1] == 0)         # phase 0 at reset
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    a = torch.randn((n, 75), device="cuda", generator=gen) * 3.0            # a flailing controller: the body drifts off the expert
    for k in range(4):
        obs, _, done, info = env.step(a)
        assert float(info["body_diff"].min()) > 0.5 and not bool(info["fail"].any())      # 'head' never fails an episode (humanoid_im.py:554-561)
        assert torch.allclose(obs[:, -1], torch.full((n,), (k + 1) / T, device="cuda"))
        assert torch.allclose(obs[:, 1 + 74 + 75:1 + 74 + 75 + 69], env._e("qpos", env.cur_t)[:, 7:])     # kin pose of expert frame t


@pytest.mark.parametrize("name", ACCEPTED)
def test_train_uhc_cfg_runs_and_checkpoint_reloads(kp, tmp_path, name):
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd.uhc_config import UhcConfig
    ckpt = str(tmp_path / "iter.p")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_uhc.py"), "--cfg", os.path.join(VDIR, name + ".yml"), "--num_envs", "256",
                        "--iters", "2", "--horizon", "8", "--clip_len", "16", "--num_optim_epoch", "2", "--save", ckpt],
                       capture_output=True, text=True, timeout=400, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 2 and all(np.isfinite([x["value_loss"], x["surr_loss"], x["avg_reward"]]).all() for x in lines)
    cfg = UhcConfig(os.path.join(VDIR, name + ".yml"))
    cp = ck.load_checkpoint(ckpt)
    pol = cfg.make_policy()
    pol.load_state_dict({k: torch.as_tensor(v) for k, v in cp["policy_dict"].items()})
    mean, std, _ = ck.running_state_arrays(cp["running_state"])
    assert len(mean) == len(std) == cfg.obs_dim
    if not cfg.is_default_controller:                                  # the kinematic-policy env refuses a controller of another variant
        from kinpoly_amd.config import ConfigError
        from kinpoly_amd.env import BatchedHumanoidAREnv
        env = BatchedHumanoidAREnv(4, 0)
        with pytest.raises(ConfigError):
            env.load_uhc_checkpoint(ckpt)
