"""GPU tests of the no-action-label ablation (use_action: false, kin_poly_wo_action.yml): the 101-wide observation and record kernels through the C ABI,
the HIP kinematic roll-out of the 101-d TrajARNet, and the agent end to end (sample, PPO, supervised step, checkpoint)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import np_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def _ctx(sim, g, T=6):
    """Per-env context of length T whose row cur_t carries the fixture's rows (the reward inputs are unused here)."""
    n = len(g["qpos"])
    rng = np.random.default_rng(5)
    t = g["t"].astype(np.int32)
    hp, hv, orl = rng.normal(size=(n, T, 7)), rng.normal(size=(n, T, 6)), rng.normal(size=(n, T, 7))
    for i in range(n):
        hp[i, t[i]], hv[i, t[i]], orl[i, t[i]] = g["head_pose"][i], g["head_vels"][i], g["obj_rel"][i]
    cur_t = torch.tensor(t, dtype=torch.int32, device="cuda")
    ctx = sim.make_ctx(T, dev(hp), dev(hv), dev(orl), dev(g["action_one_hot"]), dev(np.tile([1.0, 0, 0, 0], (n, T, 24))), dev(np.zeros((n, T, 72))), cur_t,
                       obj_qpos=dev(g["obj_qpos7"]))
    return ctx, dict(head_pose=hp, head_vels=hv, obj_rel=orl, t=t)


def test_observation_without_action_matches_reference_and_the_default_handle(kp, golden):
    g = golden("ar_obs_no_action")
    n = len(g["qpos"])
    m0, m1 = kp.KpModel(ar_obs_action=0), kp.KpModel()
    assert (m0.get_option("ar_obs_action"), m0.get_option("ar_obs_dim")) == (0, 101)
    assert (m1.get_option("ar_obs_action"), m1.get_option("ar_obs_dim")) == (1, 105)
    s0, s1 = kp.KpSim(m0, n), kp.KpSim(m1, n)                          # a 101-wide and a 105-wide handle in one process
    assert (s0.obs_ar_dim, s1.obs_ar_dim) == (101, 105)
    for s in (s0, s1):
        s.set_state(dev(g["qpos"]), dev(g["qvel"]))
    np.testing.assert_allclose(s0.get("xpos").double().cpu().numpy().reshape(n, 24, 3), g["xpos"], atol=2e-5)     # the fixture's derived state
    (c0, c), (c1, _) = _ctx(s0, g), _ctx(s1, g)
    o0, o1 = s0.obs_ar(c0), s1.obs_ar(c1)
    assert tuple(o0.shape) == (n, 101) and tuple(o1.shape) == (n, 105)
    np.testing.assert_allclose(o0.double().cpu().numpy(), g["obs_ar"], atol=5e-6, rtol=0)          # the reference's get_ar_obs_v1, use_action off
    rd = {k: s0.get(k).double().cpu().numpy() for k in ("qpos", "xpos", "xquat")}
    for i in range(n):
        t = c["t"][i]
        want = O.obs_ar(rd["qpos"][i], rd["xpos"][i].reshape(24, 3), rd["xquat"][i].reshape(24, 4), c["head_pose"][i, t], c["head_vels"][i, t], c["obj_rel"][i, t],
                        g["action_one_hot"][i], g["obj_qpos7"][i])
        np.testing.assert_allclose(o0[i].double().cpu().numpy(), want[:101], atol=5e-6, rtol=0)
    assert torch.equal(o0, o1[:, :101])
    # stepped from the same state with the same controls: the same physics, and again the first 101 columns bit for bit
    act = dev(np.random.default_rng(6).normal(size=(n, 75)) * 0.2)
    for s in (s0, s1):
        s.set_target(dev(g["qpos"])); s.step_begin(); s.step_ctrl(act, 15)
    assert torch.equal(s0.get("qpos"), s1.get("qpos"))
    o0, o1 = s0.obs_ar(c0), s1.obs_ar(c1)
    assert torch.isfinite(o0).all() and torch.equal(o0, o1[:, :101])


def test_abi_rejects_bad_widths(kp, golden):
    import ctypes as C
    with pytest.raises(kp.KinPolyNativeError, match="ar_obs_action"):
        kp.KpModel(ar_obs_action=2)
    g = golden("ar_obs_no_action")
    n = len(g["qpos"])
    s0 = kp.KpSim(kp.KpModel(ar_obs_action=0), n)
    ctx, _ = _ctx(s0, g)
    with pytest.raises(ValueError, match="101"):
        s0.obs_ar(ctx, out=torch.empty((n, 105), device="cuda"))           # a 105-row buffer handed to a 101-wide handle
    with pytest.raises(ValueError, match="obs_dim"):
        kp.record_pre(0, 2, obs=torch.zeros((n, 101), device="cuda"), obs_dim=103)
    with pytest.raises(ValueError, match="states"):
        kp.record_pre(0, 2, obs=torch.zeros((n, 101), device="cuda"), states=torch.zeros((n, 2, 105), device="cuda"), obs_dim=101)
    L = kp.load_library()
    r = kp.KpRecordPre(n, 2, 0, 0)                                       # every pointer NULL: the width is checked before anything is launched
    assert L.kp_rollout_record_pre_w(C.byref(r), 103, None) == -1 and b"obs_dim" in L.kp_last_error()
    assert L.kp_rollout_record_post_w(C.byref(kp.KpRecordPost(n, 2, 0, 0.0)), 0, None) == -1 and b"obs_dim" in L.kp_last_error()


def test_record_kernels_at_width_101(kp):
    n, T, t = 37, 4, 2
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, nxt = torch.randn((n, 101), device="cuda", generator=g), torch.randn((n, 101), device="cuda", generator=g)
    S, NS = torch.full((n, T, 101), float("nan"), device="cuda"), torch.full((n, T, 101), float("nan"), device="cuda")
    E = torch.zeros((n, T), dtype=torch.bool, device="cuda")
    fresh = torch.rand(n, device="cuda", generator=g) > 0.5
    kp.record_pre(t, T, obs=obs, fresh=fresh, states=S, episode_start=E, obs_dim=101)
    action = torch.randn((n, 80), device="cuda", generator=g)
    A = torch.zeros((n, T, 80), device="cuda")
    kp.record_post(t, T, action=action, obs=nxt, actions=A, next_states=NS, obs_dim=101)
    torch.cuda.synchronize()
    assert torch.equal(S[:, t], obs) and torch.equal(NS[:, t], nxt) and torch.equal(A[:, t], action) and torch.equal(E[:, t], fresh)
    others = [k for k in range(T) if k != t]
    assert torch.isnan(S[:, others]).all() and torch.isnan(NS[:, others]).all()          # nothing written outside row t, nor past 101 floats
    # the 105-wide default of the same wrappers is unchanged
    S5 = torch.zeros((n, T, 105), device="cuda"); o5 = torch.randn((n, 105), device="cuda", generator=g)
    kp.record_pre(t, T, obs=o5, states=S5)
    assert torch.equal(S5[:, t], o5)


def test_context_rollout_without_action_matches_reference_fixture(kp, golden):
    from kinpoly_amd.context import PolicyARContext
    from tests.test_no_action_cpu import fixture_data, seeded_net
    g = golden("traj_ar_net_no_action")
    net = seeded_net(g, torch.float32).cuda()
    data = fixture_data(g, torch.float32, "cuda")
    B, T = data["qpos"].shape[:2]
    kin_sim = kp.KpSim(kp.KpModel(ar_obs_action=0), B)
    with torch.no_grad():
        init_qpos, init_qvel, _ = net.init_states(data)
    np.testing.assert_allclose(init_qpos.double().cpu().numpy(), g["init_qpos"], atol=3e-06)        # test_gpu_env.py's tolerances
    q, v, a = net.rollout(data, kin_sim, init_qpos, init_qvel)
    np.testing.assert_allclose(a.double().cpu().numpy(), g["action"], atol=1e-06)
    np.testing.assert_allclose(q.double().cpu().numpy(), g["ar_qpos"], atol=3e-06)
    np.testing.assert_allclose(v.double().cpu().numpy(), g["ar_qvel"], atol=3e-05)
    ctx = PolicyARContext(net, kin_sim, smooth=True).init_context(data)
    np.testing.assert_allclose(ctx["ar_qpos"].double().cpu().numpy(), g["ar_qpos"], atol=3e-06)
    with pytest.raises(ValueError, match="105-d observations"):          # a 105-wide twin under the 101-d policy is named, not a GEMM shape error
        net.rollout(data, kp.KpSim(kp.KpModel(), B), init_qpos, init_qvel)


def test_agent_without_action_end_to_end(kp, tmp_path):
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd import dataset as D
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.model_compiler import read_kpm
    n, fr, H = 256, 12, 6
    fk_sim = kp.KpSim(kp.KpModel(kp.STEP_KPM), n, 0)
    takes = D.synthetic_takes(fk_sim, STD["qpos"], n_per_action=2, T_range=(fr + 4, fr + 14), body_mass=read_kpm(kp.STEP_KPM)["body_mass"], seed=3)
    ds = D.StateARDataset(takes, fr_num=fr, seed=3, device=fk_sim.device)
    agent = AgentAR(n, dataset=ds, device=0, horizon=H, num_optim_epoch=1, num_step_update=1, use_action=False, seed=2)
    assert agent.env.obs_dim == 101 and agent.env.use_action is False and agent.kin_sim.obs_ar_dim == 101
    assert agent.policy_net.state_dim == 101 and agent.policy_net.context_dim == 13
    assert agent.value_net.net.affine_layers[0].weight.shape[1] == 101
    batch = agent.sampler.sample(H)                                      # one sample() of a short horizon
    assert tuple(batch.states.shape) == (n, H, 101) and tuple(batch.last_states.shape) == (n, 101)
    assert torch.isfinite(batch.states).all() and torch.isfinite(batch.rewards).all() and float(batch.rewards.mean()) > 0
    info = agent.update_params(batch)                                    # PPO epochs + the supervised step update
    for k in ("surr_loss", "value_loss", "step_loss"):
        assert np.isfinite(info[k]), (k, info[k])
    ws = agent.train_init(1, 1, num_sample=64, batch_size=32)            # the supervised warm start, one epoch of each phase
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in ws.values()), ws
    info = agent.optimize_policy(0)                                      # and a whole iteration after it
    assert info["num_steps"] == n * H and np.isfinite(info["value_loss"])
    # checkpoint round trip: identical action means on the same observations
    path = str(tmp_path / "iter_0001.p")
    agent.save_checkpoint(path)
    obs = batch.states[:, 0].contiguous()
    with torch.no_grad():
        m0, _ = agent.policy_net.get_action(obs, agent.policy_net.init_hidden(n))
        for p in agent.policy_net.parameters():
            p.add_(0.5)
    agent.load_checkpoint(path)
    with torch.no_grad():
        m1, _ = agent.policy_net.get_action(obs, agent.policy_net.init_hidden(n))
    assert torch.equal(m0, m1)
    from kinpoly_amd.context import TrajARNet
    with pytest.raises(ck.CheckpointWidthError, match="101-d.*105-d"):           # the checkpoint under a default-width network
        ck.load_state_strict(TrajARNet(), ck.split_policy_dict(ck.load_checkpoint(path)["policy_dict"]), what=path)
