"""GPU tests of the kinematic observation's use_vel / use_head variants (model options ar_obs_vel / ar_obs_head next to ar_obs_action):
the k_obs_ar template (the 105 / 101 rows: k_obs_ar_thread) through kp_sim_obs_ar against the reference's rows (tests/golden/ar_obs_variants.npz) and, swept over batch sizes and edge rows, against the
fp64 restatement (tests/ar_obs_variants_oracle.py); the record kernels at the six new widths; the agent end to end from a variant yml.

Bounds: the fixture rows are held to 5e-6, what tests/test_gpu_no_action.py applies to the 101-d rows against its fixture, and the sweep to
tests/test_gpu_side_kernels.py::test_obs_ar_sweep's 5e-6 (random rows) / 6.6e-6 (edge rows): the blocks are the 105-d row's arithmetic on the same
inputs (checked bit for bit below), and the one new block, the velocities, is a copy (checked bit for bit).  Every figure is printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ar_obs_variants_oracle as V  # noqa: E402
import test_gpu_side_kernels as K  # noqa: E402  (its state / context builders and batch sizes; nothing of it is collected from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STD = np.load(os.path.join(GOLDEN, "standing_neutral.npz"))
NEW = V.NEW_VARIANTS
IDS = [V.key(*s) for s in NEW]
COMMON = (("pose", 74), ("diff", 7), ("obj", 7), ("tgt", 13), ("act", 4))          # the blocks of the 105-d row


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    yield kpsim
    K._SIMS.clear()
    torch.cuda.empty_cache()


dev, host, f32 = K.dev, K.host, K.f32


def _opts(kp, s):
    return kp.ar_obs_options(*s)


def _present(s, block):
    return dict(pose=True, diff=s[1], obj=True, tgt=s[1], act=s[2])[block]


def _same_as_105(obs, base, s):
    """every block the variant shares with the 105-d row equals that row's bit for bit: k_obs_ar's instantiation against k_obs_ar_thread<true>'s hand-numbered
    columns, so this holds ObsArLayout's offsets and the shared expressions; the 105-d row itself is held to its recorded words below"""
    o, o5 = V.offsets(*s), V.offsets(False, True, True)
    for block, w in COMMON:
        if _present(s, block):
            assert torch.equal(obs[:, o[block]:o[block] + w], base[:, o5[block]:o5[block] + w]), (s, block)


def _fixture_ctx(sim, g, T=6):
    """tests/test_gpu_no_action.py::_ctx on the variants fixture: per-env context whose row cur_t carries the fixture's rows"""
    n = len(g["env_qpos"])
    rng = np.random.default_rng(5)
    t = g["env_t"].astype(np.int32)
    hp, hv, orl = rng.normal(size=(n, T, 7)), rng.normal(size=(n, T, 6)), rng.normal(size=(n, T, 7))
    for i in range(n):
        hp[i, t[i]], hv[i, t[i]], orl[i, t[i]] = g["env_head_pose"][i], g["env_head_vels"][i], g["env_obj_rel"][i]
    cur_t = torch.tensor(t, dtype=torch.int32, device="cuda")
    return sim.make_ctx(T, dev(hp), dev(hv), dev(orl), dev(g["env_action_one_hot"]), dev(np.tile([1.0, 0, 0, 0], (n, T, 24))), dev(np.zeros((n, T, 72))), cur_t,
                        obj_qpos=dev(g["env_obj_qpos7"]))


@pytest.mark.parametrize("s", NEW, ids=IDS)
def test_observation_variant_matches_the_reference_rows(kp, golden, s):
    g = golden("ar_obs_variants")
    n = len(g["env_qpos"])
    m = kp.KpModel(**_opts(kp, s))
    assert m.get_option("ar_obs_dim") == V.width(*s)
    sim, base = kp.KpSim(m, n), kp.KpSim(kp.KpModel(), n)
    assert sim.obs_ar_dim == V.width(*s) and (sim.obs_ar_vel, sim.obs_ar_head, sim.obs_ar_action) == s and base.obs_ar_dim == 105
    for x in (sim, base):
        x.set_state(dev(g["env_qpos"]), dev(g["env_qvel"]))
    np.testing.assert_allclose(sim.get("xpos").double().cpu().numpy().reshape(n, 24, 3), g["env_xpos"], atol=2e-5)     # the fixture's derived state
    obs, obs5 = sim.obs_ar(_fixture_ctx(sim, g)), base.obs_ar(_fixture_ctx(base, g))
    assert tuple(obs.shape) == (n, V.width(*s))
    K.worst(f"obs_ar {V.key(*s)} vs the reference rows", host(obs), g["env_obs_" + V.key(*s)])
    np.testing.assert_allclose(obs.double().cpu().numpy(), g["env_obs_" + V.key(*s)], atol=5e-6, rtol=0)
    if s[0]:
        assert torch.equal(obs[:, 74:149], sim.get("qvel"))                  # the velocity block is a copy of KP_QVEL
    _same_as_105(obs, obs5, s)
    # stepped from the same state with the same controls: the same physics, and the velocity block follows the state rows the step leaves
    act = dev(np.random.default_rng(6).normal(size=(n, 75)) * 0.2)
    for x in (sim, base):
        x.set_target(dev(g["env_qpos"])); x.step_begin(); x.step_ctrl(act, 15)
    assert torch.equal(sim.get("qpos"), base.get("qpos")) and torch.equal(sim.get("qvel"), base.get("qvel"))
    obs, obs5 = sim.obs_ar(_fixture_ctx(sim, g)), base.obs_ar(_fixture_ctx(base, g))
    assert torch.isfinite(obs).all()
    if s[0]:
        assert torch.equal(obs[:, 74:149], sim.get("qvel"))
    _same_as_105(obs, obs5, s)
    with pytest.raises(ValueError, match=str(V.width(*s))):
        sim.obs_ar(_fixture_ctx(sim, g), out=torch.empty((n, 105), device="cuda"))          # a 105-row buffer handed to another width


@pytest.mark.parametrize("s", NEW, ids=IDS)
def test_observation_variant_sweep(kp, s):
    tot = {"rand": 0.0, "edge": 0.0}
    o = V.offsets(*s)
    for n in K.NS:
        sim, base = K.get_sim(kp, n, **_opts(kp, s)), K.get_sim(kp, n)
        st, edge = K._sim_state(kp, sim, n, 1000 + n)
        K.load(base, **st)
        c = K._ctx(kp, sim, n, 1100 + n)
        obs_t, obs5_t = sim.obs_ar(K._make_ctx(sim, c)), base.obs_ar(K._make_ctx(base, c))
        obs = host(obs_t).astype(np.float64)
        assert obs.shape == (n, V.width(*s))
        if s[0]:
            assert np.array_equal(host(obs_t)[:, o["vel"]:o["vel"] + 75], st["qvel"])
        _same_as_105(obs_t, obs5_t, s)
        for i in K.check_rows(n, 64):
            r, t = c["row"][i], min(max(int(c["cur_t"][i]), 0), c["T"] - 1)
            want = V.obs_ar_variant(st["qpos"][i].astype(np.float64), st["qvel"][i].astype(np.float64), st["xpos"][i].reshape(24, 3).astype(np.float64),
                                    st["xquat"][i].reshape(24, 4).astype(np.float64), c["head_pose"][r, t].astype(np.float64), c["head_vels"][r, t].astype(np.float64),
                                    c["obj_rel"][r, t].astype(np.float64), c["action_one_hot"][r].astype(np.float64), c["obj_qpos"][i].astype(np.float64), *s)
            tag = "edge" if edge[i] else "rand"
            tot[tag] = max(tot[tag], np.abs(obs[i] - want).max())
    print(f"MEASURED obs_ar {V.key(*s)} random / edge:", tot)
    assert tot["rand"] < 5e-6           # test_obs_ar_sweep's bounds: the same arithmetic
    assert tot["edge"] < 6.6e-6
    for key in [k for k in K._SIMS if k[1]]:                      # this variant's handles are done
        del K._SIMS[key]


@pytest.mark.parametrize("s", NEW, ids=IDS)
def test_observation_variant_is_position_independent(kp, s):
    n = 4099
    sim = K.get_sim(kp, n)
    st, _ = K._sim_state(kp, sim, n, 77)
    c = K._ctx(kp, sim, n, 78, extra=0)
    c["row"] = np.arange(n, dtype=np.int32)
    rows = dict(st)

    def run(x, idx):
        K.load(x, **{k: rows[k][idx] for k in ("qpos", "qvel", "xpos", "xquat")})
        ci = dict(c, head_pose=c["head_pose"][idx], head_vels=c["head_vels"][idx], obj_rel=c["obj_rel"][idx], gt_bquat=c["gt_bquat"][idx], gt_wbpos=c["gt_wbpos"][idx],
                  action_one_hot=c["action_one_hot"][idx], cur_t=c["cur_t"][idx], obj_qpos=c["obj_qpos"][idx], row=np.arange(len(idx), dtype=np.int32))
        return [host(x.obs_ar(K._make_ctx(x, ci)))]
    K._position_independent(kp, _opts(kp, s), rows, run)
    for key in [k for k in K._SIMS if k[1]]:
        del K._SIMS[key]


@pytest.mark.parametrize("n", [67, 1, 8, 9])
def test_the_105_and_101_rows_are_the_recorded_words(kp, golden, n):
    """kp_sim_obs_ar's 105- and 101-wide rows against the words recorded from the one-thread-per-env kernel (now k_obs_ar_thread) at the commit before
    kp_sim_obs_ar's dispatch became one table (tests/golden/obs_ar_parent_bits.npz, written by tools/make_golden_obs_ar_bits.py: inputs and uint32 views of the
    rows): not one word may differ, whichever kernel the table's two entries launch (k_obs_ar<false, true, .> wrote the same words when it was tried there).  67 envs are eight full blocks of the 8-envs-per-block mapping and a partial one of 3; 1, 8 and 9 are the first rows of the same inputs (below one
    block, one block, one block and one env).  The inputs hold cur_t below 0, at T - 1 and above it, a row map with repeats, all-zero one-hots, root
    quaternions with negative w, and every case once with an obj_qpos pointer and once with a null one."""
    g = golden("obs_ar_parent_bits")
    R, T = g["head_pose"].shape[:2]
    assert len(g["qpos"]) == 67 and g["cur_t"].min() < 0 and (g["cur_t"] == T - 1).any() and g["cur_t"].max() > T - 1 and (g["qpos"][:, 3] < 0).any()
    assert len(set(g["row"])) < 67 and (g["action_one_hot"][g["row"]].sum(1) == 0).any()
    z = torch.zeros((R, T, 96), device="cuda")
    for action in (True, False):
        sim = kp.KpSim(kp.KpModel(**kp.ar_obs_options(use_action=action)), n)
        K.load(sim, **{k: g[k][:n] for k in ("qpos", "xpos", "xquat")})
        for with_obj in (True, False):
            ctx = sim.make_ctx(T, dev(g["head_pose"]), dev(g["head_vels"]), dev(g["obj_rel"]), dev(g["action_one_hot"]), z, z[:, :, :72].contiguous(),
                               torch.tensor(g["cur_t"][:n], device="cuda"), obj_qpos=dev(g["obj_qpos"][:n]) if with_obj else None,
                               row=torch.tensor(g["row"][:n], device="cuda"))
            got = host(sim.obs_ar(ctx)).view(np.uint32)
            want = g[f"bits_{105 if action else 101}{'' if with_obj else '_null_obj'}"][:n]
            differ = int((got != want).sum())
            print(f"MEASURED obs_ar words that differ from the recorded ones, n = {n}, action {action}, obj_qpos {with_obj}: {differ} of {want.size}",
                  sorted(set(np.nonzero(got != want)[1].tolist())))
            assert got.shape == want.shape and differ == 0


@pytest.mark.parametrize("obs_dim", [180, 176, 85, 81, 160, 156])
def test_record_rows_at_the_new_widths_are_the_scatter_they_replace(kp, obs_dim):
    K.test_record_rows_are_the_scatter_they_replace(kp, obs_dim)          # the same check, at this width


def test_other_widths_are_refused_before_anything_is_launched(kp):
    n = 8
    for bad in (0, 75, 100, 104, 106, 179, 181, 784):
        with pytest.raises(ValueError, match="obs_dim"):
            kp.record_pre(0, 2, obs=torch.zeros((n, bad or 1), device="cuda"), obs_dim=bad)
    with pytest.raises(ValueError, match="states"):
        kp.record_pre(0, 2, obs=torch.zeros((n, 180), device="cuda"), states=torch.zeros((n, 2, 176), device="cuda"), obs_dim=180)
    L = kp.load_library()
    S = torch.full((n, 2, 181), -5.0, device="cuda")
    obs = torch.ones((n, 181), device="cuda")
    for bad in (0, 103, 181, 179):
        r = kp.KpRecordPre(n, 2, 0, 0, obs=obs.data_ptr(), states=S.data_ptr())          # valid pointers: a launch would write
        assert L.kp_rollout_record_pre_w(C.byref(r), bad, None) == -1
        err = L.kp_last_error().decode()
        assert "obs_dim" in err and all(str(w) in err for w in (105, 101, 180, 176, 85, 81, 160, 156)), err
        p = kp.KpRecordPost(n, 2, 0, 0.0, obs=obs.data_ptr(), next_states=S.data_ptr())
        assert L.kp_rollout_record_post_w(C.byref(p), bad, None) == -1 and "obs_dim" in L.kp_last_error().decode()
    torch.cuda.synchronize()
    assert bool((S == -5.0).all())                                             # nothing was launched
    for name in ("ar_obs_vel", "ar_obs_head"):
        with pytest.raises(kp.KinPolyNativeError, match=name):
            kp.KpModel(**{name: 2})


def _takes(n, fr, seed=3):
    from kinpoly_amd import dataset as D
    from kinpoly_amd.model_compiler import read_kpm
    from kinpoly_amd import sim as kpsim
    fk_sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), n, 0)
    return D.synthetic_takes(fk_sim, STD["qpos"], n_per_action=1, T_range=(fr + 4, fr + 14), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"], seed=seed), fk_sim


@pytest.mark.parametrize("name", ["kin_poly_use_vel", "kin_poly_no_head"])
def test_agent_from_a_variant_yml_end_to_end(kp, tmp_path, name):
    """AgentAR from Config.agent_kwargs() of the yml (its networks are the file's fixed sizes; one PPO epoch and one supervised step per iteration keep the test
    short): two iterations, a checkpoint round trip, eval_policy over the takes, and the first env.step against a 105-d env given the same actions."""
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd import dataset as D
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.config import Config
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.env import BatchedHumanoidAREnv
    cfg = Config(os.path.join(GOLDEN, name + ".yml"), base_dir=str(tmp_path / "results"))
    kw = cfg.agent_kwargs()
    s = (kw["use_vel"], kw["use_head"], kw["use_action"])
    assert s == dict(kin_poly_use_vel=(True, True, True), kin_poly_no_head=(False, False, True))[name]
    n, fr, H = 16, 12, 6
    takes, fk_sim = _takes(n, fr)
    ds = D.StateARDataset(takes, fr_num=fr, seed=3, device=fk_sim.device)
    agent = AgentAR(n, dataset=ds, device=0, horizon=H, result_dir=str(tmp_path), eval_envs=3, **{**kw, "num_optim_epoch": 1, "num_step_update": 1})
    cfg.apply_reward_weights(agent.env)
    D_ = V.width(*s)
    assert agent.env.obs_dim == D_ == agent.kin_sim.obs_ar_dim == agent.policy_net.state_dim and agent.policy_net.context_dim == 13 * s[1] + 4 * s[2]
    assert (agent.env.use_vel, agent.env.use_head, agent.env.use_action) == s and agent.value_net.net.affine_layers[0].weight.shape[1] == D_
    for it in range(2):
        info = agent.optimize_policy(it)
        assert info["num_steps"] == n * H
        for k in ("surr_loss", "value_loss", "step_loss"):
            assert np.isfinite(info[k]), (it, k, info[k])
    batch = agent.sampler.sample(H)
    assert tuple(batch.states.shape) == (n, H, D_) and torch.isfinite(batch.states).all() and torch.isfinite(batch.rewards).all()
    path = str(tmp_path / "iter_0002.p")
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
    with pytest.raises(ck.CheckpointWidthError, match=f"{D_}-d.*105-d"):           # the checkpoint under a default-width network
        ck.load_state_strict(TrajARNet(), ck.split_policy_dict(ck.load_checkpoint(path)["policy_dict"]), what=path)
    res = agent.eval_policy("train")                                                # the takes, whole, through evaluate.run_sequences
    cov = res[0]["coverage_train"]
    assert cov["all_coverage"] == ds.get_len() and 0 <= cov["num_coverage"] <= cov["all_coverage"]
    # the observation variant does not touch the physics: the first step of an episode against a 105-d env on the same clips with the same actions
    data = ds.batch(np.arange(n) % ds.get_len(), None, fr)
    ctx = agent.ctx_builder.init_context({k: (v.to(agent.device) if torch.is_tensor(v) else v) for k, v in data.items()}, need_rollout=False)
    envs = []
    for kws in (dict(use_vel=s[0], use_head=s[1], use_action=s[2]), {}):
        torch.manual_seed(11)                                                       # the same randomly initialised UHC in both
        env = BatchedHumanoidAREnv(n, 0, mode="train", seed=5, **kws)
        cfg.apply_reward_weights(env)
        env.load_context(ctx)
        env.reset()
        envs.append(env)
    assert (envs[0].obs_dim, envs[1].obs_dim) == (D_, 105)
    act = torch.randn((n, 80), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 0.05
    outs = []
    for env in envs:
        o, r, done, info = env.step(act.clone())
        outs.append((env.sim.get("qpos").clone(), env.sim.get("qvel").clone(), r.clone(), done.clone(), o.clone()))
    for a, b in list(zip(outs[0], outs[1]))[:4]:
        assert torch.equal(a, b)
    assert tuple(outs[0][4].shape) == (n, D_) and torch.equal(outs[0][4][:, :74], outs[1][4][:, :74])


def test_twin_rollout_observation_is_the_differentiable_one_with_use_vel(kp, tmp_path):
    """TrajARNet.rollout on the kinematic twin against pretrain's torch roll-out, use_vel on.  The twin's observation at frame t -- set_state(Q[t], V[t]) with the
    V[t] kp_kin_advance wrote, then obs_ar -- is compared with pretrain.observe on the same pose and the finite-difference velocity get_qvel_fd_batch(Q[t - 1],
    Q[t]) (frame 0: the context network's init_qvel), block by block, so nothing passes through the network between the two.

    Bounds, both sides fp32: the velocity block is 2 x what test_step_kin_and_kin_advance_sweep holds kp_kin_advance to against fp64 on random rows (1e-4 linear and
    joint, 3e-5 angular), the torch finite difference being the same formula in the same format; every other column 2 x (5e-6 + 5e-6), test_obs_ar_sweep's bound
    on the row's arithmetic plus test_target_fk_sweep's on the forward kinematics it reads (the two sides run their own).  The whole roll-outs, which feed the
    observation back through the network, are held to tests/test_gpu_driver.py's bounds on the 105-d pair (2e-4 pose, 5e-4 action, 2e-2 velocity)."""
    from kinpoly_amd import dataset as D
    from kinpoly_amd import pretrain as P
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.config import Config
    from kinpoly_amd.context import get_qvel_fd_batch
    kw = Config(os.path.join(GOLDEN, "kin_poly_use_vel.yml"), base_dir=str(tmp_path / "results")).agent_kwargs()
    n, fr, dt = 8, 12, 1.0 / 30.0
    takes, fk_sim = _takes(n, fr)
    ds = D.StateARDataset(takes, fr_num=fr, seed=3, device=fk_sim.device)
    agent = AgentAR(n, dataset=ds, device=0, horizon=4, result_dir=str(tmp_path), **kw)
    net, twin = agent.policy_net, agent.kin_sim
    assert net.use_vel and twin.obs_ar_vel and twin.obs_ar_dim == net.state_dim == 180
    data = next(P.sampling_batches(ds, n, n, agent.device))
    seen = []
    obs_ar = twin.obs_ar
    twin.obs_ar = lambda ctx, *a, **k: (seen.append(obs_ar(ctx, *a, **k).clone()), seen[-1])[1]         # the rows the roll-out hands to the network
    try:
        with torch.no_grad():
            pred = P.forward_supervised(net, agent.fk, data)
            iq, iv, _ = net.init_states(data, keep_feat=False)
            Q, Vfix, A = net.rollout(data, twin, iq.contiguous(), iv.contiguous())
    finally:
        del twin.obs_ar
    assert len(seen) == fr and tuple(seen[0].shape) == (n, 180)
    tot = {"vel lin": 0.0, "vel ang": 0.0, "rest": 0.0}
    with torch.no_grad():
        for t in range(fr):
            qv = iv if t == 0 else get_qvel_fd_batch(Q[:, t - 1], Q[:, t], dt)
            if t > 0:
                assert torch.equal(seen[t][:, 74:149], Vfix[:, t - 1])            # the twin's qvel is what kp_kin_advance left (fix_qvel moves it one frame back)
            want, _, _ = P.observe(agent.fk, Q[:, t].contiguous(), data, t, use_vel=True, qvel=qv)
            d = (seen[t] - want).abs()
            tot["vel ang"] = max(tot["vel ang"], float(d[:, 77:80].max()))
            tot["vel lin"] = max(tot["vel lin"], float(d[:, 74:77].max()), float(d[:, 80:149].max()))
            tot["rest"] = max(tot["rest"], float(d[:, :74].max()), float(d[:, 149:].max()))
    whole = {k: float((pred[k] - x).abs().max()) for k, x in (("qpos", Q), ("action", A), ("qvel", Vfix))}
    print("MEASURED twin vs differentiable observation, use_vel:", tot, "whole roll-out:", whole)
    assert tot["vel lin"] < 2e-4 and tot["vel ang"] < 6e-5 and tot["rest"] < 2e-5            # measured 2.4e-07, 3.8e-06, 7.2e-07
    assert whole["qpos"] < 2e-4 and whole["action"] < 5e-4 and whole["qvel"] < 2e-2          # measured 2.4e-07, 3.0e-08, 7.4e-06
