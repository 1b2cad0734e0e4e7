"""GPU: dynamic_supervision_v2 in the kinematic-policy env's step tail (kp_sim_term_reward_v2 and the fused kp_sim_post_step_v2) against the fp64
restatement of tests/reward_oracle.py, which tests/test_reward_variants_cpu.py holds to the reference's own function.

The rule of tests/test_gpu_uhc_rewards.py, for the reward and the five info columns, relative to max(1, |value|): kernel error <= max(2 x the error of
an fp32 torch evaluation on the same inputs, 1e-6) (reward_oracle.dynamic_supervision_v2_t: the package has no torch path of this reward).
n in {1, 9, 33}: 8 envs per block, so 9 and 33 leave partial blocks; T = 3 context frames; cur_t from 0 (clamped up to 1) to 3 (clamped down to T - 1).
Termination, end / done / percent and the obj7 write-back equal dynamic_supervision_v1's on the same states bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import reward_oracle as R  # noqa: E402
import side_oracle as S  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm  # noqa: E402
from oracle import np_oracle as O  # noqa: E402

KPM = read_kpm(DEFAULT_KPM)
BODY_POS, BODY_IPOS, PARENT = KPM["body_pos"].reshape(24, 3), KPM["body_ipos"].reshape(24, 3), KPM["body_parent"]
STD = np.load(os.path.join(R.GOLD, "standing_neutral.npz"))
T = 3
CUSTOM = dict(w_hp=0.15, w_hq=0.15, w_p=0.3, w_v=0.1, w_e=0.3, k_hp=45.0, k_hq=45.0, k_p=1.0, k_v=0.01, k_e=5.0)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda").contiguous()


def _steps(rng, shape):
    """joint steps of 0.01 .. 0.04 rad either way: every body turns by far more between two frames than the 2.8e-3 rad below which kin_poly's
    rotation_from_quaternion returns zero, so no row sits on that switch"""
    return rng.uniform(0.01, 0.04, shape) * rng.choice([-1.0, 1.0], shape)


def _case(sim, n, seed):
    """the state after a control step and its context rows; every third env has not moved since the previous frame (angular velocity exactly 0), env 1
    (mod 4) has the root quaternion of the opposite sign, env 4 (mod 5) is far from target and ground truth (it fails)"""
    rng = np.random.default_rng(seed)
    q0 = f32(S.random_qpos(n, seed, STD["qpos"])).astype(np.float64)
    q1 = q0.copy()
    moved = np.arange(n) % 3 != 0
    q1[:, 7:] += _steps(rng, (n, 69)) * moved[:, None]
    for e in np.flatnonzero(moved):
        q1[e, 3:7] = O.quaternion_multiply(O.quat_from_expmap(_steps(rng, 3)), q0[e, 3:7])
    q1[np.arange(n) % 4 == 1, 3:7] *= -1.0
    q1 = f32(q1).astype(np.float64)
    gq = np.zeros((n, T, 76))
    for e in range(n):
        step = np.concatenate([[0.01, 0.004, 0.001], np.zeros(4), _steps(rng, 69)])
        for t in range(T):
            gq[e, t] = q1[e] + (t - 1) * step + np.concatenate([np.zeros(7), rng.normal(size=69) * 0.03])
            gq[e, t, 3:7] = O.quaternion_multiply(O.quat_from_expmap(np.array([0.02, -0.01, 0.03 * t])), q0[e, 3:7])      # the sign of q0: opposite to q1's where e % 4 == 1
    gfk = [[O.qpos_fk(gq[e, t], BODY_POS, BODY_IPOS, PARENT) for t in range(T)] for e in range(n)]
    gt_bquat = f32([[O.get_body_quat(gq[e, t]) for t in range(T)] for e in range(n)])
    gt_wbpos = f32([[gfk[e][t]["wbpos"].reshape(-1) for t in range(T)] for e in range(n)])
    fk1 = [O.qpos_fk(q1[e], BODY_POS, BODY_IPOS, PARENT) for e in range(n)]
    xpos = np.stack([f["wbpos"].reshape(-1) for f in fk1]) + rng.normal(size=(n, 72)) * 0.02
    xpos[np.arange(n) % 5 == 4] += 2.0
    xquat = np.stack([f["wbquat"].reshape(-1) for f in fk1])
    head_pose = np.zeros((n, T, 7))
    for e in range(n):
        head_pose[e, :, :3] = xpos[e, 39:42] + rng.normal(size=(T, 3)) * 0.05
        head_pose[e, :, 3:] = O.quaternion_multiply(O.quat_from_expmap(rng.normal(size=3) * 0.1), xquat[e, 52:56])
    view = lambda k, v: sim.view(k).copy_(torch.from_numpy(f32(v)))      # noqa: E731  (the stored fields as given: the kernel reads whatever is stored)
    view("qpos", q0); view("xpos", np.zeros((n, 72))); view("xquat", np.tile([1.0, 0, 0, 0], (n, 24)))
    sim.step_begin()                                                       # prev_bquat = get_body_quat(q0)
    tq = q1.copy(); tq[:, 7:] += rng.normal(size=(n, 69)) * 0.05
    sim.set_target(dev(tq))
    view("qpos", q1); view("xpos", xpos); view("xquat", xquat)
    simobj = f32(rng.normal(size=(n, 35)))
    view("obj_qpos", simobj)
    one_hot = np.zeros((n, 4), np.float32); one_hot[np.arange(n) % 2 == 0, np.arange(n)[np.arange(n) % 2 == 0] % 4] = 1.0
    cur_t = (np.arange(n) % 4).astype(np.int32)                            # 0 clamps up to 1, 3 clamps down to T - 1 = 2
    ctx = dict(head_pose=f32(head_pose), head_vels=np.zeros((n, T, 6), np.float32), obj_rel=np.zeros((n, T, 7), np.float32), action_one_hot=one_hot,
               gt_bquat=gt_bquat, gt_wbpos=gt_wbpos, cur_t=cur_t)
    state = dict(qpos=f32(q1), xpos=f32(xpos), xquat=f32(xquat), prev_bquat=sim.get("prev_bquat").cpu().numpy(), simobj=simobj)
    return state, ctx


def _make_ctx(sim, c, cur_t):
    keep = {k: dev(c[k]) for k in ("head_pose", "head_vels", "obj_rel", "action_one_hot", "gt_bquat", "gt_wbpos")}
    keep["cur_t"] = dev(cur_t, torch.int32)
    return sim.make_ctx(T, keep["head_pose"], keep["head_vels"], keep["obj_rel"], keep["action_one_hot"], keep["gt_bquat"], keep["gt_wbpos"], keep["cur_t"]), keep


def _cfg_v2(kp, b_diffw, ws):
    cfg = kp.KpRewardCfgV2.default(b_diffw)
    for k, v in ws.items():
        setattr(cfg, k, float(v))
    return cfg


def _outs(n):
    z = lambda *s, dt=torch.float32: torch.full(s, -3, dtype=dt, device="cuda")      # noqa: E731
    return dict(reward=z(n), info=z(n, 6), fail=z(n, dt=torch.uint8), diffs=z(n, 2), done=z(n, dt=torch.uint8), end=z(n, dt=torch.uint8), percent=z(n))


@pytest.mark.parametrize("n", [1, 9, 33])
@pytest.mark.parametrize("weights", ["default", "custom"])
def test_both_forms_against_fp64_and_v1_termination(n, weights):
    from kinpoly_amd import sim as kp
    sim = kp.KpSim(kp.KpModel(), n)
    state, c = _case(sim, n, 900 + n)
    ws = {k: float(v) for k, v in {**R.DEFAULTS["dynamic_supervision_v2"], **(CUSTOM if weights == "custom" else {})}.items()}
    b_diffw = dev(KPM["uhc_b_diffw"])
    cfg2, cfg1 = _cfg_v2(kp, b_diffw, ws), kp.KpRewardCfg.default()
    dt = float(np.float32(1.0 / 30.0))                                     # kp_reward_cfg_v2.dt is a float
    # ---- the plain form
    ctx, keep = _make_ctx(sim, c, c["cur_t"])
    r2, i2, f2, d2 = (x.clone() for x in sim.term_reward(ctx, cfg2))
    r1, i1, f1, d1 = (x.clone() for x in sim.term_reward(ctx, cfg1))
    assert torch.equal(f1, f2) and torch.equal(d1, d2)                      # calc_body_diff / calc_body_gt_diff: v1's, bit for bit
    assert n < 5 or (bool(f2.any()) and not bool(f2.all()))
    assert torch.all(i2[:, 5] == 0)                                        # the row stays 6 wide, v2 fills 5
    tcl = np.clip(c["cur_t"], 1, T - 1)
    ar = np.arange(n)
    want = [R.dynamic_supervision_v2(state["qpos"][e].astype(np.float64), state["xpos"][e].astype(np.float64).reshape(24, 3),
                                     state["xquat"][e].astype(np.float64).reshape(24, 4), state["prev_bquat"][e].astype(np.float64),
                                     c["head_pose"][e, tcl[e]].astype(np.float64), c["gt_bquat"][e, tcl[e]].astype(np.float64),
                                     c["gt_bquat"][e, tcl[e] - 1].astype(np.float64), c["gt_wbpos"][e, tcl[e]].astype(np.float64), ws,
                                     KPM["uhc_b_diffw"][1:].astype(np.float64), dt) for e in range(n)]
    want_r, want_i = np.array([w[0] for w in want]), np.stack([w[1] for w in want])
    bquat = sim.fk(dev(state["qpos"]))["bquat"].clone()
    bquat[:, :4] = dev(state["qpos"])[:, 3:7]                              # get_body_quat() starts from the raw root quaternion
    tr, ti = R.dynamic_supervision_v2_t(bquat, dev(state["xpos"]), dev(state["xquat"]), dev(state["prev_bquat"]), dev(c["head_pose"][ar, tcl]),
                                        dev(c["gt_bquat"][ar, tcl]), dev(c["gt_bquat"][ar, tcl - 1]), dev(c["gt_wbpos"][ar, tcl]), ws, b_diffw, dt)
    cols = [("reward", r2, tr, want_r)] + [(f"info[{k}]", i2[:, k], ti[:, k], want_i[:, k]) for k in range(5)]
    bad = []
    for name, k, t, w in cols:
        ek, et = R.rel_err(k.double().cpu().numpy(), w), R.rel_err(t.double().cpu().numpy(), w)
        print(f"dynamic_supervision_v2 {weights} n={n} {name}: kernel {ek:.3e}  torch fp32 {et:.3e}")
        if not ek <= max(2 * et, 1e-6):
            bad.append((name, ek, et))
    assert not bad, bad
    # ---- the fused tail, one frame earlier: the same reward, and v1's end / done / percent / cur_t / obj7 / done_count
    rng = np.random.default_rng(n)
    row_len = dev(rng.integers(2, 6, n), torch.int32)                       # below and above episode_len = 3
    obj7_0 = f32(rng.normal(size=(n, 7)))
    post = {}
    for name, cfg in (("v1", cfg1), ("v2", cfg2)):
        ctx, keep = _make_ctx(sim, c, c["cur_t"] - 1)
        o = _outs(n)
        cnt, obj7 = torch.full((1,), 3, dtype=torch.int32, device="cuda"), dev(obj7_0)
        sim.post_step(ctx, cfg, keep["cur_t"], row_len, 3, o["reward"], o["info"], o["fail"], o["diffs"], o["done"], o["end"], o["percent"], cnt, obj7)
        post[name] = dict(o, cur_t=keep["cur_t"], cnt=cnt, obj7=obj7)
    assert torch.equal(post["v2"]["reward"], r2) and torch.equal(post["v2"]["info"], i2)
    assert torch.equal(post["v1"]["reward"], r1) and torch.equal(post["v1"]["info"], i1)
    for k in ("fail", "diffs", "done", "end", "percent", "cur_t", "cnt", "obj7"):
        assert torch.equal(post["v1"][k], post["v2"][k]), k
    assert torch.equal(post["v2"]["cur_t"].cpu(), torch.as_tensor(c["cur_t"]))
    hot = c["action_one_hot"].any(1)
    assert np.array_equal(post["v2"]["obj7"].cpu().numpy()[~hot], obj7_0[~hot]) and (n < 2 or not np.array_equal(post["v2"]["obj7"].cpu().numpy()[hot], obj7_0[hot]))


def test_refusals():
    from kinpoly_amd import sim as kp
    sim = kp.KpSim(kp.KpModel(), 2)
    state, c = _case(sim, 2, 5)
    ctx, keep = _make_ctx(sim, c, c["cur_t"])
    cfg = kp.KpRewardCfgV2.default(dev(KPM["uhc_b_diffw"]))
    cfg.b_diffw = None
    with pytest.raises(kp.KinPolyNativeError, match="kp_sim_term_reward_v2"):
        sim.term_reward(ctx, cfg)
    o = _outs(2)
    with pytest.raises(kp.KinPolyNativeError, match="kp_sim_post_step_v2"):
        sim.post_step(ctx, cfg, keep["cur_t"], dev([3, 3], torch.int32), 3, o["reward"], o["info"], o["fail"], o["diffs"], o["done"], o["end"], o["percent"])
    assert torch.all(o["reward"] == -3)                                    # nothing was launched


def test_agent_from_the_v2_file(tmp_path):
    """AgentAR from kin_poly_reward_v2.yml: 32 envs, one sample() and one update; the rewards the sampler records are the ones the kernel wrote"""
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.config import Config
    from kinpoly_amd.env import standing_context
    n, H = 32, 6
    cfg = Config(os.path.join(R.GOLD, "kin_poly_reward_v2.yml"), base_dir=str(tmp_path / "results"))
    fk_sim = kpsim.KpSim(kpsim.KpModel(), n, 0)

    def context_fn(m):
        return standing_context(m, H + 2, STD["qpos"], STD["qvel"], fk_sim, torch.zeros(m))
    torch.manual_seed(0)
    kw = {**cfg.agent_kwargs(), "num_optim_epoch": 1, "num_step_update": 1, "num_sample": 16, "batch_size": 8, "num_init_update": 1}
    agent = AgentAR(n, context_fn, device=0, horizon=H, use_init_context=False, **kw)
    rc = cfg.apply_reward_weights(agent.env)
    assert agent.env.reward_id == "dynamic_supervision_v2" and isinstance(rc, kpsim.KpRewardCfgV2) and rc.w_p == 0.5 and rc.k_e == 10.0 and abs(rc.k_v - 0.005) < 1e-9
    seen, plain_step = [], agent.env.step

    def step(*a, **k):
        out = plain_step(*a, **k)
        seen.append((out[3]["custom_reward"].clone(), out[3]["custom_info"].clone()))
        return out
    agent.env.step = step
    batch = agent.sampler.sample(H)
    assert len(seen) == H
    kernel = torch.stack([r for r, _ in seen], 1)
    assert bool(torch.isfinite(batch.rewards).all()) and torch.equal(batch.rewards, kernel)
    info = torch.stack([i for _, i in seen], 1)
    assert info.shape == (n, H, 6) and torch.all(info[..., 5] == 0) and float(info[..., :5].min()) > 0 and float(info.max()) <= 1
    want = 1.0 * info[..., 0] + 1.0 * info[..., 1] + 0.5 * info[..., 2] + 0.1 * info[..., 3] + 0.2 * info[..., 4]      # the file's w_p, the function's other defaults
    assert float((kernel - want).abs().max()) < 1e-5
    before = torch.cat([p.detach().reshape(-1) for p in agent.policy_net.parameters()]).clone()
    agent.update_params(batch)
    after = torch.cat([p.detach().reshape(-1) for p in agent.policy_net.parameters()])
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    # an evaluation engine takes over the training env's reward (AgentAR._eval_engine: copy_reward), with its own mode's use_gt_term
    from kinpoly_amd.env import BatchedHumanoidAREnv
    ev = BatchedHumanoidAREnv(2, 0, mode="test", cc_policy=agent.env.cc_policy, cc_running_state=agent.env.cc_running_state)
    ev.copy_reward(agent.env)
    assert ev.reward_id == "dynamic_supervision_v2" and ev.reward_cfg.w_p == 0.5 and ev.reward_cfg.use_gt_term == 0 and agent.env.reward_cfg.use_gt_term == 1
