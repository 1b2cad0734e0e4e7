"""GPU: the kinematic policy under `use_context` / `use_of` through the physics -- the ring refill kernel (kp_ctx_rows_write, kinpoly_amd/csrc/kp_obs_ctx.hip),
the env's wide observation, the sampler's ring with the two wide tables, the update on recorded wide states, and the two scripts from
tests/golden/kin_poly_of.yml.

Copies are held to bit equality (the refill against the torch composition it replaces, the wide blocks against the tables' words, the base block against
kp_sim_obs_ar on the same handle).  Against the reference's rows (tests/golden/policy_ctx.npz) the observation is held to 5e-6 absolute, the bound
tests/test_gpu_context_obs.py::test_fixture_rows holds k_obs_ar_ctx to; the fused re-unroll to tests/test_gpu_round2.py's 2e-5.  Every figure is
printed before it is asserted."""
import ctypes as C
import os
import runpy
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_side_kernels as K  # noqa: E402  (load(): rows straight into a handle's stored fields; nothing of it is collected from here)
import test_policy_ctx_cpu as PC  # noqa: E402  (the fixture's cases; its tests are not collected from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STD = np.load(os.path.join(GOLDEN, "standing_neutral.npz"))
GUARD = 64
dev = K.dev


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    yield kpsim
    K._SIMS.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 1. kp_ctx_rows_write
def _guarded_table(R, T, W, seed):
    """a seeded [R, T, W] table in the middle of a buffer with GUARD sentinel words on either side"""
    buf = torch.full((GUARD + R * T * W + GUARD,), -7.0, device="cuda")
    tab = buf[GUARD:GUARD + R * T * W].view(R, T, W)
    tab.copy_(torch.randn((R, T, W), generator=torch.Generator().manual_seed(seed)))
    return buf, tab


def _guards_intact(buf, numel):
    return bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + numel:] == -7.0).all())


def _composition(rows, seq, of, ctx_table, of_table):
    """what the kernel replaces: transpose, last-frame pad, index_copy_ (BatchedHumanoidAREnv.write_context_rows.fit)"""
    def fit(v, T):
        return v if v.shape[1] == T else torch.cat([v, v[:, -1:].expand(-1, T - v.shape[1], -1)], 1)
    if ctx_table is not None:
        ctx_table.index_copy_(0, rows, fit(seq.transpose(0, 1), ctx_table.shape[1]))
    if of_table is not None:
        of_table.index_copy_(0, rows, fit(of, of_table.shape[1]))


def _sources(m, Tp, H, F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((Tp, m, H), generator=g).cuda(), torch.randn((m, Tp, F), generator=g).cuda()


@pytest.mark.parametrize("R,T,H,F,rows,Tp", [(16, 6, 16, 12, (0, 3, 7, 12, 15), 4), (16, 6, 16, 12, (15, 0, 9, 2, 4), 6), (16, 6, 33, 1, (5,), 1),
                                             (80, 4, 256, 512, None, 3)], ids=["short_clips", "full_clips", "one_frame_odd_widths", "m65_H256_F512"])
def test_ctx_rows_write_is_the_composition_it_replaces(kp, R, T, H, F, rows, Tp):
    if rows is None:                                     # 65 clips (more than a workgroup's threads / 4), scattered, the last row among them
        rows = [R - 1] + [int(x) for x in np.random.default_rng(1).permutation(R - 1)[:64]]
    m = len(rows)
    rows_t = torch.tensor(rows, device="cuda")
    seq, of = _sources(m, Tp, H, F, 7)
    for which in ("both", "ctx", "of"):                  # each table absent in turn
        bc, ct = _guarded_table(R, T, H, 11)
        bo, ot = _guarded_table(R, T, F, 12)
        want_c, want_o = ct.clone(), ot.clone()
        use_c, use_o = which != "of", which != "ctx"
        _composition(rows_t, seq, of, want_c if use_c else None, want_o if use_o else None)
        kp.ctx_rows_write(rows_t if which != "ctx" else list(rows), seq if use_c else None, of if use_o else None, ct if use_c else None, ot if use_o else None)
        torch.cuda.synchronize()
        same_c, same_o = torch.equal(ct.view(torch.int32), want_c.view(torch.int32)), torch.equal(ot.view(torch.int32), want_o.view(torch.int32))
        print(f"MEASURED ctx_rows_write R={R} T={T} H={H} F={F} m={m} T'={Tp} tables={which}: ctx words equal {same_c}, of words equal {same_o}")
        assert same_c and same_o                         # named rows = the composition's words; every other row (and an absent table) unchanged
        assert _guards_intact(bc, R * T * H) and _guards_intact(bo, R * T * F)


def test_ctx_rows_write_refusals_leave_the_tables_alone(kp):
    R, T, H, F, m = 16, 6, 16, 12, 5
    L = kp.load_library()
    bc, ct = _guarded_table(R, T, H, 21)
    bo, ot = _guarded_table(R, T, F, 22)
    keep_c, keep_o = ct.clone(), ot.clone()
    seq, of = _sources(m, 4, H, F, 3)
    good = torch.tensor([0, 3, 7, 12, 15], device="cuda")
    # m = 0: nothing to do, nothing launched
    kp.ctx_rows_write(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros((4, 0, H), device="cuda"), torch.zeros((0, 4, F), device="cuda"), ct, ot)
    for bad in ([0, 3, 7, 12, R], [0, -1, 7, 12, 15]):                        # a row outside [0, R)
        for rows in (torch.tensor(bad, device="cuda"), bad):
            with pytest.raises(kp.KinPolyNativeError, match="outside"):
                kp.ctx_rows_write(rows, seq, of, ct, ot)
    long_seq, long_of = _sources(m, T + 1, H, F, 4)                           # T' > T
    with pytest.raises(kp.KinPolyNativeError, match="do not fit"):
        kp.ctx_rows_write(good, long_seq, long_of, ct, ot)
    with pytest.raises(kp.KinPolyNativeError, match="do not fit"):            # T' < 1
        kp.ctx_rows_write(good, torch.zeros((0, m, H), device="cuda"), torch.zeros((m, 0, F), device="cuda"), ct, ot)
    for kw in (dict(seq=seq.cpu()), dict(of=of.cpu()), dict(ctx_table=ct.cpu()), dict(seq=seq[:, :, :8].contiguous()), dict(of=of.double())):      # host tensors, other shapes / dtypes
        with pytest.raises(ValueError):
            kp.ctx_rows_write(good, **{**dict(seq=seq, of=of, ctx_table=ct, of_table=ot), **kw})
    with pytest.raises(ValueError, match="rows"):
        kp.ctx_rows_write(good[:3], seq, of, ct, ot)
    # the C entry point itself: a null table with a non-zero width, host pointers, a table without its source
    host_rows = good.cpu()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    host_seq = seq.cpu()
    for args, word in (((p(good), p(host_rows), p(seq), p(of), None, p(ot)), "null context table"), ((p(good), p(host_rows), p(seq), p(of), p(ct), None), "null `of` table"),
                       ((p(good), p(host_rows), p(host_seq), p(of), p(ct), p(ot)), "device memory"), ((p(host_rows), p(host_rows), p(seq), p(of), p(ct), p(ot)), "device memory"),
                       ((p(good), p(host_rows), None, p(of), p(ct), p(ot)), "without its source"), ((p(good), None, p(seq), p(of), p(ct), p(ot)), "null rows")):
        assert L.kp_ctx_rows_write(m, R, T, 4, H, F, *args, None) == -1
        assert word in L.kp_last_error().decode(), L.kp_last_error().decode()
    assert L.kp_ctx_rows_write(0, R, T, 4, H, F, None, None, None, None, p(ct), p(ot), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ct, keep_c) and torch.equal(ot, keep_o) and _guards_intact(bc, R * T * H) and _guards_intact(bo, R * T * F)


# ------------------------------------------------------------------ 2. the env's observation against the reference's rows
def _fixture_env(g, H, F):
    """an env whose stored state, context row and frame are fixture (a)'s 12 states (derived arrays one substep stale, as the reference read them)"""
    from kinpoly_amd.env import BatchedHumanoidAREnv
    n, T = g["env_head_pose"].shape[:2]
    env = BatchedHumanoidAREnv(n, 0, mode="train", seed=0, ctx_dim=H, of_dim=F)
    obj_pose = np.zeros((n, T, 14))
    obj_pose[:, :, :7] = g["env_obj7"][:, None]
    ctx = dict(qpos=dev(np.tile(STD["qpos"], (n, T, 1))), head_pose=dev(g["env_head_pose"]), head_vels=dev(g["env_head_vels"]), obj_head_relative_poses=dev(g["env_obj_rel"]),
               action_one_hot=dev(g["env_action_one_hot"]), init_qpos=dev(g["env_qpos"]), init_qvel=dev(g["env_qvel"]), obj_pose=dev(obj_pose),
               context_feat_rnn=dev(g["env_ctx_feat"]), of=dev(g["env_of"]))
    if not F:
        del ctx["of"]
    env.load_context(ctx)
    K.load(env.sim, qpos=g["env_qpos"], qvel=g["env_qvel"], xpos=g["env_xpos"].reshape(n, 72), xquat=g["env_xquat"].reshape(n, 96))
    env.obj7.copy_(dev(g["env_obj7"]))
    env.cur_t.copy_(torch.tensor(g["env_t"].astype(np.int32), device="cuda"))
    return env


@pytest.mark.parametrize("case", PC.CASES, ids=PC.IDS)
def test_env_observation_matches_reference_rows(kp, golden, case):
    g = golden("policy_ctx")
    H, F = PC.H, PC.F * case[1]
    env = _fixture_env(g, H, F)
    assert env.obs_dim == H + 105 + F == g["env_obs_" + PC.IDS[PC.CASES.index(case)]].shape[1]
    assert min(g["env_t"]) == 0 and max(g["env_t"]) == g["env_head_pose"].shape[1] - 1 and 0 < g["env_action_one_hot"].sum() < len(g["env_t"])
    obs = env._obs_ar(env._obs).clone()
    base = env.sim.obs_ar(env._ctx_struct)
    want = g["env_obs_" + PC.IDS[PC.CASES.index(case)]]
    err = np.abs(obs.double().cpu().numpy() - want)
    print(f"MEASURED env observation {PC.IDS[PC.CASES.index(case)]}: max |error| {err.max():.3e} (context block {err[:, :H].max():.3e}, base {err[:, H:H + 105].max():.3e}"
          + (f", of {err[:, H + 105:].max():.3e})" if F else ")"))
    assert err.max() <= 5e-6
    ar, t = torch.arange(env.n, device="cuda"), env.cur_t.long()
    assert torch.equal(obs[:, H:H + 105], base)                                          # kp_sim_obs_ar's row on the same states
    assert torch.equal(obs[:, :H], env.ctx["context_feat_rnn"][ar, t])                   # the tables' fp32 words
    if F:
        assert torch.equal(obs[:, H + 105:], env.ctx["of"][ar, t])


# ------------------------------------------------------------------ 3. rows and frames
def _standing_rows(env, R, T, H, F, seed=5):
    from kinpoly_amd.env import standing_context
    g = torch.Generator().manual_seed(seed)
    ctx = standing_context(R, T, STD["qpos"], STD["qvel"], env.sim, (torch.rand(R, generator=g) * 2 - 1) * np.pi)
    if H:
        ctx["context_feat_rnn"] = torch.randn((R, T, H), generator=g).cuda()
    if F:
        ctx["of"] = torch.randn((R, T, F), generator=g).cuda()
    return ctx


def test_wide_blocks_follow_the_env_row_and_frame(kp):
    from kinpoly_amd.env import BatchedHumanoidAREnv
    n, R, T, H, F = 5, 15, 6, 33, 12
    torch.manual_seed(2)
    env = BatchedHumanoidAREnv(n, 0, mode="train", seed=2, ctx_dim=H, of_dim=F)
    ctx = _standing_rows(env, R, T, H, F)
    env.load_context(ctx)
    assert torch.equal(env.ctx["context_feat_rnn"], ctx["context_feat_rnn"]) and torch.equal(env.ctx["of"], ctx["of"])      # whole clips: the refill kernel's copy
    rows = torch.tensor([13, 2, 14, 7, 0], dtype=torch.int32, device="cuda")
    env.set_rows(rows)
    r = rows.long()

    def blocks_are(obs, t):
        return torch.equal(obs[:, :H], ctx["context_feat_rnn"][r, t]) and torch.equal(obs[:, H + 105:], ctx["of"][r, t])
    obs = env.reset().clone()
    assert tuple(obs.shape) == (n, H + 105 + F) and blocks_are(obs, torch.zeros(n, dtype=torch.long, device="cuda"))
    frames = torch.tensor([0, T - 1, 2, 3, T - 2], dtype=torch.int32, device="cuda")
    env.cur_t.copy_(frames)
    assert blocks_are(env._obs_ar(env._obs).clone(), frames.long())
    cur, base = env.sim.get("qpos"), env._obs[:, H:H + 105]
    act = torch.zeros((n, 80), device="cuda")
    act[:, :74] = torch.cat([cur[:, 2:3], base[:, 1:5], cur[:, 7:]], 1)                    # the kinematic action that keeps the current pose
    obs, _, done, _ = env.step(act)
    inside = frames < T - 1
    assert torch.equal(env.cur_t[inside], frames[inside] + 1) and bool((env.cur_t[~inside] >= T - 1).all())      # the step moves the frame on ...
    assert blocks_are(obs, env.cur_t.long().clamp(max=T - 1))                              # ... and a frame past the clip reads its last one
    assert torch.equal(obs[:, H:H + 105], env.sim.obs_ar(env._ctx_struct))
    # without the two blocks: today's observation, from today's call
    torch.manual_seed(2)
    plain = BatchedHumanoidAREnv(n, 0, mode="train", seed=2)
    assert (plain.obs_dim, plain.ctx_dim, plain.of_dim, plain._ext) == (105, 0, 0, None)
    plain.load_context({k: v for k, v in ctx.items() if k not in ("context_feat_rnn", "of")})
    assert "context_feat_rnn" not in plain.ctx and "of" not in plain.ctx
    plain.set_rows(rows)
    o = plain.reset().clone()
    assert torch.equal(o, plain.sim.obs_ar(plain._ctx_struct)) and torch.equal(o, env.reset()[:, H:H + 105])


# ------------------------------------------------------------------ 4. the sampler's ring
def _six_takes(n, fr, F, seed=3):
    from kinpoly_amd import dataset as D
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.model_compiler import read_kpm
    fk_sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), n, 0)
    kw = dict(n_per_action=1, T_range=(fr + 4, fr + 12), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"])
    takes = D.synthetic_takes(fk_sim, STD["qpos"], seed=seed, **kw)
    free = D.synthetic_takes(fk_sim, STD["qpos"], seed=seed + 1, with_objects=False, **kw)
    takes.update({k: free[k] for k in sorted(free)[:2]})
    assert len(takes) == 6
    ds = D.StateARDataset(takes, fr_num=fr, seed=seed, device=fk_sim.device, of_features=D.synthetic_of_features(takes, F, seed=seed))
    return ds, takes, fk_sim


def test_sampler_records_the_drawn_clips_context_and_of(kp):
    from kinpoly_amd.context import PolicyARContext, TrajARNet
    from kinpoly_amd.env import BatchedHumanoidAREnv
    from kinpoly_amd.rollout import EpisodeSource, VectorSampler
    n, fr, T, H, F = 5, 5, 12, 32, 12
    ds, _, fk_sim = _six_takes(n, fr, F)
    torch.manual_seed(4)
    env = BatchedHumanoidAREnv(n, 0, mode="train", seed=4, ctx_dim=H, of_dim=F)
    net = TrajARNet(rnn_hdim=H, mlp_hsize=(64, 32, 32), use_context=True, of_dim=F, of_in_state=True).to(env.device)
    src = EpisodeSource(dataset=ds, ctx_builder=PolicyARContext(net, fk_sim, need_rollout=False, keep_context_feat=True), sampling_temp=0.3, sampling_freq=0.5)
    draws, draw = [], src.draw
    src.draw = lambda m, device: draws.append(draw(m, device)) or draws[-1]
    sampler = VectorSampler(env, net, source=src, pool_depth=1, record_full=True)
    sampler.start()
    n_init = len(draws)
    assert n_init == sampler.n_slots == 3 and env.ctx["context_feat_rnn"].shape == (3 * n, fr, H) and env.ctx["of"].shape == (3 * n, fr, F)
    b = sampler.sample(T)
    assert tuple(b.states.shape) == (n, T, H + 105 + F) == tuple(b.next_states.shape) and sampler.top_ups >= 1
    topped = {(int(a), int(c)) for d in draws[n_init:] for a, c in zip(d["take_ind"].tolist(), d["fr_start"].tolist())}
    vm, es = b.v_metas.cpu().numpy(), b.episode_start.cpu().numpy()
    memo, worst, from_top_up = {}, 0.0, 0
    for e in range(n):
        k = episode = 0
        for t in range(T):
            k, episode = (0, episode + (t > 0)) if es[e, t] else (k + 1, episode)
            ti, fs = int(vm[e, t, 0]), int(vm[e, t, 1])
            if (ti, fs) not in memo:
                data = {key: (v.to(env.device) if torch.is_tensor(v) else v) for key, v in ds.batch([ti], [fs], fr).items()}
                with torch.no_grad():
                    memo[(ti, fs)] = (net.context_sequence(data)[:, 0], data["of"][0])
            seq, of = memo[(ti, fs)]
            f = min(k, fr - 1)
            assert torch.equal(b.states[e, t, H + 105:], of[f]), (e, t)                  # a copy of the data set's words
            # the context block was computed in a batch of drawn clips, here alone: the same fp32 sums in another order.  |h| < 1, gate sums of at most
            # 29 + 32 terms, 5 recurrent frames: 5 x 61 x 6e-8 = 2e-5
            worst = max(worst, float((b.states[e, t, :H] - seq[f]).abs().max()))
            if episode >= sampler.n_slots:                                                # the ring's first n_slots clips per env came from _pool_init
                assert (ti, fs) in topped
                from_top_up += 1
    print(f"MEASURED sampler ring: {n * T} rows, {from_top_up} on clips installed by a top-up, top_ups {sampler.top_ups}, context block max |error| {worst:.3e}")
    assert worst <= 2e-5 and from_top_up >= 1


# ------------------------------------------------------------------ 5. the update
@pytest.fixture(scope="module")
def small_agent(kp, tmp_path_factory):
    """AgentAR from kin_poly_of.yml shrunk: 8 envs, horizon 6, rnn_hdim 32, clips of 8 frames, one PPO epoch and one supervised step"""
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.config import Config
    tmp = tmp_path_factory.mktemp("policy_ctx_agent")
    cfg = Config(os.path.join(GOLDEN, "kin_poly_of.yml"), base_dir=str(tmp / "results"), entry="policy_ctx")
    ds, _, _ = _six_takes(8, 8, 16)
    kw = {**cfg.agent_kwargs(of_dim=ds.of_dim), "rnn_hdim": 32, "num_optim_epoch": 1, "num_step_update": 1, "num_sample": 16, "batch_size": 8, "num_init_update": 1}
    assert (kw["use_context"], kw["of_dim"], kw["rl_update"], kw["step_update"], kw["init_update"], kw["full_update"]) == (True, 16, True, True, False, False)
    agent = AgentAR(8, dataset=ds, device=0, horizon=6, result_dir=str(tmp), eval_envs=3, **kw)
    cfg.apply_reward_weights(agent.env)
    return agent, ds, tmp


def _context_params(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith(("context_rnn", "context_mlp", "context_fc"))}


def test_update_trains_the_policy_and_leaves_the_context_network(kp, small_agent):
    agent, ds, _ = small_agent
    net = agent.policy_net
    assert (agent.env.obs_dim, agent.env.ctx_dim, agent.env.of_dim) == (32 + 105 + 16, 32, 16) and net.state_dim == 153 and agent.kin_sim.obs_ar_dim == net.base_dim == 105
    assert agent.value_net.net.affine_layers[0].weight.shape[1] == 153 and agent.ctx_builder.keep_context_feat
    batch = agent.sampler.sample(6)
    assert tuple(batch.states.shape) == (8, 6, 153) and torch.isfinite(batch.states).all()
    before, ctx0 = {k: v.detach().clone() for k, v in net.state_dict().items()}, _context_params(net)
    v0 = agent.value_net.net.affine_layers[0].weight.detach().clone()
    info = agent.update_params(batch)
    print("MEASURED update losses:", {k: info[k] for k in ("surr_loss", "value_loss", "step_loss")})
    assert all(np.isfinite(info[k]) for k in ("surr_loss", "value_loss", "step_loss"))
    assert not torch.equal(net.action_rnn.rnn_f.weight_ih, before["action_rnn.rnn_f.weight_ih"]) and not torch.equal(agent.value_net.net.affine_layers[0].weight, v0)
    for k, v in _context_params(net).items():                                             # the recorded context block is data (policy_ar.py:216-234)
        assert torch.equal(v, ctx0[k]), k
    # the fused re-unroll on the recorded wide states against the per-step loop: tests/test_gpu_round2.py's bound
    with torch.no_grad():
        err = float((net.unroll(batch.states, batch.episode_start, batch.hx0) - net.unroll_reference(batch.states, batch.episode_start, batch.hx0)).abs().max())
    print(f"MEASURED re-unroll on 153-d states: max |fused - loop| {err:.3e}")
    assert err < 2e-5
    # init_update / full_update reach the context network through the data set's batches (data['of'] among them)
    agent.upd.init_update = agent.upd.full_update = True
    info = agent.update_params(agent.sampler.sample(6))
    agent.upd.init_update = agent.upd.full_update = False
    assert np.isfinite(info["init_loss"]) and np.isfinite(info["full_loss"])
    assert not torch.equal(net.context_rnn.rnn_f.weight_ih, ctx0["context_rnn.rnn_f.weight_ih"])


def test_checkpoints_round_trip_and_other_sizes_are_refused(kp, small_agent):
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd import exp_arnet as E
    agent, ds, tmp = small_agent
    net = agent.policy_net
    obs = agent.sampler.sample(2).states[:, 0].contiguous()
    mean = lambda: net.get_action(obs, net.init_hidden(8))[0]      # noqa: E731
    path = str(tmp / "iter_0001.p")
    agent.save_checkpoint(path)
    cp = ck.load_checkpoint(path)
    assert tuple(cp["policy_dict"]["traj_ar_net.context_rnn.rnn_f.weight_ih"].shape) == (96, 16 + 17) and tuple(cp["policy_dict"]["traj_ar_net.action_rnn.rnn_f.weight_ih"].shape) == (96, 153)
    with torch.no_grad():
        m0 = mean()
        for p in net.parameters():
            p.add_(0.5)
    agent.load_checkpoint(path)
    with torch.no_grad():
        assert torch.equal(mean(), m0)
    # the supervised kinematic model's own checkpoint (exp_arnet_all.py --as_policy) of the same sizes
    torch.manual_seed(9)
    sup = E.build_net(as_policy=True, use_context=True, of_dim=16, rnn_hdim=32, mlp_hsize=(1024, 512, 256)).cuda()
    E.save_arnet(str(tmp / "models" / "iter_0003.p"), sup)
    agent.load_checkpoint(str(tmp / "models" / "iter_0003.p"))
    with torch.no_grad():
        assert torch.equal(mean(), sup.get_action(obs, sup.init_hidden(8))[0])
    # other sizes: refused with both shapes, nothing loaded
    for other, words in ((dict(rnn_hdim=64, of_dim=16), ("185-d", "153-d")), (dict(rnn_hdim=32, of_dim=12), ("149-d", "153-d")),
                         (dict(rnn_hdim=32, of_dim=16, mlp_hsize=(512, 512, 256)), ("(512,)", "(1024,)"))):
        E.save_arnet(str(tmp / "models" / "iter_0004.p"), E.build_net(as_policy=True, use_context=True, **{"mlp_hsize": (1024, 512, 256), **other}))
        with pytest.raises(ck.CheckpointWidthError) as e:
            agent.load_checkpoint(str(tmp / "models" / "iter_0004.p"))
        assert all(w in str(e.value) for w in words), str(e.value)
    with torch.no_grad():
        assert torch.equal(mean(), sup.get_action(obs, sup.init_hidden(8))[0])


def test_eval_policy_plays_whole_takes_with_the_wide_observation(kp, small_agent):
    agent, ds, _ = small_agent
    cov = agent.eval_policy("train")[0]["coverage_train"]
    env, builder = agent._eval_engine(None)
    assert (env.ctx_dim, env.of_dim, builder.keep_context_feat, builder.need_rollout) == (32, 16, True, True)
    assert cov["all_coverage"] == ds.get_len() == 6 and 0 <= cov["num_coverage"] <= 6
    assert "ar_qpos" in env.ctx and env.ctx["context_feat_rnn"].shape[2] == 32 and len(set(ds.get_seq_len(i) for i in range(6))) > 1      # ragged whole takes


# ------------------------------------------------------------------ 6. the scripts
def _run(script, *argv):
    old = sys.argv
    sys.argv = [script, *map(str, argv)]
    try:
        runpy.run_path(os.path.join(ROOT, "scripts", script), run_name="__main__")
    finally:
        sys.argv = old


@pytest.fixture(scope="module")
def trained(kp, tmp_path_factory):
    """scripts/train_ar_policy.py --cfg kin_poly_of, two iterations at 8 envs.  The yml is kin_poly_of.yml with the run's LENGTH shrunk and nothing else:
    clips of 20 frames, 48 samples per iteration, one PPO epoch and one supervised step, a checkpoint every 2 iterations."""
    import yaml
    tmp = tmp_path_factory.mktemp("policy_ctx_scripts")
    y = yaml.safe_load(open(os.path.join(GOLDEN, "kin_poly_of.yml")))
    y["fr_num"] = 20
    y["policy_specs"].update(min_batch_size=48, num_optim_epoch=1, num_step_update=1, save_model_interval=2)
    yml = tmp / "kin_poly_of.yml"
    yml.write_text(yaml.safe_dump(y))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        _run("train_ar_policy.py", "--cfg", yml, "--num_envs", 8, "--iters", 2, "--min_horizon", 6, "--no_log")
    finally:
        os.chdir(cwd)
    return tmp, yml, y


def test_train_script_writes_a_checkpoint_and_resumes_it(kp, trained, capfd, monkeypatch):
    from kinpoly_amd import checkpoint as ck
    tmp, yml, _ = trained
    path = tmp / "results" / "all" / "statear" / "kin_poly_of" / "models_policy" / "iter_0002.p"
    assert path.exists()
    pd = ck.load_checkpoint(str(path))["policy_dict"]
    assert tuple(pd["traj_ar_net.action_rnn.rnn_f.weight_ih"].shape) == (768, 256 + 105 + 512) and tuple(pd["traj_ar_net.context_rnn.rnn_f.weight_ih"].shape) == (768, 512 + 17)
    monkeypatch.chdir(tmp)
    _run("train_ar_policy.py", "--cfg", yml, "--num_envs", 8, "--iter", 2, "--iters", 1, "--min_horizon", 6, "--no_log")
    out = capfd.readouterr().out
    assert "models_policy/iter_0002.p" in out and "synthetic stand-in" in out and '"iter": 2' in out


def test_train_script_starts_from_the_kinematic_models_checkpoint(kp, trained, capfd, monkeypatch):
    from kinpoly_amd import exp_arnet as E
    tmp, yml, _ = trained
    models = tmp / "results" / "all" / "statear" / "kin_poly_of" / "models"
    E.save_arnet(str(models / "iter_0001.p"), E.build_net(as_policy=True, use_context=True, of_dim=512, rnn_hdim=256, mlp_hsize=(1024, 512, 256)))
    monkeypatch.chdir(tmp)
    _run("train_ar_policy.py", "--cfg", yml, "--num_envs", 8, "--iter", 1, "--iters", 1, "--min_horizon", 6, "--no_log")
    out = capfd.readouterr().out
    assert "models/iter_0001.p" in out and '"iter": 1' in out


def test_eval_script_plays_two_whole_takes_and_refuses_other_sizes(kp, trained, capfd, monkeypatch):
    import joblib
    import yaml
    from kinpoly_amd import checkpoint as ck
    tmp, yml, y = trained
    _, takes, _ = _six_takes(2, 20, 4, seed=8)
    two = {k: takes[k] for k in sorted(takes)[:2]}
    lens = [len(v["qpos"]) for v in two.values()]
    assert lens[0] != lens[1]
    joblib.dump(two, str(tmp / "two_takes.p"))
    monkeypatch.chdir(tmp)
    _run("eval_ar_policy.py", "--cfg", yml, "--iter", 2, "--data", tmp / "two_takes.p", "--num_seq", 2)
    out = capfd.readouterr().out
    assert "synthetic stand-in" in out and "out of 2" in out
    res = joblib.load(str(tmp / "results" / "all" / "statear" / "kin_poly_of" / "results" / "0002_mocap_annotations_coverage_full.pkl"))
    assert sorted(res) == sorted(two) and all(0 <= r["percent"] <= 1 and len(r["pred"]) >= 1 for r in res.values())
    assert (tmp / "results" / "all" / "statear" / "kin_poly_of" / "results" / "0002_mocap_annotations_coverage.pkl").exists()
    # the same checkpoint under a yml of other sizes
    other = tmp / "other" / "kin_poly_of.yml"
    other.parent.mkdir()
    other.write_text(yaml.safe_dump(dict(y, model_specs=dict(y["model_specs"], rnn_hdim=128))))
    ckpt = tmp / "results" / "all" / "statear" / "kin_poly_of" / "models_policy" / "iter_0002.p"
    with pytest.raises(ck.CheckpointWidthError) as e:
        _run("eval_ar_policy.py", "--cfg", other, "--ckpt", ckpt, "--data", tmp / "two_takes.p", "--num_seq", 2)
    assert "873-d" in str(e.value) and "745-d" in str(e.value)


# ------------------------------------------------------------------ 7. refusals come before any launch
def test_refusals_before_any_launch(kp):
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.env import BatchedHumanoidAREnv
    n, T, H, F = 4, 6, 16, 12
    env = BatchedHumanoidAREnv(n, 0, mode="train", seed=1, ctx_dim=H, of_dim=F)
    ctx = _standing_rows(env, n, T, H, F)
    for key in ("context_feat_rnn", "of"):
        with pytest.raises(ValueError, match=key):
            env.load_context({k: v for k, v in ctx.items() if k != key})
        assert env.ctx is None                                                             # nothing allocated, nothing written
    with pytest.raises(ValueError, match="context_feat_rnn"):
        env.load_context(dict(ctx, context_feat_rnn=ctx["context_feat_rnn"][:, :, :8].contiguous()))
    env.load_context(ctx)
    keep = env.ctx["context_feat_rnn"].clone()
    with pytest.raises(ValueError, match="'of'"):
        env.write_context_rows(torch.arange(2, device="cuda"), {k: v[:2] for k, v in ctx.items() if k != "of"})
    assert torch.equal(env.ctx["context_feat_rnn"], keep)
    with pytest.raises(ValueError, match="cache_init_context"):
        AgentAR(n, context_fn=lambda m: {}, device=0, use_context=True, rnn_hdim=H, mlp_hsize=(16, 8, 8), cache_init_context=True)
    # the record entry points: obs_dim = ctx + base + of, else nothing is launched
    L = kp.load_library()
    W = H + 105 + F
    obs, S = torch.ones((n, W), device="cuda"), torch.full((n, 2, W), -5.0, device="cuda")
    for bad in ((W, H, F - 1), (W, 0, 0), (W, H + 1, F), (W + 1, H, F), (W, -H, F)):
        with pytest.raises(ValueError, match="obs_dim"):
            kp.record_pre(0, 2, obs=obs, states=S, obs_dim=bad[0], ctx_dim=bad[1], of_dim=bad[2])
        with pytest.raises(ValueError, match="obs_dim"):
            kp.record_post(0, 2, action=torch.zeros((n, 80), device="cuda"), obs=obs, next_states=S, obs_dim=bad[0], ctx_dim=bad[1], of_dim=bad[2])
        r = kp.KpRecordPre(n, 2, 0, 0, obs=obs.data_ptr(), states=S.data_ptr())               # valid pointers: a launch would write
        assert L.kp_rollout_record_pre_x(C.byref(r), *bad, None) == -1 and "obs_dim" in L.kp_last_error().decode()
        p = kp.KpRecordPost(n, 2, 0, 0.0, obs=obs.data_ptr(), next_states=S.data_ptr())
        assert L.kp_rollout_record_post_x(C.byref(p), *bad, None) == -1 and "obs_dim" in L.kp_last_error().decode()
    r = kp.KpRecordPre(n, 2, 0, 0, obs=obs.data_ptr(), states=S.data_ptr())
    assert L.kp_rollout_record_pre_w(C.byref(r), W, None) == -1                                # the width-only entry point keeps refusing a wide row
    torch.cuda.synchronize()
    assert bool((S == -5.0).all())
    kp.record_pre(1, 2, obs=obs, states=S, obs_dim=W, ctx_dim=H, of_dim=F)                     # and the right split records
    kp.record_post(0, 2, action=torch.zeros((n, 80), device="cuda"), obs=obs, next_states=S, obs_dim=W, ctx_dim=H, of_dim=F)
    assert bool((S[:, 1] == 1.0).all()) and bool((S[:, 0] == 1.0).all())
