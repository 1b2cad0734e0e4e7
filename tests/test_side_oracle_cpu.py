"""The fp64 references of tests/side_oracle.py checked without a GPU: against oracle/np_oracle.py, torch.nn.GRUCell and the committed fixtures."""
import os

import numpy as np
import pytest

import side_oracle as S
from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
from oracle import np_oracle as O

torch = pytest.importorskip("torch")

KPM = read_kpm(DEFAULT_KPM)
BODY_POS, BODY_IPOS, PARENT = KPM["body_pos"].reshape(24, 3), KPM["body_ipos"].reshape(24, 3), KPM["body_parent"]
DIFFW = KPM["body_diffw"]
STD = np.load(os.path.join(os.path.dirname(__file__), "golden", "standing_neutral.npz"))


def _plain_gae(r, m, v, last, gamma, tau):
    n, T = r.shape
    adv = np.zeros((n, T))
    for e in range(n):
        pv, pa = (0.0 if last is None else last[e]), 0.0
        for t in reversed(range(T)):
            d = r[e, t] + gamma * pv * m[e, t] - v[e, t]
            adv[e, t] = d + gamma * tau * pa * m[e, t]
            pv, pa = v[e, t], adv[e, t]
    return adv, v + adv


def test_gae_ref_equals_the_oracle_and_the_recursion(golden):
    g = golden("gae_zfilter")
    r, m, v = (g[k].astype(np.float64) for k in ("rewards", "masks", "values"))
    adv, ret = S.gae_ref(r.T, m.T, v.T, None, 0.95, 0.95)                   # the fixture as one env of T = 257
    np.testing.assert_allclose(ret[0], g["ret"][:, 0], atol=1e-6)           # the fixture is stored in fp32
    want_adv, want_ret = O.estimate_advantages(r, m, v, 0.95, 0.95)
    np.testing.assert_allclose(ret[0], want_ret[:, 0], atol=1e-13)
    np.testing.assert_allclose((adv[0] - adv[0].mean()) / adv[0].std(ddof=1), want_adv[:, 0], atol=1e-12)
    # a flat batch whose masks end an episode at every cut is the same numbers re-cut into envs
    rng = np.random.default_rng(0)
    n, T = 7, 33
    r, v = rng.normal(size=(n, T)), rng.normal(size=(n, T))
    m = (rng.random((n, T)) > 0.1).astype(np.float64); m[:, -1] = 0
    adv, ret = S.gae_ref(r, m, v, None, 0.95, 0.9)
    _, flat = O.estimate_advantages(r.reshape(-1, 1), m.reshape(-1, 1), v.reshape(-1, 1), 0.95, 0.9)
    np.testing.assert_allclose(ret.reshape(-1), flat[:, 0], atol=1e-13)
    # the bootstrap term, T = 1 and the degenerate discounts against the recursion written out
    for (n, T), (gm, tu), boot in (((5, 1), (0.95, 0.95), True), ((3, 9), (1.0, 1.0), True), ((3, 9), (0.0, 0.0), False), ((4, 17), (0.95, 0.95), True)):
        r, v, m = rng.normal(size=(n, T)), rng.normal(size=(n, T)), (rng.random((n, T)) > 0.3).astype(np.float64)
        last = rng.normal(size=n) if boot else None
        a1, r1 = S.gae_ref(r, m, v, last, gm, tu)
        a2, r2 = _plain_gae(r, m, v, last, gm, tu)
        np.testing.assert_allclose(a1, a2, atol=1e-12); np.testing.assert_allclose(r1, r2, atol=1e-12)
    assert S.gae_bound(np.array([3.0]), 257, 0.95, 0.95) == pytest.approx(8 * S.EPS32 * 3.0 / (1 - 0.9025))
    assert S.gae_bound(np.array([0.5]), 33, 1.0, 1.0) == pytest.approx(8 * S.EPS32 * 33)


def test_gru_gates_ref_equals_grucell_and_autograd():
    """a 3-step masked recurrence: torch.nn.GRUCell + autograd in fp64 against the step-by-step forward / backward references chained as
    kinpoly_amd/gru_unroll.py chains the kernels (carry = dgh W_hh + dhz, masked by the step's own episode-start flag)."""
    torch.manual_seed(0)
    n, D, H, T = 5, 7, 6, 3
    cell = torch.nn.GRUCell(D, H).double()
    x = torch.randn(T, n, D, dtype=torch.float64)
    keep = (torch.rand(T, n, dtype=torch.float64) > 0.4).double()            # keep[t] = 0: an episode starts at step t (hidden state zeroed)
    w_out = torch.randn(T, n, H, dtype=torch.float64)
    x.requires_grad_(True)
    hm = torch.zeros(n, H, dtype=torch.float64)
    hs = []
    for t in range(T):
        h = cell(x[t], hm)
        hs.append(h)
        hm = h * keep[t + 1][:, None] if t + 1 < T else h
    loss = sum((hs[t] * w_out[t]).sum() for t in (0, 2))                    # step 1 has no outside consumer: its dh_out is null
    loss.backward()
    Wih, Whh, bih, bhh = (p.detach() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh))
    gi = [(x[t].detach() @ Wih.T + bih).numpy() for t in range(T)]
    hm_prev, gh, hout = np.zeros((n, H)), [], []
    hms = []
    for t in range(T):
        hms.append(hm_prev)
        gh.append(hm_prev @ Whh.T.numpy() + bhh.numpy())
        h, hm_next = S.gru_gates_fwd_ref(gi[t], gh[t], hm_prev, keep[t + 1].numpy() if t + 1 < T else None)
        np.testing.assert_allclose(h, hs[t].detach().numpy(), atol=1e-12)
        hout.append(h); hm_prev = hm_next
    carry = None
    for t in reversed(range(T)):
        dh_out = None if t == 1 else w_out[t].numpy()
        ck = keep[t + 1].numpy() if t + 1 < T else None
        dgi, dgh, dhz = S.gru_gates_bwd_ref(gi[t], gh[t], hms[t], dh_out, carry, ck)
        np.testing.assert_allclose(dgi @ Wih.numpy(), x.grad[t].numpy(), atol=1e-12)
        carry = dgh @ Whh.numpy() + dhz
    # saturated gates have their fp64 limits: finite, and the gradient through a saturated gate is 0
    big = np.full((2, 3), 100.0)
    h, _ = S.gru_gates_fwd_ref(np.concatenate([big, big, big], 1), np.zeros((2, 9)), np.full((2, 3), 0.25))
    np.testing.assert_allclose(h, 0.25, atol=1e-12)
    dgi, dgh, dhz = S.gru_gates_bwd_ref(np.concatenate([big, big, big], 1), np.zeros((2, 9)), np.full((2, 3), 0.25), np.ones((2, 3)))
    assert np.isfinite(dgi).all() and np.abs(dgi).max() < 1e-30 and np.allclose(dhz, 1.0)


def test_mcp_compose_ref_equals_the_policy_mixing_stage():
    rng = np.random.default_rng(1)
    n, K, A = 9, 8, 75
    shapes = [(f"nets.{k}.0.affine_layers.{i}.{w}", s) for k in range(K) for i, d in ((0, (32, 784)), (1, (16, 32))) for w, s in (("weight", d), ("bias", d[:1]))]
    shapes += [(f"nets.{k}.1.{w}", s) for k in range(K) for w, s in (("weight", (A, 16)), ("bias", (A,)))]
    shapes += [(f"composer.0.affine_layers.{i}.{w}", s) for i, d in ((0, (32, 784)), (1, (16, 32)), (2, (K, 16))) for w, s in (("weight", d), ("bias", d[:1]))]
    sd = O.seeded_state_dict(shapes, 3)
    x = rng.normal(size=(n, 784))
    mean, w = O.policy_mcp_mean(x, sd)
    prim = np.stack([O.mlp_relu(x, [(sd[f"nets.{k}.0.affine_layers.{i}.weight"], sd[f"nets.{k}.0.affine_layers.{i}.bias"]) for i in range(2)]) @ sd[f"nets.{k}.1.weight"].T
                     + sd[f"nets.{k}.1.bias"] for k in range(K)])
    logits = O.mlp_relu(x, [(sd[f"composer.0.affine_layers.{i}.weight"], sd[f"composer.0.affine_layers.{i}.bias"]) for i in range(3)])
    np.testing.assert_allclose(S.mcp_compose_ref(logits, prim), mean, atol=1e-13)
    noise, std = rng.normal(size=(n, A)), rng.uniform(0.1, 1, A)
    np.testing.assert_allclose(S.mcp_compose_ref(logits, prim, noise, std), mean + std * noise, atol=1e-13)
    out = S.mcp_compose_ref(np.array([[1e4, -1e4, 0.0]]), np.arange(6.0).reshape(3, 1, 2))           # the max subtraction holds
    np.testing.assert_allclose(out, [[0.0, 1.0]], atol=1e-300)
    assert np.isfinite(out).all()


def _fixture_state(g):
    n = len(g["qpos"])
    fk = [O.qpos_fk(q, BODY_POS, BODY_IPOS, PARENT) for q in g["target_qpos"].astype(np.float64)]
    return dict(qpos=g["qpos"], xpos=g["xpos"].reshape(n, 72), xquat=g["xquat"].reshape(n, 96), prev_bquat=g["prev_bquat"], prev_hpos=g["prev_hpos"],
                t_wbpos=np.stack([f["wbpos"].reshape(-1) for f in fk]), t_bquat=np.stack([f["bquat"].reshape(-1) for f in fk]))


def test_term_reward_ref_reproduces_the_fixture(golden):
    g = golden("ar_obs_reward")
    n, T = len(g["qpos"]), 6
    rng = np.random.default_rng(2)
    t = g["t"].astype(np.int64)
    assert t.min() >= 1 and t.max() <= T - 1
    R = n + 3                                                                 # a context table larger than the batch, read through a row map
    row = rng.permutation(R)[:n]
    head_pose, gt_bquat, gt_wbpos = rng.normal(size=(R, T, 7)), rng.normal(size=(R, T, 96)), rng.normal(size=(R, T, 72))
    for i in range(n):
        head_pose[row[i], t[i]] = g["head_pose"][i]; gt_bquat[row[i], t[i]] = g["gt_bquat"][i]; gt_bquat[row[i], t[i] - 1] = g["gt_prev_bquat"][i]
        gt_wbpos[row[i], t[i]] = g["gt_wbpos"][i].reshape(-1)
    one_hot = np.zeros((R, 4)); one_hot[row] = g["action_one_hot"]
    ctx = dict(T=T, head_pose=head_pose, gt_bquat=gt_bquat, gt_wbpos=gt_wbpos, action_one_hot=one_hot, cur_t=t, row=row)
    out = S.term_reward_ref(_fixture_state(g), ctx, S.reward_cfg(), None)
    np.testing.assert_allclose(out["reward"], g["reward"], atol=1e-6)        # the fixture's state rows are stored in fp32
    np.testing.assert_allclose(out["info"], g["reward_info"], atol=1e-6)
    np.testing.assert_allclose(out["diffs"][:, 1], g["body_gt_diff"], atol=1e-5)
    np.testing.assert_allclose(out["diffs"][:, 0], g["body_diff"], atol=1e-5)
    np.testing.assert_array_equal(out["fail"], (g["body_diff"] > 10) | (g["body_gt_diff"] > 12))
    assert not S.term_reward_ref(_fixture_state(g), ctx, dict(S.reward_cfg(), thresh=60.0, gt_thresh=60.0), None)["fail"].any()
    # POST: cur_t + 1 first, then end / done / percent / obj7
    ctx2 = dict(ctx, cur_t=t - 1)
    row_len = np.full(R, 5); row_len[row[::2]] = 50
    obj7 = rng.normal(size=(n, 7)); simobj = rng.normal(size=(n, 35))
    post = S.term_reward_ref(_fixture_state(g), ctx2, S.reward_cfg(), None, post=dict(row_len=row_len, episode_len=4, obj7=obj7, sim_obj_qpos=simobj))
    np.testing.assert_array_equal(post["reward"], out["reward"])
    np.testing.assert_array_equal(post["cur_t"], t)
    np.testing.assert_array_equal(post["end"], t >= np.minimum(row_len[row], 4))
    np.testing.assert_array_equal(post["done"], post["end"] | post["fail"])
    np.testing.assert_allclose(post["percent"], t / row_len[row])
    assert post["done_count"] == post["done"].sum()
    for i in range(n):
        hot = np.flatnonzero(g["action_one_hot"][i])
        want = obj7[i] if len(hot) == 0 else simobj[i, S.ACTION_START[hot[0]]:S.ACTION_START[hot[0]] + 7]
        np.testing.assert_array_equal(post["obj7"][i], want)
    # the knife-edge guard: a row 1e-4 from the threshold is refused, a NaN pose fails
    st = _fixture_state(g)
    bd0 = out["diffs"][0, 0]
    st["xpos"] = st["xpos"].astype(np.float64).copy()
    cfgk = dict(S.reward_cfg(), thresh=bd0 + 1e-4)
    with pytest.raises(AssertionError):
        S.term_reward_ref(st, ctx, cfgk, None)
    st["xpos"][3, 5] = np.nan
    with np.errstate(all="ignore"):
        bad = S.term_reward_ref(st, ctx, dict(S.reward_cfg(), thresh=60.0, gt_thresh=60.0), None)
    assert bad["fail"][3] and not bad["fail"][np.arange(n) != 3].any()


def test_generators_give_finite_references_and_are_what_they_say():
    n = 28
    q = S.edge_qpos(n, 5, STD["qpos"])
    norms = np.linalg.norm(q[:, 3:7], axis=1)
    assert (np.abs(norms[0::4] - 1) > 1e-3).any() and np.abs(q[1::4, 7:]).max() > 2.5 * np.pi
    for i in range(n):
        fk = O.qpos_fk(q[i], BODY_POS, BODY_IPOS, PARENT)
        assert all(np.isfinite(v).all() for v in fk.values())
        assert np.isfinite(O.get_body_quat(q[i])).all()
        if i % 4 >= 2:
            h = O.get_heading(O.remove_base_rot(q[i, 3:7]))
            assert abs(abs((h + np.pi) % (2 * np.pi) - np.pi) - np.pi) < 1.1e-6
    a = S.kin_actions(n, 6, edges=True)
    ang = np.linalg.norm(a[:, 77:80], axis=1) * S.DT
    np.testing.assert_allclose(ang, [S.ANGLE_EDGES[i % 7] for i in range(n)], rtol=1e-12, atol=0)
    assert (a[0::7, 77:80] == 0).all()
    qu = S.random_qpos(n, 8, STD["qpos"])
    for i in range(n):
        nxt = O.step_ar(qu[i], a[i])
        nxt[3:7] /= np.linalg.norm(nxt[3:7])
        v = O.get_qvel_fd_new(qu[i].copy(), nxt.copy(), S.DT)
        assert np.isfinite(nxt).all() and np.isfinite(v).all()
        if i % 7 == 0:
            assert (v[3:6] == 0).all()                                        # the exact-zero rotation has exactly zero angular velocity
        if i % 7 in (3, 4):                                                   # |angle| wrapped to (-pi, pi]: just below pi on both sides
            assert abs(np.linalg.norm(v[3:6]) * S.DT - (np.pi - 1e-3)) < 1e-6
    g = S.body_quat_edges(qu, 9)
    own = np.stack([O.get_body_quat(x) for x in qu])
    np.testing.assert_allclose(g[1::4], own[1::4], atol=1e-12); np.testing.assert_allclose(g[2::4], -own[2::4], atol=1e-12)
    assert (g[1::4] == own[1::4]).all() and (g[2::4] == -own[2::4]).all()
    np.testing.assert_allclose(np.linalg.norm(g.reshape(n, 24, 4), axis=2), 1.0, atol=1e-6)
    d = O.multi_quat_norm_v2(O.multi_quat_diff(g[2], own[2]))
    assert np.abs(d).max() < 1e-12                                            # q and -q are the same rotation
    raw = np.random.default_rng(1).normal(size=(6, 30))
    mean, std = S.zfilter_edges(raw, 5.0, 2)
    z = O.zfilter(raw, mean, std, 5.0)
    assert np.isfinite(z).all() and (std[0::3] == 0).all() and (z[0, 0::3] == 0).all()
    np.testing.assert_allclose(np.abs(z[0, 1::3]), 5.0, atol=1e-12)
    assert np.abs(z).max() <= 5.0


def test_heading_safe_targets_stay_off_the_wrap_and_small_turns_have_their_velocity():
    n = 64
    q = S.edge_qpos(n, 11, STD["qpos"]).astype(np.float32).astype(np.float64)          # half of these rows have a heading within 1e-6 of +-pi
    raw = S.edge_qpos(n, 12, STD["qpos"])
    near = [i for i in range(n) if abs(abs(S.rel_heading(q[i], raw[i])) - np.pi) < 0.3]
    raw[0, 3:7] = S.yawed(q[0, 3:7], np.pi - 1e-4)                                     # a row that sits on the wrap before it is turned away
    assert abs(abs(S.rel_heading(q[0], raw[0])) - np.pi) < 1e-2
    tq = S.heading_safe_targets(q, raw)
    for i in range(n):
        rel = S.rel_heading(q[i], tq[i])
        assert abs(abs(rel) - np.pi) > 1e-2, (i, rel, near)
        assert (tq[i] == tq[i].astype(np.float32)).all()
    assert not np.array_equal(tq[0, 3:7], raw[0, 3:7].astype(np.float32))
    # the analytic small-turn velocity equals get_qvel_fd_new wherever that function does not cut the turn to zero, and is the action's own where it does
    qu = S.random_qpos(14, 13, STD["qpos"])
    a = S.kin_actions(14, 14, edges=True)
    for i in range(14):
        qn = qu[i].copy(); qn[3:7] /= np.linalg.norm(qn[3:7])
        nxt = O.step_ar(qn, a[i]); nxt[3:7] /= np.linalg.norm(nxt[3:7])
        w = S.small_turn_qvel(qn, a[i])
        np.testing.assert_allclose(w, a[i, 77:80], atol=1e-12 * max(1.0, np.abs(a[i, 77:80]).max()))
        if S.ANGLE_EDGES[i % 7] in (1e-4,):
            assert (O.get_qvel_fd_new(qn, nxt.copy(), S.DT)[3:6] == 0).all() and np.linalg.norm(w) * S.DT == pytest.approx(1e-4)
        if S.ANGLE_EDGES[i % 7] == np.pi - 1e-3:
            np.testing.assert_allclose(O.get_qvel_fd_new(qn, nxt.copy(), S.DT)[3:6], w, atol=1e-9)
