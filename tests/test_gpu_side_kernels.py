"""GPU sweeps of the kernels around the control step (target FK, step_kin, kin_advance, obs_cc / obs_cc_v, obs_ar, term_reward<POST>, GAE, the GRU
gate kernels, mcp_compose, reset / copy / record rows) on an MI355X (-m gpu): (a) row by row against the fp64 references of tests/side_oracle.py on
random and edge rows at batch sizes that straddle each kernel's packing, (b) batch-position independence bit for bit (permuted, and cut into chunks
of 37), plus the argument refusals that keep these kernels in bounds.  Bounds on random rows are the suite's existing ones for the same kernel; bounds
on edge rows are 4x the deviation from the fp64 reference measured on the MI355X (`# measured ...`).  Every figure is printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import side_oracle as S  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm  # noqa: E402
from oracle import np_oracle as O  # noqa: E402

KPM = read_kpm(DEFAULT_KPM)
BODY_POS, BODY_IPOS, PARENT = KPM["body_pos"].reshape(24, 3), KPM["body_ipos"].reshape(24, 3), KPM["body_parent"]
DIFFW = KPM["body_diffw"]
GOLD = os.path.join(os.path.dirname(__file__), "golden")
STD = np.load(os.path.join(GOLD, "standing_neutral.npz"))
NS = (1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1000, 4099)
TARGET_FIELDS = ("target_qpos", "target_wbpos", "target_wbquat", "target_bquat", "target_com")
FK_KEYS = ("qpos", "wbpos", "wbquat", "bquat", "body_com")


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    yield kpsim
    _SIMS.clear()                       # the handles of this module do not stay on the device for the rest of the session
    torch.cuda.empty_cache()


_SIMS = {}


def get_sim(kp, n, **opts):
    key = (n, tuple(sorted(opts.items())))
    if key not in _SIMS:
        _SIMS[key] = kp.KpSim(kp.KpModel(**opts), n)
    return _SIMS[key]


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def dev(a):
    return torch.tensor(f32(a), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def load(sim, **rows):
    """write rows straight into the simulator's stored fields (no sim.forward(): the kernels under test read whatever is stored)"""
    for k, v in rows.items():
        sim.view(k).copy_(torch.from_numpy(f32(v)))


def check_rows(n, block, seed=0):
    """the rows compared with the (slow, per-row) fp64 reference: all of them below 1000, else the first and the last block + 64 seeded rows"""
    if n < 1000:
        return np.arange(n)
    last0 = (n - 1) // block * block
    pick = np.random.default_rng(seed).choice(n, 64, replace=False)
    return np.unique(np.concatenate([np.arange(block), np.arange(last0, n), pick]))


def worst(name, got, want):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(got) else 0.0
    print(f"MEASURED {name}: {err:.3e}")
    return err


def mixed_qpos(n, seed):
    """first half random rows, second half edge rows, then shuffled: (qpos fp32-exact as fp64, is_edge)"""
    h = n // 2
    q = np.concatenate([S.random_qpos(h, seed, STD["qpos"]), S.edge_qpos(n - h, seed + 1, STD["qpos"])])
    edge = np.arange(n) >= h
    p = np.random.default_rng(seed + 2).permutation(n)
    return f32(q[p]).astype(np.float64), edge[p]


def fk_ref(q, rows):
    out = {k: [] for k in FK_KEYS}
    for i in rows:
        f = O.qpos_fk(q[i], BODY_POS, BODY_IPOS, PARENT)
        for k in FK_KEYS:
            out[k].append(f[k].reshape(-1))
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ target FK
def test_target_fk_sweep(kp):
    tot = {"rand": 0.0, "edge": 0.0}
    for n in NS:
        sim = get_sim(kp, n)
        q, edge = mixed_qpos(n, 100 + n)
        got = {k: host(v) for k, v in sim.fk(dev(q)).items()}
        rows = check_rows(n, 4)
        ref = fk_ref(q, rows)
        for k in FK_KEYS:
            d = np.abs(got[k][rows].astype(np.float64) - ref[k]).max(1)
            tot["rand"] = max(tot["rand"], d[~edge[rows]].max(initial=0.0)); tot["edge"] = max(tot["edge"], d[edge[rows]].max(initial=0.0))
        sim.set_target(dev(q))                                      # the same kernel through set_target: the same bits
        for fld, k in zip(TARGET_FIELDS, FK_KEYS):
            assert np.array_equal(host(sim.get(fld)), got[k]), (n, fld)
    print("MEASURED target_fk random / edge:", tot)
    assert tot["rand"] < 5e-6           # measured 5.5e-07
    assert tot["edge"] < 2.6e-6         # measured 6.4e-07 (joint angles of +-3 pi, root quaternions of norm 0.25 .. 4)


def test_target_fk_masks_keep_masked_rows(kp):
    for n in NS:
        sim = get_sim(kp, n)
        q0, _ = mixed_qpos(n, 200 + n); q1, _ = mixed_qpos(n, 300 + n)
        want = {k: host(v) for k, v in sim.fk(dev(q1)).items()}
        rng = np.random.default_rng(n)
        masks = [rng.integers(0, 2, n), np.ones(n), np.zeros(n), (np.arange(n) == n - 1)]
        blk = np.ones(n); blk[(n // 8) * 4:(n // 8) * 4 + 4] = 0       # all rows of one 4-row block masked out
        masks.append(blk)
        for m in masks:
            m = np.asarray(m, np.uint8)
            sim.set_target(dev(q0))
            before = {f: host(sim.get(f)) for f in TARGET_FIELDS}
            sim.set_target(dev(q1), torch.tensor(m, device="cuda"))
            for fld, k in zip(TARGET_FIELDS, FK_KEYS):
                after = host(sim.get(fld))
                assert np.array_equal(after[m == 0], before[fld][m == 0]), (n, fld, "masked rows moved")
                assert np.array_equal(after[m != 0], want[k][m != 0]), (n, fld, "live rows")


def test_fused_step_head_equals_its_three_kernels(kp):
    for n in NS:
        q, _ = mixed_qpos(n, 400 + n)
        act = f32(S.kin_actions(n, 500 + n, edges=True))
        sim = get_sim(kp, n)
        fk0 = sim.fk(dev(q))
        load(sim, qpos=q, xpos=host(fk0["wbpos"]), xquat=host(fk0["wbquat"]))
        sim.step_begin()
        nxt = sim.step_kin(dev(act))
        sep = {k: host(v) for k, v in sim.fk(nxt).items()}
        sep_prev = (host(sim.get("prev_bquat")), host(sim.get("prev_hpos")))
        other, _ = mixed_qpos(n, 450 + n)                              # scrub everything the fused call has to write, with another pose
        sim.set_target(dev(other)); load(sim, qpos=other, xpos=np.zeros((n, 72)), xquat=np.zeros((n, 96))); sim.step_begin()
        assert not np.array_equal(host(sim.get("prev_bquat")), sep_prev[0]) and not np.array_equal(host(sim.get("prev_hpos")), sep_prev[1])
        load(sim, qpos=q, xpos=host(fk0["wbpos"]), xquat=host(fk0["wbquat"]))
        sim.step_head(dev(act))
        for fld, k in zip(TARGET_FIELDS, FK_KEYS):
            assert np.array_equal(host(sim.get(fld)), sep[k]), (n, fld)
        assert np.array_equal(host(sim.get("prev_bquat")), sep_prev[0]) and np.array_equal(host(sim.get("prev_hpos")), sep_prev[1]), n
        assert np.array_equal(host(sim.get("qpos")), f32(q))          # the head of the step does not move the state


# ------------------------------------------------------------------------------------------------ get_body_quat / the step's snapshot
def test_bquat_and_snapshot_sweep(kp):
    """k_bquat (kp_sim_get KP_BQUAT) and k_snapshot (kp_sim_step_begin: prev_bquat, prev_hpos) against O.get_body_quat in fp64 and the head rows they copy"""
    tot = {"bquat rand": 0.0, "bquat edge": 0.0, "prev rand": 0.0, "prev edge": 0.0}
    for n in NS:
        sim = get_sim(kp, n)
        q, edge = mixed_qpos(n, 550 + n)
        rng = np.random.default_rng(n)
        xpos, xquat = f32(rng.normal(size=(n, 72))), f32(rng.normal(size=(n, 96)))
        other, _ = mixed_qpos(n, 560 + n)
        load(sim, qpos=other, xpos=np.zeros((n, 72)), xquat=np.zeros((n, 96))); sim.step_begin()          # whatever an earlier call left is not the answer
        load(sim, qpos=q, xpos=xpos, xquat=xquat)
        bq = host(sim.get("bquat")).astype(np.float64)
        sim.step_begin()
        pb, ph = host(sim.get("prev_bquat")).astype(np.float64), host(sim.get("prev_hpos"))
        assert np.array_equal(ph[:, :3], xpos[:, 39:42]) and np.array_equal(ph[:, 3:], xquat[:, 52:56]), (n, "prev_hpos is the head row of xpos / xquat")
        assert np.array_equal(host(sim.get("qpos")), f32(q))
        rows = check_rows(n, 11)                                          # 256 threads = 10 2/3 envs of 24 bodies
        want = np.stack([O.get_body_quat(q[i]) for i in rows])
        for name, got in (("bquat", bq), ("prev", pb)):
            d = np.abs(got[rows] - want).max(1)
            tot[name + " rand"] = max(tot[name + " rand"], d[~edge[rows]].max(initial=0.0)); tot[name + " edge"] = max(tot[name + " edge"], d[edge[rows]].max(initial=0.0))
    print("MEASURED bquat / prev_bquat:", tot)
    assert tot["bquat rand"] < 2e-6 and tot["prev rand"] < 2e-6         # test_step_kin_and_bquat_match_golden's bound; measured 1.4e-07
    assert tot["bquat edge"] < 5.8e-7 and tot["prev edge"] < 5.8e-7     # measured 1.44e-07 (joint angles of +-3 pi, root quaternions of norm 0.25 .. 4, copied as they are)


# ------------------------------------------------------------------------------------------------ step_kin / kin_advance
def test_step_kin_and_kin_advance_sweep(kp):
    tot = {k: 0.0 for k in ("step rand", "step edge", "adv q rand", "adv q edge", "adv w rand", "adv w edge", "adv lin")}
    for n in NS:
        sim = get_sim(kp, n)
        q = f32(S.random_qpos(n, 600 + n, STD["qpos"])).astype(np.float64)
        edge = np.arange(n) % 2 == 1
        act = S.kin_actions(n, 700 + n, edges=False); act[edge] = S.kin_actions(n, 701 + n, edges=True)[edge]
        if n >= 7:
            act[0, 77:80] = 0.0
        act = f32(act).astype(np.float64)
        load(sim, qpos=q)
        nxt = host(sim.step_kin(dev(act)))
        aq, av = kp.kin_advance(dev(q), dev(act))
        aq, av = host(aq), host(av)
        rows = check_rows(n, 128)
        for i in rows:
            want = O.step_ar(q[i], act[i])
            tag = "edge" if edge[i] else "rand"
            tot["step " + tag] = max(tot["step " + tag], np.abs(nxt[i] - want).max())
            wn = want.copy(); wn[3:7] /= np.linalg.norm(wn[3:7])
            qn = q[i].copy(); qn[3:7] /= np.linalg.norm(qn[3:7])          # the fp64 formula needs the unit quaternion the fp32 row stands for (1 - |w| of a 1e-4 rad turn is 1e-9)
            wv = O.get_qvel_fd_new(qn, wn.copy(), S.DT)
            if 1 - abs(O.quaternion_multiply(wn[3:7], O.quaternion_inverse(qn[3:7]))[0]) < 1e-8 and np.any(act[i, 77:80]):
                # below math.py:45-65's `1 - |w| < 1e-8 -> no rotation` cut-off (turns of 1e-8 and 1e-4 rad) the kernel keeps the true small velocity, as
                # get_qvel_fd_batch does (torch_utils.py:315-331: its clamped acos never takes that branch); the reference there is the analytic rotation
                # vector / dt in the root frame, in fp64
                wv = wv.copy(); wv[3:6] = S.small_turn_qvel(qn, act[i])
            tot["adv q " + tag] = max(tot["adv q " + tag], np.abs(aq[i] - wn).max())
            tot["adv w " + tag] = max(tot["adv w " + tag], np.abs(av[i, 3:6] - wv[3:6]).max())
            tot["adv lin"] = max(tot["adv lin"], np.abs(av[i, :3] - wv[:3]).max(), np.abs(av[i, 6:] - wv[6:]).max())
            if not np.any(act[i, 77:80]):
                assert np.array_equal(nxt[i, 3:7], f32(q[i, 3:7])), "no rotation asked for: the root quaternion is kept"
                assert (av[i, 3:6] == 0).all(), ("the exact-zero rotation has exactly zero angular velocity", n, i, av[i, 3:6])
        # in place, as TrajARNet.rollout uses it: the next pose is a later slot of the buffer the current one lives in
        Q = torch.zeros((3, n, 76), device="cuda"); V = torch.zeros((3, n, 75), device="cuda")
        Q[1].copy_(dev(q))
        kp.kin_advance(Q[1], dev(act), S.DT, Q[2], V[2])
        assert np.array_equal(host(Q[2]), aq) and np.array_equal(host(V[2]), av) and np.array_equal(host(Q[1]), f32(q)) and not Q[0].any() and not V[:2].any()
    print("MEASURED step_kin / kin_advance:", tot)
    assert tot["step rand"] < 1e-6          # measured 1.2e-07
    assert tot["step edge"] < 3e-6          # measured 7.5e-07 (steps of 0, 1e-8, 1e-4, pi +- 1e-3, 2 pi +- 1e-3 rad)
    assert tot["adv q rand"] < 2e-6         # test_kin_advance_is_step_ar_plus_finite_difference_velocity's bound; measured 1.2e-07
    assert tot["adv q edge"] < 2.9e-6       # measured 7.2e-07
    assert tot["adv lin"] < 1e-4            # the same test's bound; measured 1.0e-05
    assert tot["adv w rand"] < 3e-5         # the same test's bound; measured 6.9e-06
    assert tot["adv w edge"] < 1.8e-4       # measured 4.3e-05 (a turn of 2 pi - 1e-3 rad wraps to -1e-3: 2 pi of fp32 cancels, x 1 / dt)


# ------------------------------------------------------------------------------------------------ obs_cc / obs_ar
def _sim_state(kp, sim, n, seed):
    """a stored state for the observation kernels: mixed qpos, qvel, and 'stale' kinematics (the FK of a slightly different pose)"""
    q, edge = mixed_qpos(n, seed)
    rng = np.random.default_rng(seed + 9)
    qv = f32(rng.normal(size=(n, 75)))
    stale = q.copy(); stale[:, 7:] += rng.normal(size=(n, 69)) * 0.05
    f = sim.fk(dev(stale))
    st = dict(qpos=f32(q), qvel=qv, xpos=host(f["wbpos"]), xquat=host(f["wbquat"]), xipos=host(f["body_com"]))
    load(sim, **st)
    return st, edge


def test_obs_cc_sweep_and_zfilter_edges(kp):
    tot = {"rand": 0.0, "edge": 0.0, "zf": 0.0}
    for n in NS:
        sim = get_sim(kp, n)
        st, edge = _sim_state(kp, sim, n, 800 + n)
        tq = S.heading_safe_targets(st["qpos"].astype(np.float64), mixed_qpos(n, 900 + n)[0])          # 1e-2 off the +-pi wrap (asserted there and in the CPU test)
        sim.set_target(dev(tq))
        obs = host(sim.obs_cc()).astype(np.float64)
        tg = {k: host(sim.get(f)).astype(np.float64) for f, k in zip(TARGET_FIELDS, FK_KEYS)}
        for i in check_rows(n, 1):
            t = dict(qpos=tg["qpos"][i], wbpos=tg["wbpos"][i].reshape(24, 3), wbquat=tg["wbquat"][i].reshape(24, 4), body_com=tg["body_com"][i].reshape(24, 3))
            want = O.obs_cc(st["qpos"][i].astype(np.float64), st["qvel"][i].astype(np.float64), st["xpos"][i].reshape(24, 3).astype(np.float64),
                            st["xquat"][i].reshape(24, 4).astype(np.float64), st["xipos"][i].reshape(24, 3).astype(np.float64), t)
            tag = "edge" if edge[i] else "rand"
            tot[tag] = max(tot[tag], np.abs(obs[i] - want).max())
        mean, std = (f32(a) for a in S.zfilter_edges(obs, 5.0, n))
        z = host(sim.obs_cc(zf_mean=dev(mean), zf_std=dev(std), clip=5.0)).astype(np.float64)
        want = np.clip((obs - mean.astype(np.float64)) / (std.astype(np.float64) + 1e-8), -5, 5)
        assert np.isfinite(z).all() and np.abs(z).max() <= 5.0 and (z[0, std == 0] == 0).all()
        tot["zf"] = max(tot["zf"], float((np.abs(z - want) - 1e-6 * np.abs(want)).max()))
    print("MEASURED obs_cc random / edge / zfilter (beyond rtol 1e-6):", tot)
    assert tot["rand"] < 5e-6           # measured 1.4e-06
    assert tot["edge"] < 6.3e-6         # measured 1.6e-06 (headings within 1e-6 of +-pi, non-unit root quaternions, +-3 pi joint angles)
    assert tot["zf"] < 1e-5             # test_obs_cc_matches_pinned_oracle's bound (atol 1e-5, rtol 1e-6); std = 0 columns and entries on +-clip; measured: inside the rtol alone


def _ctx(kp, sim, n, seed, T=6, extra=5, cur_t=None, body_q=None):
    """a context table of R = n + extra rows read through a non-identity row map; cur_t cycles over both clamps and the interior"""
    rng = np.random.default_rng(seed)
    R = n + extra
    row = rng.permutation(R)[:n].astype(np.int32)
    c = dict(T=T, head_pose=f32(rng.normal(size=(R, T, 7))), head_vels=f32(rng.normal(size=(R, T, 6))), obj_rel=f32(rng.normal(size=(R, T, 7))),
             gt_bquat=f32(rng.normal(size=(R, T, 96))), gt_wbpos=f32(rng.normal(size=(R, T, 72))), row=row)
    oh = np.zeros((R, 4), np.float32)
    for r in range(R):
        if r % 5 < 4:
            oh[r, r % 5] = 1.0                                        # each of the four actions, and the all-zero one
    c["action_one_hot"] = oh
    c["cur_t"] = np.asarray([-2, 0, 1, T - 2, T - 1, T + 3], np.int32)[np.arange(n) % 6] if cur_t is None else cur_t
    c["obj_qpos"] = f32(rng.normal(size=(n, 7)))
    return c


def _make_ctx(sim, c):
    c["_cur_t_dev"] = torch.tensor(c["cur_t"], dtype=torch.int32, device="cuda")
    return sim.make_ctx(c["T"], dev(c["head_pose"]), dev(c["head_vels"]), dev(c["obj_rel"]), dev(c["action_one_hot"]), dev(c["gt_bquat"]), dev(c["gt_wbpos"]),
                        c["_cur_t_dev"], obj_qpos=dev(c["obj_qpos"]), row=torch.tensor(c["row"], device="cuda"))


def test_obs_ar_sweep(kp):
    tot = {"rand": 0.0, "edge": 0.0}
    for n in NS:
        sim = get_sim(kp, n)
        st, edge = _sim_state(kp, sim, n, 1000 + n)
        c = _ctx(kp, sim, n, 1100 + n)
        obs = host(sim.obs_ar(_make_ctx(sim, c))).astype(np.float64)
        assert obs.shape == (n, 105)
        for i in check_rows(n, 64):
            r, t = c["row"][i], min(max(int(c["cur_t"][i]), 0), c["T"] - 1)
            want = O.obs_ar(st["qpos"][i].astype(np.float64), st["xpos"][i].reshape(24, 3).astype(np.float64), st["xquat"][i].reshape(24, 4).astype(np.float64),
                            c["head_pose"][r, t].astype(np.float64), c["head_vels"][r, t].astype(np.float64), c["obj_rel"][r, t].astype(np.float64),
                            c["action_one_hot"][r].astype(np.float64), c["obj_qpos"][i].astype(np.float64))
            tag = "edge" if edge[i] else "rand"
            tot[tag] = max(tot[tag], np.abs(obs[i] - want).max())
    print("MEASURED obs_ar random / edge:", tot)
    assert tot["rand"] < 5e-6           # measured 1.3e-06 (head poses and object poses are N(0, 1) here, not unit quaternions)
    assert tot["edge"] < 6.6e-6         # measured 1.6e-06


# ------------------------------------------------------------------------------------------------ term_reward<POST>
def _reward_case(kp, sim, n, seed, nan_env=None):
    """state after a step + its context, built so that bd / bgd sit on chosen sides of their thresholds, at least 0.5 away"""
    rng = np.random.default_rng(seed)
    q0 = f32(S.random_qpos(n, seed, STD["qpos"])).astype(np.float64)
    q1 = q0.copy()
    q1[:, 7:] += rng.normal(size=(n, 69)) * 0.02 * (np.arange(n) % 3 != 0)[:, None]          # every third env: the body quaternions equal the previous ones exactly
    q1[np.arange(n) % 4 == 1, 3:7] *= -1.0                                                  # root q vs -q between the two frames
    tq = q0.copy(); tq[:, 7:] += rng.normal(size=(n, 69)) * 0.1
    load(sim, qpos=q0, xpos=np.zeros((n, 72)), xquat=np.tile([1.0, 0, 0, 0], (n, 24)))
    sim.step_begin()
    sim.set_target(dev(tq))
    twb = host(sim.get("target_wbpos")).astype(np.float64)
    u = rng.normal(size=(n, 24, 3)); u /= np.linalg.norm(u, axis=2, keepdims=True)
    bd_t = np.where(np.arange(n) % 3 == 2, rng.uniform(11, 30, n), rng.uniform(0.5, 9, n))
    xpos = twb + (u * (bd_t / DIFFW.sum())[:, None, None]).reshape(n, 72)
    xq = rng.normal(size=(n, 24, 4)); xq /= np.linalg.norm(xq, axis=2, keepdims=True)
    xposf = f32(xpos)
    if nan_env is not None:
        xposf[nan_env, 3 * 7 + 1] = np.nan
    load(sim, qpos=q1, xpos=xposf, xquat=xq.reshape(n, 96))
    c = _ctx(kp, sim, n, seed + 1)
    bq = f32(S.body_quat_edges(f32(q1).astype(np.float64), seed + 2))
    bgd_t = np.where(np.arange(n) % 5 == 4, rng.uniform(13, 20, n), rng.uniform(0.5, 11, n))
    for e in range(n):
        r = c["row"][e]
        for t in range(c["T"]):
            v = rng.normal(size=(24, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
            c["gt_wbpos"][r, t] = f32(xposf[e].astype(np.float64) + (v * bgd_t[e] / DIFFW.sum()).reshape(72)) if np.isfinite(xposf[e]).all() else 0
            other = rng.normal(size=(24, 4)); other /= np.linalg.norm(other, axis=1, keepdims=True)
            c["gt_bquat"][r, t] = bq[e] if t % 2 else f32(other.reshape(96))
        c["head_pose"][r, :, :3] = xposf[e, 39:42] + rng.normal(size=(c["T"], 3)) * 0.05
        c["head_pose"][r, :, 3:] = f32(O.quaternion_multiply(O.quat_from_expmap(rng.normal(size=3) * 0.1), xq[e, 13]))
    state = dict(qpos=f32(q1), xpos=xposf, xquat=f32(xq.reshape(n, 96)), t_wbpos=host(sim.get("target_wbpos")), t_bquat=host(sim.get("target_bquat")),
                 prev_bquat=host(sim.get("prev_bquat")), prev_hpos=host(sim.get("prev_hpos")))
    return state, c


def _compare_reward(tot, got, ref, rows):
    for k, i in (("reward", 0), ("info", 1)):
        tot[k] = max(tot[k], np.abs(got[i][rows].astype(np.float64) - ref[k]).max())
    d = np.abs(got[3][rows].astype(np.float64) - ref["diffs"])
    tot["diffs"] = max(tot["diffs"], float((d - 1e-6 * np.abs(ref["diffs"])).max()))
    assert np.array_equal(got[2][rows].astype(bool), ref["fail"])


def _sub(d, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) and k not in ("head_pose", "head_vels", "obj_rel", "gt_bquat", "gt_wbpos", "action_one_hot") else v) for k, v in d.items()}


def test_term_reward_and_post_step_sweep(kp):
    tot = {"reward": 0.0, "info": 0.0, "diffs": 0.0}
    cfg = kp.KpRewardCfg.default()
    for n in NS:
        sim = get_sim(kp, n)
        state, c = _reward_case(kp, sim, n, 1200 + n)
        rows = check_rows(n, 8)
        ref = S.term_reward_ref(_sub(state, rows), _sub(c, rows), S.reward_cfg(), DIFFW)
        assert ref["fail"].any() or n < 3
        got = [host(x) for x in sim.term_reward(_make_ctx(sim, c), cfg)]
        _compare_reward(tot, got, ref, rows)
        # POST: the same call one frame earlier, + cur_t / end / done / percent / done_count / obj7
        c2 = dict(c, cur_t=(c["cur_t"] - 1).astype(np.int32))
        R = len(c["head_pose"])
        rng = np.random.default_rng(n)
        row_len = rng.integers(2, 12, R).astype(np.int32)                       # below and above episode_len = 5
        simobj = f32(rng.normal(size=(n, 35))); obj7_0 = f32(rng.normal(size=(n, 7)))
        load(sim, obj_qpos=simobj)
        ctx = _make_ctx(sim, c2)
        o = dict(reward=torch.zeros(n, device="cuda"), info=torch.zeros((n, 6), device="cuda"), fail=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 diffs=torch.zeros((n, 2), device="cuda"), done=torch.zeros(n, dtype=torch.uint8, device="cuda"), end=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 percent=torch.zeros(n, device="cuda"))
        cnt = torch.full((1,), 3, dtype=torch.int32, device="cuda"); obj7 = dev(obj7_0)
        sim.post_step(ctx, cfg, c2["_cur_t_dev"], torch.tensor(row_len, device="cuda"), 5, o["reward"], o["info"], o["fail"], o["diffs"], o["done"], o["end"], o["percent"], cnt, obj7)
        refp = S.term_reward_ref(_sub(state, rows), _sub(c2, rows), S.reward_cfg(), DIFFW, post=dict(row_len=row_len, episode_len=5, obj7=obj7_0[rows], sim_obj_qpos=simobj[rows]))
        gp = {k: host(v) for k, v in o.items()}
        assert np.array_equal(gp["reward"], got[0]) and np.array_equal(gp["info"], got[1]) and np.array_equal(gp["fail"], got[2]) and np.array_equal(gp["diffs"], got[3]), "POST computes the same reward"
        assert np.array_equal(host(c2["_cur_t_dev"]), c["cur_t"])
        assert np.array_equal(gp["end"][rows].astype(bool), refp["end"]) and np.array_equal(gp["done"][rows].astype(bool), refp["done"])
        np.testing.assert_allclose(gp["percent"][rows], refp["percent"], rtol=2e-7, atol=0)          # one fp32 division
        assert np.array_equal(host(obj7)[rows], f32(refp["obj7"]))
        assert int(cnt.item()) == 3 + int(gp["done"].astype(bool).sum()), "done_count"
        assert np.array_equal(gp["done"].astype(bool), gp["end"].astype(bool) | gp["fail"].astype(bool))
    print("MEASURED term_reward reward / info / diffs (beyond rtol 1e-6):", tot)
    assert tot["reward"] < 2e-6 and tot["info"] < 2e-6          # measured 9.2e-08 / 2.9e-07 (q vs -q, equal quaternions, both cur_t clamps)
    assert tot["diffs"] < 3e-5                                  # the existing bound (rtol 1e-6 / atol 3e-5); measured: inside the rtol alone


def test_a_nan_pose_fails_its_env_and_leaves_the_neighbours_alone(kp):
    n = 20
    sim = get_sim(kp, n)
    cfg = kp.KpRewardCfg.default()
    state, c = _reward_case(kp, sim, n, 1300)
    clean = [host(x) for x in sim.term_reward(_make_ctx(sim, c), cfg)]
    state2, c2 = _reward_case(kp, sim, n, 1300, nan_env=11)
    bad = [host(x) for x in sim.term_reward(_make_ctx(sim, c2), cfg)]
    keep = np.arange(n) != 11
    assert bad[2][11] == 1
    for a, b in zip(clean, bad):
        assert np.array_equal(a[keep], b[keep])                 # env 11 shares its 256-thread block with envs 8 .. 15; only its 32-lane butterfly is its own
    # POST = true on the same two states: the NaN env is done, its block neighbours' outputs (cur_t, end, done, percent included) do not move
    R = len(c["head_pose"])
    row_len = torch.full((R,), 50, dtype=torch.int32, device="cuda")
    posts = []
    for nan_env in (None, 11):
        _, cc = _reward_case(kp, sim, n, 1300, nan_env=nan_env)
        cc = dict(cc, cur_t=(cc["cur_t"] - 1).astype(np.int32))
        ctx = _make_ctx(sim, cc)
        o = [torch.zeros(n, device="cuda"), torch.zeros((n, 6), device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros((n, 2), device="cuda"),
             torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, device="cuda")]
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        sim.post_step(ctx, cfg, cc["_cur_t_dev"], row_len, 40, *o, cnt)
        posts.append([host(x) for x in o] + [host(cc["_cur_t_dev"])] + [int(cnt.item())])
    assert posts[1][2][11] == 1 and posts[1][4][11] == 1 and posts[1][-1] == int(posts[1][4].astype(bool).sum())
    for a, b, cl in zip(posts[0][:4], posts[1][:4], clean):
        assert np.array_equal(a[keep], b[keep]) and np.array_equal(a[keep], cl[keep])
    for a, b in zip(posts[0][4:-1], posts[1][4:-1]):
        assert np.array_equal(a[keep], b[keep])


# ------------------------------------------------------------------------------------------------ GAE
@pytest.mark.parametrize("n,T", [(1, 1), (1, 257), (7, 1), (257, 99), (4099, 33)])
def test_gae_sweep(kp, n, T):
    rng = np.random.default_rng(n * 1000 + T)
    r, v, lv = f32(rng.normal(size=(n, T))), f32(rng.normal(size=(n, T))), f32(rng.normal(size=n))
    last0 = np.ones((n, T)); last0[-1] = 0
    rows = check_rows(n, 64)
    for mname, m in (("random", rng.random((n, T)) > 0.1), ("ones", np.ones((n, T))), ("zeros", np.zeros((n, T))), ("last row 0", last0)):
        m = f32(m)
        for gamma, tau in ((0.95, 0.95), (1.0, 1.0), (0.0, 0.0)):
            for boot in (None, lv):
                adv, ret = kp.gae(dev(r), dev(m), dev(v), gamma, tau, None if boot is None else dev(boot))
                a_ref, r_ref = S.gae_ref(r[rows], m[rows], v[rows], None if boot is None else boot[rows], float(np.float32(gamma)), float(np.float32(tau)))
                bound = S.gae_bound(r_ref, T, gamma, tau)
                ea, er = np.abs(host(adv)[rows] - a_ref).max(), np.abs(host(ret)[rows] - r_ref).max()
                print(f"MEASURED gae n={n} T={T} masks={mname} gamma={gamma} boot={boot is not None}: adv {ea:.2e} ret {er:.2e} bound {bound:.2e}")
                assert ea <= bound and er <= bound


# ------------------------------------------------------------------------------------------------ GRU gates
def _gates_call(kp, gi, gh, hp, keep, dh, carry, ck, hm_null=False):
    L = kp.load_library()
    n, H = hp.shape
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    d = lambda a: None if a is None else dev(a)  # noqa: E731
    tg = [d(a) for a in (gi, gh, hp, keep, dh, carry, ck)]
    h, hm = torch.full((n, H), 7.0, device="cuda"), torch.full((n, H), 7.0, device="cuda")
    assert L.kp_gru_gates_forward(n, H, p(tg[0]), p(tg[1]), p(tg[2]), p(tg[3]), p(h), None if hm_null else p(hm), None) == 0
    dgi, dgh, dhz = torch.zeros((n, 3 * H), device="cuda"), torch.zeros((n, 3 * H), device="cuda"), torch.zeros((n, H), device="cuda")
    assert L.kp_gru_gates_backward(n, H, p(tg[0]), p(tg[1]), p(tg[2]), p(tg[4]), p(tg[5]), p(tg[6]), p(dgi), p(dgh), p(dhz), None) == 0
    torch.cuda.synchronize()
    return [host(x) for x in (h, hm, dgi, dgh, dhz)]


@pytest.mark.parametrize("n,H", [(1, 1), (3, 63), (5, 64), (7, 65), (257, 1024)])
def test_gru_gate_kernels_direct(kp, n, H):
    rng = np.random.default_rng(n + H)
    tot = {}
    for scale in ("normal", 30.0, 100.0):
        gi, gh = f32(rng.normal(size=(n, 3 * H))), f32(rng.normal(size=(n, 3 * H)))
        if scale != "normal":
            gi = f32(np.where(rng.random((n, 3 * H)) < 0.5, -scale, scale)); gh = f32(rng.normal(size=(n, 3 * H)) * 0.5)
        hp, dh, carry = f32(rng.normal(size=(n, H))), f32(rng.normal(size=(n, H))), f32(rng.normal(size=(n, H)))
        keep, ck = f32(rng.integers(0, 2, n)), f32(rng.integers(0, 2, n))
        for ki, (k_, d_, c_, ck_, hm_null) in enumerate(((keep, dh, carry, ck, False), (None, dh, None, None, False), (keep, None, carry, None, True), (None, None, None, None, False))):
            h, hm, dgi, dgh, dhz = _gates_call(kp, gi, gh, hp, k_, d_, c_, ck_, hm_null)
            rh, rhm = S.gru_gates_fwd_ref(gi, gh, hp, k_)
            rgi, rgh, rhz = S.gru_gates_bwd_ref(gi, gh, hp, d_, c_, ck_)
            assert all(np.isfinite(x).all() for x in (h, hm, dgi, dgh, dhz))
            if hm_null:
                assert (hm == 7.0).all()                              # a null hm_next is not written
            e_f = max(np.abs(h - rh).max(), 0.0 if hm_null else np.abs(hm - rhm).max())
            e_b = max(np.abs(dgi - rgi).max(), np.abs(dgh - rgh).max(), np.abs(dhz - rhz).max()) / max(1.0, np.abs(rgi).max(), np.abs(rgh).max(), np.abs(rhz).max())
            tot[scale] = (max(tot.get(scale, (0, 0))[0], e_f), max(tot.get(scale, (0, 0))[1], e_b))
            if d_ is None and c_ is None:
                assert not dgi.any() and not dgh.any() and not dhz.any()
            if ki == 0:                                               # batch-position independence, bit for bit
                pm = rng.permutation(n)
                h2 = _gates_call(kp, gi[pm], gh[pm], hp[pm], keep[pm], dh[pm], carry[pm], ck[pm])
                for a, b in zip((h, hm, dgi, dgh, dhz), h2):
                    assert np.array_equal(a[pm], b)
                parts = [_gates_call(kp, gi[a:a + 37], gh[a:a + 37], hp[a:a + 37], keep[a:a + 37], dh[a:a + 37], carry[a:a + 37], ck[a:a + 37]) for a in range(0, n, 37)]
                for k, a in enumerate((h, hm, dgi, dgh, dhz)):      # chunks of 37 rows: another n * H, so another last partial 256-thread block
                    assert np.array_equal(np.concatenate([p_[k] for p_ in parts]), a)
    print(f"MEASURED gru gates n={n} H={H} (forward, backward):", tot)
    assert tot["normal"][0] < 1e-6 and tot["normal"][1] <= 2e-5         # the unroll test's bounds (h 1e-6, gradients 2e-5 max(1, |ref|)); measured 4.3e-07 / 1.9e-07
    for s in (30.0, 100.0):                                             # __expf(100) is inf: 1 / (1 + inf) = 0 is the fp64 limit to 1e-44
        assert tot[s][0] < 8e-12 and tot[s][1] < 1.7e-7                 # measured 1.9e-12 / 4.1e-08 at +-30, 0 / 3.8e-08 at +-100


# ------------------------------------------------------------------------------------------------ mcp_compose
@pytest.mark.parametrize("K", [1, 8, 16])
@pytest.mark.parametrize("A", [1, 75, 80])
def test_mcp_compose_sweep(kp, K, A):
    worst_e = 0.0
    for n in (1, 257, 4099):
        rng = np.random.default_rng(n + K * 100 + A)
        prim = f32(rng.normal(size=(K, n, A)))
        wide = dev(rng.normal(size=(n, A + 80))); noise = wide[:, 80:]; std = f32(rng.uniform(0.05, 1.0, A))
        for lname in ("normal", "equal", "huge"):
            lg = f32(rng.normal(size=(n, K)) if lname == "normal" else np.full((n, K), 0.37) if lname == "equal" else rng.choice([-1e4, 1e4], (n, K)))
            out = host(kp.mcp_compose(dev(lg), dev(prim)))
            outn = host(kp.mcp_compose(dev(lg), dev(prim), noise=noise, std=dev(std)))
            assert np.isfinite(out).all()
            worst_e = max(worst_e, np.abs(out - S.mcp_compose_ref(lg, prim)).max(), np.abs(outn - S.mcp_compose_ref(lg, prim, host(noise), std)).max())
        pm = rng.permutation(n)                                       # batch-position independence
        lg = f32(rng.normal(size=(n, K)))
        whole = host(kp.mcp_compose(dev(lg), dev(prim)))
        assert np.array_equal(host(kp.mcp_compose(dev(lg[pm]), dev(prim[:, pm]))), whole[pm])
        parts = [host(kp.mcp_compose(dev(lg[a:a + 37]), dev(prim[:, a:a + 37]))) for a in range(0, n, 37)]
        assert np.array_equal(np.concatenate(parts), whole)
    print(f"MEASURED mcp_compose K={K} A={A}: {worst_e:.3e}")
    assert worst_e < 2e-5           # test_mcp_tail_matches_fp64's bound; measured 6.6e-07


def test_mcp_compose_agrees_with_mcp_tail_mixing(kp):
    """kp_mcp_tail with an identity-free last layer reduced to a copy: h2 = relu-able positive rows, w3 = a [J, A] selection, so its mixing stage sees prim = h2[:, :, :A] + b3"""
    rng = np.random.default_rng(5)
    n, K, J, A = 257, 8, 64, 48
    h2 = f32(np.abs(rng.normal(size=(K, n, J)))); b2 = np.zeros((K, J), np.float32)
    w3 = np.zeros((K, J, A), np.float32); w3[:, np.arange(A), np.arange(A)] = 1.0
    b3 = f32(rng.normal(size=(K, A))); lg = f32(rng.normal(size=(n, K)))
    tail = host(kp.mcp_tail(dev(h2), dev(b2), dev(w3), dev(b3), dev(lg)))
    prim = h2[:, :, :A] + b3[:, None, :]
    comp = host(kp.mcp_compose(dev(lg), dev(prim)))
    e = worst("mcp_tail vs mcp_compose", tail, comp)
    assert e < 2e-5                 # the same bound; measured 7.2e-07
    assert worst("mcp_compose vs fp64 (tail shapes)", comp, S.mcp_compose_ref(lg, prim)) < 2e-5


# ------------------------------------------------------------------------------------------------ reset / copy / record rows
@pytest.mark.parametrize("aux_cols", [0, 1, 129, 1024])
def test_reset_rows_is_the_gather_it_replaces(kp, aux_cols):
    for n in (1, 9, 257):
        sim = get_sim(kp, n, contact=0)
        rng = np.random.default_rng(n + aux_cols)
        R = n + 4
        iq = f32(S.random_qpos(R, n, STD["qpos"])); iq[:, 2] += 5.0
        iv = f32(rng.normal(size=(R, 75)) * 0.1)
        row = rng.integers(0, R, n).astype(np.int32)                  # a row map with repeats
        q0 = f32(S.random_qpos(n, n + 1, STD["qpos"])); v0 = f32(rng.normal(size=(n, 75)))
        for mask in (None, rng.integers(0, 2, n).astype(np.uint8), np.zeros(n, np.uint8)):
            sim.set_state(dev(q0), dev(v0))
            before = {k: host(sim.get(k)) for k in ("qpos", "qvel", "qpos_d", "qvel_d")}
            aux = None if aux_cols == 0 else torch.full((n, aux_cols), 3.0, device="cuda")
            cur_t = torch.full((n,), 9, dtype=torch.int32, device="cuda")
            sim.reset_rows(dev(iq), dev(iv), torch.tensor(row, device="cuda"), None if mask is None else torch.tensor(mask, device="cuda"), cur_t, False, aux)
            live = np.ones(n, bool) if mask is None else mask.astype(bool)
            for k, src in (("qvel", iv), ("qvel_d", iv)):
                want = before[k].copy(); want[live] = src[row[live]]
                assert np.array_equal(host(sim.get(k)), want), (n, k)
            for k in ("qpos", "qpos_d"):                              # sim.forward() normalises the root quaternion of the rows it touched
                got, want = host(sim.get(k)), before[k].copy()
                want[live] = iq[row[live]]
                assert np.array_equal(got[~live], want[~live]) and np.array_equal(got[:, :3], want[:, :3]) and np.array_equal(got[:, 7:], want[:, 7:])
                assert np.abs(got[:, 3:7] - want[:, 3:7]).max() < 5e-7          # 4 ulp of 1: |q|^2 of an fp32 "unit" row is off by up to 2.4e-7
            assert np.array_equal(host(cur_t), np.where(live, 0, 9))
            if aux is not None:
                assert np.array_equal(host(aux), np.where(live[:, None], 0.0, 3.0) * np.ones((1, aux_cols)))


def test_set_state_copy_rows_masks(kp):
    for n in (1, 5, 257, 1000):
        sim = get_sim(kp, n, contact=0)
        rng = np.random.default_rng(n)
        qa, qb = f32(S.random_qpos(n, 1, STD["qpos"])), f32(S.random_qpos(n, 2, STD["qpos"]))
        va, vb = f32(rng.normal(size=(n, 75))), f32(rng.normal(size=(n, 75)))
        for mask in (rng.integers(0, 2, n).astype(np.uint8), np.zeros(n, np.uint8), (np.arange(n) == n - 1).astype(np.uint8)):
            sim.set_state(dev(qa), dev(va))
            before = {k: host(sim.get(k)) for k in ("qpos", "qvel", "qpos_d", "qvel_d", "xpos")}
            sim.set_state(dev(qb), dev(vb), torch.tensor(mask, device="cuda"))
            live = mask.astype(bool)
            for k in before:
                assert np.array_equal(host(sim.get(k))[~live], before[k][~live]), (n, k)
            assert np.array_equal(host(sim.get("qvel"))[live], vb[live]) and np.array_equal(host(sim.get("qvel_d"))[live], vb[live])
            assert np.array_equal(host(sim.get("qpos"))[live][:, 7:], qb[live][:, 7:])


@pytest.mark.parametrize("obs_dim", [105, 101])
def test_record_rows_are_the_scatter_they_replace(kp, obs_dim):
    n, T, ctx_T = 37, 5, 7
    rng = np.random.default_rng(obs_dim)
    R = n + 3
    src = dict(obs=f32(rng.normal(size=(n, obs_dim))), qpos=f32(rng.normal(size=(n, 76))), fresh=rng.integers(0, 2, n).astype(np.uint8))
    ctx_qpos = f32(rng.normal(size=(R, ctx_T, 76))); row = rng.integers(0, R, n).astype(np.int32)
    row_len = rng.integers(1, ctx_T, R).astype(np.int32); cur_t = rng.integers(-1, ctx_T + 2, n).astype(np.int32); row_meta = f32(rng.normal(size=(R, 2)))
    post = dict(action=f32(rng.normal(size=(n, 80))), reward=f32(rng.normal(size=n)), fail=rng.integers(0, 2, n).astype(np.uint8), done=rng.integers(0, 2, n).astype(np.uint8),
                percent=f32(rng.random(n)), c_info=f32(rng.normal(size=(n, 6))), cc_action=f32(rng.normal(size=(n, 75))), cc_state=f32(rng.normal(size=(n, 784))))
    T_ = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    for t in (0, T - 1):                                              # the first and the last record position
        bufs = dict(states=(n, T, obs_dim), curr_qpos=(n, T, 76), gt_target_qpos=(n, T, 76), meta=(n, T, 2), actions=(n, T, 80), rewards=(n, T), percents=(n, T),
                    c_infos=(n, T, 6), next_states=(n, T, obs_dim), res_qpos=(n, T, 76), cc_actions=(n, T, 75), cc_states=(n, T, 784), v_metas=(n, T, 3))
        B = {k: torch.full(s, -5.0, device="cuda") for k, s in bufs.items()}
        U = {k: torch.full((n, T), 9, dtype=torch.uint8, device="cuda") for k in ("episode_start", "fails", "dones")}
        kp.record_pre(t, T, obs=T_(src["obs"]), fresh=T_(src["fresh"]), qpos=T_(src["qpos"]), ctx_qpos=T_(ctx_qpos), row=T_(row), cur_t=T_(cur_t), row_len=T_(row_len),
                      row_meta=T_(row_meta), states=B["states"], episode_start=U["episode_start"], curr_qpos=B["curr_qpos"], gt_target_qpos=B["gt_target_qpos"], meta=B["meta"], obs_dim=obs_dim)
        kp.record_post(t, T, fr_num=42.0, obs=T_(src["obs"]), qpos=T_(src["qpos"]), meta=B["meta"], **{k: T_(v) for k, v in post.items()}, actions=B["actions"], rewards=B["rewards"],
                       fails=U["fails"], dones=U["dones"], percents=B["percents"], c_infos=B["c_infos"], next_states=B["next_states"], res_qpos=B["res_qpos"], cc_actions=B["cc_actions"],
                       cc_states=B["cc_states"], v_metas=B["v_metas"], obs_dim=obs_dim)
        f = np.minimum(cur_t + 1, row_len[row])
        want = dict(states=src["obs"], curr_qpos=src["qpos"], gt_target_qpos=ctx_qpos[row, f], meta=row_meta[row], actions=post["action"], rewards=post["reward"], percents=post["percent"],
                    c_infos=post["c_info"], next_states=src["obs"], res_qpos=src["qpos"], cc_actions=post["cc_action"], cc_states=post["cc_state"],
                    v_metas=np.concatenate([row_meta[row], np.full((n, 1), 42.0, np.float32)], 1), episode_start=src["fresh"], fails=post["fail"], dones=post["done"])
        for k, w in want.items():
            g = host(B[k] if k in B else U[k])
            assert np.array_equal(g[:, t], w), (k, t)
            others = np.delete(g, t, axis=1)
            assert (others == (-5.0 if k in B else 9)).all(), (k, "untouched positions")


# ------------------------------------------------------------------------------------------------ batch-position independence of the simulator-state kernels
def _position_independent(kp, opts, rows, run, n_chunk=37):
    """run(sim, idx) loads rows[idx] into sim (len(idx) envs) and returns a list of outputs; whole vs permuted vs chunks of 37, bit for bit"""
    n = len(next(iter(rows.values())))
    whole = run(get_sim(kp, n, **opts), np.arange(n))
    pm = np.random.default_rng(3).permutation(n)
    for a, b in zip(whole, run(get_sim(kp, n, **opts), pm)):
        assert np.array_equal(a[pm], b), "permuted rows"
    parts = [run(get_sim(kp, min(n_chunk, n - a), **opts), np.arange(a, min(a + n_chunk, n))) for a in range(0, n, n_chunk)]
    for k, a in enumerate(whole):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), a), "chunks of 37"


def test_every_obs_cc_variant_is_position_independent(kp):
    g = np.load(os.path.join(GOLD, "uhc_obs_variants.npz"))
    n = 4099
    tile = np.arange(n) % len(g["qpos"])
    base = get_sim(kp, n)
    base.set_state(dev(g["qpos"][tile]), dev(g["qvel"][tile]))
    rows = {k: host(base.get(k)) for k in ("qpos", "qvel", "xpos", "xquat", "xipos")}
    for var in g["variants"]:
        opts = dict(cc_obs_v=int(var[0]), cc_obs_vel_root=int(var[1]), cc_obs_heading=int(var[2]), cc_obs_deheading=int(var[3]), cc_obs_phase=int(var[4]))
        tq = f32(g["clip"][(g["t"] if var[0] == 0 else g["t"] + 1)[tile]])
        phase = f32((g["t"] / int(g["len"]))[tile])
        rows_v = dict(rows, tq=tq, phase=phase)

        def run(sim, idx, var=var, rows_v=rows_v):
            load(sim, **{k: rows_v[k][idx] for k in ("qpos", "qvel", "xpos", "xquat", "xipos")})
            sim.set_target(dev(rows_v["tq"][idx]))
            return [host(sim.obs_cc(phase=dev(rows_v["phase"][idx]) if (var[0] == 0 and var[4]) else None))]
        _position_independent(kp, opts, rows_v, run)
        whole = run(get_sim(kp, n, **opts), np.arange(n))[0]
        assert np.array_equal(whole[12:24], whole[:12]) and np.array_equal(whole[n - 12 - n % 12:n - n % 12], whole[:12]), "tiled rows repeat bit for bit"
        for key in [k for k in _SIMS if k[1]]:                      # this variant's three handles are done
            del _SIMS[key]


def test_fk_obs_ar_reward_and_gae_are_position_independent(kp):
    n = 4099
    q, _ = mixed_qpos(n, 77)
    act = f32(S.kin_actions(n, 78, edges=True))
    state, c = _reward_case(kp, get_sim(kp, 256), 256, 79)
    tile = np.arange(n) % 256
    rows = {k: v[tile] for k, v in state.items()}
    rows["q0"] = f32(q); rows["act"] = act
    R = len(c["head_pose"])
    cfg = kp.KpRewardCfg.default()

    def run(sim, idx):
        m = len(idx)
        out = [host(v) for v in sim.fk(dev(rows["q0"][idx])).values()]
        load(sim, qpos=rows["q0"][idx], xpos=rows["xpos"][idx], xquat=rows["xquat"][idx])
        sim.step_begin()
        out += [host(sim.get("bquat")), host(sim.get("prev_bquat")), host(sim.get("prev_hpos"))]          # k_bquat, k_snapshot
        out.append(host(sim.step_kin(dev(rows["act"][idx]))))
        out += [host(x) for x in kp.kin_advance(dev(rows["q0"][idx]), dev(rows["act"][idx]))]
        sim.set_target(dev(rows["q0"][idx]))
        load(sim, qpos=rows["qpos"][idx])
        ci = dict(c, cur_t=c["cur_t"][tile[idx]], row=c["row"][tile[idx]], obj_qpos=c["obj_qpos"][tile[idx]])
        ctx = _make_ctx(sim, ci)
        out.append(host(sim.obs_ar(ctx)))
        out += [host(x) for x in sim.term_reward(ctx, cfg)]
        assert len(out[-1]) == m
        return out
    _position_independent(kp, {}, rows, run)
    rng = np.random.default_rng(80)
    T = 33
    r, m, v, lv = f32(rng.normal(size=(n, T))), f32(rng.random((n, T)) > 0.1), f32(rng.normal(size=(n, T))), f32(rng.normal(size=n))
    whole = [host(x) for x in kp.gae(dev(r), dev(m), dev(v), 0.95, 0.95, dev(lv))]
    pm = rng.permutation(n)
    for a, b in zip(whole, kp.gae(dev(r[pm]), dev(m[pm]), dev(v[pm]), 0.95, 0.95, dev(lv[pm]))):
        assert np.array_equal(a[pm], host(b))
    for k in range(2):
        parts = [host(kp.gae(dev(r[a:a + 37]), dev(m[a:a + 37]), dev(v[a:a + 37]), 0.95, 0.95, dev(lv[a:a + 37]))[k]) for a in range(0, n, 37)]
        assert np.array_equal(np.concatenate(parts), whole[k])


# ------------------------------------------------------------------------------------------------ refusals: no launch, -1, kp_last_error, outputs untouched
def test_bad_sizes_and_null_pointers_are_refused(kp):
    L = kp.load_library()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    z = torch.full((4, 3 * 8), 2.5, device="cuda"); o = torch.full((4, 3 * 8), -1.0, device="cuda")
    f = C.c_float

    def refused(rc, name):
        torch.cuda.synchronize()
        assert rc == -1 and name in L.kp_last_error(), (rc, L.kp_last_error())
        assert (o == -1.0).all() and (z == 2.5).all()
    for n_, T_ in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        refused(L.kp_gae(n_, T_, p(z), p(z), p(z), f(0.9), f(0.9), p(o), p(o), None), b"kp_gae")
        refused(L.kp_gae_bootstrap(n_, T_, p(z), p(z), p(z), p(z), f(0.9), f(0.9), p(o), p(o), None), b"kp_gae")
    for k in range(5):
        a = [p(z), p(z), p(z), p(o), p(o)]; a[k] = None
        refused(L.kp_gae(4, 4, a[0], a[1], a[2], f(0.9), f(0.9), a[3], a[4], None), b"kp_gae: bad arguments")
    for n_, K_, A_ in ((0, 2, 3), (-4, 2, 3), (4, 0, 3), (4, 65, 3), (4, 2, 0), (4, 2, -1)):
        refused(L.kp_mcp_compose(n_, K_, A_, p(z), p(z), None, 0, None, p(o), None), b"kp_mcp_compose")
    refused(L.kp_mcp_compose(4, 2, 3, None, p(z), None, 0, None, p(o), None), b"kp_mcp_compose")
    refused(L.kp_mcp_compose(4, 2, 3, p(z), None, None, 0, None, p(o), None), b"kp_mcp_compose")
    refused(L.kp_mcp_compose(4, 2, 3, p(z), p(z), None, 0, None, None, None), b"kp_mcp_compose")
    refused(L.kp_mcp_compose(4, 2, 3, p(z), p(z), p(z), 3, None, p(o), None), b"kp_mcp_compose")          # noise without std
    refused(L.kp_mcp_compose(4, 2, 3, p(z), p(z), p(z), 2, p(z), p(o), None), b"noise_stride")            # rows of the noise window would overlap / run past it
    for n_, H_ in ((0, 8), (-2, 8), (4, 0), (4, -8)):
        refused(L.kp_gru_gates_forward(n_, H_, p(z), p(z), p(z), None, p(o), p(o), None), b"kp_gru_gates_forward")
        refused(L.kp_gru_gates_backward(n_, H_, p(z), p(z), p(z), p(z), None, None, p(o), p(o), p(o), None), b"kp_gru_gates_backward")
    for k in range(4):
        a = [p(z), p(z), p(z), p(o)]; a[k] = None
        refused(L.kp_gru_gates_forward(1, 8, a[0], a[1], a[2], None, a[3], None, None), b"kp_gru_gates_forward")
    for k in range(6):
        a = [p(z), p(z), p(z), p(o), p(o), p(o)]; a[k] = None
        refused(L.kp_gru_gates_backward(1, 8, a[0], a[1], a[2], None, None, None, a[3], a[4], a[5], None), b"kp_gru_gates_backward")
    for n_, dt_ in ((0, 0.03), (-1, 0.03), (1, 0.0), (1, -0.03), (1, float("nan"))):
        refused(L.kp_kin_advance(n_, p(z), p(z), f(dt_), p(o), p(o), None), b"kp_kin_advance")
    for k in range(4):
        a = [p(z), p(z), p(o), p(o)]; a[k] = None
        refused(L.kp_kin_advance(1, a[0], a[1], f(0.03), a[2], a[3], None), b"kp_kin_advance")
    with pytest.raises(ValueError):
        kp.mcp_compose(torch.zeros((4, 3), device="cuda"), torch.zeros((2, 4, 5), device="cuda"))


def test_context_and_record_refusals_keep_the_kernels_in_bounds(kp):
    """T = 1 would make k_term_reward read ground-truth frame t - 1 = -1; t >= T would record past the buffers: refused on the host, nothing launched"""
    L = kp.load_library()
    n = 4
    sim = get_sim(kp, n)
    T = 3
    c = _ctx(kp, sim, n, 5, T=T)
    out = dict(reward=torch.full((n,), -1.0, device="cuda"), info=torch.full((n, 6), -1.0, device="cuda"), fail=torch.full((n,), 7, dtype=torch.uint8, device="cuda"),
               diffs=torch.full((n, 2), -1.0, device="cuda"), done=torch.full((n,), 7, dtype=torch.uint8, device="cuda"), end=torch.full((n,), 7, dtype=torch.uint8, device="cuda"),
               percent=torch.full((n,), -1.0, device="cuda"), obs=torch.full((n, 105), -1.0, device="cuda"), obj7=torch.full((n, 7), -1.0, device="cuda"))
    row_len = torch.full((n + 5,), 3, dtype=torch.int32, device="cuda")
    cfg = kp.KpRewardCfg.default()

    def untouched(name):
        torch.cuda.synchronize()
        assert name in L.kp_last_error(), L.kp_last_error()
        for k, v in out.items():
            assert (v == (7 if v.dtype == torch.uint8 else -1.0)).all(), k
    for badT in (1, 0, -2):
        ctx = _make_ctx(sim, c); ctx.T = badT
        with pytest.raises(kp.KinPolyNativeError):
            sim.term_reward(ctx, cfg, out["reward"], out["info"], out["fail"], out["diffs"])
        untouched(b"kp_sim_term_reward")
        before = host(c["_cur_t_dev"]).copy()
        with pytest.raises(kp.KinPolyNativeError):
            sim.post_step(ctx, cfg, c["_cur_t_dev"], row_len, 5, out["reward"], out["info"], out["fail"], out["diffs"], out["done"], out["end"], out["percent"])
        untouched(b"kp_sim_post_step")
        assert np.array_equal(host(c["_cur_t_dev"]), before)
        if badT < 1:
            with pytest.raises(kp.KinPolyNativeError):
                sim.obs_ar(ctx, out["obs"])
            untouched(b"kp_sim_obs_ar")
    ctx = _make_ctx(sim, c)
    other = torch.zeros(n, dtype=torch.int32, device="cuda")
    with pytest.raises(kp.KinPolyNativeError, match="cur_t"):          # POST increments the buffer the context reads
        sim.post_step(ctx, cfg, other, row_len, 5, out["reward"], out["info"], out["fail"], out["diffs"], out["done"], out["end"], out["percent"])
    untouched(b"kp_sim_post_step")
    ctx.action_one_hot = None
    with pytest.raises(kp.KinPolyNativeError, match="action_one_hot"):
        sim.post_step(ctx, cfg, c["_cur_t_dev"], row_len, 5, out["reward"], out["info"], out["fail"], out["diffs"], out["done"], out["end"], out["percent"], None, out["obj7"])
    untouched(b"kp_sim_post_step")
    with pytest.raises(kp.KinPolyNativeError):
        sim.obs_ar(ctx, out["obs"])
    untouched(b"kp_sim_obs_ar")
    for name in ("head_pose", "gt_bquat", "gt_wbpos", "cur_t"):
        ctx = _make_ctx(sim, c); setattr(ctx, name, None)
        with pytest.raises(kp.KinPolyNativeError):
            sim.term_reward(ctx, cfg, out["reward"], out["info"], out["fail"], out["diffs"])
        untouched(b"kp_sim_term_reward")
    # the record calls: t outside [0, T), sizes <= 0, a destination without its source
    obs = torch.zeros((n, 105), device="cuda"); states = torch.full((n, T, 105), -1.0, device="cuda")
    act = torch.zeros((n, 80), device="cuda"); actions = torch.full((n, T, 80), -1.0, device="cuda")
    for t in (T, T + 4, -1):
        with pytest.raises(kp.KinPolyNativeError):
            kp.record_pre(t, T, obs=obs, states=states)
        assert b"kp_rollout_record_pre" in L.kp_last_error()
        with pytest.raises(kp.KinPolyNativeError):
            kp.record_post(t, T, action=act, actions=actions)
        assert b"kp_rollout_record_post" in L.kp_last_error()
    r = kp.KpRecordPre(n, T, 0, 0, None, None, None, None, None, None, None, None, states.data_ptr(), None, None, None, None)
    assert L.kp_rollout_record_pre_w(C.byref(r), 105, None) == -1 and b"destination without its source" in L.kp_last_error()
    assert L.kp_rollout_record_pre_w(C.byref(r), 104, None) == -1 and b"obs_dim" in L.kp_last_error()
    r = kp.KpRecordPre(0, T, 0, 0, obs.data_ptr(), None, None, None, None, None, None, None, states.data_ptr(), None, None, None, None)
    assert L.kp_rollout_record_pre_w(C.byref(r), 105, None) == -1 and L.kp_rollout_record_pre_w(None, 105, None) == -1
    torch.cuda.synchronize()
    assert (states == -1.0).all() and (actions == -1.0).all()
