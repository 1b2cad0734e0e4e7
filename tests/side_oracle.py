"""fp64 references and input generators for the kernels around the control step (observation, reward, termination, GAE, GRU gates,
MCP mixing).  Not a test module: tests/test_side_oracle_cpu.py checks these helpers without a GPU, tests/test_gpu_side_kernels.py
compares the HIP kernels with them.  Everything is built on oracle/np_oracle.py (pinned to the reference by tests/test_oracle_golden.py)
wherever a function exists there.  Quaternions are (w, x, y, z)."""
import math

import numpy as np

from oracle import np_oracle as O

EPS32 = float(np.finfo(np.float32).eps)
DT = 1.0 / 30.0


# ------------------------------------------------------------------ GAE (k_gae)
def gae_ref(rewards, masks, values, last_values, gamma, tau):
    """[n, T] fp64 -> (adv, ret), un-normalised, per env.  O.estimate_advantages on every row; the bootstrap of the comment above k_gae
    (prev_value starts at last_values[e] instead of 0, prev_adv at 0) is one extra row behind the last with reward = value = last_values[e]:
    its own delta is 0, so its advantage is 0 and it hands exactly `last_values[e]` to the row before it."""
    rewards, masks, values = (np.asarray(a, np.float64) for a in (rewards, masks, values))
    n, T = rewards.shape
    adv = np.zeros((n, T)); ret = np.zeros((n, T))
    for e in range(n):
        r, m, v = rewards[e], masks[e], values[e]
        if last_values is not None:
            lv = float(last_values[e])
            r, m, v = np.append(r, lv), np.append(m, 1.0), np.append(v, lv)
        with np.errstate(all="ignore"):                 # the reference's normalisation (unused here) divides by the std of one row when T = 1
            _, rt = O.estimate_advantages(r[:, None], m[:, None], v[:, None], gamma, tau)
        ret[e] = rt[:T, 0]
        adv[e] = rt[:T, 0] - v[:T]
    return adv, ret


def gae_bound(ret_ref, T, gamma, tau):
    """|adv - adv_ref| <= 8 eps32 S min(T, 1 / (1 - gamma tau)), S = max(1, |ret|_max): each step rounds a handful of fp32 operations on values
    of size S and the recursion amplifies them by at most 1 / (1 - gamma tau)."""
    S = max(1.0, float(np.abs(ret_ref).max()))
    gt = gamma * tau
    amp = T if gt >= 1.0 else min(T, 1.0 / (1.0 - gt))
    return 8.0 * EPS32 * S * amp


# ------------------------------------------------------------------ GRU gates (k_gru_gates_fwd / k_gru_gates_bwd)
def _gates(torch, gi, gh, hm_prev):
    H = hm_prev.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    nn = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return r, z, nn, (1.0 - z) * nn + z * hm_prev               # torch.nn.GRUCell


def _t64(torch, a):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float64))


def gru_gates_fwd_ref(gi, gh, hm_prev, next_keep=None):
    """(h, hm_next) in fp64: the GRUCell formulas; hm_next = h * next_keep[e] (h when next_keep is None)."""
    import torch
    gi, gh, hm_prev, next_keep = (_t64(torch, a) for a in (gi, gh, hm_prev, next_keep))
    h = _gates(torch, gi, gh, hm_prev)[3]
    hm = h if next_keep is None else h * next_keep[:, None]
    return h.numpy(), hm.numpy()


def gru_gates_bwd_ref(gi, gh, hm_prev, dh_out=None, carry=None, carry_keep=None):
    """(dgi, dgh, dhz) in fp64 by autograd on the GRUCell formulas with dh = dh_out + carry * carry_keep[e] (null terms are 0, a null
    carry_keep is 1); dhz is the gradient that reaches hm_prev directly (dh * z)."""
    import torch
    gi, gh, hm_prev, dh_out, carry, carry_keep = (_t64(torch, a) for a in (gi, gh, hm_prev, dh_out, carry, carry_keep))
    gi = gi.clone().requires_grad_(True); gh = gh.clone().requires_grad_(True); hp = hm_prev.clone().requires_grad_(True)
    h = _gates(torch, gi, gh, hp)[3]
    dh = torch.zeros_like(h) if dh_out is None else dh_out.clone()
    if carry is not None:
        dh = dh + (carry if carry_keep is None else carry * carry_keep[:, None])
    h.backward(dh)
    return gi.grad.numpy(), gh.grad.numpy(), hp.grad.numpy()


# ------------------------------------------------------------------ PolicyMCP mixing (k_mcp_compose)
def mcp_compose_ref(logits, prim, noise=None, std=None):
    """logits [n, K], prim [K, n, A] -> [n, A]: softmax over K (max subtracted, uhc/core/policy_mcp.py:30-38) mixing the primitives, + std * noise."""
    logits, prim = np.asarray(logits, np.float64), np.asarray(prim, np.float64)
    w = np.exp(logits - logits.max(1, keepdims=True)); w /= w.sum(1, keepdims=True)
    out = np.einsum("nk,kna->na", w, prim)
    if noise is not None:
        out = out + np.asarray(std, np.float64)[None, :] * np.asarray(noise, np.float64)
    return out


# ------------------------------------------------------------------ termination + reward (k_term_reward<POST>)
ACTION_START = (0, 7, 21, 28)          # action_index_map (humanoid_ar_v1.py:37-39): first column of the action's object in data.qpos[76:111]


def term_reward_ref(state, ctx, cfg, diffw, post=None, margin=1e-3):
    """k_term_reward as its header comment states it, per env in fp64.
    state: dict of [n, .] arrays qpos, xpos, xquat, t_wbpos, t_bquat, prev_bquat, prev_hpos (what the kernel reads from the simulator);
    ctx: dict T, head_pose [R,T,7], gt_bquat [R,T,96], gt_wbpos [R,T,72], action_one_hot [R,4], cur_t [n], row [n] or None;
    cfg: dict of the reward weights (O.REWARD_WEIGHTS) + dt, thresh, gt_thresh, use_gt;
    post (POST = true): dict row_len [R], episode_len, and optionally obj7 [n,7] (the rows before the call) with sim_obj_qpos [n,35].
    Rows whose bd / bgd lies within `margin` of its threshold are refused (AssertionError): no test row may sit on that knife edge."""
    n, T = len(state["qpos"]), int(ctx["T"])
    row = np.arange(n) if ctx.get("row") is None else np.asarray(ctx["row"])
    out = dict(reward=np.zeros(n), info=np.zeros((n, 6)), fail=np.zeros(n, bool), diffs=np.zeros((n, 2)))
    if post is not None:
        out.update(cur_t=np.zeros(n, np.int64), end=np.zeros(n, bool), done=np.zeros(n, bool), percent=np.zeros(n),
                   obj7=None if post.get("obj7") is None else np.array(post["obj7"], np.float64))
    gtb = np.asarray(ctx["gt_bquat"], np.float64)
    for e in range(n):
        r = int(row[e])
        t_now = int(ctx["cur_t"][e]) + (1 if post is not None else 0)
        t = min(max(t_now, 1), T - 1)                                            # the previous ground-truth row is t - 1 >= 0
        qpos = np.asarray(state["qpos"][e], np.float64)
        xpos = np.asarray(state["xpos"][e], np.float64).reshape(24, 3); xquat = np.asarray(state["xquat"][e], np.float64).reshape(24, 4)
        tgt = dict(wbpos=np.asarray(state["t_wbpos"][e], np.float64).reshape(24, 3), bquat=np.asarray(state["t_bquat"][e], np.float64))
        head = np.concatenate([xpos[13], xquat[13]])
        rew, inf = O.dynamic_supervision_v1(head, np.asarray(state["prev_hpos"][e], np.float64), O.get_body_quat(qpos), np.asarray(state["prev_bquat"][e], np.float64),
                                            xpos, tgt, np.asarray(ctx["head_pose"][r, t], np.float64), gtb[r, t], gtb[r, t - 1], cfg["dt"], cfg)
        bd = O.calc_body_diff(xpos, tgt["wbpos"], diffw)
        bgd = O.calc_body_diff(xpos, np.asarray(ctx["gt_wbpos"][r, t], np.float64).reshape(24, 3), diffw)
        if np.isfinite(bd):
            assert abs(bd - cfg["thresh"]) > margin and (not cfg["use_gt"] or abs(bgd - cfg["gt_thresh"]) > margin), (e, bd, bgd)
        fail = bool(bd > cfg["thresh"]) or bool(cfg["use_gt"] and bgd > cfg["gt_thresh"]) or not (bd == bd)     # a NaN pose fails the episode
        out["reward"][e], out["info"][e], out["fail"][e], out["diffs"][e] = rew, inf, fail, (bd, bgd)
        if post is not None:                                                     # the tail of HumanoidAREnv.step (humanoid_ar_v1.py:288-316)
            clen = int(post["row_len"][r])
            end = t_now >= min(clen, int(post["episode_len"]))
            out["cur_t"][e], out["end"][e], out["done"][e], out["percent"][e] = t_now, end, fail or end, t_now / clen
            if out["obj7"] is not None:                                          # get_obj_qpos(action_one_hot): rows without an action keep theirs
                hot = np.flatnonzero(np.asarray(ctx["action_one_hot"][r]) != 0)
                if len(hot):
                    st = ACTION_START[int(hot[0])]
                    out["obj7"][e] = np.asarray(post["sim_obj_qpos"][e], np.float64)[st:st + 7]
    if post is not None:
        out["done_count"] = int(out["done"].sum())
    return out


def reward_cfg(use_gt=True):
    """KpRewardCfg.default() as the dict term_reward_ref takes"""
    return dict(O.REWARD_WEIGHTS, dt=DT, thresh=10.0, gt_thresh=12.0, use_gt=bool(use_gt))


# ------------------------------------------------------------------ generators of edge rows
def yawed(q, h):
    """rotation by h about z in front of q: the heading (O.get_heading, math.py:118-127) of the result is the heading of q plus h"""
    w1, z1 = math.cos(h / 2), math.sin(h / 2)
    w2, x2, y2, z2 = q
    return np.array([w1 * w2 - z1 * z2, w1 * x2 - z1 * y2, w1 * y2 + z1 * x2, w1 * z2 + z1 * w2])


def random_qpos(n, seed, base_qpos, noise=0.3):
    """well-conditioned rows: the standing pose + N(0, noise) joint angles, a random unit root quaternion near upright, root position N(0, 1)"""
    rng = np.random.default_rng(seed)
    q = np.tile(np.asarray(base_qpos, np.float64), (n, 1))
    q[:, :2] += rng.normal(size=(n, 2)); q[:, 2] += rng.normal(size=n) * 0.1
    q[:, 7:] += rng.normal(size=(n, 69)) * noise
    for i in range(n):
        tilt = O.quat_from_expmap(rng.normal(size=3) * 0.3)
        q[i, 3:7] = O.quaternion_multiply(yawed(tilt, rng.uniform(-np.pi, np.pi)), q[i, 3:7])
    return q


def edge_qpos(n, seed, base_qpos):
    """random_qpos rows turned into edges, cycling over four kinds (row i has kind i % 4):
      0  non-unit root quaternion (norm 0.25 .. 4): qpos_fk divides by the norm (numpy_smpl_humanoid.py:194-196), quaternion_inverse by the
         dot product and quaternion_matrix rescales by sqrt(2 / dot) (transformation.py:1267-1292) -- none of them may assume a unit input;
      1  joint angles uniform in +-3 pi: quaternion_from_euler takes sin / cos of the half angle (transformation.py:1194-1250), where an fp32
         argument reduction of 4.7 rad has fewer digits left than one of 0.3 rad;
      2  heading of the base-rotation-free root within 1e-6 of +pi (w of the heading quaternion ~ 0): get_heading's 2 acos(w) (math.py:118-127)
         is at its best conditioned there but get_heading_q's normalisation divides by |(w, z)| with w cancelling;
      3  the same at -pi + 1e-6, reached from the other side (z < 0, the sign flip of get_heading)."""
    rng = np.random.default_rng(seed + 7)
    q = random_qpos(n, seed, base_qpos)
    for i in range(n):
        k = i % 4
        if k == 0:
            q[i, 3:7] *= 2.0 ** rng.uniform(-2, 2)
        elif k == 1:
            q[i, 7:] = rng.uniform(-3 * np.pi, 3 * np.pi, 69)
        else:
            h0 = O.get_heading(O.remove_base_rot(q[i, 3:7]))
            want = (np.pi - 1e-6 * rng.uniform(0.1, 1.0)) * (1 if k == 2 else -1)
            q[i, 3:7] = yawed(q[i, 3:7], want - h0)
    return q


def rel_heading(q, tq):
    """target heading minus current heading of the base-rotation-free root quaternions, before the wrap (humanoid_im.py:185-190)"""
    return O.get_heading(O.remove_base_rot(tq[3:7])) - O.get_heading(O.remove_base_rot(q[3:7]))


def heading_safe_targets(q, tq, margin=1e-2):
    """The rows of tq [n, 76], each turned about z by the first of (0, 0.7, 1.9, -1.3) rad that keeps its relative heading to the row of q at least
    `margin` away from +-pi, where the wrap of humanoid_im.py:185-190 (rel_h > pi: -= 2 pi; < -pi: += 2 pi) would make an fp32 and an fp64 evaluation
    differ by 2 pi.  The rows are rounded to fp32 before they are judged (what the kernel is given); asserted for every row."""
    out = np.array(tq, np.float64)
    for i in range(len(q)):
        for turn in (0.0, 0.7, 1.9, -1.3):
            cand = out[i].copy(); cand[3:7] = yawed(cand[3:7], turn)
            cand = cand.astype(np.float32).astype(np.float64)
            if abs(abs(rel_heading(q[i], cand)) - np.pi) > margin:
                break
        assert abs(abs(rel_heading(q[i], cand)) - np.pi) > margin, i
        out[i] = cand
    return out


def small_turn_qvel(qpos, act):
    """angular part of the finite-difference velocity of one step_ar frame, analytically: the step turns the root by the rotation vector dt * R(rot) w
    (humanoid_ar_v1.py:216-241), so rotation vector / dt taken into the current root frame (transform_vec 'root', math.py:45-65) is R^T R w.  Exact for
    any turn below pi; used where get_qvel_fd_new's `1 - |w| < 1e-8 -> no rotation` cut-off (turns under 2.8e-4 rad) hides the true small velocity."""
    return O.transform_vec(O.quat_mul_vec(qpos[3:7], act[77:80]), qpos[3:7], "root")


ANGLE_EDGES = (0.0, 1e-8, 1e-4, np.pi - 1e-3, np.pi + 1e-3, 2 * np.pi - 1e-3, 2 * np.pi + 1e-3)


def kin_actions(n, seed, edges=False, dt=DT):
    """[n, 80] kinematic-policy actions (z, root quaternion slot, 69 joint angles, local linear velocity, local angular velocity).
    edges: row i turns by dt |w| = ANGLE_EDGES[i % 7] -- exactly 0 and 1e-8 (quat_from_expmap's angle < 1e-12 branch and its neighbour, math.py:188-198),
    1e-4 (below rotation_from_quaternion's 1 - |w| < 1e-8 cut-off, transformation.py:348-356), and within 1e-3 of pi and of 2 pi (w of the step
    quaternion ~ 0 and ~ -1: get_qvel_fd's wrap to (-pi, pi], math.py:45-65)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 80)) * 0.3
    a[:, 0] = 0.9 + rng.normal(size=n) * 0.05
    if edges:
        for i in range(n):
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            a[i, 77:80] = ax * (ANGLE_EDGES[i % len(ANGLE_EDGES)] / dt)
    return a


def body_quat_edges(qpos, seed):
    """Ground-truth body quaternions [n, 96] for the rows of qpos, cycling over (row i has kind i % 4): 0 random unit quaternions; 1 exactly the body's own
    (O.get_body_quat: multi_quat_norm_v2 is 0 and rotation_from_quaternion sees w = 1, transformation.py:348-356); 2 exactly minus it (|w| - 1 = 0 again:
    q and -q are one rotation, math_utils.py:111-118); 3 random with every second body negated."""
    rng = np.random.default_rng(seed)
    n = len(qpos)
    out = np.zeros((n, 96))
    for i in range(n):
        own = O.get_body_quat(np.asarray(qpos[i], np.float64)).reshape(24, 4)
        rnd = rng.normal(size=(24, 4)); rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
        k = i % 4
        g = rnd if k == 0 else own if k == 1 else -own if k == 2 else rnd * np.where(np.arange(24) % 2, -1.0, 1.0)[:, None]
        out[i] = g.reshape(-1)
    return out


def zfilter_edges(raw, clip, seed):
    """(mean, std) for a ZFilter over the columns of raw [n, D] (zfilter.py:58-67: (x - mean) / (std + 1e-8), clipped): a third of the columns has
    std = 0 exactly (the division is by 1e-8 alone, and mean = the column of row 0, so that row gives 0 / 1e-8 = 0 and the others saturate at +-clip), a
    third is placed so that row 0 lands on +clip or -clip exactly in fp64 (mean = x - +-clip * std with std a power of two), the rest is ordinary."""
    rng = np.random.default_rng(seed)
    D = raw.shape[1]
    mean, std = rng.normal(size=D), rng.uniform(0.1, 2.0, D)
    kind = np.arange(D) % 3
    std[kind == 0] = 0.0; mean[kind == 0] = raw[0, kind == 0]
    std[kind == 1] = 2.0 ** rng.integers(-2, 2, (kind == 1).sum())
    sgn = np.where(rng.random(D) < 0.5, -1.0, 1.0)
    mean[kind == 1] = raw[0, kind == 1] - (sgn * clip * std)[kind == 1]
    return mean, std
