"""Generate tests/golden/reward_variants.npz by IMPORTING the reference's Python, as tools/make_golden.py does (where a reference checkout can be
imported; only data is written, no reference source): the reference's own reward functions in fp64 on seeded states,

    uhc/core/reward_function.py        world_rfc_implicit_v1_mul (:56-102), local_rfc_implicit_reward (:172-231), world_rfc_implicit_v2 (:301-372),
                                       world_rfc_implicit_v3 (:376-450)
    kin_poly/core/reward_function.py   dynamic_supervision_v2 (:999-1050)

make_golden.py is imported for its stubs and helpers (its own generation runs only under __main__); the set-up is gen_uhc_expert_reward's: make_env, a
sim.forward() played by this repository's fp64 oracle, get_expert on a seeded 12-frame clip.  No fixture of make_golden.py is written.

UHC cases (arrays over the case axis): rid, name, t (env.cur_t, start_ind 0), qpos, prev_qpos, prev_bquat, the body read-outs xpos / xquat / xipos / com at
qpos, action (zero-padded to 75; action_dim, vf_dim), ws (the reward_weights dict as JSON; jpos_diffw is the array the function used) -> reward, info
(NaN-padded to 6; info_dim).  The expert tables of the clip are e_*; b_diffw is cfg.b_diffw (23).  Kin cases: k_*.

Also written, settings only: tests/golden/uhc_rewards/<reward_id>.yml and tests/golden/kin_poly_reward_v2.yml (write_ymls).

    python tools/make_golden_rewards.py      (from an empty working directory)
"""
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs the reference's absent dependencies, puts the reference and this repository on sys.path)

from uhc.core import reward_function as uhc_rf  # noqa: E402
from uhc.utils.tools import get_expert  # noqa: E402
from kin_poly.core.reward_function import dynamic_supervision_v2  # noqa: E402

NB = G.NB
UHC_FUNCS = {"world_rfc_implicit_v1_mul": uhc_rf.world_rfc_implicit_v1_mul, "local_rfc_implicit": uhc_rf.local_rfc_implicit_reward,
             "world_rfc_implicit_v2": uhc_rf.world_rfc_implicit_v2, "world_rfc_implicit_v3": uhc_rf.world_rfc_implicit_v3}
# one non-default weight set per function (every key the function reads)
NON_DEFAULT = {
    "world_rfc_implicit_v1_mul": dict(k_p=1.5, k_v=0.01, k_e=8.0, k_c=300.0, k_vf=0.7),
    "local_rfc_implicit": dict(w_p=0.3, w_v=0.15, w_e=0.25, w_rp=0.12, w_rv=0.08, w_vf=0.1, k_p=1.0, k_v=0.01, k_e=10.0, k_vf=0.5, k_rh=100.0, k_rq=50.0, k_rl=2.0, k_ra=0.25),
    "world_rfc_implicit_v2": dict(k_p=0.8, k_wp=0.3, k_v=0.01, k_j=40.0, k_c=60.0, k_vf=0.5, jpos_diffw=[round(0.5 + 0.05 * b, 2) for b in range(24)]),
    "world_rfc_implicit_v3": dict(w_p=0.3, w_wp=0.2, w_v=0.1, w_j=0.25, w_c=0.1, w_vf=0.05, k_p=0.8, k_wp=0.3, k_v=0.01, k_j=40.0, k_c=60.0, k_vf=0.5,
                                  jpos_diffw=[round(1.5 - 0.04 * b, 2) for b in range(24)]),
}


def z_quat(angle):
    return np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)])


def turned(rng, bquat, s=0.02):
    """every quaternion of a [96] record turned by a small random rotation (stays unit: the reference takes acos of the difference's w)"""
    return np.concatenate([G.quaternion_multiply(G.quat_from_expmap(rng.normal(size=3) * s), bquat[4 * b: 4 * b + 4]) for b in range(24)])


def uhc_env_and_clip(rng):
    env = G.make_env(G.him.HumanoidEnv)
    env.frame_skip = 15
    env.cur_t, env.start_ind = 0, 0
    o = G.OracleSim()

    class Sim:
        def get_state(self): return None
        def set_state(self, st): pass
        def forward(self_inner):
            o.reset(env.data.qpos[:76].copy(), np.zeros(75))
            d = env.data
            d.body_xpos = np.vstack([np.zeros((1, 3)), o.get("xpos").reshape(NB, 3)])
            d.body_xquat = np.vstack([[[1, 0, 0, 0]], o.get("xquat").reshape(NB, 4)])
            d.xipos = np.vstack([np.zeros((1, 3)), o.get("xipos").reshape(NB, 3)])
            d.subtree_com = np.vstack([o.get("subtree_com")[None], np.zeros((24, 3))])
    env.sim = Sim()
    d = G.FakeData(); d.qpos = np.zeros(76); d.qvel = np.zeros(75)
    d.get_body_xipos = lambda name: d.xipos[(["world"] + G.NAMES).index(name)]
    env.data = d
    T = 12
    base = G.rand_qpos(rng, 0.3)
    clip = np.tile(base, (T, 1))
    for t in range(T):                               # a smooth clip around one pose, the root turning about z
        clip[t, :3] = base[:3] + 0.02 * t * np.array([1.0, 0.5, 0.1])
        clip[t, 3:7] = G.quaternion_multiply(z_quat(0.05 * t), base[3:7])
        clip[t, 7:] = base[7:] + 0.1 * np.sin(0.5 * t + np.arange(69))
    clip[:, 7 + 20] = np.linspace(3.0, 3.4, T)       # a joint crossing pi
    expert = get_expert(clip.copy(), {"cyclic": False, "seq_name": "synthetic"}, env)
    env.expert = expert
    return env, clip, expert


def uhc_states(rng, clip, expert):
    """(name, t, qpos, prev_qpos, prev_bquat) of the states every function is called on"""
    T = clip.shape[0]
    bq = np.asarray(expert["bquat"])

    def near(t, s=1.0):
        q = clip[min(t, T - 1)] + np.concatenate([rng.normal(size=3) * 0.02 * s, np.zeros(4), rng.normal(size=69) * 0.05 * s])
        q[3:7] = G.quaternion_multiply(q[3:7], G.quat_from_expmap(rng.normal(size=3) * 0.05 * s))
        q[3:7] /= np.linalg.norm(q[3:7])
        p = clip[min(t, T - 1) - 1] + np.concatenate([rng.normal(size=3) * 0.01 * s, np.zeros(4), rng.normal(size=69) * 0.03 * s])
        p[3:7] /= np.linalg.norm(p[3:7])
        return q, p

    out = []
    for name, t in (("plain", 4), ("plain_late", 9), ("last_row", T - 1), ("past_the_end", T + 2)):      # the last two: get_expert_index clamps to row T - 1
        q, p = near(t)
        out.append((name, t, q, p, turned(rng, bq[min(t, T - 1) - 1])))
    t = 5                                             # the state IS the expert: every distance that compares like with like is 0
    out.append(("expert", t, clip[t].copy(), clip[t - 1].copy(), bq[t - 1].copy()))
    q, p = near(6)                                    # the root quaternion and the whole previous record with the opposite sign
    q[3:7] *= -1.0
    out.append(("sign_flip", 6, q, p, -turned(rng, bq[5])))
    q, p = near(7)                                    # joints crossing +-pi between prev_qpos and qpos
    p[7 + 20], q[7 + 20] = 3.13, -3.12
    p[7 + 41], q[7 + 41] = -3.14, 3.135
    out.append(("joint_pi", 7, q, p, turned(rng, bq[6])))
    for name, ang in (("heading_pi", np.pi - 5e-4), ("heading_minus_pi", -np.pi + 5e-4)):      # root heading within 1e-3 of +-pi
        q, p = near(8)
        q[3:7] = G.quaternion_multiply(z_quat(ang), G.quat_from_expmap(np.array([0.05, -0.03, 0.0])))
        p[3:7] = G.quaternion_multiply(z_quat(ang - 0.02), G.quat_from_expmap(np.array([0.04, -0.03, 0.0])))
        out.append((name, 8, q, p, turned(rng, bq[7])))
    return out


def gen_uhc(out):
    rng = np.random.default_rng(4242)
    env, clip, expert = uhc_env_and_clip(rng)
    b_diffw = G.KPM["uhc_b_diffw"][1:].copy()
    out["clip"], out["b_diffw"], out["dt"] = clip, b_diffw, np.float64(env.dt)      # env.dt = model.opt.timestep * frame_skip, not exactly 1 / 30
    for k in ("qvel", "rlinv_local", "rangv", "rq_rmh", "com", "body_com", "ee_pos", "ee_wpos", "bquat", "bangvel", "wbpos", "wbquat"):
        out["e_" + k] = np.asarray(expert[k])
    states = uhc_states(rng, clip, expert)
    rec = {k: [] for k in ("rid", "name", "t", "qpos", "prev_qpos", "prev_bquat", "xpos", "xquat", "xipos", "com", "action", "action_dim", "vf_dim", "ws",
                           "jpos_diffw", "reward", "info", "info_dim")}
    for rid, fn in UHC_FUNCS.items():
        # (state, weights, vf_dim): every state with the defaults and residual force on; then the other weight set, vf_dim 0 and (local) w_vf 0
        plan = [(s, {}, 6) for s in states] + [(states[1], NON_DEFAULT[rid], 6), (states[0], {}, 0), (states[4], NON_DEFAULT[rid], 0)]
        if rid == "local_rfc_implicit":
            plan += [(states[0], {"w_vf": 0.0}, 6), (states[1], {**NON_DEFAULT[rid], "w_vf": 0.0}, 0)]
        for (name, t, q, p, pbq), ws, vf_dim in plan:
            env.cfg = types.SimpleNamespace(reward_weights=dict(ws), b_diffw=b_diffw.copy(), obs_coord="root")
            env.vf_dim = vf_dim
            env.data.qpos = q.copy(); env.data.qvel = np.zeros(75)
            env.sim.forward()
            env.cur_t, env.prev_qpos, env.prev_bquat = t, p.copy(), pbq.copy()
            adim = 69 + vf_dim
            action = np.zeros(adim) if name == "expert" else rng.normal(size=adim) * 0.3
            r, info = fn(env, None, action.copy(), None)
            rec["rid"].append(rid); rec["name"].append(name); rec["t"].append(t)
            rec["qpos"].append(q); rec["prev_qpos"].append(p); rec["prev_bquat"].append(pbq)
            rec["xpos"].append(env.data.body_xpos[1:25].reshape(-1).copy()); rec["xquat"].append(env.data.body_xquat[1:25].reshape(-1).copy())
            rec["xipos"].append(env.data.xipos[1:25].reshape(-1).copy()); rec["com"].append(env.data.subtree_com[0].copy())
            rec["action"].append(np.concatenate([action, np.zeros(75 - adim)])); rec["action_dim"].append(adim); rec["vf_dim"].append(vf_dim)
            rec["ws"].append(json.dumps({k: v for k, v in ws.items() if k != "jpos_diffw"}))
            rec["jpos_diffw"].append(np.asarray(ws.get("jpos_diffw", [1.0] * 24), dtype=np.float64))
            rec["reward"].append(r); rec["info"].append(np.concatenate([info, np.full(6 - len(info), np.nan)])); rec["info_dim"].append(len(info))
    out.update({k: np.array(v) if k in ("rid", "name", "ws") else np.stack(v) for k, v in rec.items()})


def gen_kin(out):
    """dynamic_supervision_v2 on the set-up of make_golden.gen_ar_obs_reward; cur_t at 1 and at T - 1 among the cases"""
    rng = np.random.default_rng(4343)
    hum = G.make_humanoid()
    T = 6
    env = G.make_env(G.har.HumanoidAREnv)
    env.smpl_humanoid = hum
    env.frame_skip = 15
    env.cc_cfg.b_diffw = G.KPM["uhc_b_diffw"][1:].copy()
    rec = {k: [] for k in ("t", "qpos", "xpos", "xquat", "prev_bquat", "head_pose", "gt_bquat", "gt_wbpos", "ws", "reward", "info")}
    custom = dict(w_hp=0.15, w_hq=0.15, w_p=0.3, w_v=0.1, w_e=0.3, k_hp=45.0, k_hq=45.0, k_p=1.0, k_v=0.01, k_e=5.0)
    for i, (t, ws) in enumerate([(1, {}), (T - 1, {}), (3, {}), (1, custom), (T - 1, custom), (2, custom), (4, {}), (3, custom)]):
        gt_qpos = np.stack([G.rand_qpos(rng, 0.2) for _ in range(T)])
        for f in range(1, T):                         # a smooth ground truth, so that its finite-difference velocities are those of a motion
            gt_qpos[f] = gt_qpos[0] + 0.03 * f * np.concatenate([np.array([1.0, 0.4, 0.05]), np.zeros(4), np.sin(np.arange(69) + f)])
            gt_qpos[f, 3:7] = G.quaternion_multiply(z_quat(0.04 * f), gt_qpos[0, 3:7])
        gt = hum.qpos_fk_batch(gt_qpos)
        q0 = gt_qpos[t] + np.concatenate([rng.normal(size=3) * 0.02, np.zeros(4), rng.normal(size=69) * 0.05])
        if i == 6:
            q0[3:7] *= -1.0                           # the root quaternion with the sign opposite to the ground truth's
        env.data = G.oracle_data(q0, rng.normal(size=75) * 0.3)
        head = np.concatenate([gt["wbpos"].reshape(T, 24, 3)[:, 13] + rng.normal(size=(T, 3)) * 0.02, gt["wbquat"].reshape(T, 24, 4)[:, 13]], 1)
        env.ar_context = dict(head_pose=head, qpos=gt_qpos, bquat=gt["bquat"].reshape(T, -1), wbquat=gt["wbquat"].reshape(T, -1), wbpos=gt["wbpos"].reshape(T, -1))
        env.kin_cfg = types.SimpleNamespace(policy_specs={"reward_weights": dict(ws)})
        env.cur_t = t
        env.prev_bquat = turned(rng, gt["bquat"].reshape(T, -1)[t - 1])
        env.prev_hpos = head[t - 1].copy()
        r, info = dynamic_supervision_v2(env, None, None, {"end": False})
        d = env.data
        rec["t"].append(t); rec["qpos"].append(d.qpos[:76].copy()); rec["xpos"].append(d.body_xpos[1:25].reshape(-1).copy())
        rec["xquat"].append(d.body_xquat[1:25].reshape(-1).copy()); rec["prev_bquat"].append(env.prev_bquat.copy()); rec["head_pose"].append(head)
        rec["gt_bquat"].append(env.ar_context["bquat"]); rec["gt_wbpos"].append(env.ar_context["wbpos"]); rec["ws"].append(json.dumps(ws))
        rec["reward"].append(r); rec["info"].append(info)
    out.update({"k_" + k: np.array(v) if k == "ws" else np.stack(v) for k, v in rec.items()})


def write_ymls():
    """settings-only files, written from this repository's own fixtures: uhc.yml (uhc_variants/uhc_meta_pd.yml without meta_pd) with each reward_id and
    no reward_weights, so that every key is the function's default; kin_poly.yml (kin_poly_wo_action.yml with use_action on) with dynamic_supervision_v2
    and two of its weights"""
    import yaml
    base = yaml.safe_load(open(os.path.join(G.OUT, "uhc_variants", "uhc_meta_pd.yml")))
    base.pop("meta_pd"); base.pop("reward_weights")
    os.makedirs(os.path.join(G.OUT, "uhc_rewards"), exist_ok=True)
    for rid in UHC_FUNCS:
        with open(os.path.join(G.OUT, "uhc_rewards", rid + ".yml"), "w") as f:
            f.write(f"# uhc.yml with reward_id {rid} and no reward_weights: the function's own defaults (tools/make_golden_rewards.py)\n")
            yaml.safe_dump({**base, "reward_id": rid}, f, sort_keys=False, default_flow_style=None)
    kin = yaml.safe_load(open(os.path.join(G.OUT, "kin_poly_wo_action.yml")))
    kin["use_action"] = True
    kin["policy_specs"]["reward_id"] = "dynamic_supervision_v2"
    kin["policy_specs"]["reward_weights"] = {"w_p": 0.5, "k_e": 10.0}          # the other eight keys: dynamic_supervision_v2's defaults
    with open(os.path.join(G.OUT, "kin_poly_reward_v2.yml"), "w") as f:
        f.write("# kin_poly.yml with policy_specs.reward_id dynamic_supervision_v2 and two of its weights (tools/make_golden_rewards.py)\n")
        yaml.safe_dump(kin, f, sort_keys=False, default_flow_style=None)


if __name__ == "__main__":
    write_ymls()
    out = {}
    gen_uhc(out)
    gen_kin(out)
    path = os.path.join(G.OUT, "reward_variants.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes;", len(out["rid"]), "UHC cases,", len(out["k_t"]), "kin cases")
