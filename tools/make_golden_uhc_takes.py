"""Write tests/golden/uhc_takes_small.pkl: a small take pickle in the schema DatasetAMASSSingle reads ({take: {pose_aa, pose_6d, trans, qpos}}), six takes
built from tests/golden/standing_neutral.npz with seeded joint sinusoids and a slow root drift, of 20, 95, 96, 130, 200 and 64 frames -- so that
t_min: 90 drops two and the kept four differ in length.  Arrays, names and numbers only.

    python tools/make_golden_uhc_takes.py
"""
import os

import joblib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
LENGTHS = {"take_a_20": 20, "take_b_95": 95, "take_c_96": 96, "take_d_130": 130, "take_e_200": 200, "take_f_64": 64}


def make_takes():
    std = np.load(os.path.join(OUT, "standing_neutral.npz"))["qpos"].reshape(-1)[:76].astype(np.float64)
    rng = np.random.default_rng(2024)
    takes = {}
    for name, T in LENGTHS.items():
        amp, freq, ph = rng.uniform(0, 0.12, 69), rng.uniform(0.2, 1.0, 69), rng.uniform(0, 2 * np.pi, 69)
        t = np.arange(T)[:, None] / 30.0
        qpos = np.tile(std, (T, 1))
        qpos[:, 7:] += amp * (np.sin(2 * np.pi * freq * t + ph) - np.sin(ph))
        qpos[:, :2] += t * rng.uniform(-0.05, 0.05, 2)                   # slow root drift
        yaw = 0.1 * t[:, 0] * rng.uniform(-1, 1)
        qz = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], 1)
        w0, x0, y0, z0 = std[3:7]
        w1, x1, y1, z1 = qz.T                                           # qz (x) root
        qpos[:, 3:7] = np.stack([w1 * w0 - x1 * x0 - y1 * y0 - z1 * z0, w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0,
                                 w1 * y0 - x1 * z0 + y1 * w0 + z1 * x0, w1 * z0 + x1 * y0 - y1 * x0 + z1 * w0], 1)
        takes[name] = {"pose_aa": np.zeros((T, 72), np.float32), "pose_6d": np.zeros((T, 144), np.float32), "trans": qpos[:, :3].astype(np.float32),
                       "qpos": qpos.astype(np.float32), "obj_pose": qpos.astype(np.float32)}
    return takes




# ---------------------------------------------------------------------------------------------------------------------------------------------
# tests/golden/uhc_takes.npz: fp64 values from the reference's own Python (imported from a reference checkout, as tools/make_golden.py does; only arrays
# and numbers are written).  sim.forward() is played by this repository's fp64 oracle.
#
#     python tools/make_golden_uhc_takes.py --npz
DERIVED = ("com", "ee_pos", "rq_rmh", "qvel", "rlinv_local", "bangvel")      # rlinv / rangv are qvel[:, :3] / [:, 3:6]; the FK tables are checked bit for bit against kp_sim_fk
STEP_N, STEP_T, STEP_STEPS = 8, 12, 8


def step_clips():
    """the clips of the fused-step test: 8 clips of 12 frames (tiled over 64 envs by the test), float32 values"""
    std = np.load(os.path.join(OUT, "standing_neutral.npz"))["qpos"]
    rng = np.random.default_rng(11)
    clips = np.tile(std, (STEP_N, STEP_T, 1))
    clips[:, :, 7:] += rng.uniform(0, 0.1, (STEP_N, 1, 69)) * np.sin(0.3 * np.arange(STEP_T)[None, :, None] + rng.uniform(0, 6, (STEP_N, 1, 69)))
    actions = (np.random.default_rng(5).normal(size=(STEP_STEPS, STEP_N, 75)) * 0.1).astype(np.float32)
    return clips.astype(np.float32), actions


FREQ_CASES = {
    "empty": {"take_b_95": [], "take_c_96": [], "take_d_130": [], "take_e_200": []},
    "all_successes": {"take_b_95": [[1.0, 0]] * 5, "take_c_96": [[1.0, 0]] * 40, "take_d_130": [[1.0, 0]], "take_e_200": [[1.0, 0]] * 12},
    "mixed": {"take_b_95": [], "take_c_96": [[1.0, 0]] * 7, "take_d_130": [[1.0, 0] if i % 3 else [0.4, 0] for i in range(40)], "take_e_200": [[0.3, 0], [1.0, 0]]},
}


def reference_env(frame_skip=15):
    """(G, env, o, load): a HumanoidEnv of the reference whose sim.forward() is this repository's fp64 oracle `o` (load(env.data) copies o's bodies in), for
    the reference's get_expert; env.dt is the reference's property timestep * frame_skip.  tools/make_golden_take_edges.py runs on the same scaffolding."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden as G
    env = G.make_env(G.him.HumanoidEnv)
    env.frame_skip = frame_skip
    env.cur_t, env.start_ind = 0, 0
    o = G.OracleSim()

    def load(d):
        d.body_xpos = np.vstack([np.zeros((1, 3)), o.get("xpos").reshape(24, 3)])
        d.body_xquat = np.vstack([[[1, 0, 0, 0]], o.get("xquat").reshape(24, 4)])
        d.xipos = np.vstack([np.zeros((1, 3)), o.get("xipos").reshape(24, 3)])
        d.subtree_com = np.vstack([o.get("subtree_com")[None], np.zeros((24, 3))])

    class Sim:
        def get_state(self): return None
        def set_state(self, st): pass
        def forward(self_inner):
            o.reset(env.data.qpos[:76].copy(), np.zeros(75))
            load(env.data)
    env.sim = Sim()
    d = G.FakeData(); d.qpos = np.zeros(76); d.qvel = np.zeros(75)
    d.get_body_xipos = lambda name: d.xipos[(["world"] + G.NAMES).index(name)]
    env.data = d
    return G, env, o, load


def write_npz():
    import json
    import types
    G, env, o, load = reference_env()
    from uhc.utils.tools import get_expert
    from uhc.core.reward_function import world_rfc_implicit_reward
    from uhc.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from oracle import np_oracle as O
    out = {}
    takes = make_takes()
    for k, (name, tk) in enumerate(takes.items()):
        ex = get_expert(tk["qpos"].astype(np.float64), {"cyclic": False, "seq_name": name}, env)
        for t in DERIVED:
            out[f"t{k}_{t}"] = np.asarray(ex[t], np.float64)
        out[f"t{k}_height_lb"], out[f"t{k}_head_height_lb"] = np.float64(ex["height_lb"]), np.float64(ex["head_height_lb"])
    out["take_names"] = np.array(list(takes.keys()))
    # the fused-step test: the fp64 trajectory of each clip under the recorded actions, with reward / terms / body_diff of the reference at every step
    clips, actions = step_clips()
    env.cfg = types.SimpleNamespace(reward_weights=dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=2.0, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0),
                                    b_diffw=G.KPM["uhc_b_diffw"][1:].copy())
    rew, info, bd = np.zeros((STEP_STEPS, STEP_N)), np.zeros((STEP_STEPS, STEP_N, 5)), np.zeros((STEP_STEPS, STEP_N))
    for c in range(STEP_N):
        clip = clips[c].astype(np.float64)
        ex = get_expert(clip.copy(), {"cyclic": False, "seq_name": f"step{c}"}, env)
        env.expert = ex
        o.reset(clip[0], np.asarray(ex["qvel"][0]))
        for s in range(STEP_STEPS):
            env.prev_bquat = O.get_body_quat(o.get("qpos"))
            a = actions[s, c].astype(np.float64)
            o.do_simulation(a, clip[s], 15)
            env.data.qpos, env.data.qvel = o.get("qpos").copy(), o.get("qvel").copy()
            load(env.data)
            env.cur_t = s + 1
            r, i5 = world_rfc_implicit_reward(env, None, a, None)
            rew[s, c], info[s, c], bd[s, c] = r, i5, env.calc_body_diff()
    assert np.abs(bd - 0.5).min() >= 1e-3, "a compared step comes within 1e-3 of the body_diff threshold: choose other clips"
    out.update(step_clips=clips, step_actions=actions, step_reward=rew, step_info=info, step_body_diff=bd)
    # sample_seq's init_probs (dataset_amass_single.py:162-175) for recorded freq_dicts: the reference's own code, its draw intercepted
    ds = DatasetAMASSSingle.__new__(DatasetAMASSSingle)
    ds.data_keys = list(FREQ_CASES["empty"].keys())
    ds.data = {k2: {k: takes[k][k2] for k in ds.data_keys} for k2 in ("qpos", "pose_aa", "pose_6d", "trans")}
    ds.data["obj_pose"] = ds.data["qpos"]
    ds.t_min, ds.t_max = 90, -1
    import numpy.random as npr
    seen = {}
    real_choice, real_binom = npr.choice, npr.binomial
    try:
        npr.binomial = lambda *a, **k: 1
        def choice(keys, p=None):
            seen["p"] = np.asarray(p, np.float64).copy()
            return keys[0]
        npr.choice = choice
        for case, fd in FREQ_CASES.items():
            ds.sample_seq(full_sample=True, freq_dict=fd)
            out[f"probs_{case}"] = seen["p"]
    finally:
        npr.choice, npr.binomial = real_choice, real_binom
    out["freq_cases"] = np.array(json.dumps(FREQ_CASES))
    np.savez_compressed(os.path.join(OUT, "uhc_takes.npz"), **out)
    print(os.path.getsize(os.path.join(OUT, "uhc_takes.npz")), "bytes")


if __name__ == "__main__":
    import sys
    if "--npz" in sys.argv:
        write_npz()
    else:
        joblib.dump(make_takes(), os.path.join(OUT, "uhc_takes_small.pkl"), compress=3)
        print(os.path.getsize(os.path.join(OUT, "uhc_takes_small.pkl")), "bytes")
