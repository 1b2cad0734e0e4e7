"""Impulse pushes (kp_sim_apply_impulse) on a real MI355X: the kernel against the fp64 reference tests/push_oracle.py
(OracleSim's own kinematics and solveM), the bitwise invariants, object pushes, the control step after a push, launch-form independence, and
the envs / PushSchedule on top.  Every test prints the figure it asserts on."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import push_oracle as PO  # noqa: E402
from kinpoly_amd.model_compiler import STEP_KPM, read_kpm  # noqa: E402
from oracle.kpo import OracleSim  # noqa: E402

STD = np.load(os.path.join(os.path.dirname(__file__), "golden", "standing_neutral.npz"))

# Relative infinity-norm bound of a pushed velocity jump against the fp64 reference, |dv_gpu - dv_ref|_inf / |dv_ref|_inf, for tests 1 - 3.
# Measured on MI355X over the seeded inputs of this file: worst 7.5e-6 (humanoid, 48 envs: dqvel 7.504e-6, the stored KP_QVEL 7.490e-6), 7.3e-7 (objects),
# 1.5e-6 (two pushes against their sum); the constant is 4 x the worst, rounded up to one digit.  The first-order ceiling of a backward-stable fp32 solve
# of this matrix is cond(M) 2^-23 ~ 1e-3: an error near that would be a bug, not a tolerance.
PUSH_TOL = 3e-5


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def f32(a):
    """the fp32 rounding of a: device and reference then start from the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


def _quat(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def six_poses(seed=3):
    """standing; lying on the back; a deep squat; root yaw at exactly pi; hinge angles spread over +-3 pi on the left arm chain; joints uniform in +-1.2 rad"""
    rng = np.random.default_rng(seed)
    std = STD["qpos"].copy()
    lying = std.copy(); lying[2] = 0.25; lying[3:7] = _quat([0, 1, 0], -np.pi / 2)
    squat = std.copy(); squat[2] = 0.55
    for hip, knee, ankle in ((1, 2, 3), (5, 6, 7)):            # the x hinge (third of z, y, x) of hip, knee and ankle
        squat[7 + 3 * (hip - 1) + 2] = -1.6; squat[7 + 3 * (knee - 1) + 2] = 2.2; squat[7 + 3 * (ankle - 1) + 2] = -0.7
    yaw = std.copy(); yaw[3:7] = [np.cos(np.pi / 2), 0.0, 0.0, 1.0]
    arm = std.copy(); arm[7 + 3 * 13: 7 + 3 * 18] = np.linspace(-3 * np.pi, 3 * np.pi, 15)      # L_Thorax .. L_Hand
    rnd = std.copy(); rnd[7:] = rng.uniform(-1.2, 1.2, 69); rnd[3:7] = _quat(rng.normal(size=3), 0.9)
    return f32(np.stack([std, lying, squat, yaw, arm, rnd]))


def rel_inf(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_body_pushes_match_the_oracle(kp):
    """Test 1: 24 bodies x 2 poses drawn from the six, random offsets within 0.15 m, |p| <= 60 N s, |l| <= 5 N m s, random qvel: dqvel and the
    new KP_QVEL against push_oracle.delta_qvel, every env."""
    rng = np.random.default_rng(17)
    poses = six_poses()
    n = 48
    body = np.repeat(np.arange(24), 2)
    pidx = np.concatenate([rng.choice(6, 2, replace=False) for _ in range(24)])
    assert set(pidx) == set(range(6))
    qpos = poses[pidx]
    qvel = f32(rng.normal(size=(n, 75)) * 0.5)
    off = f32(rng.uniform(-0.15, 0.15, (n, 3)))
    d = rng.normal(size=(n, 3)); p = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 60, (n, 1))
    d = rng.normal(size=(n, 3)); l = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 5, (n, 1))
    imp = f32(np.concatenate([p, l], 1))
    sim = kp.KpSim(kp.KpModel(), n)
    sim.set_state(dev(qpos), dev(qvel))
    v0 = sim.get("qvel").clone()
    dq = sim.apply_impulse(dev(body, torch.int32), dev(imp), dev(off), want_dqvel=True)
    v1 = sim.get("qvel")
    assert torch.equal(v1, v0 + dq)                              # the store is one fp32 add of the jump
    dq = dq.double().cpu().numpy()
    o = OracleSim(contact=False, limits=False)
    worst = worst_v = 0.0
    for e in range(n):
        ref = PO.delta_qvel(o, qpos[e], body[e], off[e], imp[e])
        err = rel_inf(dq[e], ref)
        worst = max(worst, err)
        print(f"env {e:2d} body {body[e]:2d} pose {pidx[e]} |dv|inf {np.abs(ref).max():.3f} rel err {err:.2e}")
        assert err < PUSH_TOL, (e, body[e], pidx[e], err)
        err_v = rel_inf(v1[e].double().cpu().numpy() - qvel[e], ref)
        worst_v = max(worst_v, err_v)
        assert err_v < PUSH_TOL, (e, body[e], pidx[e], err_v)
    print(f"worst relative error over {n} envs: dqvel {worst:.3e}, new KP_QVEL {worst_v:.3e} (bound {PUSH_TOL:g})")


def _stepped(kp, n, seed, model=None, steps=1):
    rng = np.random.default_rng(seed)
    qpos = np.tile(STD["qpos"], (n, 1)); qpos[:, 7:] += np.clip(rng.normal(size=(n, 69)) * 0.1, -1, 1)
    qvel = rng.normal(size=(n, 75)) * 0.3
    act = dev(rng.normal(size=(n, 75)) * 0.2)
    sim = kp.KpSim(model or kp.KpModel(), n)
    sim.set_state(dev(qpos), dev(qvel)); sim.set_target(dev(np.tile(STD["qpos"], (n, 1))))
    for _ in range(steps):
        sim.step_begin()
        sim.step_ctrl(act, 15)
    return sim, act


KEEP = ("qpos", "qpos_d", "qvel_d", "xpos", "target_qpos", "prev_bquat")


def test_bitwise_invariants_and_linearity(kp):
    """Test 2 (N = 5, after one control step so that qpos_d, the warm start and prev_bquat differ from the state)."""
    n = 5
    sim, _ = _stepped(kp, n, 5)
    before = {k: sim.get(k).clone() for k in KEEP + ("qvel",)}
    rng = np.random.default_rng(6)
    imp = rng.normal(size=(n, 6)) * [20, 20, 20, 2, 2, 2]; imp[4] = 0.0
    ent = dev([11, -1, 999, -7, 11], torch.int32)
    mask = dev([0, 1, 1, 1, 1], torch.uint8)
    dq = sim.apply_impulse(ent, dev(imp), dev(rng.uniform(-0.1, 0.1, (n, 3))), env_mask=mask, want_dqvel=True)
    assert torch.equal(sim.get("qvel"), before["qvel"]), "masked-out, entity -1 / 999 / -7 and a zero impulse must leave KP_QVEL bit for bit"
    assert not dq.any()
    # a real push of every env moves KP_QVEL and nothing else
    imp1, imp2 = f32(rng.normal(size=(n, 6)) * [20, 20, 20, 2, 2, 2]), f32(rng.normal(size=(n, 6)) * [20, 20, 20, 2, 2, 2])
    off = dev(rng.uniform(-0.1, 0.1, (n, 3)))
    ent = dev([0, 4, 11, 13, 22], torch.int32)
    d1 = sim.apply_impulse(ent, dev(imp1), off, want_dqvel=True)
    for k in KEEP:
        assert torch.equal(sim.get(k), before[k]), k
    assert (d1.abs().amax(1) > 1e-3).all()
    d2 = sim.apply_impulse(ent, dev(imp2), off, want_dqvel=True)
    two = sim.get("qvel").clone()
    for k in KEEP:
        assert torch.equal(sim.get(k), before[k]), k
    # the same two pushes as one: a handle restored to the state before them
    sim.set_full_state(before["qpos"], before["qvel"], before["qpos_d"], before["qvel_d"])
    d12 = sim.apply_impulse(ent, dev(f32(imp1 + imp2)), off, want_dqvel=True)
    one = sim.get("qvel")
    for e in range(n):
        ref = d12[e].double().cpu().numpy()
        err = rel_inf((d1[e] + d2[e]).double().cpu().numpy(), ref)
        err_v = rel_inf((two[e] - before["qvel"][e]).double().cpu().numpy(), (one[e] - before["qvel"][e]).double().cpu().numpy())
        print(f"env {e}: push(w1) + push(w2) against push(w1 + w2): dqvel {err:.2e}, KP_QVEL {err_v:.2e}")
        assert err < PUSH_TOL and err_v < PUSH_TOL


def _obj_block(n, active):
    blk = np.zeros((n, 35))
    for i in range(5):
        blk[:, 7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    for e, d in enumerate(active):
        for oi, pose in d.items():
            blk[e, 7 * oi: 7 * oi + 7] = pose
    return blk


def test_object_pushes_match_the_oracle(kp):
    """Test 3: the push scene (box = object 1 in slot 0, table = object 2 in slot 1) in every env, env 3 with the box parked (its slot 1 is empty):
    entity 24 and 25 against M_obj^-1 g of OracleSim.object_dyn; the humanoid and every other object row stay bit for bit."""
    n = 4
    rng = np.random.default_rng(9)
    kpm = read_kpm(STEP_KPM)
    x, y = STD["qpos"][0] + 1.2, STD["qpos"][1]
    box = [f32(np.concatenate([[x, y, 0.921], _quat(rng.normal(size=3), 0.4 * (e + 1))])) for e in range(n)]
    tab = [f32(np.concatenate([[x, y, 0.7905], _quat(rng.normal(size=3), 0.3 * (e + 1))])) for e in range(n)]
    blk = _obj_block(n, [{1: box[e], 2: tab[e]} if e < 3 else {2: tab[e]} for e in range(n)])
    sim = kp.KpSim(kp.KpModel(STEP_KPM), n)
    sim.set_objects(dev(blk))
    qpos = np.tile(STD["qpos"], (n, 1)); qvel = rng.normal(size=(n, 75)) * 0.3
    sim.set_state(dev(qpos), dev(qvel))
    ov0 = f32(rng.normal(size=(n, 30)) * 0.2)
    sim.set_obj_state(sim.get("obj_qpos"), dev(ov0))
    hv = sim.get("qvel").clone()
    oracles = []
    for e in range(n):
        o = OracleSim(kpm=STEP_KPM)
        if e < 3:
            o.set_object(0, kpm, 1, box[e]); o.set_object(1, kpm, 2, tab[e])
        else:
            o.set_object(0, kpm, 2, tab[e])
        o.reset(qpos[e], np.zeros(75))
        oracles.append(o)
    worst = 0.0
    for slot in (0, 1):
        imp = f32(rng.normal(size=(n, 6)) * [30, 30, 30, 3, 3, 3])
        off = f32(rng.uniform(-0.15, 0.15, (n, 3)))
        ent = [24 + slot] * 3 + [25]                             # env 3: slot 1 is parked
        prev = sim.get("obj_qvel").clone()
        dq = sim.apply_impulse(dev(ent, torch.int32), dev(imp), dev(off), want_dqvel=True)
        now = sim.get("obj_qvel")
        assert not dq.any() and torch.equal(sim.get("qvel"), hv), "an object push leaves the humanoid alone"
        assert torch.equal(now[3], prev[3]), "a push of a parked slot is a no-op"
        for e in range(3):
            oi = 1 + slot
            ref = PO.object_delta_qvel(oracles[e], slot, (box if slot == 0 else tab)[e], off[e], imp[e])
            got = (now[e, 6 * oi: 6 * oi + 6] - prev[e, 6 * oi: 6 * oi + 6]).double().cpu().numpy()
            err = rel_inf(got, ref)                              # of the stored sum: its own rounding is part of the figure
            worst = max(worst, err)
            print(f"env {e} entity {24 + slot}: |dv|inf {np.abs(ref).max():.3e} rel err {err:.2e}")
            assert err < PUSH_TOL
            keep = [c for c in range(30) if not 6 * oi <= c < 6 * oi + 6]
            assert torch.equal(now[e, keep], prev[e, keep])
    # env 3's only simulated slot is the table in slot 0
    imp = f32(rng.normal(size=(n, 6)) * [30, 30, 30, 3, 3, 3])
    prev = sim.get("obj_qvel").clone()
    sim.apply_impulse(dev([-1, -1, -1, 24], torch.int32), dev(imp))
    now = sim.get("obj_qvel")
    assert torch.equal(now[:3], prev[:3])
    ref = PO.object_delta_qvel(oracles[3], 0, tab[3], np.zeros(3), imp[3])
    err = rel_inf((now[3, 12:18] - prev[3, 12:18]).double().cpu().numpy(), ref)
    print(f"env 3 entity 24 (the table): rel err {err:.2e}; worst object error {max(worst, err):.3e}")
    assert err < PUSH_TOL


def test_next_control_step_follows_the_oracle(kp):
    """Test 4: one control step, a 40 N s horizontal push of the chest, one more control step, on both sides; the bounds are those of
    test_gpu_parity.py::test_contact_matches_oracle (qpos 8e-6, qvel 1e-3).  Without the push the end states differ by more than 10 x that."""
    n = 8
    rng = np.random.default_rng(31)
    qpos = np.tile(STD["qpos"], (n, 1)); qpos[:, 7:] += np.clip(rng.normal(size=(n, 69)) * 0.1, -1, 1)
    for e in range(4, n):                                         # half of them squat a little
        for hip, knee, ankle in ((1, 2, 3), (5, 6, 7)):
            qpos[e, 7 + 3 * (hip - 1) + 2] -= 0.3; qpos[e, 7 + 3 * (knee - 1) + 2] += 0.6; qpos[e, 7 + 3 * (ankle - 1) + 2] -= 0.3
        qpos[e, 2] -= 0.04
    qpos, qvel = f32(qpos), f32(rng.normal(size=(n, 75)) * 0.3)
    act, target = f32(rng.normal(size=(n, 75)) * 0.3), f32(np.tile(STD["qpos"], (n, 1)))
    ang = rng.uniform(0, 2 * np.pi, n)
    imp = f32(np.stack([40 * np.cos(ang), 40 * np.sin(ang), 0 * ang, 0 * ang, 0 * ang, 0 * ang], 1))
    ent = dev([11] * n, torch.int32)
    out = {}
    for pushed in (True, False):
        sim = kp.KpSim(kp.KpModel(), n)
        sim.set_state(dev(qpos), dev(qvel)); sim.set_target(dev(target))
        sim.step_ctrl(dev(act), 15)
        if pushed:
            sim.apply_impulse(ent, dev(imp))
        sim.step_ctrl(dev(act), 15)
        out[pushed] = (sim.get("qpos").double().cpu().numpy(), sim.get("qvel").double().cpu().numpy())
        assert (sim.diag()[:, 3] & 255).max() >= 6               # feet on the floor
    o, o2 = OracleSim(), OracleSim()
    eq = ev = 0.0
    for e in range(n):
        o.reset(qpos[e], qvel[e]); o.do_simulation(act[e], target[e], 15)
        q1, v1 = o.get("qpos"), o.get("qvel")
        dv = PO.delta_qvel(o2, q1, 11, np.zeros(3), imp[e])      # a second oracle: the first one's stale derived arrays stay
        o.set_state_raw(q1, v1 + dv)
        o.do_simulation(act[e], target[e], 15)
        eq = max(eq, float(np.abs(out[True][0][e] - o.get("qpos")).max())); ev = max(ev, float(np.abs(out[True][1][e] - o.get("qvel")).max()))
        assert np.abs(out[False][0][e] - o.get("qpos")).max() > 10 * 8e-6 and np.abs(out[False][1][e] - o.get("qvel")).max() > 10 * 1e-3
    print(f"after the push and one more control step: max |dqpos| {eq:.2e} (bound 8e-6), max |dqvel| {ev:.2e} (bound 1e-3)")
    assert eq < 8e-6 and ev < 1e-3


def test_push_is_launch_form_independent(kp):
    """Test 5: the same pushes on a handle forced onto the job queue / lean layout and on a default handle (one workgroup per env, full layout)."""
    n = 64
    rng = np.random.default_rng(41)
    ent = dev(rng.integers(0, 24, n), torch.int32)
    imp = dev(rng.normal(size=(n, 6)) * [20, 20, 20, 2, 2, 2]); off = dev(rng.uniform(-0.1, 0.1, (n, 3)))
    res = []
    for model in (kp.KpModel(lean_queue=1, queue_slots=24), kp.KpModel()):
        sim, act = _stepped(kp, n, 42, model)
        lean = sim.queue_counters()["lean_layout_next_launch"]
        sim.apply_impulse(ent, imp, off)
        pushed = sim.get("qvel").clone()
        sim.step_begin(); sim.step_ctrl(act, 15)
        res.append((lean, pushed, [sim.get(k).clone() for k in ("qpos", "qvel", "xpos", "xquat", "qpos_d", "qvel_d")]))
        assert int(sim.diag()[:, 2].max() & 1) == 0
    assert torch.equal(res[0][1], res[1][1]), "KP_QVEL after the push"
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b), "the state after the next control step"
    assert res[0][0] and not res[1][0], "the first handle runs the lean job queue, the second one workgroup per env"


# ---------------------------------------------------------------------------------------------------------------- test 6: the envs and the schedule

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PKL = os.path.join(GOLD, "uhc_takes_small.pkl")


def _uhc_env(n, schedule=None):
    from kinpoly_amd.dataset import AmassSingleDataset
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv
    ds = AmassSingleDataset({"file_path": PKL, "test_file_path": PKL, "t_min": 90}, "train")
    env = BatchedHumanoidEnv(n, 0, push_schedule=schedule)
    env.load_takes(ds.to_library(env.sim))
    env.reset()
    return env


def _schedule(n, **kw):
    from kinpoly_amd.push import PushSchedule
    return PushSchedule(**{**dict(n_envs=n, device="cuda", interval=2, bodies=("Chest", "Pelvis"), impulse=(30.0, 40.0), seed=3), **kw})


def test_uhc_env_pushes_at_the_tail_of_step():
    n = 6
    plain, quiet, pushed = _uhc_env(n), _uhc_env(n, _schedule(n, impulse=(0.0, 0.0))), _uhc_env(n, _schedule(n))
    a = torch.zeros((n, 75), device="cuda")
    rewards = {k: [] for k in ("plain", "quiet", "pushed")}
    due = 0
    for step in range(1, 5):
        for name, env in (("plain", plain), ("quiet", quiet), ("pushed", pushed)):
            obs, _, done, info = env.step(a)
            rewards[name].append(info["custom_reward"].clone())
            if name == "pushed":
                got = obs.clone()
                assert torch.equal(env._obs_takes(), got), "the returned observation is that of the state after the push"
                due += int((~done).sum()) if step % 2 == 0 else 0
        if step == 2:                                            # the first push fell due at this step's tail: the velocities the policy sees have jumped
            assert not done.any() and (pushed.sim.get("qvel") - plain.sim.get("qvel")).abs().amax(1).min() > 1e-2
        assert torch.equal(rewards["quiet"][-1], rewards["plain"][-1]), "a schedule of zero impulses changes nothing"
        if step <= 2:                                            # ... and its reward is that of the step that just ended
            assert torch.equal(rewards["pushed"][-1], rewards["plain"][-1]), step
    assert not torch.equal(rewards["pushed"][2], rewards["plain"][2]), "the push arrived: step 3 plays out differently"
    assert int(pushed.push_schedule.count) == due and due >= n
    # push() by hand: the same kernel, between two steps
    ent = torch.full((n,), 11, dtype=torch.int32, device="cuda")
    imp = torch.zeros((n, 6), device="cuda"); imp[:, 0] = 20.0
    v0 = plain.sim.get("qvel").clone()
    plain.push(ent, imp, env_mask=torch.arange(n, device="cuda") % 2 == 0)
    v1 = plain.sim.get("qvel")
    assert torch.equal(v1[1::2], v0[1::2]) and (v1[0::2] - v0[0::2]).abs().amax(1).min() > 1e-2


def test_ar_env_pushes_at_the_tail_of_step():
    from kinpoly_amd.env import BatchedHumanoidAREnv, standing_context
    n = 4
    envs = {}
    for name, sched in (("plain", None), ("pushed", _schedule(n))):
        torch.manual_seed(0)
        env = BatchedHumanoidAREnv(n, 0, mode="test", seed=0, use_vel=True, push_schedule=sched)     # use_vel: the observation carries KP_QVEL
        env.load_context(standing_context(n, 20, STD["qpos"], STD["qvel"], env.sim))
        env.reset()
        envs[name] = env
    from oracle import np_oracle as O
    a = torch.zeros((n, 80), device="cuda")                      # the kinematic action that keeps the standing pose (what a trained policy emits)
    cur = STD["qpos"].copy(); cur[3:7] = O.de_heading(cur[3:7])
    a[:, :74] = torch.tensor(cur[2:], dtype=torch.float32, device="cuda")
    for step in range(1, 5):
        out = {}
        for name, env in envs.items():
            obs, _, done, info = env.step(a)
            out[name] = (obs.clone(), info["custom_reward"].clone(), done.clone())
        env = envs["pushed"]
        assert torch.equal(env._obs_ar(env._obs_next), out["pushed"][0]), "the returned observation is that of the state after the push"
        assert torch.equal(out["pushed"][0][:, 74:149], env.sim.get("qvel")), "use_vel: the observation's velocity block is KP_QVEL"
        if step <= 2:
            assert torch.equal(out["pushed"][1], out["plain"][1]), step
        if step == 2:
            assert not out["pushed"][2].any(), "no env ends within two steps of standing"
            dv = (env.sim.get("qvel") - envs["plain"].sim.get("qvel")).abs().amax(1)
            print("AR env: |qvel pushed - qvel plain|inf per env after the first push", dv.tolist(), "pushes drawn", int(env.push_schedule.count))
            assert dv.min() > 1e-2, "the push fell at the tail of step 2"
            assert not torch.equal(out["pushed"][0], out["plain"][0]), "the pushed velocities are in the observation of the same step"
    assert not torch.equal(out["pushed"][1], out["plain"][1]), "the push arrived"
    assert int(envs["pushed"].push_schedule.count) == 2 * n


def test_eval_uhc_under_pushes(tmp_path):
    """scripts/eval_uhc.py with a zero policy: pushes of 1e4 N s at every step end every take early and are logged; pushes of 0 N s leave the
    coverage pickle byte for byte."""
    import pickle
    import subprocess
    import sys
    import joblib
    from kinpoly_amd.nets import PolicyMCP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = str(tmp_path / "iter_0001.p")
    with open(ckpt, "wb") as f:                                  # the zero policy: every weight zero, no running state
        pickle.dump({"policy_dict": {k: torch.zeros_like(v) for k, v in PolicyMCP().state_dict().items()}, "running_state": None}, f)
    run = lambda it, *a: subprocess.run([sys.executable, "scripts/eval_uhc.py", "--mode", "stats", "--ckpt", ckpt, "--takes", PKL, "--iter", str(it), "--data", "usr",      # noqa: E731
                                         "--num_envs", "4", "--no_full", *a], cwd=root, capture_output=True, text=True, timeout=300)
    jobs = {1: (), 2: ("--push_impulse", "0"), 3: ("--push_impulse", "1e4", "--push_interval", "1", "--push_bodies", "Chest")}
    for it, flags in jobs.items():
        p = run(it, *flags)
        assert p.returncode == 0, p.stderr[-2000:]
        if flags:
            assert "pushes applied:" in p.stdout and "coverage under pushes:" in p.stdout
        else:
            assert "pushes" not in p.stdout and not os.path.exists(str(tmp_path / "push_log_1_usr.pkl"))
    raw = [open(str(tmp_path / f"{it}_usr_coverage.pkl"), "rb").read() for it in (1, 2)]
    assert raw[0] == raw[1], "pushes of zero impulse leave the coverage pickle byte for byte"
    cov, log = joblib.load(str(tmp_path / "3_usr_coverage.pkl")), joblib.load(str(tmp_path / "push_log_3_usr.pkl"))
    assert list(log.keys()) == list(cov.keys()) and all(set(v.keys()) == {"percent"} for v in cov.values())
    for k, v in cov.items():
        assert v["percent"] < 1, k
        assert len(log[k]) >= 1 and log[k][0][0] == 1 and log[k][0][1] == "Chest" and len(log[k][0][2]) == 6
        assert abs(np.linalg.norm(log[k][0][2][:3]) - 1e4) < 1.0 and log[k][0][2][2] == 0 and not any(log[k][0][2][3:])
