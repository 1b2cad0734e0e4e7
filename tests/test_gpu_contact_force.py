"""Contact-force read-out (kp_sim_contact_forces) on a real MI355X: the kernel against the fp64 reference
tests/contact_force_oracle.py on identical fp32 state values, exact identities of its own outputs, bitwise consistency (controller, mask, neighbours,
non-interference with the control step), the refusals, the envs and the evaluation's grf records.

Parity tolerances = 4 x the largest deviation measured on the MI355X over the states below (the factor leaves room for another Newton path from another
warm start); every figure is printed before it is asserted.  Body weight m g = 787.7 N."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import contact_force_oracle as CF  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402
from oracle.kpo import OracleSim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPMS = {DEFAULT_KPM: read_kpm(DEFAULT_KPM), STEP_KPM: read_kpm(STEP_KPM)}
BODY_WEIGHT = float(KPMS[DEFAULT_KPM]["body_mass"].sum()) * 9.81
N_ENVS = (1, 5, 67)
OUT_KEYS = ("ncon", "contact", "wrench", "qfrc_constraint", "qacc", "torque", "obj_qacc")

# 4 x the largest deviation from the oracle measured on the MI355X over all states, scenes, modes and env counts of test_parity (measured value in the
# comment; body weight 787.7 N).  The entity forces are looser than the per-contact ones because of scene (h): the 2 t table's 22 kN floor reaction is an
# entity force whose fp32 rounding alone is 2e-3 N per contact.
TOL_F_CONTACT = 4 * 5.93e-3   # N, per-contact forces; measured 5.93e-3 N = 7.5e-6 of body weight -> 3.0e-5 of body weight
TOL_F = 4 * 4.80e-2           # N, entity forces; measured 4.80e-2 N = 6.1e-5 of body weight (scene h, the table; 5.1e-3 N on the humanoid's bodies) -> 2.4e-4 of body weight
TOL_TAU = 4 * 4.34e-2         # N m, entity torques about the world origin; measured 4.34e-2 (scene h; 3.0e-3 on the floor states)
TOL_QFRC = 4 * 5.08e-3        # N / N m, qfrc_constraint; measured 5.08e-3
TOL_QACC = 4 * 1.69e-2        # rad/s^2 (m/s^2), qacc; measured 1.69e-2 on accelerations up to 1.0e3
TOL_TORQUE = 4 * 3.68e-4      # N m, the controller's torque (mode 2); measured 3.20e-4 (default controller), 3.68e-4 (meta-PD against tests/uhc_ctrl_oracle.py)
TOL_OBJ_QACC = 4 * 5.74e-4    # object accelerations; measured 5.74e-4
MEASURED = H.Measured()


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------- states

_STATES = {}


def states(kp, scene):
    """list of dict(name, q, v, qd, vd, blk, slots) with fp32-representable values; scene: floor | parked | g_sit | h_push"""
    if scene in _STATES:
        return _STATES[scene]
    if scene in ("floor", "parked"):
        fl = CF.floor_states(KPMS[DEFAULT_KPM], STD["qpos"], STD["qvel"])
        out = [dict(name=k, q=f32(q), v=f32(v), qd=f32(q), vd=f32(v)) for k, (q, v) in fl.items()]
        # (b): standing after 30 zero-action control steps on the device (state and derived state differ there)
        sim = kp.KpSim(kp.KpModel(), 1)
        q0 = dev(out[0]["q"][None]); sim.set_state(q0, dev(out[0]["v"][None])); sim.set_target(q0)
        z = torch.zeros((1, 75), device="cuda")
        for _ in range(30):
            sim.step_ctrl(z, 15)
        g = {k: sim.get(k)[0].double().cpu().numpy() for k in ("qpos", "qvel", "qpos_d", "qvel_d")}
        out.insert(1, dict(name="b_settled", q=g["qpos"], v=g["qvel"], qd=g["qpos_d"], vd=g["qvel_d"]))
        for s in out:
            s["blk"], s["slots"] = (f32(CF.parked_block()), {}) if scene == "parked" else (None, {})
    else:
        q, v, blk, slots = CF.object_scenes(KPMS[STEP_KPM], STD["qpos"])[scene]
        out = [dict(name=scene, q=f32(q), v=f32(v), qd=f32(q), vd=f32(v), blk=f32(blk), slots=slots)]
    _STATES[scene] = out
    return out


def blob(scene):
    return DEFAULT_KPM if scene == "floor" else STEP_KPM


def inputs(name, width=75):
    """the seeded action / torque / PD target of a state"""
    rng = np.random.default_rng(sum(map(ord, name)))
    action = f32(rng.normal(size=width) * 0.3)
    torque = f32(np.concatenate([rng.normal(size=6) * 10.0, rng.normal(size=69) * 20.0]))
    target = f32(STD["qpos"] + np.concatenate([np.zeros(7), rng.normal(size=69) * 0.1]))
    return action, torque, target


def make_sim(kp, scene, sts, **opts):
    """a handle holding state sts[e] in env e"""
    n = len(sts)
    sim = kp.KpSim(kp.KpModel(blob(scene), **opts), n)
    if sts[0]["blk"] is not None:
        sim.set_objects(dev(np.stack([s["blk"] for s in sts])))
    st = lambda k: dev(np.stack([s[k] for s in sts]))  # noqa: E731
    sim.set_state(st("q"), st("v"))                               # zeroes the warm start
    sim.set_full_state(st("q"), st("v"), st("qd"), st("vd"))
    sim.set_target(dev(np.stack([inputs(s["name"])[2] for s in sts])))
    return sim


def call(sim, sts, mode, env_mask=None, want=OUT_KEYS, width=75):
    if mode == 0:
        out = sim.contact_forces(env_mask=env_mask, want=want)
    elif mode == 1:
        out = sim.contact_forces(torque=dev(np.stack([inputs(s["name"])[1] for s in sts])), env_mask=env_mask, want=want)
    else:
        out = sim.contact_forces(action=dev(np.stack([inputs(s["name"], width)[0] for s in sts])), env_mask=env_mask, want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


_GPU, _REF = {}, {}


def gpu_out(kp, scene, n, mode, stale=1):
    key = (scene, n, mode, stale)
    if key not in _GPU:
        base = states(kp, scene)
        if not stale:
            base = [s for s in base if s["name"] in ("a_standing", "f_falling")]
        sts = [base[e % len(base)] for e in range(n)]
        sim = make_sim(kp, scene, sts, **({} if stale else {"stale_kinematics": 0}))
        _GPU[key] = (sts, call(sim, sts, mode))
        assert int(sim.diag()[:, 2].max()) == 0
    return _GPU[key]


def oracle_ref(scene, s, mode, stale=1):
    key = (blob(scene), s["name"], mode, stale)
    if key not in _REF:
        kpm = KPMS[blob(scene)]
        o = OracleSim(kpm=blob(scene), ls_exact=True)
        for slot, oi in s["slots"].items():
            o.set_object(slot, kpm, oi, s["blk"][7 * oi: 7 * oi + 7])
        if stale:
            o.reset(s["qd"], s["vd"]); o.set_state_raw(s["q"], s["v"])
        else:
            o.reset(s["q"], s["v"])
        action, torque, target = inputs(s["name"])
        _REF[key] = CF.oracle_contact_forces(o, mode, torque if mode == 1 else action, target, kpm)
    return _REF[key]


def rows_of(out, e):
    n = int(out["ncon"][e]); c = out["contact"][e].astype(np.float64)
    return dict(body=c[:n, 0].astype(int), b2=c[:n, 1].astype(int), dist=c[:n, 2], pos=c[:n, 3:6], normal=c[:n, 6:9], force=c[:n, 9:12])


_LOCAL = {}


def note(key, v):
    MEASURED.note(key, v, _LOCAL)


# ---------------------------------------------------------------- 4. parity

PARITY = [(sc, n, 1) for sc in ("floor", "parked", "g_sit", "h_push") for n in N_ENVS] + [("floor", 5, 0)]


@pytest.mark.parametrize("scene,n,stale", PARITY)
def test_parity(kp, scene, n, stale):
    unmatched_with_force = 0
    _LOCAL.clear()
    for mode in (0, 1, 2):
        sts, out = gpu_out(kp, scene, n, mode, stale)
        for e, s in enumerate(sts):
            ref = oracle_ref(scene, s, mode, stale)
            if s["name"] == "d_lying":
                assert len(ref["force"]) >= 12, "the lying state must hold at least 12 contacts on the oracle side"
            got = rows_of(out, e)
            pairs, only_got, only_ref = CF.match_contacts(got, ref["contacts"])
            for i, j in pairs:
                note("contact_force", np.abs(got["force"][i] - ref["force"][j]).max())
            for i in only_got:
                note("unmatched_force", np.abs(got["force"][i]).max()); unmatched_with_force += np.abs(got["force"][i]).max() > TOL_F_CONTACT
            for j in only_ref:
                note("unmatched_force", np.abs(ref["force"][j]).max()); unmatched_with_force += np.abs(ref["force"][j]).max() > TOL_F_CONTACT
            note("wrench_force", np.abs(out["wrench"][e][:, :3] - ref["wrench"][:, :3]).max())
            note("wrench_torque", np.abs(out["wrench"][e][:, 3:] - ref["wrench"][:, 3:]).max())
            note("qfrc_constraint", np.abs(out["qfrc_constraint"][e] - ref["qfrc_constraint"]).max())
            note("qacc", np.abs(out["qacc"][e] - ref["qacc"]).max())
            note("torque", np.abs(out["torque"][e] - ref["torque"]).max())
            note("obj_qacc", np.abs(out["obj_qacc"][e] - ref["obj_qacc"]).max())
    print(f"parity {scene} n={n} stale={stale}: " + ", ".join(f"{k} {v:.3e}" for k, v in _LOCAL.items()) + " || running maxima " + ", ".join(f"{k} {v:.3e}" for k, v in MEASURED.items()) +
          f" | force / body weight {max(MEASURED.get('contact_force', 0), MEASURED.get('wrench_force', 0)) / BODY_WEIGHT:.2e}")
    assert unmatched_with_force == 0, "a contact present on one side only must carry no force"
    assert MEASURED.get("contact_force", 0) <= TOL_F_CONTACT and MEASURED["wrench_force"] <= TOL_F and MEASURED["wrench_torque"] <= TOL_TAU
    assert MEASURED["qfrc_constraint"] <= TOL_QFRC and MEASURED["qacc"] <= TOL_QACC and MEASURED["torque"] <= TOL_TORQUE and MEASURED["obj_qacc"] <= TOL_OBJ_QACC
    assert max(MEASURED.get("contact_force", 0), MEASURED["wrench_force"]) <= 1e-3 * BODY_WEIGHT


# ---------------------------------------------------------------- 5. identities of the device output alone

@pytest.mark.parametrize("scene", ["floor", "parked", "g_sit", "h_push"])
def test_identities(kp, scene):
    worst = 0.0
    for mode in (0, 1, 2):
        sts, out = gpu_out(kp, scene, 67, mode)
        for e, s in enumerate(sts):
            c = rows_of(out, e)
            n = len(c["body"])
            assert not out["contact"][e][n:].any(), "rows >= ncon are exactly zero"
            bound = 1e-5 * np.abs(c["force"]).sum() + 1e-5
            w = out["wrench"][e].astype(np.float64)
            d1 = np.abs(out["qfrc_constraint"][e][:3] - w[:24, :3].sum(0)).max()
            host = CF.entity_wrenches(c, c["force"])
            d2 = np.abs(w - host)
            assert d1 <= bound and d2.max() <= bound, (s["name"], mode, d1, d2.max(), bound)
            worst = max(worst, d1 / bound, d2[:, :3].max() / bound)
            for k in (24, 25):                     # the object entity's force is the negative of what the other side received from it
                on_obj = sum((-c["force"][i] for i in range(n) if c["b2"][i] == k), np.zeros(3)) + sum((c["force"][i] for i in range(n) if c["body"][i] == k), np.zeros(3))
                assert np.abs(w[k, :3] - on_obj).max() <= bound
            if s["name"] == "c_airborne":
                assert n == 0 and not out["wrench"][e].any() and not out["qfrc_constraint"][e].any() and not out["contact"][e].any()
                assert np.isfinite(out["qacc"][e]).all()
    print(f"identities {scene}: worst deviation / bound {worst:.3f}")


# ---------------------------------------------------------------- 6. controller consistency

def _bits_equal(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k], b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]), k


def test_controller_torque_round_trip_is_bitwise(kp):
    sts = [states(kp, "floor")[e % 6] for e in range(5)]
    sim = make_sim(kp, "floor", sts)
    m2 = call(sim, sts, 2)
    m1 = {k: v.cpu().numpy() for k, v in sim.contact_forces(torque=dev(m2["torque"])).items()}
    _bits_equal(m2, m1, ("ncon", "contact", "wrench", "qfrc_constraint", "qacc", "torque"))
    assert np.abs(m2["torque"]).max() > 1.0


def test_extended_controller_round_trip_and_torque(kp):
    from oracle import np_spd
    from uhc_ctrl_oracle import compute_torque_xc
    kpm = KPMS[DEFAULT_KPM]
    sts = [states(kp, "floor")[e % 6] for e in range(5)]
    sim = make_sim(kp, "floor", sts, cc_action_v=1, cc_rfc=1, cc_meta_pd=1)
    A = 69 + 6 + 30
    assert sim.cc_action_dim == A
    acts = []
    for s in sts:
        a = inputs(s["name"], A)[0].copy()
        a[75:] = f32(np.random.default_rng(len(s["name"])).uniform(-1.3, 1.5, 30))
        acts.append(a)
    m2 = {k: v.cpu().numpy() for k, v in sim.contact_forces(action=dev(np.stack(acts))).items()}
    m1 = {k: v.cpu().numpy() for k, v in sim.contact_forces(torque=dev(m2["torque"])).items()}
    _bits_equal(m2, m1, ("ncon", "contact", "wrench", "qfrc_constraint", "qacc", "torque"))
    worst = 0.0
    for e, s in enumerate(sts):
        o = OracleSim()
        o.reset(s["qd"], s["vd"])
        tau = compute_torque_xc(s["q"], s["v"], o.fullM(), o.get("qfrc_bias"), acts[e], inputs(s["name"])[2][7:], kpm, 1, 1, 1, 0)
        tau = np.clip(tau, -kpm["torque_lim"], kpm["torque_lim"])
        worst = max(worst, np.abs(m2["torque"][e][6:] - tau).max(), np.abs(m2["torque"][e][:6] - np_spd.rfc_implicit_np(s["q"], acts[e][69:75], kpm)).max())
    print(f"extended controller: torque of mode 2 against the controller oracle, substep 0: {worst:.3e} N m")
    assert worst <= TOL_TORQUE


# ---------------------------------------------------------------- 7. non-interference

@pytest.mark.parametrize("scene", ["floor", "h_push"])
def test_read_out_leaves_the_control_step_bit_identical(kp, scene):
    base = states(kp, scene)
    sts = [base[e % len(base)] for e in range(67)]
    sims = [make_sim(kp, scene, sts, queue_slots=16) for _ in range(2)]        # 67 envs on 16 wave slots: the job queue (lean layout on the floor handle)
    act = dev(np.stack([inputs(s["name"])[0] for s in sts]))

    def between(sim):
        a = sim.contact_forces(action=act)
        b = sim.contact_forces(action=act)
        for k in a:
            assert torch.equal(a[k], b[k]), f"the same call twice: {k}"
    H.control_step_untouched(kp, scene, between, pair=(sims, act))


# ---------------------------------------------------------------- 8. mask

def test_mask_and_neighbours(kp):
    base = states(kp, "floor")
    sts = [base[e % 6] for e in range(67)]
    mask = np.random.default_rng(8).random(67) < 0.6
    mask[:6] = True
    sim = make_sim(kp, "floor", sts)
    out = call(sim, sts, 2, env_mask=dev(mask, torch.uint8))
    for k, v in out.items():
        assert not v[~mask].any(), f"masked-out rows of {k} are zero"
    for e in range(6):                                 # every state alone on a one-env handle: the same bits
        one = call(make_sim(kp, "floor", [sts[e]]), [sts[e]], 2)
        for k in OUT_KEYS:
            assert np.array_equal(out[k][e], one[k][0]), (sts[e]["name"], k)
    assert out["ncon"][0] == 11 and out["ncon"][2] == 0


# ---------------------------------------------------------------- 9. refusals

def test_refusals(kp):
    sts = [states(kp, "floor")[0]] * 5
    sim = make_sim(kp, "floor", sts)
    before = call(sim, sts, 2)
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    bufs, full = H.sentinel(kp.CONTACT_OUTPUTS, kp.KpContactOut)
    act = dev(np.zeros((5, 75)))
    ap = ctypes.c_void_p(act.data_ptr())
    assert L.kp_sim_contact_forces(None, 0, None, None, ctypes.byref(full)) != 0 and "null handle" in err()
    assert L.kp_sim_contact_forces(sim.h, 0, None, None, None) != 0 and "null out" in err()
    assert L.kp_sim_contact_forces(sim.h, 0, None, None, ctypes.byref(kp.KpContactOut())) != 0 and "every output of out is null" in err()
    for bad in (-1, 3):
        assert L.kp_sim_contact_forces(sim.h, bad, ap, None, ctypes.byref(full)) != 0 and "actuation" in err()
    for mode in (1, 2):
        assert L.kp_sim_contact_forces(sim.h, mode, None, None, ctypes.byref(full)) != 0 and "act is null" in err()
    wide = kp.KpSim(kp.KpModel(threads_per_env=128), 5)
    assert L.kp_sim_contact_forces(wide.h, 0, None, None, ctypes.byref(full)) != 0 and "threads_per_env" in err()
    H.refused_calls_wrote_nothing(bufs)
    with pytest.raises(ValueError):
        sim.contact_forces(action=act, torque=act)
    after = call(sim, sts, 2)
    for k in OUT_KEYS:
        assert np.array_equal(before[k], after[k]), k


# ---------------------------------------------------------------- 10. envs

def test_ar_env_contact_forces(kp):
    from kinpoly_amd.env import BatchedHumanoidAREnv, standing_context
    n = 5
    torch.manual_seed(0)
    env = BatchedHumanoidAREnv(n, 0, mode="test", seed=0)
    env.load_context(standing_context(n, 8, STD["qpos"], STD["qvel"], env.sim))
    env.reset()
    with pytest.raises(RuntimeError, match="step"):
        env.contact_forces()
    _, _, _, info = env.step(torch.zeros((n, 80), device=env.device))
    a, b = env.contact_forces(), env.sim.contact_forces(action=info["cc_action"])
    assert set(a) == set(OUT_KEYS)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["ncon"].min()) > 0 and float(a["wrench"][:, :24, 2].sum(1).min()) > 0.2 * BODY_WEIGHT


def test_uhc_env_contact_forces(kp):
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv
    n = 5
    env = BatchedHumanoidEnv(n, 0)
    env.load_expert(torch.tensor(np.tile(STD["qpos"], (n, 6, 1)), dtype=torch.float32))
    env.reset()
    with pytest.raises(RuntimeError, match="step"):
        env.contact_forces()
    act = torch.zeros((n, 75), device=env.device)
    env.step(act)
    a, b = env.contact_forces(), env.sim.contact_forces(action=act)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["ncon"].min()) > 0


# ---------------------------------------------------------------- 11. evaluation

def test_run_sequences_grf(kp):
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.env import BatchedHumanoidAREnv, standing_context
    from kinpoly_amd.evaluate import GRF_KEYS, run_sequences
    from kinpoly_amd.metrics import grf_metrics
    n, T = 2, 8
    torch.manual_seed(3)
    env = BatchedHumanoidAREnv(n, 0, mode="test", seed=3)
    env.load_context(standing_context(n, T, STD["qpos"], STD["qvel"], env.sim))
    net = TrajARNet().to(env.device)
    keys = ["take-0", "take-1"]
    plain = run_sequences(env, net, keys)
    with_grf = run_sequences(env, net, keys, grf=True)
    again = run_sequences(env, net, keys, grf=False)
    for k in keys:
        assert set(plain[k]) == {"target", "pred", "obj_pose", "percent", "fail_safe"} and set(with_grf[k]) == set(plain[k]) | set(GRF_KEYS)
        L = len(with_grf[k]["pred"])
        r = with_grf[k]
        assert r["grf"].shape == (L, 2, 3) and r["cop"].shape == (L, 2, 2) and r["foot_contact"].shape == (L, 2) and r["foot_contact"].dtype == bool and r["load"].shape == (L, 26)
        for other in (again[k], {x: with_grf[k][x] for x in plain[k]}):
            assert other["percent"] == plain[k]["percent"] and other["fail_safe"] == plain[k]["fail_safe"]
            for x in ("target", "pred", "obj_pose"):
                assert len(other[x]) == len(plain[k][x]) and all(np.array_equal(p, q) for p, q in zip(other[x], plain[k][x])), x
    m = grf_metrics(with_grf, BODY_WEIGHT)
    assert m["frames"] == sum(len(r["pred"]) for r in with_grf.values()) and np.isfinite(m["grf_mean_bw"])
