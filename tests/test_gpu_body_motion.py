"""Body motion, momentum and energy (kp_sim_body_motion) on a real MI355X: the kernel against the fp64 finite-difference reference
tests/body_motion_oracle.py on identical fp32 inputs, bitwise consistency, device-only checks against the mass matrix, the contact solve and the control
step's conservation laws, non-interference, the refusals and the balance scores end to end.

Parity figures are RELATIVE to the row's scale of the quantity, max(1, largest |reference entry| of that quantity in the row): the rows span standing
still to 20 rad/s on every joint and accelerations of 0 to 1e4 rad/s^2, and fp32 rounding scales with the terms.  Tolerances = 4 x the largest figure
measured on the MI355X over the parity tests (the project's convention); every figure is printed, absolute and relative, before it
is asserted."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import body_motion_oracle as BM  # noqa: E402
import contact_force_oracle as CF  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, OPT_FIELDS, STEP_KPM, read_kpm  # noqa: E402
from oracle.kpo import OracleSim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)
MASS = float(KPM["body_mass"].sum())
G = np.asarray(KPM["opt"][1:4], float)
ROWS = (1, 5, 67)
OUT_KEYS = ("body_vel", "body_acc", "body_com_vel", "centroid")
C = BM.CENTROID

# quantity -> (output, columns): what a parity figure is taken over
QUANT = {"w": ("body_vel", slice(0, 3)), "v": ("body_vel", slice(3, 6)), "alpha": ("body_acc", slice(0, 3)), "a": ("body_acc", slice(3, 6)),
         "vc": ("body_com_vel", slice(0, 3)), **{k: ("centroid", s) for k, s in C.items()}}
# 4 x the largest relative deviation measured on the MI355X over test_parity, test_parity_sweep and test_parity_edge_rows (measured value in the comment)
# w 2.8e-7 means: the angular velocities of a row deviate by at most 2.8e-7 of the row's largest one (or of 1 rad/s).  All are a few fp32 roundings of the
# terms involved; the largest, Ldot_com on a_standing at its own forward acceleration (3.4e3 rad/s^2), is 2.5e-4 N m on 43 N m where body terms of
# m r a ~ 5e3 N m cancel: 5e-8 of the terms.
TOL = {
    "w": 4 * 2.775e-07,          # body angular velocity; measured 2.775e-07
    "v": 4 * 6.692e-07,          # body linear velocity; measured 6.692e-07
    "alpha": 4 * 5.481e-07,      # body angular acceleration; measured 5.481e-07
    "a": 4 * 1.607e-06,          # body linear acceleration; measured 1.607e-06
    "vc": 4 * 7.433e-07,         # body centre-of-mass velocity; measured 7.433e-07
    "com": 4 * 6.282e-08,        # measured 6.282e-08
    "com_vel": 4 * 5.865e-07,    # measured 5.865e-07
    "L_com": 4 * 1.074e-06,      # measured 1.074e-06
    "ke": 4 * 6.970e-07,         # measured 6.970e-07
    "pe": 4 * 1.505e-07,         # measured 1.505e-07
    "com_acc": 4 * 2.197e-06,    # measured 2.197e-06
    "Ldot_com": 4 * 5.850e-06,   # measured 5.850e-06
    "mass": 4 * 7.877e-09,       # measured 7.877e-09
}
MEASURED = H.Measured()


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


# ---------------------------------------------------------------- cases: (q, v, a) with the fp64 reference, computed once

_CASES = {}


def cases(scene):
    """list of dict(name, q, v, a, ref); scene: floor (named floor states x qacc_choices) | sweep (64 falling states x {0, N(0, 30^2)}) | edge.
    Inputs are fp32-representable; ref = BM.reference on them."""
    if scene in _CASES:
        return _CASES[scene]
    o = BM.oracle(DEFAULT_KPM)
    out = []

    def add(name, q, v, a):
        a = ID.f32(a)
        out.append(dict(name=name, q=q, v=v, a=a, ref=BM.reference(o, KPM, q, v, a)))

    if scene == "floor":
        for s in ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"])[:-1]:
            f = ID.prepared(DEFAULT_KPM, KPM, s["q"], s["v"])
            for k, a in ID.qacc_choices(f, s["name"]).items():
                add(f"{s['name']}/{k}", s["q"], s["v"], a)
    elif scene == "sweep":
        for s in ID.sweep_states(KPM, STD["qpos"]):
            rng = np.random.default_rng(sum(map(ord, s["name"])) + 2)
            add(s["name"] + "/zero", s["q"], s["v"], np.zeros(75))
            add(s["name"] + "/random", s["q"], s["v"], rng.normal(size=75) * 30.0)
    else:
        rng = np.random.default_rng(4)
        for k, (q, v) in BM.edge_rows(STD["qpos"]).items():
            add(k, q, v, rng.normal(size=75) * 30.0)
    _CASES[scene] = out
    return out


def run(sim, cs, want=OUT_KEYS, qvel=True, qacc=True):
    st = lambda k: dev(np.stack([c[k] for c in cs]))  # noqa: E731
    out = sim.body_motion(st("q"), st("v") if qvel else None, st("a") if qacc else None, outputs=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(out, e, ref, local, absl):
    for k, (o, cols) in QUANT.items():
        got, want = np.atleast_1d(out[o][e][..., cols].astype(np.float64)), np.atleast_1d(ref[o][..., cols])
        d = float(np.abs(got - want).max())
        r = d / max(1.0, float(np.abs(want).max()))
        local[k] = max(local.get(k, 0.0), r); absl[k] = max(absl.get(k, 0.0), d)
        MEASURED[k] = max(MEASURED.get(k, 0.0), r)


def check(label, cs, out, local=None, absl=None, last=True):
    local, absl = {} if local is None else local, {} if absl is None else absl
    for e, c in enumerate(cs):
        assert np.isfinite(out["centroid"][e]).all(), c["name"]
        compare(out, e, c["ref"], local, absl)
    if not last:
        return
    print(f"parity {label}: relative (absolute) " + ", ".join(f"{k} {local[k]:.3e} ({absl[k]:.3e})" for k in local))
    print("   running maxima, relative: " + ", ".join(f"{k} {v:.3e}" for k, v in MEASURED.items()))
    for k, tol in TOL.items():
        assert local[k] <= tol, (label, k, local[k], tol)


# ---------------------------------------------------------------- parity with the fp64 reference

@pytest.mark.parametrize("n", ROWS)
def test_parity(kp, n):
    base = cases("floor")
    assert len(base) == 15
    local, absl = {}, {}
    starts = list(range(0, len(base) if n < len(base) else 1, n))       # every case is seen at every batch size
    for lo in starts:
        cs = [base[(lo + e) % len(base)] for e in range(n)]
        check(f"floor n={n}, {len(starts)} calls", cs, run(handle(kp), cs), local, absl, lo == starts[-1])


def test_parity_sweep(kp):
    cs = cases("sweep")
    assert len(cs) == 128
    check("sweep (128 rows)", cs, run(handle(kp), cs))


@pytest.mark.parametrize("n", ROWS)
def test_parity_edge_rows(kp, n):
    base = cases("edge")
    assert [c["name"] for c in base] == ["nonunit_quat", "joints_3pi", "heading_+pi", "heading_-pi", "fast_joints", "zero_qvel"]
    local, absl = {}, {}
    starts = list(range(0, len(base) if n < len(base) else 1, n))
    for lo in starts:
        cs = [base[(lo + e) % len(base)] for e in range(n)]
        out = run(handle(kp), cs)
        check(f"edge n={n}, {len(starts)} calls", cs, out, local, absl, lo == starts[-1])
        for e, c in enumerate(cs):
            if c["name"] == "zero_qvel":
                assert not out["body_vel"][e].any() and not out["body_com_vel"][e].any() and not out["centroid"][e][3:10].any()


# ---------------------------------------------------------------- bitwise

def test_bitwise(kp):
    base = cases("floor") + cases("edge")
    cs = [base[e % len(base)] for e in range(67)]
    sim = handle(kp)
    out = run(sim, cs)
    H.same_bits(out, run(sim, cs))                                            # a second identical call
    for e in (0, 7, 64, 66):                                            # a row of the R = 67 call against the same row alone
        one = run(sim, [cs[e]])
        for k in OUT_KEYS:
            assert np.array_equal(out[k][e].view(np.int32), one[k][0].view(np.int32)), (cs[e]["name"], k)
    for k in OUT_KEYS:                                                  # each output requested alone
        H.same_bits(out, run(sim, cs, want=(k,)), (k,))
    still = [dict(c, v=np.zeros(75)) for c in cs]                       # qvel = NULL equals explicit zeros
    H.same_bits(run(sim, still), run(sim, still, qvel=False))
    flat = [dict(c, a=np.zeros(75)) for c in cs]                        # qacc = NULL equals explicit zeros
    H.same_bits(run(sim, flat), run(sim, flat, qacc=False))
    lead = sim.body_motion(dev(np.stack([c["q"] for c in cs[:6]])).view(2, 3, 76), dev(np.stack([c["v"] for c in cs[:6]])).view(2, 3, 75))      # leading shape
    assert lead["body_vel"].shape == (2, 3, 24, 6) and lead["body_com_vel"].shape == (2, 3, 24, 3) and lead["centroid"].shape == (2, 3, 18)
    assert np.array_equal(lead["centroid"].cpu().numpy().reshape(6, 18).view(np.int32), run(sim, flat[:6])["centroid"].view(np.int32))
    q0 = dev(np.stack([c["q"] for c in cs[:5]]))[:0]                    # R = 0
    empty = sim.body_motion(q0)
    assert empty["body_vel"].shape == (0, 24, 6) and empty["centroid"].shape == (0, 18)


# ---------------------------------------------------------------- on the device alone

M_TOL = 2e-6          # kp_sim_mass_matrix against the oracle, of the largest entry (tests/test_gpu_round2.py)


@pytest.mark.parametrize("n", ROWS)
def test_energy_and_momentum_against_the_mass_matrix(kp, n):
    """centroid.ke against 1/2 v^T M v and m com_vel against (M v)[0:3] with kp_sim_mass_matrix of the same state (products formed in fp64 from the
    fp32 matrix).  Bound: the two sides' parity tolerances added -- an entry of M is good to M_TOL max|M|, so v^T M v to |v|_1^2 M_TOL max|M|."""
    base = cases("sweep")[1::2] + cases("floor")
    cs = [base[(3 * e) % len(base)] for e in range(n)]
    sim = kp.KpSim(kp.KpModel(), n)
    q, v = dev(np.stack([c["q"] for c in cs])), dev(np.stack([c["v"] for c in cs]))
    sim.set_state(q, v)
    M = sim.mass_matrix()[0].double().cpu().numpy()
    cen = sim.body_motion(q, v, outputs=("centroid",))["centroid"].double().cpu().numpy()
    worst = [0.0, 0.0]
    for e, c in enumerate(cs):
        vv = c["v"]
        Mv = M[e] @ vv
        ke, p = 0.5 * vv @ Mv, Mv[:3]
        v1, mmax = np.abs(vv).sum(), np.abs(M[e]).max()
        b_ke = TOL["ke"] * max(1.0, abs(ke)) + 0.5 * v1 * v1 * M_TOL * mmax
        b_p = MASS * TOL["com_vel"] * max(1.0, np.abs(p).max() / MASS) + v1 * M_TOL * mmax
        d_ke, d_p = abs(cen[e, C["ke"]] - ke), np.abs(MASS * cen[e, C["com_vel"]] - p).max()
        worst = [max(worst[0], d_ke / b_ke), max(worst[1], d_p / b_p)]
        assert d_ke <= b_ke and d_p <= b_p, (c["name"], d_ke, b_ke, d_p, b_p)
    print(f"mass matrix n={n}: largest share of the bound used: ke {worst[0]:.3f}, momentum {worst[1]:.3f}")


@pytest.mark.parametrize("n", ROWS)
def test_contact_forces_move_the_centre_of_mass(kp, n):
    """kp_sim_contact_forces mode 1 solves for qacc under a joint torque that applies nothing at the root; body_motion at that qacc: m (com_acc - g) is
    the summed contact force and Ldot_com the contacts' moment about the centre of mass.  The solve stops on scale |gradient| < tol and the gradient's
    root rows ARE that force and (about the root position) that moment, so the bound is tol / scale (section 15) plus the parity tolerance."""
    fl = {c["name"].split("/")[0]: c for c in cases("floor")}
    base = [fl[k] for k in ("a_standing", "d_lying", "f_falling")]
    cs = [base[e % 3] for e in range(n)]
    sim = kp.KpSim(kp.KpModel(), n)
    q, v = dev(np.stack([c["q"] for c in cs])), dev(np.stack([c["v"] for c in cs]))
    sim.set_state(q, v)
    tau = np.random.default_rng(5).normal(size=(n, 75)) * 20.0
    tau[:, :6] = 0.0
    fwd = sim.contact_forces(torque=dev(tau), want=("qacc", "contact", "ncon"))
    assert int(sim.diag()[:, 2].max()) == 0
    cen = sim.body_motion(q, v, fwd["qacc"], outputs=("centroid",))["centroid"].double().cpu().numpy()
    con, ncon = fwd["contact"].double().cpu().numpy(), fwd["ncon"].cpu().numpy()
    opt = dict(zip(OPT_FIELDS, KPM["opt"]))
    stop = sim.model.get_option("solver_tol") * opt["meaninertia"] * opt["nv_full"]            # tol / scale
    root = q[:, :3].double().cpu().numpy()
    worst = (0.0, "")
    for e in range(n):
        rows = con[e, :ncon[e]]
        assert np.all(rows[:, 0] < 24) and np.all(rows[:, 1] == -1), "floor scene: every contact acts on the humanoid"
        F = rows[:, 9:12].sum(0)
        com = cen[e, C["com"]]
        tq = np.cross(rows[:, 3:6] - com, rows[:, 9:12]).sum(0)
        acc, Ld = cen[e, C["com_acc"]], cen[e, C["Ldot_com"]]
        d_f = np.abs(MASS * (acc - G) - F).max()
        d_t = np.abs(Ld - tq).max()
        b_f = stop + MASS * TOL["com_acc"] * max(1.0, np.abs(acc).max())
        b_t = stop * (1.0 + np.linalg.norm(com - root[e])) + TOL["Ldot_com"] * max(1.0, np.abs(Ld).max())
        line = (f"forces against motion n={n}, worst row {e} ({cs[e]['name']}): {ncon[e]} contacts, |F| {np.abs(F).max():.3e} N; m (a - g) - sum F {d_f:.3e} N (bound {b_f:.3e}); "
                f"Ldot_com - moment {d_t:.3e} N m (bound {b_t:.3e}); tol / scale {stop:.3e}")
        worst = max(worst, (max(d_f / b_f, d_t / b_t), line))
        assert d_f <= b_f and d_t <= b_t, line
    print(worst[1])


# ---------------------------------------------------------------- against the control step

def test_a_control_step_in_flight_keeps_the_laws(kp):
    """One control step (15 substeps) of an airborne, tumbling state: no contact, zero residual force, PD targets = the pose, so every force but gravity is
    internal.  m com_vel changes by m g T, L_com and ke + pe (the PD damping takes energy out) drift as the integrator makes them: the deviations stay
    within those of the fp64 oracle running the same step (second order in dt, tests/test_body_motion_cpu.py) plus the parity tolerance of the two
    read-outs.  This checks the step kernel by a law, not by the oracle's dynamics."""
    fl = {c["name"].split("/")[0]: c for c in cases("floor")}
    q0, v0 = fl["c_airborne"]["q"], fl["f_falling"]["v"]
    sim = kp.KpSim(kp.KpModel(), 1)
    sim.set_state(dev(q0[None]), dev(v0[None])); sim.set_target(dev(q0[None]))
    read = lambda: sim.body_motion(sim.view("qpos"), sim.view("qvel"), outputs=("centroid",))["centroid"][0].double().cpu().numpy()  # noqa: E731
    c0 = read()
    sim.step_ctrl(dev(np.zeros((1, 75))), 15)
    c1 = read()
    assert int(sim.diag()[0, 0]) == 0, "no contact"
    T = 15 * float(KPM["opt"][0])
    got = BM.conservation_drift(KPM, c0, c1, T)
    f = OracleSim()
    f.reset(q0, v0); f.do_simulation(np.zeros(75), q0, 15)
    assert len(f.contacts()[0]) == 0
    ref = BM.oracle(DEFAULT_KPM)
    r0, r1 = BM.reference(ref, KPM, q0, v0)["centroid"], BM.reference(ref, KPM, f.get("qpos"), f.get("qvel"))["centroid"]
    want = BM.conservation_drift(KPM, r0, r1, T)
    scale = lambda k: max(1.0, np.abs(np.atleast_1d(r0[C[k]])).max(), np.abs(np.atleast_1d(r1[C[k]])).max())  # noqa: E731
    tol = (2 * MASS * TOL["com_vel"] * scale("com_vel"), 2 * TOL["L_com"] * scale("L_com"), 2 * (TOL["ke"] * scale("ke") + TOL["pe"] * scale("pe")))
    for name, g_, w_, t_ in zip(("dp - m g T [N s]", "dL_com [N m s]", "d(ke + pe) [J]"), got, want, tol):
        dg, dw = float(np.abs(g_).max()), float(np.abs(w_).max())
        print(f"flight, one control step: {name}: device {dg:.7e}, fp64 oracle {dw:.7e}, difference {dg - dw:.3e}, parity share {t_:.3e}; m g T = {MASS * 9.81 * T:.3e}")
        assert dg <= dw + t_, name


# ---------------------------------------------------------------- nothing else moves

@pytest.mark.parametrize("scene", ["floor", "h_push"])
def test_the_control_step_is_bit_identical(kp, scene):
    fl = cases("floor")

    def between(sim):
        H.same_bits(run(sim, fl[:5]), run(sim, fl[:5]), OUT_KEYS)
        stored = sim.body_motion(sim.view("qpos"), sim.view("qvel"))      # on the stored rows too
        assert torch.isfinite(stored["centroid"]).all()
    H.control_step_untouched(kp, scene, between)


# ---------------------------------------------------------------- refusals

def test_refusals(kp):
    sim = handle(kp)
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    bufs, full = H.sentinel(kp.MOTION_OUTPUTS, kp.KpMotionOut)
    q = dev(np.tile(ID.f32(STD["qpos"]), (5, 1)))
    qp = ctypes.c_void_p(q.data_ptr())
    f = L.kp_sim_body_motion
    assert f(None, 5, qp, None, None, ctypes.byref(full)) != 0 and "null handle" in err()
    assert f(sim.h, -1, qp, None, None, ctypes.byref(full)) != 0 and "n_rows" in err()
    assert f(sim.h, 5, None, None, None, ctypes.byref(full)) != 0 and "null qpos" in err()
    assert f(sim.h, 5, qp, None, None, None) != 0 and "null out" in err()
    assert f(sim.h, 5, qp, None, None, ctypes.byref(kp.KpMotionOut())) != 0 and "every output of out is null" in err()
    wide = kp.KpSim(kp.KpModel(threads_per_env=128), 5)
    assert f(wide.h, 5, qp, None, None, ctypes.byref(full)) != 0 and "threads_per_env" in err()
    assert f(sim.h, 0, qp, None, None, ctypes.byref(full)) == 0, "n_rows == 0 does nothing"
    H.refused_calls_wrote_nothing(bufs)
    with pytest.raises(ValueError):
        sim.body_motion(q, outputs=("qacc",))
    with pytest.raises(ValueError):
        sim.body_motion(q, qvel=q)
    with pytest.raises(ValueError):
        sim.body_motion(q, outputs=())


# ---------------------------------------------------------------- balance end to end

def leaning_pose():
    """The standing pose with the root pitched about its lateral axis, in steps of 5 degrees, until the REFERENCE's capture point (at rest: the ground
    projection of the centre of mass) lies 2 cm or more outside the REFERENCE's support polygon (hull of the oracle's floor contacts); the lowest hull
    vertex is put 3 mm into the floor.  Chosen on the CPU."""
    from kinpoly_amd import balance
    ref = BM.oracle(DEFAULT_KPM)
    for deg in range(5, 90, 5):
        q = np.array(STD["qpos"], float)
        q[3:7] = BM.qmul(q[3:7] / np.linalg.norm(q[3:7]), BM.qexp([0.0, np.radians(deg), 0.0]))
        q[2] = 0.0
        q[2] = -0.003 - CF.hull_world_verts(KPM, q, range(24))[:, 2].min()
        q = ID.f32(q)
        f = OracleSim()
        f.reset(q, np.zeros(75))
        pos = f.contacts()[1]
        com = BM.reference(ref, KPM, q)["centroid"][:3]
        rows = np.zeros((1, 64, 12)); rows[0, :len(pos), 1] = -1.0; rows[0, :len(pos), 3:6] = pos; rows[0, :len(pos), 8] = 1.0
        m = balance.margin(com[None, :2], balance.support_polygon(rows, np.array([len(pos)])))[0]
        if len(pos) and m <= -0.02:
            return q, deg, m
    raise AssertionError("no pitch below 90 degrees takes the centre of mass off the support")


def test_balance_end_to_end(kp):
    from kinpoly_amd import balance
    sim = handle(kp)
    T = 4
    stand = np.tile(ID.f32(STD["qpos"]), (T, 1))
    s = balance.balance_sequence(sim, stand, 1.0 / 30.0)
    print(f"standing: com_margin {s['com_margin']}, xcom_margin {s['xcom_margin']}, zmp_margin {s['zmp_margin']}, stable_frac {s['stable_frac']}, npoly {s['npoly']}")
    assert np.all(s["com_margin"] > 0.0) and s["stable_frac"] == 1.0 and s["airborne_frac"] == 0.0
    q, deg, m_ref = leaning_pose()
    lean = balance.balance_sequence(sim, np.tile(q, (T, 1)), 1.0 / 30.0)
    print(f"leaning {deg} degrees (reference margin {m_ref:.4f} m): xcom_margin {lean['xcom_margin']}, stable_frac {lean['stable_frac']}")
    assert np.all(lean["xcom_margin"] < 0.0) and lean["stable_frac"] == 0.0 and lean["airborne_frac"] == 0.0
    assert np.abs(lean["xcom_margin"] - m_ref).max() <= 1e-4, "the reference's margin: contact points and centre of mass agree to fp32 rounding (1e-6 m); 1e-4 m leaves two orders"
    up = stand.copy(); up[:, 2] += 1.0
    air = balance.balance_sequence(sim, up, 1.0 / 30.0)
    assert air["airborne_frac"] == 1.0 and np.isnan(air["com_margin"]).all() and np.isnan(air["stable_frac"])
    # the envs' methods: the stored state, no host round trip
    from kinpoly_amd.env import BatchedHumanoidAREnv
    env = BatchedHumanoidAREnv(3, 0, seed=0)
    env.sim.set_state(dev(stand[:3]), dev(np.zeros((3, 75))))
    cen = env.centroidal()
    assert cen["com"].shape == (3, 3) and cen["mass"].shape == (3,) and abs(float(cen["mass"][0]) - MASS) <= TOL["mass"] * MASS
    assert torch.equal(env.body_motion()["centroid"], sim.body_motion(dev(stand[:3]), dev(np.zeros((3, 75))), outputs=("centroid",))["centroid"])


def test_coverage_balance_metrics_and_imu(kp, tmp_path):
    from kinpoly_amd.metrics import write_balance_metrics
    from kinpoly_amd.render import HEAD_BODY, HeadCamera
    sim = handle(kp)
    T = 6
    stand = np.tile(ID.f32(STD["qpos"]), (T, 1))
    up = stand.copy(); up[:, 2] += 1.0
    res = {"none-stand": dict(pred=np.concatenate([stand, np.zeros((T, 3))], 1)), "none-air": dict(pred=up)}
    gt = {"none-stand": dict(qpos=stand), "none-air": dict(qpos=stand)}
    m = write_balance_metrics(res, gt, sim, str(tmp_path), 3, "usr")
    assert os.path.exists(str(tmp_path / "balance_metrics_3_usr.json"))
    a, b = m["per_take"]["none-stand"], m["per_take"]["none-air"]
    print(f"balance metrics: standing {a}, one metre up {b}")
    assert a["stable_frac_pred"] == 1.0 and a["com_margin_pred"] > 0.0 and a["com_margin_pred"] == a["com_margin_gt"] and a["zmp_out_mean_pred"] == 0.0
    assert b["airborne_frac_pred"] == 1.0 and b["airborne_frac_gt"] == 0.0 and np.isnan(b["com_margin_pred"])
    assert m["airborne_frac_pred"] == 0.5 and set(m["by_action"]) == {"none"}
    # the head's IMU of a figure held still: no rate, 9.81 up in the head's frame (to fp32 rounding of the rotation)
    gyro, accel = HeadCamera().imu(sim, stand, 1.0 / 30.0)
    R = BM.qmat(sim.fk(dev(stand[:1]))["wbquat"][0].double().cpu().numpy().reshape(24, 4)[HEAD_BODY])
    assert not gyro.any() and gyro.shape == (T, 3)
    assert np.abs(accel[0].double().cpu().numpy() - R.T @ np.array([0.0, 0.0, 9.81])).max() <= 1e-5
