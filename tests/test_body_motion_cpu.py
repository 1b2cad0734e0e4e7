"""Body motion, momentum and energy without a GPU: the fp64 reference tests/body_motion_oracle.py against closed forms, against the
oracle's own forward() and step() (contact forces, flight), kinpoly_amd.balance on known answers and brute force, dynamics.body_imu, and the surface
(header, binding table, symbol, struct mirror).

Bounds.  The reference differentiates the oracle's forward kinematics (positions of order 1 m, rounding 2e-16) with the step auto_eps() gives; its
velocities are good to ~1e-11 relative, its accelerations to ~1e-9 relative of the row's largest acceleration (body_motion_oracle's docstring,
test_plateau below).  Every comparison with a closed form is asserted at 1e-8 relative to the row's scale, an order above that."""
import ctypes
import os

import numpy as np
import pytest

import body_motion_oracle as BM
import contact_force_oracle as CF
import inverse_dynamics_oracle as ID
from kinpoly_amd import build as kpbuild
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm, write_kpm
from oracle.kpo import OracleSim

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)
G = np.asarray(KPM["opt"][1:4], float)
MASS = float(KPM["body_mass"].sum())
REL = 1e-8
C = BM.CENTROID


@pytest.fixture(scope="module")
def o():
    return BM.oracle(DEFAULT_KPM)


@pytest.fixture(scope="module")
def states():
    """name -> (q, v, a): the named floor states with a seeded acceleration, and the first four sweep states"""
    out = {}
    for s in ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"])[:-1] + ID.sweep_states(KPM, STD["qpos"])[:4]:
        rng = np.random.default_rng(sum(map(ord, s["name"])))
        out[s["name"]] = (s["q"], s["v"], rng.normal(size=75) * 30.0)
    return out


def rel(a, b, scale=None):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max() if scale is None else scale))


# ---------------------------------------------------------------- the reference against closed forms

def test_plateau(o, states):
    """three steps around the chosen one agree: the chosen step sits on the plateau between truncation and rounding"""
    q, v, a = states["f_falling"]
    e0 = BM.auto_eps(v, a)
    refs = [BM.reference(o, KPM, q, v, a, eps=e) for e in (0.5 * e0, e0, 2.0 * e0)]
    for k in ("body_vel", "body_acc", "body_com_vel", "centroid"):
        scale = np.abs(refs[1][k]).max()
        d = [np.abs(r[k] - refs[1][k]).max() / scale for r in refs]
        print(f"plateau {k}: eps {e0:.2e}; deviation of eps / 2 and 2 eps from eps, relative to {scale:.3e}: {d[0]:.2e}, {d[2]:.2e}")
        assert max(d) <= REL
    one = BM.reference(o, KPM, q, v, a, eps=e0, richardson=False)
    assert np.abs(one["body_acc"] - refs[1]["body_acc"]).max() > np.abs(refs[0]["body_acc"] - refs[1]["body_acc"]).max(), "the Richardson step earns its keep"


def test_energy_and_momentum_against_the_mass_matrix(o, states):
    worst = {}
    for name, (q, v, a) in states.items():
        r = BM.reference(o, KPM, q, v, a)
        o.reset(q, v)
        M = o.fullM()
        Mv = M @ v
        cen = r["centroid"]
        d = dict(ke=rel(cen[C["ke"]], 0.5 * v @ Mv), p=rel(MASS * cen[C["com_vel"]], Mv[:3]), L_root=rel(r["R"][0].T @ r["L_root"], Mv[3:6]),
                 com=rel(cen[C["com"]], o.get("subtree_com")), mass=rel(cen[C["mass"]], MASS))
        cv = o.get("cvel").reshape(24, 6)                                # [ang; lin] about the subtree centre of mass
        sc = o.get("subtree_com")
        d["w"] = rel(r["body_vel"][:, :3], cv[:, :3])
        d["v"] = rel(r["body_vel"][:, 3:], cv[:, 3:] + np.cross(cv[:, :3], r["xpos"] - sc))
        d["vc"] = rel(r["body_com_vel"], cv[:, 3:] + np.cross(cv[:, :3], r["xipos"] - sc))
        d["pe"] = rel(cen[C["pe"]], -MASS * G @ o.get("subtree_com"))
        for k, x in d.items():
            worst[k] = max(worst.get(k, 0.0), x)
            assert x <= REL, (name, k, x)
    print("closed forms, worst relative deviation: " + ", ".join(f"{k} {x:.2e}" for k, x in worst.items()))


def test_a_state_held_still_has_only_potential_energy(o, states):
    q = states["a_standing"][0]
    r = BM.reference(o, KPM, q)
    assert not r["body_vel"].any() and not r["body_acc"].any() and not r["body_com_vel"].any()
    cen = r["centroid"]
    assert not cen[3:10].any() and not cen[11:17].any()
    assert cen[C["pe"]] > 0.0 and abs(cen[C["pe"]] - MASS * 9.81 * cen[2]) <= 1e-9


def test_rigid_spin_about_the_vertical(o, states):
    q = states["f_falling"][0]
    w = np.array([0.0, 0.0, 2.5])
    v = np.zeros(75); v[3:6] = BM.qmat(q[3:7]).T @ w                   # the free joint's angular velocity is in the root's own axes
    r = BM.reference(o, KPM, q, v)
    cen = r["centroid"]
    assert rel(cen[C["L_com"]], r["I_total"] @ w) <= REL
    assert rel(cen[C["ke"]], 0.5 * w @ r["I_total"] @ w + 0.5 * MASS * cen[C["com_vel"]] @ cen[C["com_vel"]]) <= REL
    assert rel(r["body_vel"][:, :3], np.tile(w, (24, 1))) <= REL
    assert rel(cen[C["com_acc"]], np.cross(w, cen[C["com_vel"]])) <= REL, "the centre of mass circles the root: centripetal acceleration"
    assert rel(cen[C["Ldot_com"]], np.cross(w, cen[C["L_com"]])) <= REL, "L_com turns with the figure"


# ---------------------------------------------------------------- contact and flight on the oracle's own forward() and step()

@pytest.mark.parametrize("name", ["a_standing", "d_lying", "f_falling"])
def test_contact_forces_move_the_centre_of_mass(o, states, name):
    """m (com_acc - g) = the sum of the contact forces, at the qacc forward() finds under a joint torque that applies nothing at the root"""
    q, v, _ = states[name]
    f = OracleSim(kpm=DEFAULT_KPM, ls_exact=True)
    f.reset(q, v)
    tau = np.random.default_rng(11).normal(size=69) * 20.0
    res = CF.oracle_contact_forces(f, 1, np.concatenate([np.zeros(6), tau]), None, KPM)
    F = res["force"].sum(0) if len(res["force"]) else np.zeros(3)
    r = BM.reference(o, KPM, q, v, res["qacc"])
    cen = r["centroid"]
    got = MASS * (cen[C["com_acc"]] - G)
    scale = max(np.abs(res["force"]).sum() if len(res["force"]) else 0.0, MASS * 9.81)
    tq = sum((np.cross(p - cen[C["com"]], fc) for p, fc in zip(res["contacts"]["pos"], res["force"])), np.zeros(3))
    print(f"{name}: {len(res['force'])} contacts, |qacc| {np.abs(res['qacc']).max():.3e}, sum F {F}, m (a - g) {got}, deviation {np.abs(got - F).max():.3e} N of {scale:.3e} N; "
          f"Ldot_com - contact moment {np.abs(cen[C['Ldot_com']] - tq).max():.3e} N m")
    assert np.abs(got - F).max() <= REL * scale
    assert np.abs(cen[C["Ldot_com"]] - tq).max() <= REL * scale, "and their moment about the centre of mass turns it (joint torques are internal)"


def flight_drift(kpm_path, q, v, n_steps, ctrl=None):
    """n_steps of the oracle's step() without contacts and limits -> (dp - m g t [3], dL_com - 0 [3], d(ke + pe), t): the deviation of the integrator from
    the conservation laws of free flight (exact dynamics: all zero)"""
    kpm = read_kpm(kpm_path)
    f = OracleSim(kpm=kpm_path, contact=False, limits=False)
    f.set_ctrl(np.zeros(69) if ctrl is None else ctrl, np.zeros(6))
    f.reset(q, v)
    ref = BM.oracle(kpm_path)
    c0 = BM.reference(ref, kpm, q, v)["centroid"]
    for _ in range(n_steps):
        f.step()
    c1 = BM.reference(ref, kpm, f.get("qpos"), f.get("qvel"))["centroid"]
    t = n_steps * float(kpm["opt"][0])
    return (*BM.conservation_drift(kpm, c0, c1, t), t)


def test_flight_changes_momentum_by_m_g_t(states, tmp_path):
    """Contacts off, no actuation: linear momentum changes by m g t, L_com and ke + pe stay.  The semi-implicit Euler step keeps these laws up to its
    local error, which is second order in dt (momentum is m J_com(q) v, and the step evaluates J_com at the old pose): so what is asserted is the order,
    not a magnitude -- halving dt quarters the deviation of one step (ratio 4 +- 10 %) and halves the deviation over a fixed time (ratio 2 +- 20 %):
    the laws hold in the limit dt -> 0.  The figures printed here are the reference of the GPU flight test."""
    q = states["c_airborne"][0]
    v = states["f_falling"][1]                                           # the airborne pose, tumbling at up to 5 rad/s on every joint
    half = dict(KPM); half["opt"] = KPM["opt"].copy(); half["opt"][0] *= 0.5
    write_kpm(half, str(tmp_path / "half_dt.kpm"))
    dp1, dL1, dE1, t1 = flight_drift(DEFAULT_KPM, q, v, 1)
    dp2, dL2, dE2, t2 = flight_drift(str(tmp_path / "half_dt.kpm"), q, v, 1)
    print(f"flight, one step of {t1:.3e} s: |dp - m g dt| {np.abs(dp1).max():.3e} N s of m g dt = {MASS * 9.81 * t1:.3e}; |dL_com| {np.abs(dL1).max():.3e} N m s; "
          f"d(ke + pe) {dE1:.3e} J; at dt / 2: {np.abs(dp2).max():.3e}, {np.abs(dL2).max():.3e}, {dE2:.3e}")
    assert t2 == pytest.approx(0.5 * t1)
    for a, b in ((dp1, dp2), (dL1, dL2), (dE1, dE2)):
        assert 3.6 <= np.abs(a).max() / np.abs(b).max() <= 4.4
    dp15, dL15, dE15, t15 = flight_drift(DEFAULT_KPM, q, v, 15)
    dp30, dL30, dE30, t30 = flight_drift(str(tmp_path / "half_dt.kpm"), q, v, 30)
    print(f"flight, a control step of 15 substeps ({t15:.3e} s): |dp - m g T| {np.abs(dp15).max():.3e} N s of m g T = {MASS * 9.81 * t15:.3e}, |dL_com| {np.abs(dL15).max():.3e} N m s, "
          f"d(ke + pe) {dE15:.3e} J; with 30 substeps of dt / 2: {np.abs(dp30).max():.3e}, {np.abs(dL30).max():.3e}, {dE30:.3e}")
    assert t30 == pytest.approx(t15)
    for a, b in ((dp15, dp30), (dL15, dL30), (dE15, dE30)):
        assert 1.6 <= np.abs(a).max() / np.abs(b).max() <= 2.4


# ---------------------------------------------------------------- balance.py

def brute_margin(p, pts):
    """Signed distance by exhaustion: the boundary is made of the segments between two points that have every other point on one side (all pairs
    tried); p is inside when some non-degenerate triangle of three points holds it (all triples tried)."""
    pts = np.asarray(pts, float)
    n = len(pts)
    if n == 1:
        return -float(np.linalg.norm(p - pts[0]))
    best = np.inf
    for i in range(n):
        for j in range(i + 1, n):
            ab = pts[j] - pts[i]
            side = ab[0] * (pts[:, 1] - pts[i, 1]) - ab[1] * (pts[:, 0] - pts[i, 0])
            if np.all(side >= 0.0) or np.all(side <= 0.0):
                den = ab @ ab
                t = 0.0 if den == 0.0 else min(max((p - pts[i]) @ ab / den, 0.0), 1.0)
                best = min(best, float(np.linalg.norm(p - pts[i] - t * ab)))
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    A, B, Cc = pts[i.ravel()], pts[j.ravel()], pts[k.ravel()]
    cr = lambda u, w: u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]      # noqa: E731
    area = cr(B - A, Cc - A)
    inside = (area > 1e-12) & (cr(B - A, p - A) >= 0.0) & (cr(Cc - B, p - B) >= 0.0) & (cr(A - Cc, p - Cc) >= 0.0)
    return best if inside.any() else -best


def point_sets():
    rng = np.random.default_rng(2)
    sets = [rng.normal(size=(n, 2)) for n in (3, 4, 7, 20, 64)]
    sets.append(np.stack([np.linspace(-1, 1, 9), 0.5 * np.linspace(-1, 1, 9) + 0.25], 1))          # collinear
    sets.append(np.repeat(rng.normal(size=(5, 2)), 3, 0))                                              # duplicates
    sets.append(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.0], [1.0, 0.5], [0.5, 0.5]]))      # points on edges and inside
    sets += [np.zeros((0, 2)), np.array([[0.3, -0.2]]), np.array([[0.3, -0.2], [-0.4, 0.1]]), np.array([[0.3, -0.2], [0.3, -0.2]])]
    return sets


def as_contacts(sets):
    """the point sets as contact rows [T, 64, 12] + ncon, with two decoys per row that are no floor contact (a contact on a slot, one on a seat)"""
    c, n = np.zeros((len(sets), 64, 12)), np.zeros(len(sets), np.int32)
    for t, s in enumerate(sets):
        k = len(s)
        c[t, :k, 1] = -1.0; c[t, :k, 3:5] = s; c[t, :k, 8] = 1.0
        if k <= 62:
            c[t, k] = [3, 24, 0, 50.0, 50.0, 0.0, 0, 0, 1, 0, 0, 0]
            c[t, k + 1] = [3, -1, 0, -50.0, 50.0, 0.41, 0, 0, 1, 0, 0, 0]
            k += 2
        c[t, k:, 3:5] = 99.0                                             # rows >= ncon are never read
        n[t] = k
    return c, n


def test_hull_and_margin_against_brute_force():
    from kinpoly_amd import balance
    sets = point_sets()
    poly, npoly = balance.support_polygon(*as_contacts(sets))
    assert list(npoly[-4:]) == [0, 1, 2, 1] and npoly[5] == 2 and npoly[7] == 4
    rng = np.random.default_rng(3)
    worst = 0.0
    for t, s in enumerate(sets):
        h = poly[t, :npoly[t]]
        assert not poly[t, npoly[t]:].any()
        assert all(any(np.array_equal(x, y) for y in s) for x in h), "hull vertices are input points"
        if npoly[t] >= 3:
            e = np.roll(h, -1, 0) - h
            assert np.all(e[:, 0] * np.roll(e, -1, 0)[:, 1] - e[:, 1] * np.roll(e, -1, 0)[:, 0] > 0.0), "counter-clockwise, strictly convex"
        probes = rng.normal(size=(12, 2)) * 1.2
        if len(s):
            probes[:3] = s[:3].mean(0) if len(s) >= 3 else s[0]
        got = balance.margin(np.tile(probes, (1, 1)), (np.tile(poly[t], (12, 1, 1)), np.tile(npoly[t], 12)))
        if npoly[t] == 0:
            assert np.isnan(got).all()
            continue
        want = np.array([brute_margin(p, s) for p in probes])
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got - want).max() <= 1e-12, (t, got, want)
        if npoly[t] <= 2:
            assert np.all(got <= 0.0)
    print(f"margin against brute force: worst deviation {worst:.2e}")
    assert balance.margin(np.array([[0.5, 0.5]]), (poly[7:8], npoly[7:8]))[0] == pytest.approx(0.5, abs=1e-12)


def test_capture_point_and_zmp_of_a_point_mass():
    from kinpoly_amd import balance
    com = torch.tensor([[0.2, -0.1, 0.9]], dtype=torch.float64)
    vel = torch.tensor([[0.5, -0.3, 0.1]], dtype=torch.float64)
    cp = balance.capture_point(com, vel, 9.81)
    assert torch.allclose(cp, com[:, :2] + vel[:, :2] * (0.9 / 9.81) ** 0.5, atol=1e-15)
    z0 = torch.zeros(1, 3, dtype=torch.float64)
    assert torch.allclose(balance.zmp(com, z0, z0, 70.0), com[:, :2], atol=1e-15), "at rest the ZMP is the ground projection"
    acc = torch.tensor([[1.5, -0.5, 2.0]], dtype=torch.float64)
    z = balance.zmp(com, acc, z0, torch.tensor([70.0], dtype=torch.float64))
    # a point mass: the force line m (a + g e_z) through the mass meets the floor at com_xy - z a_xy / (a_z + g)
    assert torch.allclose(z, com[:, :2] - 0.9 * acc[:, :2] / (2.0 + 9.81), atol=1e-14)
    Ld = torch.tensor([[3.0, -2.0, 5.0]], dtype=torch.float64)
    z2 = balance.zmp(com, acc, Ld, 70.0)
    F = 70.0 * (acc[0] + torch.tensor([0.0, 0.0, 9.81], dtype=torch.float64))
    r = torch.cat([z2[0], torch.zeros(1, dtype=torch.float64)]) - com[0]
    assert torch.allclose(torch.linalg.cross(r, F)[:2], Ld[0, :2], atol=1e-11), "the force at the ZMP has the horizontal moment Ldot_com about the centre of mass"
    assert torch.isnan(balance.zmp(com, torch.tensor([[0.0, 0.0, -9.81]], dtype=torch.float64), z0, 70.0)).all(), "free fall has no ZMP"


class FakeSim:
    """records the calls balance_sequence makes; answers with a centre of mass over / beside a unit square of contacts, or no contact"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def body_motion(self, q, qvel, qacc, outputs):
        self.calls.append(("body_motion", q.clone(), qvel.clone(), qacc.clone(), tuple(outputs)))
        cen = torch.zeros(len(q), 18); cen[:, 0] = q[:, 0]; cen[:, 1] = 0.5; cen[:, 2] = 1.0; cen[:, 17] = 70.0
        return {"centroid": cen}

    def inverse_dynamics(self, q, qvel, qacc, want):
        self.calls.append(("inverse_dynamics", q.clone(), qvel.clone(), qacc.clone(), tuple(want)))
        c = torch.zeros(len(q), 64, 12); n = torch.zeros(len(q), dtype=torch.int32)
        for t in range(len(q)):
            if q[t, 2] < 1.5:
                c[t, :4, 1] = -1.0; c[t, :4, 8] = 1.0
                c[t, :4, 3:5] = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]); n[t] = 4
        return {"contact": c, "ncon": n}


def test_balance_sequence_bookkeeping():
    from kinpoly_amd import balance, dynamics
    T = 9
    q = torch.zeros(T, 76); q[:, 3] = 1.0
    q[:, 0] = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 1.5, 1.5, 0.5, 0.5])        # two frames beside the square
    q[:, 2] = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0])        # two frames airborne
    q[5:, 7] = torch.arange(4.0)                                                 # the second take moves a joint; the first holds still
    sim = FakeSim()
    out = balance.balance_sequence(sim, q, 1.0 / 30.0, take_off=[0, 5, 9])
    assert [c[0] for c in sim.calls] == ["body_motion", "inverse_dynamics"], "one call each for the whole sequence"
    qv, qa = dynamics.motion_derivatives(q, 1.0 / 30.0, [0, 5, 9])
    for c in sim.calls:
        assert torch.equal(c[1], q) and torch.equal(c[2], qv) and torch.equal(c[3], qa)
    assert not qv[:5].any(), "no difference crosses the take boundary (row 4 does not see row 5's jump in x)"
    assert sim.calls[0][4] == ("centroid",) and sim.calls[1][4] == ("contact", "ncon")
    assert np.allclose(out["com_margin"][:5], 0.5) and np.allclose(out["com_margin"][5:7], -0.5) and np.isnan(out["com_margin"][7:]).all()
    assert out["airborne_frac"] == pytest.approx(2 / 9) and out["stable_frac"] == pytest.approx(5 / 7) and out["zmp_out_mean"] == pytest.approx(2 * 0.5 / 7)
    assert list(out["npoly"]) == [4] * 7 + [0, 0]


def test_coverage_balance_metrics_bookkeeping():
    """pred and gt of every take go through ONE balance_sequence call, back to back, and come out per take, per side and per action prefix"""
    from kinpoly_amd.metrics import coverage_balance_metrics
    T = 5
    on = np.zeros((T, 76)); on[:, 3] = 1.0; on[:, 0] = 0.5; on[:, 2] = 1.0         # over the square
    off_ = on.copy(); off_[:, 0] = 1.5                                              # beside it
    up = on.copy(); up[:, 2] = 2.0                                                  # airborne
    res = {"sit-a": dict(pred=np.concatenate([off_, np.zeros((T, 3))], 1)), "none-b": dict(pred=up[:4]), "none-short": dict(pred=on[:2]), "none-nogt": dict(pred=on)}
    gt = {"sit-a": dict(qpos=on), "none-b": dict(qpos=on), "none-short": dict(qpos=on)}
    sim = FakeSim()
    m = coverage_balance_metrics(res, gt, sim)
    assert [c[0] for c in sim.calls] == ["body_motion", "inverse_dynamics"] and len(sim.calls[0][1]) == 2 * T + 2 * 4
    assert set(m["per_take"]) == {"sit-a", "none-b"} and set(m["by_action"]) == {"sit", "none"}
    a, b = m["per_take"]["sit-a"], m["per_take"]["none-b"]
    assert a["com_margin_pred"] == pytest.approx(-0.5) and a["com_margin_gt"] == pytest.approx(0.5) and a["stable_frac_pred"] == 0.0 and a["stable_frac_gt"] == 1.0
    assert b["airborne_frac_pred"] == 1.0 and np.isnan(b["com_margin_pred"]) and np.isnan(b["stable_frac_pred"]) and b["airborne_frac_gt"] == 0.0
    assert m["com_margin_pred"] == pytest.approx(-0.5), "means over the takes skip the takes without a value"
    assert m["airborne_frac_pred"] == pytest.approx(0.5) and m["by_action"]["none"]["airborne_frac_pred"] == 1.0


@pytest.mark.parametrize("script", ["eval_ar_policy.py", "eval_uhc.py"])
def test_scripts_take_balance_metrics(script):
    import importlib.util
    spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(ROOT, "scripts", script))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert p.parse_args([]).balance_metrics is False and p.parse_args(["--balance_metrics"]).balance_metrics is True


# ---------------------------------------------------------------- ABI and Python surface

def test_header_binding_and_symbol():
    from kinpoly_amd import sim as kpsim
    hdr = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    assert "int kp_sim_body_motion(kp_sim*, int n_rows, const float* qpos, const float* qvel, const float* qacc, const kp_motion_out* out);" in hdr
    assert "typedef struct { float *body_vel, *body_acc, *body_com_vel, *centroid; } kp_motion_out;" in hdr
    for word in ("body_xvelp", "mj_objectAcceleration", "mj_energyVel", "does not synchronise"):
        assert word in hdr, word
    assert len(kpsim._SIGNATURES["kp_sim_body_motion"][1]) == 6
    assert [f[0] for f in kpsim.KpMotionOut._fields_] == list(kpsim.MOTION_OUTPUTS)
    assert ctypes.sizeof(kpsim.KpMotionOut) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert kpsim.CENTROID_FIELDS == BM.CENTROID
    if not os.path.exists(kpbuild.LIB):
        pytest.fail(f"{kpbuild.LIB} is missing: build() first")
    assert hasattr(ctypes.CDLL(kpbuild.LIB), "kp_sim_body_motion")


def test_body_imu_on_a_turntable():
    """a body turning at a constant rate about the vertical through its frame origin: the gyro reads the rate, the accelerometer the centripetal pull
    towards the axis plus 9.81 up, in the body's own (turned) frame"""
    from kinpoly_amd import dynamics
    w, th, body = 3.0, 0.7, 13
    vel, acc = torch.zeros(2, 24, 6, dtype=torch.float64), torch.zeros(2, 24, 6, dtype=torch.float64)
    vel[:, body, 2] = w
    xq = torch.zeros(2, 24, 4, dtype=torch.float64); xq[..., 0] = 1.0
    xq[:, body] = torch.tensor([np.cos(th / 2), 0.0, 0.0, np.sin(th / 2)], dtype=torch.float64)
    off = (0.2, -0.1, 0.05)
    gyro, accel = dynamics.body_imu(dict(body_vel=vel, body_acc=acc), xq, body, off)
    assert torch.allclose(gyro, torch.tensor([0.0, 0.0, w], dtype=torch.float64).expand(2, 3), atol=1e-15)
    assert torch.allclose(accel, torch.tensor([-w * w * 0.2, w * w * 0.1, 9.81], dtype=torch.float64).expand(2, 3), atol=1e-13)
    g0, a0 = dynamics.body_imu(dict(body_vel=vel, body_acc=acc), xq.reshape(2, 96), body)
    assert torch.allclose(a0, torch.tensor([0.0, 0.0, 9.81], dtype=torch.float64).expand(2, 3), atol=1e-15) and torch.equal(g0, gyro)
