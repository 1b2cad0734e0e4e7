"""Contact forces estimated from kinematics (kp_sim_estimate_contacts) on a real MI355X: the kernel against the fp64 reference
tests/contact_estimate_oracle.py on identical fp32 inputs, the solver against its own definition (no oracle), the known answers of
tests/test_contact_estimate_cpu.py on the device, bitwise consistency, non-interference with the control step, the refusals and the Python layers.

Deviations are measured RELATIVE to a case's demand: scale = max(|r|, m g) with |r| = sqrt(|force|^2 + |moment|^2 / (1 m)^2), the norm the default
weights induce (a row in free fall has r ~ 0 formed from terms of size m g).  Parity tolerances = 4 x the largest such deviation measured on the MI355X
over the parity tests (the project's convention); every figure is printed before it is asserted.  fp32 rounding of e is amplified into
lambda by w_f / rho = 1e3: a force figure above FINDING = 16 (w_f / rho) 2^-23 = 1.9e-3 would be a finding to explain, not a tolerance to widen.
Body weight m g = 787.7 N."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import contact_estimate_oracle as CE  # noqa: E402
import contact_force_oracle as CF  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPMS = {DEFAULT_KPM: read_kpm(DEFAULT_KPM), STEP_KPM: read_kpm(STEP_KPM)}
BODY_WEIGHT = float(KPMS[DEFAULT_KPM]["body_mass"].sum()) * 9.81
CFG = CE.f32_cfg(CE.default_cfg(KPMS[DEFAULT_KPM]))
W6 = np.array([CFG["w_f"]] * 3 + [CFG["w_m"]] * 3)
MU = float(KPMS[DEFAULT_KPM]["opt"][11])
BOUND = float(np.sqrt(CFG["rho"] / CFG["w_f"]))          # sqrt(rho / w_f) = 0.0316: the derived bound of the known answers, in body weights
ROWS = (1, 5, 67)
OUT_KEYS = ("qfrc_inverse", "qfrc_contact", "contact", "lambda", "resid", "net_wrench", "ncon", "info")
EDGE_CAP = 0.05
FINDING = 16 * (CFG["w_f"] / CFG["rho"]) * 2.0 ** -23

# 4 x the largest deviation / scale from the fp64 reference measured on the MI355X over test_parity and test_parity_sweep (measured value in the comment).
# e itself agrees to 3.4 fp32 steps.  lambda = max(0, G^T W e) / rho multiplies e's rounding by w_f / rho = 1e3, and the forces, their sums and the
# projections inherit it: the largest figures come from the lying pose (31 candidates, 124 active columns) and stay 15 times below FINDING.
TOL_RESID = 4 * 4.018e-7      # resid [6] (N, N m) / scale; measured 4.018e-7
TOL_QINV = 4 * 1.280e-4       # qfrc_inverse [75] / scale; measured 1.280e-4
TOL_QCON = 4 * 1.281e-4       # qfrc_contact [75] / scale; measured 1.281e-4
TOL_F_CONTACT = 4 * 1.210e-4  # per-contact force / scale; measured 1.210e-4
TOL_LAMBDA = 4 * 1.210e-4     # multipliers / scale; measured 1.210e-4
TOL_NET_F = 4 * 1.281e-4      # net contact force / scale; measured 1.281e-4
TOL_NET_TAU = 4 * 3.446e-5    # net contact torque about the world origin / scale; measured 3.446e-5
TOL_POS = 4 * 3.093e-7        # m, candidate positions; measured 3.093e-7
TOL_DIST = 4 * 1.965e-7       # m, candidate distances; measured 1.965e-7
TOLS = dict(resid=TOL_RESID, qfrc_inverse=TOL_QINV, qfrc_contact=TOL_QCON, contact_force=TOL_F_CONTACT, lam=TOL_LAMBDA, net_force=TOL_NET_F,
            net_torque=TOL_NET_TAU, pos=TOL_POS, dist=TOL_DIST)
# the solver against its own definition, same rule (test_solver_against_its_definition).  e - (r - G lambda) IS F(e) at exit: the fixed point holds to
# the rounding of lambda, which is again e's rounding times w_f / rho.
TOL_KKT = 4 * 6.204e-5        # |lambda - max(0, G^T W e) / rho|_inf / scale; measured 6.204e-5
TOL_E = 4 * 1.281e-4          # |e - (r - G lambda)|_inf / scale; measured 1.281e-4
TOL_ROOT = 4 * 1.280e-4       # |root part of qfrc_inverse - resid in the root convention|_inf / scale; measured 1.280e-4
MEASURED = H.Measured()


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


def cases(scene):
    return CE.cases(scene, (DEFAULT_KPM, STEP_KPM), STD["qpos"], STD["qvel"], CFG)


def run(sim, cs, blk="own", want=OUT_KEYS, qvel=True, cfg=None):
    """the kernel on the rows of cs -> numpy outputs.  blk: 'own' the cases' blocks, None no object argument, 'parked' all five parked"""
    st = lambda k: dev(np.stack([c[k] for c in cs]))  # noqa: E731
    obj = None
    if blk == "parked":
        obj = dev(np.tile(ID.f32(CF.parked_block()), (len(cs), 1)))
    elif blk == "own" and cs[0]["blk"] is not None:
        obj = st("blk")
    out = sim.estimate_contacts(st("q"), st("v") if qvel else None, st("a"), obj, cfg=cfg, want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def rows_of(out, e):
    n = int(out["ncon"][e]); c = out["contact"][e].astype(np.float64)
    return dict(body=c[:n, 0].astype(int), b2=c[:n, 1].astype(int), dist=c[:n, 2], pos=c[:n, 3:6], normal=c[:n, 6:9], force=c[:n, 9:12])


def scale_of(r):
    return max(float(np.linalg.norm(r)), BODY_WEIGHT)


def compare(out, e, ref, local, name):
    """deviations of row e from the reference, relative to the case's scale -> local and MEASURED.  The candidate sets must be equal."""
    def rec(k, v):
        MEASURED.note(k, v, local)
    sc = scale_of(ref["r"])
    got = rows_of(out, e)
    con = ref["contacts"]
    assert int(out["ncon"][e]) == ref["ncon"], (name, "candidate count", int(out["ncon"][e]), ref["ncon"])
    assert np.array_equal(got["body"], con["body"]) and np.all(got["b2"] == -1), (name, "candidate bodies in stored order")
    assert not out["contact"][e][ref["ncon"]:].any() and not out["lambda"][e][ref["ncon"]:].any(), "rows >= ncon are exactly zero"
    if ref["ncon"]:
        rec("pos", np.abs(got["pos"] - con["pos"]).max())
        rec("dist", np.abs(got["dist"] - con["dist"]).max())
        rec("contact_force", np.abs(got["force"] - ref["force"]).max() / sc)
        rec("lam", np.abs(out["lambda"][e][:ref["ncon"]] - ref["lam"]).max() / sc)
    for k in ("qfrc_inverse", "qfrc_contact", "resid"):
        rec(k, np.abs(out[k][e] - ref[k]).max() / sc)
    rec("net_force", np.abs(out["net_wrench"][e][:3] - ref["net_wrench"][:3]).max() / sc)
    rec("net_torque", np.abs(out["net_wrench"][e][3:] - ref["net_wrench"][3:]).max() / sc)
    info = out["info"][e]
    assert info[7] == (2.0 if ref["ncon"] == 64 else 0.0), (name, "status", info)


def check(label, local):
    print(f"parity {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in local.items()) + " || running maxima " + ", ".join(f"{k} {v:.3e}" for k, v in MEASURED.items())
          + f" || finding threshold on forces {FINDING:.3e}")
    for k, tol in TOLS.items():
        assert local.get(k, 0.0) <= tol, (k, local[k], tol)
    assert max(local.get(k, 0.0) for k in ("contact_force", "lam", "net_force", "qfrc_contact")) <= FINDING


# ---------------------------------------------------------------- parity with the fp64 reference

def test_default_config_is_the_convention(kp):
    c = kp.KpEstimateCfg.default(handle(kp, DEFAULT_KPM).model)
    for k in ("reach", "w_f", "w_m", "rho", "mu"):
        assert float(getattr(c, k)) == CFG[k], (k, getattr(c, k), CFG[k])
    assert c.n_iters == 20


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("scene", ["floor", "parked", "g_sit"])
def test_parity(kp, scene, n):
    base = cases("g_sit" if scene == "g_sit" else "floor")
    assert not any(c["edge"] for c in base), "no named case is on an edge (tests/test_contact_estimate_cpu.py)"
    cs = [base[e % len(base)] for e in range(n)]
    sim = handle(kp, DEFAULT_KPM if scene == "floor" else STEP_KPM)
    out = run(sim, cs, blk=None if scene != "g_sit" else "own")
    local = {}
    for e, c in enumerate(cs):
        compare(out, e, c["ref"], local, c["name"])
    if scene == "parked":            # an object blob without the object argument and with all five parked: the same bits
        other = run(sim, cs, blk="parked")
        for k in OUT_KEYS:
            assert np.array_equal(out[k].view(np.int32), other[k].view(np.int32)), k
    if scene == "g_sit":
        assert all(np.any(rows_of(out, e)["pos"][:, 2] > 0.3) for e in range(n)), "the seat carries candidates"
    check(f"{scene} n={n}", local)


def test_parity_sweep(kp):
    cs_all = cases("sweep")
    cs = [c for c in cs_all if not c["edge"]]
    assert len(cs_all) == 3 * 64 and len(cs_all) - len(cs) <= EDGE_CAP * len(cs_all)
    out = run(handle(kp, DEFAULT_KPM), cs)
    local = {}
    worst = []
    for e, c in enumerate(cs):
        compare(out, e, c["ref"], local, c["name"])
        if c["ref"]["ncon"]:
            worst.append((np.abs(rows_of(out, e)["force"] - c["ref"]["force"]).max() / scale_of(c["ref"]["r"]), np.linalg.norm(c["ref"]["r"]) / BODY_WEIGHT, c["name"]))
    print("sweep, largest per-contact force deviations (deviation / scale, |r| in body weights, case): " + "; ".join(f"{d:.3e} at {f:.2f} {n}" for d, f, n in sorted(worst, reverse=True)[:4]))
    print("sweep, iterations max %d, line searches max %d, |F| max %.3e" % (out["info"][:, 2].max(), out["info"][:, 5].max(), out["info"][:, 4].max()))
    assert sum(int(n) > 0 for n in out["ncon"]) >= len(cs) // 2, "the sweep has candidates"
    check(f"sweep ({len(cs)} of {len(cs_all)} cases)", local)


# ---------------------------------------------------------------- the solver against its own definition, no oracle

def quat_rot(q, v, inverse=False):
    R = CE.quat_matrix(q)
    return (R.T if inverse else R) @ v


def test_solver_against_its_definition(kp):
    """From the returned lambda, contact rows and resid alone: G rebuilt in fp64, then the KKT identity lambda = max(0, G^T W e) / rho, the definition
    e = r - G lambda (r from need = qfrc_inverse + qfrc_contact, the two outputs whose sum is the demand) and the root part of qfrc_inverse against
    resid in the root convention, which holds the projection path (project_contact_forces) to the solver path."""
    cs = cases("floor") + cases("sweep")
    out = run(handle(kp, DEFAULT_KPM), cs)
    local = {}
    for e, c in enumerate(cs):
        q = c["q"]
        got = rows_of(out, e)
        lam = out["lambda"][e][:len(got["body"])].astype(np.float64).reshape(-1)
        G = CE.build_G(got["pos"], got["normal"], q[:3], MU)
        need = out["qfrc_inverse"][e].astype(np.float64) + out["qfrc_contact"][e].astype(np.float64)
        r = np.concatenate([need[:3], quat_rot(q[3:7], need[3:6])])
        sc = scale_of(r)
        ev = out["resid"][e].astype(np.float64)
        d_kkt = np.abs(lam - np.maximum(0.0, G.T @ (W6 * ev)) / CFG["rho"]).max() / sc if len(lam) else 0.0
        d_e = np.abs(ev - (r - (G @ lam if len(lam) else 0.0))).max() / sc
        root = np.concatenate([ev[:3], quat_rot(q[3:7], ev[3:], inverse=True)])
        d_root = np.abs(out["qfrc_inverse"][e][:6] - root).max() / sc
        for k, v in (("kkt", d_kkt), ("e_definition", d_e), ("root_part", d_root)):
            MEASURED.note(k, v, local)
    print("solver definition: " + ", ".join(f"{k} {v:.3e}" for k, v in local.items()))
    assert local["kkt"] <= TOL_KKT and local["e_definition"] <= TOL_E and local["root_part"] <= TOL_ROOT


# ---------------------------------------------------------------- known answers on the device (the derived bounds of test_contact_estimate_cpu.py)

def state(name, a=None):
    c = next(c for c in cases("floor") if c["name"] == f"{name}/zero")
    return dict(c, a=np.zeros(75) if a is None else ID.f32(a))


def test_known_answers(kp):
    sim = handle(kp, DEFAULT_KPM)
    push = np.zeros(75); push[0] = 2 * MU * 9.81
    cs = [state("standing"), state("lifted_2cm"), state("airborne"), state("standing", push)]
    out = run(sim, cs)
    soft = sim.inverse_dynamics(dev(np.stack([c["q"] for c in cs])), want=("qfrc_inverse",))["qfrc_inverse"].cpu().numpy()
    mass = BODY_WEIGHT / 9.81
    for e in (0, 1):        # standing and lifted 2 cm, qacc = 0: the residual force within sqrt(rho / w_f) body weights, the net vertical force within it of m g
        got = rows_of(out, e)
        hull = CE.hull2d(got["pos"][:, :2])
        assert CE.inside_hull2d(hull, CE.com_xy(KPMS[DEFAULT_KPM], cs[e]["q"])), "precondition: the COM's ground projection lies in the candidates' hull"
        ef = np.linalg.norm(out["resid"][e][:3]) / BODY_WEIGHT
        fz = out["net_wrench"][e][2] / BODY_WEIGHT
        cop = np.array([-out["net_wrench"][e][4], out["net_wrench"][e][3]]) / out["net_wrench"][e][2]
        print(f"{cs[e]['name']}: |e_force| / m g {ef:.3e} (bound {BOUND:.3e}), net F_z / m g {fz:.6f}, cop {cop}, soft resid_force {np.linalg.norm(soft[e][:3]) / BODY_WEIGHT:.4f}")
        assert ef <= BOUND and abs(fz - 1.0) <= BOUND
        assert CE.inside_hull2d(hull, cop), "the centre of pressure is inside the candidates' hull"
    # the motivating contrast: the same lifted row scores 1.0 body weight in the soft inverse (no hull within the 1 mm margin)
    assert abs(np.linalg.norm(soft[1][:3]) / BODY_WEIGHT - 1.0) <= 1e-4
    # one metre up: no candidate, e = r
    need = out["qfrc_inverse"][2].astype(np.float64)
    assert int(out["ncon"][2]) == 0 and not out["qfrc_contact"][2].any() and not out["lambda"][2].any() and out["info"][2][7] == 0.0
    r = np.concatenate([need[:3], quat_rot(cs[2]["q"][3:7], need[3:6])])
    assert np.abs(out["resid"][2] - r).max() <= 1e-6 * BODY_WEIGHT and abs(need[2] / BODY_WEIGHT - 1.0) <= 1e-4
    # every force inside its pyramid (fp32: 1e-6 of the normal component + 1e-6 of m g of slack)
    for e in range(len(cs)):
        got = rows_of(out, e)
        for c in range(len(got["body"])):
            fr = CE.make_frame(got["normal"][c])
            fn, f1, f2 = fr @ got["force"][c]
            slack = 1e-6 * (abs(fn) + BODY_WEIGHT)
            assert fn >= -slack and abs(f1) <= MU * fn + slack and abs(f2) <= MU * fn + slack, (cs[e]["name"], c, fn, f1, f2)
    # standing, the root accelerating horizontally at 2 mu g: the pyramid supplies at most sqrt(2) mu per unit of normal force
    eh = np.linalg.norm(out["resid"][3][:2])
    low = mass * 2 * MU * 9.81 - np.sqrt(2.0) * MU * BODY_WEIGHT - BOUND * BODY_WEIGHT
    print(f"standing at 2 mu g: horizontal residual {eh:.2f} N, at least {low:.2f} N")
    assert eh >= low


# ---------------------------------------------------------------- bitwise

@pytest.mark.parametrize("scene", ["floor", "g_sit"])
def test_bitwise(kp, scene):
    base = cases(scene) + (cases("sweep")[:30] if scene == "floor" else [])
    cs = [base[e % len(base)] for e in range(67)]
    sim = handle(kp, DEFAULT_KPM if scene == "floor" else STEP_KPM)
    out = run(sim, cs)
    H.same_bits(out, run(sim, cs))                                            # a second identical call
    for e in (0, 7, 64, 66) if scene == "floor" else (0, 66):           # a row of the R = 67 call against the same row alone
        one = run(sim, [cs[e]])
        for k in OUT_KEYS:
            assert np.array_equal(out[k][e].view(np.int32), one[k][0].view(np.int32)), (cs[e]["name"], k)
    for k in OUT_KEYS:                                                  # outputs requested one at a time
        H.same_bits(out, run(sim, cs, want=(k,)), (k,))
    still = [dict(c, v=np.zeros(75)) for c in cs]                       # qvel = NULL equals explicit zeros
    H.same_bits(run(sim, still), run(sim, still, qvel=False))
    # a non-finite row reports status 1, writes zeros and leaves its neighbours' bits alone
    bad = [dict(c) for c in cs]
    bad[5] = dict(bad[5], q=np.where(np.arange(76) == 9, np.nan, bad[5]["q"])); bad[64] = dict(bad[64], a=np.where(np.arange(75) == 0, np.inf, bad[64]["a"]))
    ob = run(sim, bad)
    for e in range(67):
        for k in OUT_KEYS:
            if e in (5, 64):
                want = np.zeros_like(ob[k][e]); want = np.where(np.arange(8) == 7, 1.0, 0.0).astype(np.float32) if k == "info" else want
                assert np.array_equal(ob[k][e], want), (e, k)
            else:
                assert np.array_equal(ob[k][e].view(np.int32), out[k][e].view(np.int32)), (e, k)
    if scene == "floor":                                                # leading shape; qvel = qacc = NULL
        lead = sim.estimate_contacts(dev(np.stack([c["q"] for c in cs[:6]])).view(2, 3, 76), want=("qfrc_inverse", "ncon", "lambda"))
        zero = [dict(c, v=np.zeros(75), a=np.zeros(75)) for c in cs[:6]]
        assert lead["qfrc_inverse"].shape == (2, 3, 75) and lead["ncon"].shape == (2, 3) and lead["lambda"].shape == (2, 3, 64, 4)
        assert np.array_equal(lead["qfrc_inverse"].cpu().numpy().reshape(6, 75).view(np.int32), run(sim, zero)["qfrc_inverse"].view(np.int32))


@pytest.mark.parametrize("scene", ["floor", "h_push"])
def test_the_control_step_is_bit_identical(kp, scene):
    """every stored field and kp_sim_diag of a floor handle (lean job queue) and of an object handle after three control steps, with and without estimate
    calls in between"""
    fl = cases("floor")
    rows = fl[:5] if scene == "floor" else [dict(fl[0], blk=ID.f32(CF.object_scenes(KPMS[STEP_KPM], STD["qpos"])["h_push"][2]))] * 5
    H.control_step_untouched(kp, scene, lambda sim: H.same_bits(run(sim, rows), run(sim, rows), OUT_KEYS), floor=fl[::3])


# ---------------------------------------------------------------- refusals

def test_refusals(kp, tmp_path):
    sim = handle(kp, DEFAULT_KPM)
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    bufs, full = H.sentinel(kp.ESTIMATE_OUTPUTS, kp.KpEstimateOut)
    q = dev(np.tile(ID.f32(STD["qpos"]), (5, 1)))
    qp, blk = ctypes.c_void_p(q.data_ptr()), dev(np.tile(ID.f32(CF.parked_block()), (5, 1)))
    good = kp.KpEstimateCfg.default(sim.model)
    f = L.kp_sim_estimate_contacts
    by = ctypes.byref
    assert f(None, 5, qp, None, None, None, by(good), by(full)) != 0 and "null handle" in err()
    assert f(sim.h, 5, None, None, None, None, by(good), by(full)) != 0 and "null qpos" in err()
    assert f(sim.h, 5, qp, None, None, None, None, by(full)) != 0 and "null cfg" in err()
    assert f(sim.h, 5, qp, None, None, None, by(good), None) != 0 and "null out" in err()
    assert f(sim.h, 5, qp, None, None, None, by(good), by(kp.KpEstimateOut())) != 0 and "every output of out is null" in err()
    assert f(sim.h, -1, qp, None, None, None, by(good), by(full)) != 0 and "n_rows" in err()
    for field, value in (("reach", 0.0), ("reach", -1.0), ("reach", float("nan")), ("w_f", float("inf")), ("w_f", 0.0), ("w_m", float("nan")), ("rho", 0.0),
                         ("rho", float("inf")), ("mu", -0.1), ("n_iters", -1)):
        c = kp.KpEstimateCfg.default(sim.model)
        setattr(c, field, value)
        assert f(sim.h, 5, qp, None, None, None, by(c), by(full)) != 0 and field in err(), (field, value, err())
    from kinpoly_amd.model_compiler import write_kpm
    m = read_kpm(DEFAULT_KPM)
    m["obj_geoms"] = np.zeros((0, 18), m["obj_geoms"].dtype)
    write_kpm(m, str(tmp_path / "no_objects.kpm"))
    bare = kp.KpSim(kp.KpModel(str(tmp_path / "no_objects.kpm")), 1)
    assert f(bare.h, 5, qp, None, None, ctypes.c_void_p(blk.data_ptr()), by(good), by(full)) != 0 and "obj_qpos" in err() and "no object geoms" in err()
    wide = kp.KpSim(kp.KpModel(threads_per_env=128), 5)
    assert f(wide.h, 5, qp, None, None, None, by(good), by(full)) != 0 and "threads_per_env" in err()
    assert f(sim.h, 0, qp, None, None, None, by(good), by(full)) == 0, "n_rows == 0 does nothing"
    H.refused_calls_wrote_nothing(bufs)
    with pytest.raises(ValueError):
        sim.estimate_contacts(q, want=("qacc",))
    with pytest.raises(ValueError):
        sim.estimate_contacts(q, qvel=q)
    assert sim.estimate_contacts(q[:0])["qfrc_inverse"].shape == (0, 75)


# ---------------------------------------------------------------- the Python layers

def test_sequence_plausibility_and_metrics(kp):
    from kinpoly_amd import contact, dynamics
    from kinpoly_amd.metrics import DYNAMICS_KEYS, coverage_dynamics_metrics
    sim = handle(kp, STEP_KPM)
    T = 12
    lifted = np.tile(state("lifted_2cm")["q"], (T, 1))
    air = np.tile(state("airborne")["q"], (T, 1))
    Q = dev(np.concatenate([lifted, air]))
    est = dynamics.estimate_contacts_sequence(sim, Q, 1.0 / 30.0, take_off=[0, T, 2 * T], chunk_rows=7)
    assert float(est["qvel"].abs().max()) == 0.0 and float(est["qacc"].abs().max()) == 0.0, "still takes: zero derivatives, also across the take boundary"
    one = sim.estimate_contacts(Q, est["qvel"], est["qacc"], want=dynamics.ESTIMATE_WANT)
    for k in dynamics.ESTIMATE_WANT:                                    # chunked launches equal one launch, bit for bit
        assert torch.equal(est[k], one[k]), k
    lim = torch.tensor(np.asarray(KPMS[STEP_KPM]["torque_lim"], np.float32), device="cuda")
    p = dynamics.plausibility_estimated(est, Q, lim, BODY_WEIGHT)
    soft = dynamics.plausibility(sim.inverse_dynamics(Q)["qfrc_inverse"], Q, est["qvel"], lim, BODY_WEIGHT)
    assert set(soft) <= set(p) and p["grf"].shape == (2 * T, 3)
    print(f"lifted 2 cm: estimated resid_force {float(p['resid_force'][0]):.3e}, soft {float(soft['resid_force'][0]):.4f}; support_share {float(p['mean']['support_share'])}")
    assert float(p["resid_force"][:T].max()) <= BOUND and abs(float(soft["resid_force"][0]) - 1.0) <= 1e-4          # the motivating contrast
    assert abs(float(p["resid_force"][T:].min()) - 1.0) <= 1e-4 and float(p["mean"]["support_share"]) == 0.5
    assert abs(float(p["grf"][0, 2]) - 1.0) <= BOUND and float(p["grf"][T:].abs().max()) == 0.0
    # the contact rows are section 14's: ground_reaction takes them through the adapter
    gr = contact.ground_reaction(contact.wrench_from_contacts(est["contact"]))
    assert bool(gr["support"][:T].all()) and not bool(gr["support"][T:].any())
    assert abs(float(gr["force"][0, :, 2].sum()) / BODY_WEIGHT - float(p["grf"][0, 2])) <= 1e-5, "the feet carry the whole estimated ground reaction"
    # the metric: the default is today's output key for key; the estimated scores go under *_est
    obj = np.tile(ID.f32(CF.parked_block()), (T, 1))
    results = {"none-lifted": dict(pred=lifted, obj_pose=obj), "none-air": dict(pred=air, obj_pose=obj)}
    gt = {"none-lifted": dict(qpos=lifted), "none-air": dict(qpos=air)}
    m_soft = coverage_dynamics_metrics(results, gt, sim)
    m_both = coverage_dynamics_metrics(results, gt, sim, contacts="both")
    m_est = coverage_dynamics_metrics(results, gt, sim, contacts="estimated")
    base = [f"{a}_{b}" for a in DYNAMICS_KEYS for b in ("pred", "gt")]
    assert [k for k in m_soft if k not in ("per_take", "by_action")] == base and list(m_soft["per_take"]["none-air"]) == base
    assert all(m_both[k] == m_soft[k] for k in base) and all(m_both[k + "_est"] == m_est[k + "_est"] for k in base) and not any(k in m_est for k in base)
    lt = m_both["per_take"]["none-lifted"]
    assert abs(lt["resid_force_pred"] - 1.0) <= 1e-4 and lt["resid_force_pred_est"] <= BOUND and lt["support_share_pred_est"] == 1.0
    assert m_both["per_take"]["none-air"]["support_share_gt_est"] == 0.0 and abs(lt["grf_z_pred_est"] - 1.0) <= BOUND
