"""Inverse dynamics (kp_sim_inverse_dynamics) on a real MI355X: the kernel against the fp64 composition
tests/inverse_dynamics_oracle.py on identical fp32 inputs, the device-only round trip forward -> inverse through kp_sim_contact_forces, bitwise
consistency, non-interference with the control step, the refusals and coverage_dynamics_metrics.

Parity tolerances = 4 x the largest deviation measured on the MI355X over the cases of the parity tests (the project's convention);
every figure is printed before it is asserted.  Body weight m g = 787.7 N."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import contact_force_oracle as CF  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, OPT_FIELDS, STEP_KPM, read_kpm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPMS = {DEFAULT_KPM: read_kpm(DEFAULT_KPM), STEP_KPM: read_kpm(STEP_KPM)}
BODY_WEIGHT = float(KPMS[DEFAULT_KPM]["body_mass"].sum()) * 9.81
ROWS = (1, 5, 67)
OUT_KEYS = ("qfrc_inverse", "qfrc_constraint", "qfrc_bias", "contact", "net_wrench", "ncon")
EDGE_CAP = 0.05

# 4 x the largest deviation from the fp64 composition measured on the MI355X over test_parity and test_parity_sweep (measured value in the comment).
# The largest ones all come from the sweep: states falling at up to 5 rad/s on every joint, where one contact carries 7e3 .. 3.4e4 N at the given
# accelerations; the worst case (seed 1007, qacc = 0) is 0.405 N on a contact of 7.4e3 N, 5.5e-5 of the force; on the named states (forces up to 9.8e4 N, mostly at rest) the figures are 4.7e-2 N
# (qfrc_inverse), 5.0e-2 (qfrc_constraint, net force), 3.0e-2 N m (net torque), 2.6e-2 N (per contact), 1.2e-4 (qfrc_bias).
TOL_QINV = 4 * 4.052e-1       # N / N m, qfrc_inverse; measured 4.052e-1
TOL_QCON = 4 * 4.050e-1       # N / N m, qfrc_constraint; measured 4.050e-1
TOL_BIAS = 4 * 4.960e-4       # N / N m, qfrc_bias; measured 4.960e-4
TOL_F_CONTACT = 4 * 3.966e-1  # N, per-contact forces; measured 3.966e-1
TOL_NET_F = 4 * 4.050e-1      # N, net contact force; measured 4.050e-1
TOL_NET_TAU = 4 * 2.321e-1    # N m, net contact torque about the world origin; measured 2.321e-1
TOLS = dict(qfrc_inverse=TOL_QINV, qfrc_constraint=TOL_QCON, qfrc_bias=TOL_BIAS, contact_force=TOL_F_CONTACT, net_force=TOL_NET_F, net_torque=TOL_NET_TAU)
MEASURED = H.Measured()


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


# ---------------------------------------------------------------- cases: (state, qacc) with the fp64 reference, computed once

_CASES = {}


def cases(scene):
    """list of dict(name, q, v, a, blk, ref, edge); scene: floor | g_sit | sweep.  Inputs are fp32-representable; ref = the oracle composition on them."""
    if scene in _CASES:
        return _CASES[scene]
    kf, ks = KPMS[DEFAULT_KPM], KPMS[STEP_KPM]
    named = ID.named_states(kf, ks, STD["qpos"], STD["qvel"])
    sts = {"floor": named[:-1], "g_sit": named[-1:], "sweep": None}[scene] or ID.sweep_states(kf, STD["qpos"])
    margin = float(kf["opt"][ID.MARGIN_OPT])
    out = []
    for s in sts:
        path = STEP_KPM if s["step"] else DEFAULT_KPM
        o = ID.prepared(path, KPMS[path], s["q"], s["v"], s["blk"])
        for k, a in ID.qacc_choices(o, s["name"]).items():
            a = ID.f32(a)
            ref = ID.compose(o, KPMS[path], a)
            out.append(dict(name=f"{s['name']}/{k}", q=s["q"], v=s["v"], a=a, blk=s["blk"], ref=ref, edge=ID.on_edge(o, KPMS[path], ref, margin)))
    _CASES[scene] = out
    return out


def run(sim, cs, blk="own", want=OUT_KEYS, qvel=True):
    """the kernel on the rows of cs -> numpy outputs.  blk: 'own' the cases' blocks, None no object argument, 'parked' all five parked"""
    st = lambda k: dev(np.stack([c[k] for c in cs]))  # noqa: E731
    obj = None
    if blk == "parked":
        obj = dev(np.tile(ID.f32(CF.parked_block()), (len(cs), 1)))
    elif blk == "own" and cs[0]["blk"] is not None:
        obj = st("blk")
    out = sim.inverse_dynamics(st("q"), st("v") if qvel else None, st("a"), obj, want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def rows_of(out, e):
    n = int(out["ncon"][e]); c = out["contact"][e].astype(np.float64)
    return dict(body=c[:n, 0].astype(int), b2=c[:n, 1].astype(int), dist=c[:n, 2], pos=c[:n, 3:6], normal=c[:n, 6:9], force=c[:n, 9:12])


def compare(out, e, ref, local):
    """deviations of row e from the reference -> local and MEASURED; returns the number of contacts present on one side only WITH a force"""
    def rec(k, v):
        MEASURED.note(k, v, local)
    for k in ("qfrc_inverse", "qfrc_constraint", "qfrc_bias"):
        rec(k, np.abs(out[k][e] - ref[k]).max())
    rec("net_force", np.abs(out["net_wrench"][e][:3] - ref["net_wrench"][:3]).max())
    rec("net_torque", np.abs(out["net_wrench"][e][3:] - ref["net_wrench"][3:]).max())
    got = rows_of(out, e)
    assert not out["contact"][e][len(got["body"]):].any(), "rows >= ncon are exactly zero"
    pairs, only_got, only_ref = CF.match_contacts(got, ref["contacts"])
    bad = 0
    for i, j in pairs:
        rec("contact_force", np.abs(got["force"][i] - ref["force"][j]).max())
    for f in [got["force"][i] for i in only_got] + [ref["force"][j] for j in only_ref]:
        rec("unmatched_force", np.abs(f).max()); bad += np.abs(f).max() > TOL_F_CONTACT
    return bad


def check(label, local, bad):
    print(f"parity {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in local.items()) + " || running maxima " + ", ".join(f"{k} {v:.3e}" for k, v in MEASURED.items()))
    assert bad == 0, "a contact present on one side only must carry no force"
    for k, tol in TOLS.items():
        assert local.get(k, 0.0) <= tol, (k, local[k], tol)


# ---------------------------------------------------------------- (f) parity with the fp64 composition

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("scene", ["floor", "parked", "g_sit"])
def test_parity(kp, scene, n):
    base = cases("g_sit" if scene == "g_sit" else "floor")
    assert not any(c["edge"] for c in base), "no named case is on an edge (tests/test_inverse_dynamics_cpu.py)"
    cs = [base[e % len(base)] for e in range(n)]
    sim = handle(kp, DEFAULT_KPM if scene == "floor" else STEP_KPM)
    out = run(sim, cs, blk=None if scene != "g_sit" else "own")
    local, bad = {}, 0
    for e, c in enumerate(cs):
        bad += compare(out, e, c["ref"], local)
    if scene == "parked":            # an object blob without the object argument and with all five parked: the same bits
        other = run(sim, cs, blk="parked")
        for k in OUT_KEYS:
            assert np.array_equal(out[k].view(np.int32), other[k].view(np.int32)), k
    if scene == "g_sit":
        assert all(np.any(rows_of(out, e)["pos"][:, 2] > 0.3) for e in range(n)), "the seat carries contacts"
    check(f"{scene} n={n}", local, bad)


def test_parity_sweep(kp):
    cs_all = cases("sweep")
    cs = [c for c in cs_all if not c["edge"]]
    assert len(cs_all) == 3 * 64 and len(cs_all) - len(cs) <= EDGE_CAP * len(cs_all)
    out = run(handle(kp, DEFAULT_KPM), cs)
    local, bad = {}, 0
    worst = []
    for e, c in enumerate(cs):
        bad += compare(out, e, c["ref"], local)
        fmax = np.abs(c["ref"]["force"]).max() if c["ref"]["ncon"] else 0.0
        worst.append((np.abs(out["qfrc_constraint"][e] - c["ref"]["qfrc_constraint"]).max(), fmax, c["name"]))
    print("sweep, largest qfrc_constraint deviations (deviation, largest contact force, case): " + "; ".join(f"{d:.3e} N at {f:.3e} N {n}" for d, f, n in sorted(worst, reverse=True)[:4]))
    assert sum(int(n) > 0 for n in out["ncon"]) >= len(cs) // 2, "the sweep is in contact"
    check(f"sweep ({len(cs)} of {len(cs_all)} cases)", local, bad)


# ---------------------------------------------------------------- (g) device-only round trip forward -> inverse

@pytest.mark.parametrize("n", ROWS)
def test_forward_inverse_round_trip(kp, n):
    """kp_sim_contact_forces mode 1 solves for qacc under a given torque; the inverse at that qacc returns the torque.  The Newton solve stops on
    scale |gradient| < tol and that gradient IS qfrc_inverse - torque, so the bound is tol / scale plus the fp32 error of the parity tests."""
    kpm = KPMS[DEFAULT_KPM]
    fl = {c["name"].split("/")[0]: c for c in cases("floor")}
    base = [fl[k] for k in ("a_standing", "d_lying", "f_falling")]
    cs = [base[e % 3] for e in range(n)]
    sim = kp.KpSim(kp.KpModel(), n)
    q, v = dev(np.stack([c["q"] for c in cs])), dev(np.stack([c["v"] for c in cs]))
    sim.set_state(q, v)
    rng = np.random.default_rng(5)
    tau = dev(np.concatenate([rng.normal(size=(n, 6)) * 10.0, rng.normal(size=(n, 69)) * 20.0], 1))
    fwd = sim.contact_forces(torque=tau, want=("qacc", "qfrc_constraint", "torque", "ncon"))
    assert torch.equal(fwd["torque"], tau)
    inv = sim.inverse_dynamics(q, v, fwd["qacc"], want=("qfrc_inverse", "qfrc_constraint", "ncon"))
    assert torch.equal(inv["ncon"], fwd["ncon"])
    opt = dict(zip(OPT_FIELDS, kpm["opt"]))
    stop = sim.model.get_option("solver_tol") * opt["meaninertia"] * opt["nv_full"]            # tol / scale
    d_tau = (inv["qfrc_inverse"] - tau).abs().max().item()
    d_con = (inv["qfrc_constraint"] - fwd["qfrc_constraint"]).abs().max().item()
    print(f"round trip n={n}: |qfrc_inverse - torque| {d_tau:.3e}, |qfrc_constraint difference| {d_con:.3e}, tol / scale {stop:.3e}, fp32 share {TOL_QINV:.3e}")
    assert int(sim.diag()[:, 2].max()) == 0
    assert d_tau <= stop + TOL_QINV and d_con <= stop + TOL_QINV


# ---------------------------------------------------------------- (h) bitwise

@pytest.mark.parametrize("scene", ["floor", "g_sit"])
def test_bitwise(kp, scene):
    base = cases(scene)
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
    lead = sim.inverse_dynamics(dev(np.stack([c["q"] for c in cs[:6]])).view(2, 3, 76), want=("qfrc_inverse", "ncon"))     # leading shape; qacc = NULL
    zero = [dict(c, v=np.zeros(75), a=np.zeros(75)) for c in cs[:6]]
    if scene == "floor":
        assert lead["qfrc_inverse"].shape == (2, 3, 75) and lead["ncon"].shape == (2, 3)
        assert np.array_equal(lead["qfrc_inverse"].cpu().numpy().reshape(6, 75).view(np.int32), run(sim, zero)["qfrc_inverse"].view(np.int32))


# ---------------------------------------------------------------- (i) nothing else moves

@pytest.mark.parametrize("scene", ["floor", "h_push"])
def test_the_control_step_is_bit_identical(kp, scene):
    fl = cases("floor")
    rows = fl[:5] if scene == "floor" else [dict(fl[0], blk=ID.f32(CF.object_scenes(KPMS[STEP_KPM], STD["qpos"])["h_push"][2]))] * 5
    H.control_step_untouched(kp, scene, lambda sim: H.same_bits(run(sim, rows), run(sim, rows), OUT_KEYS))


# ---------------------------------------------------------------- (j) refusals

def test_refusals(kp, tmp_path):
    sim = handle(kp, DEFAULT_KPM)
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    bufs, full = H.sentinel(kp.INVDYN_OUTPUTS, kp.KpInvDynOut)
    q = dev(np.tile(ID.f32(STD["qpos"]), (5, 1)))
    qp, blk = ctypes.c_void_p(q.data_ptr()), dev(np.tile(ID.f32(CF.parked_block()), (5, 1)))
    f = L.kp_sim_inverse_dynamics
    assert f(None, 5, qp, None, None, None, ctypes.byref(full)) != 0 and "null handle" in err()
    assert f(sim.h, 5, None, None, None, None, ctypes.byref(full)) != 0 and "null qpos" in err()
    assert f(sim.h, 5, qp, None, None, None, None) != 0 and "null out" in err()
    assert f(sim.h, 5, qp, None, None, None, ctypes.byref(kp.KpInvDynOut())) != 0 and "every output of out is null" in err()
    assert f(sim.h, -1, qp, None, None, None, ctypes.byref(full)) != 0 and "n_rows" in err()
    from kinpoly_amd.model_compiler import write_kpm
    m = read_kpm(DEFAULT_KPM)
    m["obj_geoms"] = np.zeros((0, 18), m["obj_geoms"].dtype)
    write_kpm(m, str(tmp_path / "no_objects.kpm"))
    bare = kp.KpSim(kp.KpModel(str(tmp_path / "no_objects.kpm")), 1)
    assert f(bare.h, 5, qp, None, None, ctypes.c_void_p(blk.data_ptr()), ctypes.byref(full)) != 0 and "obj_qpos" in err() and "no object geoms" in err()
    wide = kp.KpSim(kp.KpModel(threads_per_env=128), 5)
    assert f(wide.h, 5, qp, None, None, None, ctypes.byref(full)) != 0 and "threads_per_env" in err()
    assert f(sim.h, 0, qp, None, None, None, ctypes.byref(full)) == 0, "n_rows == 0 does nothing"
    H.refused_calls_wrote_nothing(bufs)
    with pytest.raises(ValueError):
        sim.inverse_dynamics(q, want=("qacc",))
    with pytest.raises(ValueError):
        sim.inverse_dynamics(q, qvel=q)
    assert sim.inverse_dynamics(q[:0])["qfrc_inverse"].shape == (0, 75)


# ---------------------------------------------------------------- (k) the metric

def test_coverage_dynamics_metrics(kp):
    from kinpoly_amd.metrics import coverage_dynamics_metrics
    T = 12
    still = np.tile(ID.f32(STD["qpos"]), (T, 1))
    # a standing-still take is plausible only where the pose is in static balance on its contacts; what the score must show is that the contacts are
    # credited: the same pose held still one metre up needs the whole body weight from nowhere
    air = still.copy(); air[:, 2] += 1.0
    obj = np.tile(ID.f32(CF.parked_block()), (T, 1))
    results = {"sit-still": dict(pred=np.concatenate([still, np.zeros((T, 3))], 1), obj_pose=obj), "none-air": dict(pred=air, obj_pose=obj)}
    gt = {"sit-still": dict(qpos=still), "none-air": dict(qpos=air)}
    m = coverage_dynamics_metrics(results, gt, handle(kp, STEP_KPM))
    keys = [f"{a}_{b}" for a in ("resid_force", "resid_torque", "torque_rms", "over_limit", "power") for b in ("pred", "gt")]
    assert all(np.isfinite(m[k]) for k in keys) and set(m["by_action"]) == {"sit", "none"}
    tol = TOL_QINV / BODY_WEIGHT
    a = m["per_take"]["none-air"]
    print(f"dynamics metrics: still {m['per_take']['sit-still']}, air {a}; tolerance {tol:.2e}")
    assert abs(a["resid_force_pred"] - 1.0) <= tol and abs(a["resid_force_gt"] - 1.0) <= tol
    assert a["power_pred"] == 0.0 and m["per_take"]["sit-still"]["resid_force_pred"] == m["per_take"]["sit-still"]["resid_force_gt"]
    assert m["by_action"]["none"]["resid_force_pred"] == a["resid_force_pred"]
    s = static_balance_take(kp, T)
    ms = coverage_dynamics_metrics({"none-balance": dict(pred=s, obj_pose=obj)}, {"none-balance": dict(qpos=s)}, handle(kp, DEFAULT_KPM))
    print(f"standing still in balance: resid_force {ms['resid_force_pred']:.3e} of body weight")
    assert ms["resid_force_pred"] <= tol


def static_balance_take(kp, T):
    """A standing-still take: the standing pose at the height where the floor carries the weight, held for T frames.  Held still (qvel = qacc = 0) the
    contacts push straight up with a force that rises by about 4e6 N per metre of depth (solref 0.02 s: the weight sits 0.2 mm deep), so balance to
    the parity tolerance (5e-5 of body weight) is finer than one fp32 step of the root height (6e-8 m = 0.2 N).  Two bisections on the sign of the
    vertical residual: the root height down to neighbouring floats, then a common offset on the two ankles' pitch hinges (1e-9 m per step)."""
    sim = handle(kp, DEFAULT_KPM)
    base = ID.f32(STD["qpos"]).astype(np.float32)

    def resid_z(q):
        return float(sim.inverse_dynamics(torch.tensor(q[None], device="cuda"))["qfrc_inverse"][0, 2])

    def bisect(make, lo, hi):
        lo, hi = np.float32(lo), np.float32(hi)
        flo, fhi = resid_z(make(lo)), resid_z(make(hi))
        assert flo * fhi <= 0.0, ("the bracket holds no balance point", lo, hi, flo, fhi)
        for _ in range(64):
            mid = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
            if mid == lo or mid == hi:
                break
            fm = resid_z(make(mid))
            if fm * flo > 0.0:
                lo, flo = mid, fm
            else:
                hi, fhi = mid, fm
        return (lo, flo) if abs(flo) <= abs(fhi) else (hi, fhi)

    def at_height(z):
        q = base.copy(); q[2] = z
        return q
    z, fz = bisect(at_height, base[2] - 0.03, base[2] + 0.03)

    def with_ankles(d):
        q = at_height(z); q[7 + 3 * 2 + 2] += d; q[7 + 3 * 6 + 2] += d        # bodies 3 and 7 (the ankles), third hinge
        return q
    d, fd = bisect(with_ankles, -2e-3, 2e-3)
    print(f"balanced standing pose: root height {z:.8f} leaves {fz:.3e} N, ankle offset {d:.3e} rad leaves {fd:.3e} N")
    return np.tile(with_ankles(d).astype(np.float64), (T, 1))
