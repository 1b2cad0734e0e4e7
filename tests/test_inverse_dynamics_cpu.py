"""Inverse dynamics without a GPU: the fp64 composition tests/inverse_dynamics_oracle.py is an inverse of OracleSim's own forward,
its known answers, kinpoly_amd.dynamics on CPU tensors, the edge classification the GPU sweep relies on, and the surface (header, binding table, symbol)."""
import ctypes
import os

import numpy as np
import pytest

import inverse_dynamics_oracle as ID
from kinpoly_amd import build as kpbuild
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm
from oracle import np_oracle as O

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM, KPM_STEP = read_kpm(DEFAULT_KPM), read_kpm(STEP_KPM)
WEIGHT = float(KPM["body_mass"].sum()) * 9.81
EDGE_CAP = 0.05


def blob(s):
    return (STEP_KPM, KPM_STEP) if s["step"] else (DEFAULT_KPM, KPM)


@pytest.fixture(scope="module")
def named():
    return ID.named_states(KPM, KPM_STEP, STD["qpos"], STD["qvel"])


# ---------------------------------------------------------------- (a) the composition inverts the oracle's forward

def test_round_trip(named):
    """qfrc_inverse put in as actuation: forward() returns the given qacc to 1e-8 relative (the forward problem is strictly convex: one minimiser)"""
    worst, ncons = 0.0, {}
    for s in named:
        path, kpm = blob(s)
        o = ID.prepared(path, kpm, s["q"], s["v"], s["blk"])
        cases = {k: (a, ID.compose(o, kpm, a)) for k, a in ID.qacc_choices(o, s["name"]).items()}
        for k, (a, r) in cases.items():
            tau = r["qfrc_inverse"]
            o.set_ctrl(tau[6:], tau[:6])
            o.forward()
            err = np.abs(o.get("qacc") - a).max() / max(1.0, np.abs(a).max())
            worst = max(worst, err)
            assert err <= 1e-8, (s["name"], k, err)
            ncons[s["name"]] = r["ncon"]
        assert np.abs(cases["forward"][1]["qfrc_inverse"]).max() <= 1e-6, "the state's own unactuated acceleration needs no force"
    print(f"round trip: worst relative deviation {worst:.2e}; contacts {ncons}")
    assert ncons["d_lying"] >= 12 and ncons["g_sit"] >= 1 and ncons["c_airborne"] == 0


def test_sit_touches_the_chair(named):
    s = named[-1]
    o = ID.prepared(STEP_KPM, KPM_STEP, s["q"], s["v"], s["blk"])
    con = o.contacts_full()
    assert np.all(con["b2"] == -1), "no dynamic object slot: the chair is a static obstacle (B = -1 like the floor)"
    assert np.any(con["pos"][:, 2] > 0.3), "g_sit must press on the chair's seat (0.41 m above the floor)"


# ---------------------------------------------------------------- (b) known answers

def airborne():
    q = ID.f32(STD["qpos"]); q[2] += 1.0
    return q, np.zeros(75)


def test_known_answer_hold_still_in_the_air():
    """airborne, all velocities zero, qacc = 0: the root force is the weight, straight up, and its torque about the COM is zero"""
    from kinpoly_amd import dynamics as DY
    q, v = airborne()
    o = ID.prepared(DEFAULT_KPM, KPM, q, v)
    r = ID.compose(o, KPM, np.zeros(75))
    assert r["ncon"] == 0 and r["nlim"] == 0
    f, tq = DY.root_residual(torch.tensor(r["qfrc_inverse"]), torch.tensor(q))
    f, tq = f.numpy(), tq.numpy()
    assert np.abs(f - [0.0, 0.0, WEIGHT]).max() <= 1e-9 * WEIGHT
    com = (o.get("xipos").reshape(24, 3) * KPM["body_mass"][:, None]).sum(0) / KPM["body_mass"].sum()
    assert np.abs(tq - np.cross(com - q[:3], f)).max() <= 1e-9 * WEIGHT, "torque about the root = (com - root) x F: zero about the COM"


def test_known_answer_free_fall():
    """the same pose with qacc[2] = -g: nothing is needed, neither on the root nor at any joint"""
    q, v = airborne()
    o = ID.prepared(DEFAULT_KPM, KPM, q, v)
    a = np.zeros(75); a[2] = -9.81
    r = ID.compose(o, KPM, a)
    assert np.abs(r["qfrc_inverse"]).max() <= 1e-9 * WEIGHT


# ---------------------------------------------------------------- (c) motion_derivatives

def _clip(T, seed):
    rng = np.random.default_rng(seed)
    q = np.tile(STD["qpos"].astype(np.float64), (T, 1))
    q[:, :3] += np.cumsum(rng.normal(size=(T, 3)) * 0.01, 0)
    q[:, 7:] += np.cumsum(rng.normal(size=(T, 69)) * 0.02, 0)
    for t in range(T):
        ang = 0.05 * t
        q[t, 3:7] = O.quaternion_multiply(np.array([np.cos(ang), 0.0, np.sin(ang) * 0.6, np.sin(ang) * 0.8]), q[t, 3:7])
    return q


def _reference_derivatives(q, dt):
    T = len(q)
    v = np.zeros((T, 75))
    for t in range(T - 1):
        v[t] = O.get_qvel_fd_new(q[t], q[t + 1], dt)
    if T > 1:
        v[T - 1] = v[T - 2]
    a = np.zeros((T, 75))
    for t in range(T - 2):
        a[t] = (v[t + 1] - v[t]) / dt
    if T > 2:
        a[T - 2] = a[T - 1] = a[T - 3]
    return v, a


def test_motion_derivatives_rows():
    from kinpoly_amd import dynamics as DY
    dt = 1.0 / 30.0
    qa, qb = _clip(9, 1), _clip(6, 2)
    v, a = DY.motion_derivatives(torch.tensor(qa), dt)
    vr, ar = _reference_derivatives(qa, dt)
    assert np.abs(v.numpy() - vr).max() <= 1e-9 and np.abs(a.numpy() - ar).max() <= 1e-7
    assert np.abs(ar).max() > 10.0, "no clamp at +-10: the clip's accelerations exceed it"
    # two takes back to back: no difference crosses the boundary
    both = np.concatenate([qa, qb])
    v2, a2 = DY.motion_derivatives(torch.tensor(both), dt, take_off=[0, 9, 15])
    vb, ab = _reference_derivatives(qb, dt)
    assert np.abs(v2.numpy() - np.concatenate([vr, vb])).max() <= 1e-9 and np.abs(a2.numpy() - np.concatenate([ar, ab])).max() <= 1e-7
    v1, _ = DY.motion_derivatives(torch.tensor(both), dt)
    assert np.abs(v1.numpy()[8] - v2.numpy()[8]).max() > 1e-3, "without the table the difference does cross"
    # short takes
    v3, a3 = DY.motion_derivatives(torch.tensor(both[:3]), dt, take_off=[0, 1, 3])
    assert not v3[0].any() and not a3.any()
    with pytest.raises(ValueError):
        DY.motion_derivatives(torch.tensor(both), dt, take_off=[0, 9, 14])


# ---------------------------------------------------------------- (d) plausibility / root_residual arithmetic

def test_root_residual_and_plausibility_arithmetic():
    from kinpoly_amd import dynamics as DY
    # root turned 90 degrees about z: the root's x axis is world y
    q = torch.zeros(2, 76, dtype=torch.float64); q[:, 3] = 1.0
    q[1, 3:7] = torch.tensor([np.cos(np.pi / 4), 0.0, 0.0, np.sin(np.pi / 4)])
    tau = torch.zeros(2, 75, dtype=torch.float64)
    tau[:, :3] = torch.tensor([3.0, 0.0, 4.0]); tau[:, 3:6] = torch.tensor([2.0, 0.0, 0.0])
    tau[0, 6:] = 1.0; tau[1, 6] = 10.0; tau[1, 7] = -30.0
    f, t = DY.root_residual(tau, q)
    assert torch.equal(f, tau[:, :3])
    assert np.abs(t[0].numpy() - [2.0, 0.0, 0.0]).max() <= 1e-15 and np.abs(t[1].numpy() - [0.0, 2.0, 0.0]).max() <= 1e-15
    v = torch.zeros(2, 75, dtype=torch.float64); v[0, 6:] = 2.0; v[1, 6] = -1.0; v[1, 7] = 0.5; v[:, :6] = 100.0
    lim = torch.full((69,), 20.0, dtype=torch.float64)
    p = DY.plausibility(tau, q, v, lim, weight=10.0)
    assert np.allclose(p["resid_force"].numpy(), [0.5, 0.5], rtol=0, atol=1e-15)
    assert np.allclose(p["resid_torque"].numpy(), [2.0, 2.0], rtol=0, atol=1e-15)
    assert np.allclose(p["joint_torque_rms"].numpy(), [1.0, np.sqrt(1000.0 / 69)], rtol=0, atol=1e-14)
    assert np.allclose(p["over_limit"].numpy(), [0.0, 1.0 / 69], rtol=0, atol=1e-15)
    assert np.allclose(p["power"].numpy(), [138.0, 25.0], rtol=0, atol=1e-13)
    assert abs(float(p["mean"]["power"]) - 81.5) <= 1e-13 and abs(float(p["mean"]["over_limit"]) - 0.5 / 69) <= 1e-15
    assert set(p["mean"]) == {"resid_force", "resid_torque", "joint_torque_rms", "over_limit", "power"}


# ---------------------------------------------------------------- (e) edge classification

def _edges(states):
    margin = float(KPM["opt"][ID.MARGIN_OPT])
    out = {}
    for s in states:
        path, kpm = blob(s)
        o = ID.prepared(path, kpm, s["q"], s["v"], s["blk"])
        for k, a in ID.qacc_choices(o, s["name"]).items():
            out[(s["name"], k)] = ID.on_edge(o, kpm, ID.compose(o, kpm, a), margin)
    return out


def test_no_named_case_is_on_an_edge(named):
    e = _edges(named)
    assert len(e) == 3 * len(named)
    assert not [k for k, v in e.items() if v]


def test_sweep_edge_share_is_under_the_cap():
    e = _edges(ID.sweep_states(KPM, STD["qpos"]))
    bad = [k for k, v in e.items() if v]
    print(f"sweep: {len(bad)} of {len(e)} cases on an edge: {bad}")
    assert len(e) == 3 * 64 and len(bad) <= EDGE_CAP * len(e)


# ---------------------------------------------------------------- the surface

def test_header_binding_and_symbol():
    from kinpoly_amd import sim as kpsim
    hdr = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    assert "int kp_sim_inverse_dynamics(kp_sim*, int n_rows, const float* qpos, const float* qvel, const float* qacc, const float* obj_qpos, const kp_invdyn_out* out);" in hdr
    assert "typedef struct { float *qfrc_inverse, *qfrc_constraint, *qfrc_bias, *contact, *net_wrench; int32_t* ncon; } kp_invdyn_out;" in hdr
    assert "mj_inverse" in hdr
    assert len(kpsim._SIGNATURES["kp_sim_inverse_dynamics"][1]) == 7
    assert [f[0] for f in kpsim.KpInvDynOut._fields_] == list(kpsim.INVDYN_OUTPUTS)
    if not os.path.exists(kpbuild.LIB):
        pytest.fail(f"{kpbuild.LIB} is missing: build() first")
    assert hasattr(ctypes.CDLL(kpbuild.LIB), "kp_sim_inverse_dynamics")
