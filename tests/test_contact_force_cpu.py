"""Contact-force read-out without a GPU: identities of the fp64 reference tests/contact_force_oracle.py on OracleSim alone, the closed forms of
kinpoly_amd.contact on CPU tensors, and the surface (header, binding table, exported symbol, documents, script flags, grf_metrics)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import contact_force_oracle as CF
from kinpoly_amd import build as kpbuild
from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
from oracle.kpo import OracleSim

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)


@pytest.fixture(scope="module")
def rollout_states():
    """(qpos, qvel) after each of 40 control steps from standing_neutral (and the start): zero action for 10 steps, then seeded Gaussian actions of scale 0.3"""
    o = OracleSim(ls_exact=True)
    o.reset(STD["qpos"], STD["qvel"])
    rng = np.random.default_rng(2024)
    out = [(o.get("qpos"), o.get("qvel"))]
    for k in range(40):
        a = np.zeros(75) if k < 10 else rng.normal(size=75) * 0.3
        o.do_simulation(a, STD["qpos"], 15)
        out.append((o.get("qpos"), o.get("qvel")))
    return out


def test_oracle_identities(rollout_states):
    """J^T efc_force == qfrc_constraint and qfrc_constraint[0:3] == sum of the contact forces, to 1e-10 max(1, |.|_inf), on every state of the roll-out"""
    o = OracleSim(ls_exact=True)
    ncons, worst = [], 0.0
    for qpos, qvel in rollout_states:
        o.reset(qpos, qvel)
        r = CF.oracle_contact_forces(o, 0, None, None, KPM)
        qc = r["qfrc_constraint"]
        bound = 1e-10 * max(1.0, np.abs(qc).max())
        jtf = r["J"][:, :75].T @ r["efc_force"] if len(r["efc_force"]) else np.zeros(75)
        assert np.abs(jtf - qc).max() <= bound
        hum = r["contacts"]["body"] < 24
        fsum = r["force"][hum].sum(0) if hum.any() else np.zeros(3)
        assert np.abs(qc[:3] - fsum).max() <= bound
        assert np.abs(r["wrench"][:24, :3].sum(0) - fsum).max() <= bound
        worst = max(worst, np.abs(jtf - qc).max(), np.abs(qc[:3] - fsum).max())
        ncons.append(len(r["contacts"]["body"]))
    print(f"identities hold to {worst:.1e}; contacts per state {min(ncons)}..{max(ncons)}")
    assert max(ncons) >= 8          # the roll-out is in contact (the identity is not vacuous)


def test_oracle_joint_limit_row():
    """a joint pushed past its limit: the contact list is unaffected and the limit row's force shows on its own dof"""
    lo_hi = KPM["jnt_range"].reshape(69, 2)
    j = 48                                                  # a wrist hinge: no hull that touches the floor moves with it
    assert KPM["jnt_limited"][j]
    o = OracleSim(ls_exact=True)
    o.reset(STD["qpos"], STD["qvel"])
    base = CF.oracle_contact_forces(o, 0, None, None, KPM)
    assert base["nlim"] == 0
    q = STD["qpos"].copy(); q[7 + j] = lo_hi[j, 1] + 0.2
    o.reset(q, STD["qvel"])
    r = CF.oracle_contact_forces(o, 0, None, None, KPM)
    assert r["nlim"] == 1 and r["qfrc_constraint"][6 + j] != 0.0
    assert list(r["contacts"]["body"]) == list(base["contacts"]["body"])
    np.testing.assert_allclose(r["contacts"]["pos"], base["contacts"]["pos"], atol=1e-12)
    jtf = r["J"][:, :75].T @ r["efc_force"]
    assert np.abs(jtf - r["qfrc_constraint"]).max() <= 1e-10 * max(1.0, np.abs(jtf).max())


# ---------------------------------------------------------------- kinpoly_amd.contact closed forms

def _wrench_of(points, forces):
    w = torch.zeros(1, 26, 6, dtype=torch.float64)
    for b, p, f in zip((3, 4, 7, 8), points, forces):
        p, f = torch.tensor(p, dtype=torch.float64), torch.tensor(f, dtype=torch.float64)
        w[0, b, :3] += f; w[0, b, 3:] += torch.linalg.cross(p, f)
    return w


def test_ground_reaction_closed_forms():
    from kinpoly_amd.contact import FOOT_BODIES, ground_reaction, shift_wrench
    assert FOOT_BODIES == {"L": (3, 4), "R": (7, 8)}
    # one force at a point of z = 0 on the left ankle: CoP = the point, free moment 0; the right foot carries nothing -> NaN, no support
    w = _wrench_of([(0.3, -0.2, 0.0)], [(12.0, -7.0, 400.0)])
    g = ground_reaction(w, min_fz=1.0)
    assert g["force"].shape == (1, 2, 3) and g["cop"].shape == (1, 2, 2) and g["support"].shape == (1, 2)
    np.testing.assert_allclose(g["cop"][0, 0].numpy(), [0.3, -0.2], atol=1e-12)
    assert abs(float(g["free_moment"][0, 0])) < 1e-12
    assert bool(g["support"][0, 0]) and not bool(g["support"][0, 1])
    assert torch.isnan(g["cop"][0, 1]).all() and torch.isnan(g["free_moment"][0, 1])
    # two forces on one foot (ankle + toe): the F_z-weighted mean of the points
    w = _wrench_of([(0.1, 0.0, 0.0), (0.3, 0.1, 0.0)], [(0.0, 0.0, 100.0), (0.0, 0.0, 300.0)])
    g = ground_reaction(w)
    np.testing.assert_allclose(g["cop"][0, 0].numpy(), [0.25, 0.075], atol=1e-12)
    np.testing.assert_allclose(g["force"][0, 0].numpy(), [0, 0, 400.0])
    # F_z <= min_fz: NaN and support False, at the threshold too
    w = _wrench_of([(0.1, 0.0, 0.0)], [(0.0, 0.0, 5.0)])
    g = ground_reaction(w, min_fz=5.0)
    assert not bool(g["support"][0, 0]) and torch.isnan(g["cop"][0, 0]).all()
    # group sums are the sums of the entity rows
    rng = torch.Generator().manual_seed(3)
    w = torch.randn(4, 26, 6, generator=rng, dtype=torch.float64)
    g = ground_reaction(w, groups={"a": (0, 5, 9), "b": (24,), "c": tuple(range(26))}, min_fz=-1e9)
    np.testing.assert_allclose(g["force"][:, 0].numpy(), w[:, [0, 5, 9], :3].sum(1).numpy(), atol=1e-12)
    np.testing.assert_allclose(g["torque"][:, 1].numpy(), w[:, 24, 3:].numpy(), atol=1e-12)
    np.testing.assert_allclose(g["force"][:, 2].numpy(), w[..., :3].sum(1).numpy(), atol=1e-12)
    # shift_wrench composes, keeps the force, and moving to the point of application removes the torque of a pure force
    a, b = torch.tensor([0.3, -1.0, 2.0], dtype=torch.float64), torch.tensor([-0.7, 0.2, 0.1], dtype=torch.float64)
    np.testing.assert_allclose(shift_wrench(shift_wrench(w, a), b).numpy(), shift_wrench(w, a + b).numpy(), atol=1e-12)
    np.testing.assert_allclose(shift_wrench(w, a)[..., :3].numpy(), w[..., :3].numpy())
    w1 = _wrench_of([(0.3, -0.2, 0.5)], [(1.0, 2.0, 3.0)])
    assert shift_wrench(w1, (0.3, -0.2, 0.5))[0, 3, 3:].abs().max() < 1e-12


def test_mass_and_weight():
    from kinpoly_amd.contact import body_weight, total_mass
    m = total_mass(DEFAULT_KPM)
    assert abs(m - float(KPM["body_mass"].sum())) < 1e-9 and abs(m - total_mass(KPM)) < 1e-12
    assert abs(body_weight(KPM) - 9.81 * m) < 1e-9
    assert abs(float(np.linalg.norm(KPM["opt"][1:4])) - 9.81) < 1e-12          # the constant is the model's gravity


# ---------------------------------------------------------------- surface

def test_entry_point_surface():
    header = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    assert "kp_sim_contact_forces(" in header and "kp_contact_out" in header
    from kinpoly_amd.sim import _SIGNATURES, ABI_SYMBOLS, KpContactOut
    assert "kp_sim_contact_forces" in _SIGNATURES and "kp_sim_contact_forces" in ABI_SYMBOLS
    assert [f[0] for f in KpContactOut._fields_] == ["ncon", "contact", "wrench", "qfrc_constraint", "qacc", "torque", "obj_qacc"]
    if not os.path.exists(kpbuild.LIB):
        kpbuild.build_native()
    L = ctypes.CDLL(kpbuild.LIB)
    assert hasattr(L, "kp_sim_contact_forces")
    L.kp_sim_contact_forces.restype = ctypes.c_int
    L.kp_sim_contact_forces.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.kp_last_error.restype = ctypes.c_char_p
    assert L.kp_sim_contact_forces(None, 0, None, None, None) == -1 and b"kp_sim_contact_forces: null handle" in L.kp_last_error()
    assert "kp_sim_contact_forces" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("script", ["eval_ar_policy.py", "eval_uhc.py"])
def test_scripts_take_grf(script):
    spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(ROOT, "scripts", script))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert p.parse_args([]).grf is False and p.parse_args(["--grf"]).grf is True


def test_grf_metrics_known_answer():
    from kinpoly_amd.metrics import grf_metrics
    W = 800.0
    grf = np.zeros((3, 2, 3)); grf[0, :, 2] = [400.0, 400.0]; grf[1, 0, 2] = 1200.0; grf[2] = 0.0
    res = {"a": {"grf": grf[:2], "foot_contact": np.array([[True, True], [True, False]])},
           "b": {"grf": grf[2:], "foot_contact": np.array([[False, False]])}}
    m = grf_metrics(res, W)
    assert m["frames"] == 3
    assert abs(m["grf_mean_bw"] - (1.0 + 1.5 + 0.0) / 3) < 1e-12 and abs(m["grf_peak_bw"] - 1.5) < 1e-12
    assert abs(m["no_support"] - 1 / 3) < 1e-12 and abs(m["double_support"] - 1 / 3) < 1e-12
    with pytest.raises(KeyError):
        grf_metrics({"c": {"pred": []}}, W)
