"""Pose fitting and point Jacobians without a GPU: the fp64 reference tests/fit_pose_oracle.py against finite differences, the
inertia analogy the kernel rests on, the reference's convergence on EVERY case the GPU tests use (this is where the inputs are chosen), the host logic
of kinpoly_amd/fit.py and scripts/fit_takes.py, and the library's surface."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fit_pose_oracle as FP  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import push_oracle as PO  # noqa: E402
from kinpoly_amd import build as kpbuild  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)
GOLDEN = os.path.join(ROOT, "tests", "golden", "fit_pose_noisy_ref.npz")


@pytest.fixture(scope="module")
def o():
    return FP.oracle(DEFAULT_KPM)


@pytest.fixture(scope="module")
def states():
    named = ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"])
    return named, ID.sweep_states(KPM, STD["qpos"])


# ---------------------------------------------------------------- the reference itself

def test_reference_jacobian_against_central_differences(o, states):
    """J of the reference (origin velocities and angular velocities per unit dof velocity) = d/d eps of the oracle's FK along q (+) eps e_k"""
    eps = 1e-6
    worst = 0.0
    for name, q in FP.jacobian_poses(STD["qpos"], states[0]).items():
        J, xpos, xquat = FP.origin_jacobians(o, q)
        for k in range(FP.NV):
            e = np.zeros(FP.NV); e[k] = eps
            xp, xq = FP.fk(o, FP.oplus(q, e)); xm, xqm = FP.fk(o, FP.oplus(q, -e))
            lin = (xp - xm) / (2 * eps)
            ang = np.stack([FP.quat_log(FP.qmul(xq[b], xqm[b] * np.array([1.0, -1, -1, -1]))) for b in range(FP.NB)]) / (2 * eps)
            d = max(float(np.abs(lin - J[:, :3, k]).max()), float(np.abs(ang - J[:, 3:, k]).max()))
            worst = max(worst, d)
    print(f"reference Jacobian vs central differences: max abs deviation {worst:.3e}")
    assert worst < 1e-8          # eps^2 truncation ~1e-12 and 1e-16 / eps = 1e-10 rounding on entries of order 1


def test_point_jacobian_matches_origin_jacobian_and_offsets(o, states):
    q = FP.jacobian_poses(STD["qpos"], states[0])["deep_squat"]
    J, xpos, xquat = FP.origin_jacobians(o, q)
    for b in (0, 4, 13, 23):
        Jp, r = PO.point_jacobian(o, q, b, np.zeros(3))
        assert np.allclose(Jp, J[b], atol=1e-13) and np.allclose(r, xpos[b])
        off = np.array([0.1, -0.2, 0.05])
        Jo, ro = PO.point_jacobian(o, q, b, off)
        assert np.allclose(Jo[:3], J[b, :3] - PO._skew(ro - xpos[b]) @ J[b, 3:], atol=1e-13) and np.allclose(Jo[3:], J[b, 3:])


def test_inertia_analogy(o, states):
    """J^T W J is the joint-space inertia of the tree with point masses w_pos at the body origins and spherical inertias w_rot: the oracle cannot
    take inertias, so the right-hand side is the composite-rigid-body algorithm written out in fit_pose_oracle.pseudo_inertia_crba"""
    db, bp = np.asarray(KPM["dof_body"]).astype(int), np.asarray(KPM["body_parent"]).astype(int)
    rng = np.random.default_rng(3)
    for name, q in FP.jacobian_poses(STD["qpos"], states[0]).items():
        wp, wr = rng.uniform(0.0, 2.0, 24), rng.uniform(0.0, 1.0, 24)
        wp[rng.integers(24)] = 0.0; wr[rng.integers(24)] = 0.0
        xpos, xquat = FP.fk(o, q)
        _, _, H = FP.normal_system(o, FP.problem(xpos, xquat, wp, wr), q, 0.0, np.ones(75))
        M = FP.pseudo_inertia_crba(o, q, wp, wr, db, bp)
        d = float(np.abs(H - M).max())
        print(f"{name}: |J^T W J - M_pseudo| max {d:.2e} on entries up to {np.abs(M).max():.1f}")
        assert d < 1e-12 * max(1.0, float(np.abs(M).max()))
        # M's sparsity: dofs of bodies on different branches do not couple
        anc = lambda a, b: a == b or any(p == a for p in _path(bp, b))      # noqa: E731
        for i in range(6, 75, 7):
            for j in range(6, 75, 5):
                if not (anc(db[i], db[j]) or anc(db[j], db[i])):
                    assert H[i, j] == pytest.approx(0.0, abs=1e-13)


def _path(bp, b):
    out = []
    while bp[b] >= 0:
        b = bp[b]; out.append(b)
    return out


def test_residual_definitions():
    """log / exp round trip, the shortest arc and the guarded forms"""
    rng = np.random.default_rng(0)
    for a in (0.0, 1e-12, 1e-9, 1e-5, 0.3, np.pi - 1e-3, np.pi - 1e-9):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        w = a * ax
        assert np.allclose(FP.quat_log(FP.quat_exp(w)), w, atol=1e-12, rtol=1e-9)
        assert np.allclose(FP.quat_log(-FP.quat_exp(w)), w, atol=1e-12, rtol=1e-9), "either sign of the quaternion"
    q = FP.oplus(np.concatenate([[0, 0, 0], [1, 0, 0, 0], np.zeros(69)]), np.concatenate([[1, 2, 3], [0, 0, np.pi / 2], np.ones(69)]))
    assert np.allclose(q[:3], [1, 2, 3]) and np.allclose(q[3:7], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)]) and np.allclose(q[7:], 1.0)
    lim, rngs = np.asarray(KPM["jnt_limited"])[:69], np.asarray(KPM["jnt_range"], float).reshape(-1, 2)[:69]
    qc = FP.oplus(np.concatenate([[0, 0, 0], [1, 0, 0, 0], np.zeros(69)]), np.concatenate([np.zeros(6), np.full(69, 50.0)]), KPM["jnt_range"], KPM["jnt_limited"])
    assert np.all(qc[7:][lim.astype(bool)] == rngs[lim.astype(bool), 1]) and np.all(qc[7:][~lim.astype(bool)] == 50.0)


# ---------------------------------------------------------------- the cases of the GPU tests

def test_reference_converges_on_every_reachable_case(o, states):
    """every one of the 67 reachable cases: under 1e-9 m and 1e-9 rad within CONVERGENCE_ITERS iterations, hinge angles back at the truth (mod 2 pi)"""
    worst_it, worst_h = 0, 0.0
    for i, q in enumerate(FP.truth_poses(*states)):
        c = FP.reachable_case(o, q, 100 + i, exact=True)
        r = FP.lm(o, c["q0"], FP.problem(c["tgt_pos"], c["tgt_quat"], c["w_pos"], c["w_rot"]), dict(n_iters=FP.CONVERGENCE_ITERS), stop=lambda a, b: a < 1e-9 and b < 1e-9)
        assert r["iters_to_stop"] is not None, f"case {i}: errors {r['info'][4]:.2e} m, {r['info'][5]:.2e} rad after {FP.CONVERGENCE_ITERS} iterations"
        dh = float(np.abs((r["qpos"][7:] - c["q_true"][7:] + np.pi) % (2 * np.pi) - np.pi).max())
        worst_it, worst_h = max(worst_it, r["iters_to_stop"]), max(worst_h, dh)
        assert dh < 1e-8 and np.abs(r["qpos"][:3] - c["q_true"][:3]).max() < 1e-9
    print(f"reachable cases: at most {worst_it} iterations, hinge angles within {worst_h:.2e} rad of the truth")
    assert worst_it == FP.CONVERGENCE_ITERS, "GPU_CONVERGENCE_ITERS is this count + 50 %"
    assert FP.GPU_CONVERGENCE_ITERS == int(np.ceil(1.5 * FP.CONVERGENCE_ITERS))


def test_reference_reaches_one_minimum_on_every_noisy_case(o, states):
    """every one of the 67 noisy cases: the two inits end at the same minimum (cost to 1e-9 relative, qpos to 1e-5) after NOISY_ITERS iterations; the
    minima are the committed fixture the GPU test compares with"""
    gold = np.load(GOLDEN)
    for i, q in enumerate(FP.truth_poses(*states)):
        c = FP.noisy_case(o, q, STD["qpos"], 500 + i)
        pb = FP.problem(c["tgt_pos"], None, None, None, c["q_prior"], c["w_prior"])
        ra, rb = (FP.lm(o, c[k], pb, dict(n_iters=FP.NOISY_ITERS)) for k in ("q0", "q0_alt"))
        rel = abs(ra["info"][1] - rb["info"][1]) / ra["info"][1]
        dq = float(np.abs(ra["qpos"] - rb["qpos"]).max())
        assert rel < 1e-9 and dq < 1e-5, f"case {i}: costs {ra['info'][1]:.6e} / {rb['info'][1]:.6e}, qpos apart by {dq:.2e}"
        assert np.allclose(gold["qpos"][i], ra["qpos"], atol=1e-9) and np.isclose(gold["cost"][i], ra["info"][1], rtol=1e-10), f"case {i}: the fixture is stale"


# ---------------------------------------------------------------- host logic

class StubSim:
    """answers fit_pose with the init moved onto the pelvis target, fk with the root position on every body; records the calls"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def fit_pose(self, qpos0, tgt_pos, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None, cfg=None, want_dq=False):
        self.calls.append(dict(qpos0=qpos0.clone(), tgt_pos=tgt_pos.clone(), tgt_quat=tgt_quat, w_rot=w_rot, q_prior=None if q_prior is None else q_prior.clone(),
                               w_prior=None if w_prior is None else w_prior.clone(), cfg=cfg))
        q = qpos0.clone(); q[..., :3] = tgt_pos[..., 0, :]; q[..., 7] = q[..., 7] + 1.0
        info = torch.zeros(tuple(q.shape[:-1]) + (8,)); info[..., 2] = 3.0
        return {"qpos": q, "info": info}

    def fk(self, rows):
        return {"wbpos": rows[:, :3].repeat(1, 24)}


def test_fit_config_refusals():
    from kinpoly_amd.fit import FitConfig
    c = FitConfig(n_iters=7, damp=2.0, clamp_limits=True).native()
    assert c.n_iters == 7 and c.clamp_limits == 1 and list(c.damp) == [2.0] * 75 and c.mu0 == pytest.approx(1e-2)
    for bad in (dict(n_iters=-1), dict(n_iters=2.5), dict(mu0=0.0), dict(mu_min=-1.0), dict(mu_max=float("nan")), dict(mu_up=0.0), dict(mu_down=0.0), dict(damp=0.0),
                dict(damp=[1.0] * 74 + [-1.0])):
        with pytest.raises(ValueError, match="FitConfig"):
            FitConfig(**bad).native()
    with pytest.raises(ValueError, match="75 numbers"):
        FitConfig(damp=[1.0, 2.0]).native()


def test_fit_sequence_host_logic():
    from kinpoly_amd import fit
    B, T = 3, 4
    tp = torch.arange(B * T * 24 * 3, dtype=torch.float32).view(B, T, 24, 3)
    sim = StubSim()
    out = fit.fit_sequence(sim, tp, mode="independent")
    assert len(sim.calls) == 1 and tuple(sim.calls[0]["qpos0"].shape) == (B, T, 76), "all B T rows in one call"
    std = torch.tensor(fit.standing_qpos(), dtype=torch.float32)
    assert torch.equal(sim.calls[0]["qpos0"][..., :3], tp[:, :, 0]) and torch.equal(sim.calls[0]["qpos0"][1, 2, 3:], std[3:]), "standing pose, pelvis on its target"
    assert tuple(out["qpos"].shape) == (B, T, 76) and sim.calls[0]["q_prior"] is None
    sim = StubSim()
    out = fit.fit_sequence(sim, tp, mode="chained", smooth=0.25)
    assert len(sim.calls) == T and all(tuple(c["qpos0"].shape) == (B, 76) for c in sim.calls), "frame t of all tracks in one call"
    assert sim.calls[0]["q_prior"] is None
    for t in range(1, T):
        assert torch.equal(sim.calls[t]["qpos0"], out["qpos"][:, t - 1]), "warm start from the solution at t - 1"
        assert torch.equal(sim.calls[t]["q_prior"], out["qpos"][:, t - 1, 7:]) and torch.all(sim.calls[t]["w_prior"] == 0.25)
    assert torch.allclose(out["qpos"][:, :, 7], std[7] + torch.arange(1.0, T + 1)[None, :])
    tq = torch.zeros(B, T, 24, 4); tq[..., 0] = 1.0
    sim = StubSim()
    fit.fit_sequence(sim, tp, tq, mode="independent")
    assert sim.calls[0]["tgt_quat"] is not None and torch.all(sim.calls[0]["w_rot"] == 1.0), "orientations count once they are given"
    rep = fit.fit_report(sim, ["a", "b", "c"], out["qpos"], tp, out["info"], n_iters=6)
    assert set(rep) == {"a", "b", "c"} and rep["a"]["accepted_share"] == pytest.approx(0.5) and rep["a"]["failed_rows"] == 0
    want = (tp[0] - tp[0, :, :1]).norm(dim=-1)
    assert rep["a"]["max_pos_err"] == pytest.approx(float(want.max()), rel=1e-6) and rep["a"]["mean_pos_err"] == pytest.approx(float(want.mean()), rel=1e-6)
    for bad in (dict(mode="other"), dict(smooth=-1.0)):
        with pytest.raises(ValueError, match="fit_sequence"):
            fit.fit_sequence(sim, tp, **bad)
    with pytest.raises(ValueError, match="tgt_pos must be"):
        fit.fit_sequence(sim, tp[..., :2])
    with pytest.raises(ValueError, match="tgt_pos must be"):
        fit.fit_pose(sim, tp[..., :23, :])
    with pytest.raises(ValueError, match="tgt_quat must be"):
        fit.fit_pose(sim, tp, tq[:, :2])


def test_fit_takes_round_trip(tmp_path):
    """scripts/fit_takes.py with a stub solver: its output loads with AmassSingleDataset, takes of different lengths come back at their own lengths"""
    import joblib
    from kinpoly_amd.dataset import AmassSingleDataset
    spec = importlib.util.spec_from_file_location("fit_takes", os.path.join(ROOT, "scripts", "fit_takes.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    rng = np.random.default_rng(0)
    tracks = {"walk": {"wbpos": rng.normal(size=(120, 24, 3))}, "sit": {"wbpos": rng.normal(size=(95, 72)), "obj_pose": np.zeros((95, 35))},
              "short": {"wbpos": rng.normal(size=(10, 24, 3))}}
    joblib.dump(tracks, tmp_path / "in.pkl")
    sim = StubSim()
    takes, rep = mod.main(["--tracks", str(tmp_path / "in.pkl"), "--out", str(tmp_path / "o" / "takes.pkl"), "--iters", "4", "--mode", "chained", "--limits"], sim=sim)
    assert len(sim.calls) == 120 and sim.calls[0]["cfg"].n_iters == 4 and sim.calls[0]["cfg"].clamp_limits == 1
    assert set(json.load(open(tmp_path / "o" / "fit_report.json"))) == set(tracks)
    ds = AmassSingleDataset({"file_path": str(tmp_path / "o" / "takes.pkl"), "t_min": 90}, "train")
    assert ds.data_keys == ["walk", "sit"] and list(ds.lens) == [120, 95], "the loader's length filter reads pose_aa's length"
    assert np.allclose(ds.qpos["walk"][:, :3], tracks["walk"]["wbpos"][:, 0], atol=1e-6) and takes["sit"]["obj_pose"].shape == (95, 35)
    assert takes["short"]["qpos"].shape == (10, 76) and takes["short"]["pose_aa"].shape == (10, 72) and takes["short"]["trans"].shape == (10, 3)
    with pytest.raises(ValueError, match="wbpos must be"):
        joblib.dump({"x": {"wbpos": np.zeros((5, 23, 3))}}, tmp_path / "bad.pkl"); mod.load_tracks(str(tmp_path / "bad.pkl"))


# ---------------------------------------------------------------- surface

def test_header_binding_and_symbols():
    """fails on the parent commit: the three symbols are new"""
    from kinpoly_amd import sim as kpsim
    hdr = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    assert "int kp_sim_point_jacobian(kp_sim*, int n_rows, const float* qpos, const int32_t* body, const float* offset, float* J);" in hdr
    assert "int kp_sim_fit_pose(kp_sim*, int n_rows, const kp_fit_in* in, const kp_fit_cfg* cfg, const kp_fit_out* out);" in hdr
    assert "void kp_fit_cfg_default(kp_fit_cfg* cfg);" in hdr
    for word in ("mj_jac", "No reference counterpart", "does not synchronise"):
        assert word in hdr, word
    assert len(kpsim._SIGNATURES["kp_sim_point_jacobian"][1]) == 6 and len(kpsim._SIGNATURES["kp_sim_fit_pose"][1]) == 5 and "kp_fit_cfg_default" in kpsim._SIGNATURES
    assert [f[0] for f in kpsim.KpFitIn._fields_] == ["qpos0", "tgt_pos", "tgt_quat", "w_pos", "w_rot", "q_prior", "w_prior"]
    assert [f[0] for f in kpsim.KpFitOut._fields_] == ["qpos", "info", "dq"]
    assert ctypes.sizeof(kpsim.KpFitCfg) == 4 * (1 + 5 + 75 + 1)
    assert list(kpsim.FIT_INFO) == ["cost0", "cost", "accepted", "mu", "max_epos", "max_erot", "dq_inf", "status"]
    assert hasattr(kpsim.KpSim, "point_jacobian") and hasattr(kpsim.KpSim, "fit_pose")
    if not os.path.exists(kpbuild.LIB):
        pytest.fail(f"{kpbuild.LIB} is missing: build() first")
    L = ctypes.CDLL(kpbuild.LIB)
    for sym in ("kp_sim_point_jacobian", "kp_sim_fit_pose", "kp_fit_cfg_default"):
        assert hasattr(L, sym), sym
    cfg = kpsim.KpFitCfg()
    L.kp_fit_cfg_default(ctypes.byref(cfg))
    d = FP.DEFAULT_CFG
    assert cfg.n_iters == d["n_iters"] and cfg.clamp_limits == 0 and list(cfg.damp) == [1.0] * 75
    for k in ("mu0", "mu_min", "mu_max", "mu_up", "mu_down"):
        assert getattr(cfg, k) == pytest.approx(d[k], rel=1e-6), k
    # the refusals that need no device: null handle, and the argument checks come before anything touches the GPU
    L.kp_last_error.restype = ctypes.c_char_p
    L.kp_sim_fit_pose.restype = ctypes.c_int; L.kp_sim_fit_pose.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    assert L.kp_sim_fit_pose(None, 1, None, None, None) == -1 and b"kp_sim_fit_pose: null handle" in L.kp_last_error()
    L.kp_sim_point_jacobian.restype = ctypes.c_int; L.kp_sim_point_jacobian.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert L.kp_sim_point_jacobian(None, 1, None, None, None, None) == -1 and b"kp_sim_point_jacobian: null handle" in L.kp_last_error()
