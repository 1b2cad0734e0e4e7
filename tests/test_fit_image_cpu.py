"""Pose fitting to 2D key points seen by calibrated cameras, without a GPU: the gradient of the reprojection term against central
differences, the majoriser, the identity the matrix rests on (weighted observations are point masses), the two camera conversions against the renderers'
own formulas, the library's surface, and the fp64 reference tests/fit_image_oracle.py on EVERY row the GPU tests compare (this is where the inputs are
chosen: the margin to z_near, the accepted steps), the binding's checks on CPU tensors and the host logic of kinpoly_amd/fit.py and
scripts/fit_takes.py --keypoints."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fit_image_oracle as FI  # noqa: E402
import fit_points_oracle as FT  # noqa: E402
import fit_pose_oracle as FP  # noqa: E402
import fit_scene_oracle as FS  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import render_oracle as RO  # noqa: E402
from kinpoly_amd import build as kpbuild  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)
F32 = torch.float32


@pytest.fixture(scope="module")
def o():
    return FI.oracle(DEFAULT_KPM)


@pytest.fixture(scope="module")
def truths():
    return FP.truth_poses(ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"]), ID.sweep_states(KPM, STD["qpos"]))


# ---------------------------------------------------------------- (1) the gradient

def test_gradient_against_central_differences(o, truths):
    """one, two and three cameras, a point near the image edge, fx != fy: central differences of the fp64 cost, section 20's measure
    (|fd + g| / max(1, |g|)), cap 1e-7"""
    eps = 1e-6
    body, off = FI.marker_choice(53)
    qt = FP.normalized(truths[0])
    q = FP.oplus(qt, 0.3 * FI._perturbation(5))
    # the figure at a side edge of a 640 x 480 image: the camera looks 1.5 m beside it from 3 m
    edge = FI.look_at(qt[:3] + [3.0, 0.0, 0.3], [qt[0], qt[1] + 1.5, 0.9], f=600.0, cx=320.0, cy=240.0)
    px = FI.observe(o, q, body, off, [edge])[0][0]
    assert min(px[:, 0].min(), 640.0 - px[:, 0].max()) < 60.0 and px[:, 0].min() > -100.0 and px[:, 0].max() < 740.0, f"a point near the image edge: u {px[:, 0].min():.1f} .. {px[:, 0].max():.1f}"
    for name, cams in (("one camera", FI.ring(qt[:3], 1)), ("two cameras", FI.ring(qt[:3], 2)), ("three cameras", FI.ring(qt[:3], 3)), ("image edge", edge[None]),
                       ("fx != fy", FI.look_at([2.5, -1.0, 1.6], [0.0, 0.0, 0.9], f=900.0, fy=1250.0)[None])):
        uv, _ = FI.observe(o, qt, body, off, cams)
        # weights of the order 1 / f^2: the cost is O(1) as in section 20, so that the measure's absolute part (eps_double cost / 2 eps) stays at 1e-9
        w = np.random.default_rng(3).uniform(0.2, 2.0, uv.shape[:2]) / float(cams[0][12]) ** 2
        pb = FI.problem(KPM, None, cams, uv, w, pt_body=body, pt_offset=off, q_prior=STD["qpos"][7:], w_prior=np.full(69, 0.1))
        cfg = dict(FI.DEFAULT_CFG)
        _, g, _, res = FI.normal_system(o, pb, q, 0.0, cfg)
        assert len(res["img"]) == 53 * len(cams) and not res["behind"]
        worst = 0.0
        for k in range(0, 75, 3):
            e = np.zeros(75); e[k] = eps
            fd = (FI.evaluate(o, pb, FP.oplus(q, e), cfg)[0] - FI.evaluate(o, pb, FP.oplus(q, -e), cfg)[0]) / (2 * eps)
            worst = max(worst, abs(fd + g[k]) / max(1.0, abs(g[k])))
        print(f"{name}: |g| up to {np.abs(g).max():.3e}, gradient against central differences {worst:.2e}")
        assert worst < 1e-7, name


# ---------------------------------------------------------------- (2) the majoriser, (3) the identity

def test_the_isotropic_mass_majorises_the_gauss_newton_block():
    """m I - w J^T J has no negative eigenvalue on 1000 seeded points and cameras.  Its smallest eigenvalue is 0 in exact arithmetic (along the top
    eigenvector of J^T J), so the assertion allows the rounding of the 3 x 3 eigenvalue computation: 8 eps m.  R_cw is orthonormal to fp64 here: the
    statement is about J_pi J_pi^T, and a record rounded to fp32 has R R^T = I only to 1e-7, which moves the smallest eigenvalue by as much."""
    rng = np.random.default_rng(22)
    worst, equal = 0.0, 0.0
    for i in range(1000):
        eye = rng.uniform(-3, 3, 3)
        fx = rng.uniform(200, 2000)
        fy = fx if i % 3 == 0 else rng.uniform(200, 2000)
        cam = FI.look_at(eye, eye + rng.normal(size=3), f=fx, fy=fy, cx=rng.uniform(0, 1000), cy=rng.uniform(0, 1000), up=(0.1, 0.2, 1.0), exact=True)
        R, t = cam[:9].reshape(3, 3), cam[9:12]
        c = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.06, 8.0)])      # camera coordinates, wide of the axis too
        p = R.T @ (c - t)
        _, J, lam, z = FI.projection(cam, p)
        w = rng.uniform(0.1, 5.0)
        ev = np.linalg.eigvalsh(w * lam * np.eye(3) - w * J.T @ J)
        worst = min(worst, ev.min() / (w * lam))
        if i % 3 == 0:
            equal = max(equal, abs(lam - (cam[12] / z) ** 2 * (1 + (c[0] / z) ** 2 + (c[1] / z) ** 2)) / lam)
    print(f"smallest eigenvalue of m I - w J^T J over m: {worst:.2e}; fx == fy: closed form against (f/z)^2 (1 + a^2 + b^2) {equal:.2e}")
    assert worst >= -8 * np.finfo(float).eps and equal < 1e-12


def test_weighted_observations_are_point_masses(o, truths):
    """the dense sum m J_p^T J_p over the weighted observations = the joint-space inertia assembled from the ten floats per body the kernel writes"""
    db, bp = np.asarray(KPM["dof_body"]).astype(int), np.asarray(KPM["body_parent"]).astype(int)
    body, off = FI.marker_choice(53)
    for i, C in ((0, 1), (3, 3)):
        qt = FP.normalized(truths[i])
        cams = FI.ring(qt[:3], C)
        uv, _ = FI.observe(o, qt, body, off, cams)
        pb = FI.problem(KPM, None, cams, uv, None, pt_body=body, pt_offset=off)
        q = FP.oplus(qt, 0.2 * FI._perturbation(9))
        _, _, H, res = FI.normal_system(o, pb, q, 0.0, dict(FI.DEFAULT_CFG))
        xpos, _ = FP.fk(o, q)
        ks = np.array([t["k"] for t in res["img"]])
        M = FT.inertia_from_floats(o, q, FT.body_floats(xpos, res["p"][ks], body[ks], np.array([t["w"] * t["lam"] for t in res["img"]])), db, bp)
        d = float(np.abs(H - M).max() / np.abs(M).max())
        print(f"truth {i}, {C} cameras: {len(ks)} observations, |sum m J^T J - M(ten floats)| / |M| {d:.2e} on entries up to {np.abs(M).max():.3e}")
        assert len(ks) == 53 * C and d < 1e-13


# ---------------------------------------------------------------- (4), (5) the camera conversions

def test_from_head_camera_against_the_header_formula():
    """fails on the parent commit: Pinhole is new.  u' = (W/2)(1 + (-c_x/c_z)/(th W/H)), v' = (H/2)(1 - (c_y/c_z)/th), c = R^T (p - eye)"""
    from kinpoly_amd.fit import Pinhole
    rng = np.random.default_rng(4)
    for W, H in ((16, 16), (64, 48), (7, 11)):
        q = rng.normal(size=4)
        cam8 = np.concatenate([rng.normal(size=3), q, [rng.uniform(40, 100)]])
        Rm = RO.qmat(q / np.linalg.norm(q))
        th = np.tan(0.5 * np.radians(cam8[7]))
        c = np.concatenate([rng.uniform(-1, 1, (50, 2)), rng.uniform(0.1, 5, (50, 1))], 1)
        p = cam8[:3] + c @ Rm.T
        want = np.stack([(W / 2) * (1 + (-c[:, 0] / c[:, 2]) / (th * W / H)), (H / 2) * (1 - (c[:, 1] / c[:, 2]) / th)], 1)
        ph = Pinhole.from_head_camera(cam8, W, H)
        assert np.abs(ph.project(p) - want).max() < 1e-10 * max(W, H) and np.abs(ph.camera_points(p)[:, 2] - c[:, 2]).max() < 1e-12
        assert ph.fx == ph.fy == pytest.approx(H / (2 * th)) and (ph.cx, ph.cy) == (W / 2, H / 2)
        rec = ph.pack()
        assert rec.dtype == np.float32 and rec.shape == (16,) and np.allclose(rec[:9].reshape(3, 3), ph.R, atol=1e-7) and np.allclose(rec[12:], [ph.fx, ph.fy, ph.cx, ph.cy])


def test_from_camera_against_the_renderer_rays():
    """fails on the parent commit.  project(eye + s dir(px)) is the pixel centre for every pixel of an 8 x 6 image, at two depths"""
    from kinpoly_amd.fit import Pinhole
    W, H = 8, 6
    for cam7 in ([0.2, -0.1, 0.9, 3.0, 40.0, -20.0, 45.0], [1.0, 2.0, 0.5, 1.5, -135.0, 10.0, 70.0]):
        eye, d = RO.camera_rays(cam7, W, H)
        ph = Pinhole.from_camera(cam7, W, H)
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        centre = np.stack([x.ravel() + 0.5, y.ravel() + 0.5], 1)
        for s in (0.7, 12.0):
            assert np.abs(ph.project(eye + s * d) - centre).max() < 1e-10
            assert (ph.camera_points(eye + s * d)[:, 2] > 0).all()


# ---------------------------------------------------------------- (6) the library's surface

def test_header_binding_and_symbols():
    """fails on the parent commit: the symbols are new"""
    from kinpoly_amd import sim as kpsim
    hdr = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    for decl in ("typedef struct { kp_fit_scene_cfg scene; float z_near; } kp_fit_image_cfg;",
                 "typedef struct { int n_cams, camera_rows; const float *cam, *uv, *uv_w; } kp_fit_image_obs;",
                 "typedef struct { float *qpos, *info, *dq, *pt_err, *uv_err; } kp_fit_image_out;", "void kp_fit_image_cfg_default(kp_fit_image_cfg* cfg);",
                 "int kp_sim_fit_image(kp_sim*, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const float* obj_qpos, const kp_fit_image_obs* obs,"):
        assert decl in hdr, decl
    for word in ("deviation 45", "section 22", "status 2", "largest eigenvalue"):
        assert word in hdr, word
    assert len(kpsim._SIGNATURES["kp_sim_fit_image"][1]) == 8 and "kp_fit_image_cfg_default" in kpsim._SIGNATURES
    assert ctypes.sizeof(kpsim.KpFitImageCfg) == ctypes.sizeof(kpsim.KpFitSceneCfg) + 4
    assert list(kpsim.FIT_IMAGE_INFO)[:15] == list(kpsim.FIT_SCENE_INFO) and [kpsim.FIT_IMAGE_INFO[k] for k in ("max_euv", "rms_euv", "n_uv", "min_depth")] == [16, 17, 18, 19]
    t = kpsim.fit_image_outputs(5, 3)
    assert list(t) == ["qpos", "info", "dq", "pt_err", "uv_err"] and t["info"][0] == (20,) and t["uv_err"][0] == (3, 5)
    if not os.path.exists(kpbuild.LIB):
        pytest.fail(f"{kpbuild.LIB} is missing: build() first")
    L = ctypes.CDLL(kpbuild.LIB)
    for sym in ("kp_sim_fit_image", "kp_fit_image_cfg_default"):
        assert hasattr(L, sym), sym
    cfg = kpsim.KpFitImageCfg()
    cfg.z_near = 3.0; cfg.scene.w_obj = 2.0
    L.kp_fit_image_cfg_default(ctypes.byref(cfg))
    ref = kpsim.KpFitSceneCfg(); L.kp_fit_scene_cfg_default(ctypes.byref(ref))
    assert bytes(cfg.scene) == bytes(ref) and cfg.z_near == pytest.approx(0.05)
    L.kp_last_error.restype = ctypes.c_char_p
    L.kp_sim_fit_image.restype = ctypes.c_int; L.kp_sim_fit_image.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6
    assert L.kp_sim_fit_image(None, 1, None, None, None, None, None, None) == -1 and b"kp_sim_fit_image: null handle" in L.kp_last_error()


# ---------------------------------------------------------------- (7) the rows the GPU tests compare

def test_compared_rows_keep_clear_of_z_near_and_of_the_discrete_choices(o, truths):
    """On every row the GPU compares with the reference, at every pose the fp64 loop evaluates: no weighted observation within 1e-3 m of z_near; the
    loop accepts its steps (so the comparison is of steps taken, not of rejections); on the rows with the floor term, section 21's vertex margin to
    the plane (FS.margins_hold).  A row that fails is replaced and listed in fit_image_oracle (SEED_OF, LIFT, FLOOR_COMPARE_TRUTHS).  The thirty-iteration
    floor rows are held to section 20's derived bound, not to the reference's active sets: their vertices settle micrometres around the plane."""
    for K, C in FI.COMPARE_SHAPES:
        for cname, mk in FI.CAMERA_CONFIGS.items():
            body, off, rows = FI.compare_rows(o, truths, K, C, **mk["rows"])
            for r in rows:
                pb = FI.row_problem(KPM, body, off, r)
                for iters in (1, FI.COMPARE_ITERS):
                    out = FI.lm(o, r["q0"], pb, dict(mk["cfg"], n_iters=iters))
                    assert out["info"][7] == 0 and out["z_margin"] >= FI.Z_MARGIN and out["crossed"] == 0, f"{r['name']} {cname}: z margin {out['z_margin']:.2e}"
                    assert out["info"][2] == iters and out["info"][18] == K * C, f"{r['name']} {cname}: accepted {out['info'][2]:.0f} of {iters}"
                    ok, m = FS.margins_hold(out)
                    assert ok, f"{r['name']} {cname}: section 21's margins {m}"
                    assert ("pt_tgt" in r) == (K == 24) and (out["info"][8] > 0) == (K == 24)
                print(f"{r['name']} ({cname}): cost {out['info'][0]:.3e} -> {out['info'][1]:.3e}, rms {out['info'][17]:.3e} px, z margin {out['z_margin']:.2f} m, |dq| {np.abs(out['dq']).max():.3f}")
    # the one-camera case with the floor term
    oS = FI.oracle(DEFAULT_KPM)
    for r in FI.floor_rows(oS, KPM, truths):
        out = FI.lm(oS, r["q0"], r["pb"], r["cfg"])
        print(f"{r['name']}: depth {r['depth0'] * 1e3:.1f} -> {out['info'][10] * 1e3:.3f} mm (bound {FT.FLOOR_BOUND * 1e3:.1f}), rms {out['info'][17]:.3e} px, accepted {out['info'][2]:.0f}, "
              f"cost {out['info'][0]:.3e} -> {out['info'][1]:.3e} (candidate {r['cand_cost']:.3e})")
        assert out["info"][7] == 0 and out["z_margin"] >= FI.Z_MARGIN and r["depth0"] >= 0.029
        assert out["info"][1] <= r["cand_cost"], "the bound's premise: the reference ends below the candidate's cost"
        assert out["info"][10] <= FT.FLOOR_BOUND
    # the floor rows compared iteration by iteration: the active floor term keeps section 21's margins at every evaluated pose
    rows = FI.floor_compare_rows(oS, KPM, truths)
    assert len(rows) == FI.N_DISTINCT
    for r in rows:
        out = FI.lm(oS, r["q0"], r["pb"], r["cfg"])
        ok, m = FS.margins_hold(out)
        print(f"{r['name']}: accepted {out['info'][2]:.0f}, {out['info'][11]:.0f} vertices below at the end, depth {out['info'][10] * 1e3:.3f} mm, margins " + ", ".join(f"{k} {v:.1e}" for k, v in m.items()))
        assert ok and out["info"][2] == r["cfg"]["n_iters"] and out["info"][11] > 0 and out["info"][7] == 0 and out["z_margin"] >= FI.Z_MARGIN, f"{r['name']}: {m}"
    # the two-camera convergence case: the reference ends below 0.05 px
    for r in FI.convergence_rows(o, KPM, truths):
        out = FI.lm(o, r["q0"], r["pb"], r["cfg"])
        print(f"{r['name']}: rms {out['info'][17]:.3e} px after {r['cfg']['n_iters']} iterations, accepted {out['info'][2]:.0f}")
        assert out["info"][17] < 0.05 and out["z_margin"] >= FI.Z_MARGIN
    # the row whose first trial crosses z_near
    r = FI.crossing_row(o, KPM, truths)
    out = FI.lm(o, r["q0"], r["pb"], r["cfg"])
    print(f"{r['name']}: crossed {out['crossed']}, accepted {out['info'][2]:.0f} of {r['cfg']['n_iters']}, z margin {out['z_margin']:.2e}")
    assert out["info"][7] == 0 and out["crossed"] >= 1 and out["costs"][0] == out["info"][0] and out["z_margin"] >= FI.Z_MARGIN
    behind = FI.lm(o, r["q_behind"], r["pb"], r["cfg"])
    assert behind["info"][7] == 2 and np.isinf(behind["info"][0]) and np.array_equal(behind["qpos"], r["q_behind"]) and not behind["info"][8:].any()


# ---------------------------------------------------------------- the binding and the host logic

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def cpu_sim(monkeypatch):
    from kinpoly_amd import sim as S
    monkeypatch.setattr(S, "_dev", lambda name, t, shape, dtype=F32: None if t is None else 1)
    sim = object.__new__(S.KpSim)
    sim.L, sim.h, sim.device, sim.model = _Recorder(), None, "cpu", None
    return sim


def test_binding_shapes_and_want(cpu_sim):
    from kinpoly_amd import sim as S
    body, off = FI.marker_choice(53)
    cfg = S.KpFitImageCfg(); cfg.z_near = 0.05
    ALL = ("qpos", "info", "dq", "pt_err", "uv_err")
    for lead in ((), (5,), (2, 3)):
        for cam in (torch.zeros(3, 16), torch.zeros(lead + (3, 16))):
            out = cpu_sim.fit_image(torch.zeros(lead + (76,)), body, off, cam, torch.zeros(lead + (3, 53, 2)), cfg=cfg, want=ALL)
            assert {k: tuple(v.shape) for k, v in out.items()} == {"qpos": lead + (76,), "info": lead + (20,), "dq": lead + (75,), "pt_err": lead + (53,), "uv_err": lead + (3, 53)}
    calls = cpu_sim.L.calls
    assert [c[0] for c in calls] == ["kp_sim_fit_image"] * 6 and len(calls[0][1]) == 8
    obs = [ctypes.cast(c[1][5], ctypes.POINTER(S.KpFitImageObs)).contents for c in calls]
    assert [(b.n_cams, b.camera_rows) for b in obs] == [(3, 1), (3, 1), (3, 1), (3, 5), (3, 1), (3, 6)], "a shared camera table is camera_rows 1"
    calls.clear()
    out = cpu_sim.fit_image(torch.zeros(4, 76), body, off, pt_tgt=torch.zeros(4, 53, 3), cfg=cfg)
    assert tuple(out["info"].shape) == (4, 20) and ctypes.cast(calls[0][1][5], ctypes.POINTER(S.KpFitImageObs)).contents.n_cams == 0, "no cameras: fit_scene's problem"
    q, uv, cam = torch.zeros(5, 76), torch.zeros(5, 2, 53, 2), torch.zeros(2, 16)
    bad = S.KpFitImageCfg(); bad.z_near = 0.0
    for call, msg in ((lambda: cpu_sim.fit_image(q, body, off, cam, uv, want=("nope",), cfg=cfg), "want must name"),
                      (lambda: cpu_sim.fit_image(q, body, off, cam, cfg=cfg), "go together"),
                      (lambda: cpu_sim.fit_image(q, body, off, cfg=cfg), "nothing to fit"),
                      (lambda: cpu_sim.fit_image(q, body, off, torch.zeros(9, 16), torch.zeros(5, 9, 53, 2), cfg=cfg), "at most 8"),
                      (lambda: cpu_sim.fit_image(q, body, off, torch.zeros(2, 15), uv, cfg=cfg), "cam must be"),
                      (lambda: cpu_sim.fit_image(q, body, off, torch.zeros(4, 2, 16), uv, cfg=cfg), "cam must be"),
                      (lambda: cpu_sim.fit_image(q, body, off, cam, torch.zeros(5, 3, 53, 2), cfg=cfg), "uv must be"),
                      (lambda: cpu_sim.fit_image(q, body, off, cam, uv, torch.zeros(5, 2, 52), cfg=cfg), "uv_w must be"),
                      (lambda: cpu_sim.fit_image(q, body, off, cam, uv, cfg=bad), "z_near")):
        with pytest.raises(ValueError, match=msg):
            call()


class StubSim:
    """a sim that records fit_image and answers with its init"""
    device = torch.device("cpu")

    def __init__(self, o=None):
        self.o, self.calls = o, []

    def fk(self, rows):
        xp, xq = zip(*[FP.fk(self.o, r.double().numpy()) for r in rows])
        return {"wbpos": torch.tensor(np.stack(xp).reshape(len(rows), 72), dtype=F32), "wbquat": torch.tensor(np.stack(xq).reshape(len(rows), 96), dtype=F32)}

    def fit_image(self, qpos0, pt_body, pt_offset, cam=None, uv=None, uv_w=None, pt_tgt=None, pt_w=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None,
                  w_prior=None, obj_qpos=None, cfg=None, want=("qpos", "info")):
        lead, K, C = tuple(qpos0.shape[:-1]), len(pt_body), cam.shape[-2]
        self.calls.append(dict(qpos0=qpos0.clone(), cam=cam, uv=uv, uv_w=uv_w, pt_tgt=pt_tgt, pt_w=pt_w, q_prior=q_prior, obj_qpos=obj_qpos, cfg=cfg, want=want))
        info = torch.zeros(lead + (20,)); info[..., 2] = 3.0; info[..., 16] = 2.0; info[..., 17] = 1.0; info[..., 18] = float(K * C); info[..., 19] = 2.5
        out = {"qpos": qpos0.clone(), "info": info, "pt_err": torch.zeros(lead + (K,)), "uv_err": torch.full(lead + (C, K), 1.5), "dq": torch.zeros(lead + (75,))}
        return {k: out[k] for k in want}


def test_fit_module_keypoints(o):
    from kinpoly_amd import fit
    assert fit.FitConfig().z_near == pytest.approx(0.05)
    c = fit.FitConfig(n_iters=7, w_floor=5.0, w_obj=3.0, z_near=0.2).native_image()
    assert c.scene.pts.fit.n_iters == 7 and c.scene.pts.w_floor == 5.0 and c.scene.w_obj == 3.0 and c.z_near == pytest.approx(0.2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="FitConfig: z_near"):
            fit.FitConfig(z_near=bad).native_image()
    sim, m = StubSim(o), fit.MarkerSet.body_origins()
    cams = [fit.Pinhole.from_camera([0, 0, 1, 3, 90 * i, -10, 45], 640, 480) for i in range(2)]
    uv = torch.zeros(2, 3, 2, 24, 2); uv[0, 1, 1, 5, 0] = float("nan")
    conf = torch.ones(2, 3, 2, 24); conf[1, 2, 0, 7] = -1.0
    out = fit.fit_keypoints(sim, m, uv[:, 0], cams, conf[:, 0], want=("qpos", "info", "uv_err"))
    last = sim.calls[-1]
    assert last["cam"].shape == (2, 16) and last["uv_w"].shape == (2, 2, 24) and last["pt_tgt"] is None and out["uv_err"].shape == (2, 2, 24) and out["info"].shape == (2, 20)
    assert np.allclose(last["qpos0"][0].numpy(), fit.standing_qpos(), atol=1e-6), "no 3D information: the standing pose where the fixture has it"
    fit.fit_keypoints(sim, m, uv[:, 1], cams, conf[:, 1])
    assert sim.calls[-1]["uv_w"][0, 1, 5] == 0.0 and sim.calls[-1]["uv_w"][0, 1, 4] == 1.0, "a NaN uv is an undetected key point"
    tgt = torch.zeros(2, 24, 3); tgt[1, 3] = float("nan")
    fit.fit_keypoints(sim, m, uv[:, 0], torch.zeros(2, 2, 16), tgt=tgt)
    assert sim.calls[-1]["pt_w"][1, 3] == 0.0 and sim.calls[-1]["cam"].shape == (2, 2, 16)
    for call, msg in ((lambda: fit.fit_keypoints(sim, m, uv[:, 0, :, :23], cams), "uv must be"), (lambda: fit.fit_keypoints(sim, m, uv[:, 0], cams[:1]), "cameras in uv"),
                      (lambda: fit.fit_keypoints(sim, m, uv[:, 0], cams, conf[:, 0, :1]), "uv_w must be"), (lambda: fit.fit_keypoints(sim, m, uv[:, 0], cams, tgt=tgt[:1]), "tgt must be")):
        with pytest.raises(ValueError, match=msg):
            call()
    n0 = len(sim.calls)
    out = fit.fit_sequence_keypoints(sim, m, uv, cams, conf, mode="independent")
    assert len(sim.calls) == n0 + 1 and out["info"].shape == (2, 3, 20) and out["uv_err"].shape == (2, 3, 2, 24)
    out = fit.fit_sequence_keypoints(sim, m, uv, cams, conf, mode="chained", smooth=0.5)
    assert len(sim.calls) == n0 + 4 and sim.calls[n0 + 1]["q_prior"] is None and sim.calls[-1]["q_prior"] is not None and out["qpos"].shape == (2, 3, 76)
    assert sim.calls[-1]["uv_w"][1, 0, 7] <= 0.0, "frame 2 of take 1: confidence -1 reaches the kernel, which skips it"
    moving = torch.zeros(2, 3, 2, 16); moving[:, 2] = 1.0
    fit.fit_sequence_keypoints(sim, m, uv, moving, mode="chained")
    assert bool((sim.calls[-1]["cam"] == 1.0).all()) and sim.calls[-1]["cam"].shape == (2, 2, 16)
    info = np.zeros((2, 3, 20)); info[..., 2] = 3; info[..., 18] = 48; info[..., 19] = [[2.0, 1.5, 3.0], [4, 4, 4]]; info[1, 1, 7] = 2; info[0, 0, 7] = 1
    rep = fit.keypoints_report(["a", "b"], m.names, np.full((2, 3, 2, 24), 1.5), (conf > 0).numpy(), info, n_iters=6)
    assert rep["a"]["mean_px_err"] == pytest.approx(1.5) and rep["a"]["min_depth"] == 1.5 and rep["b"]["rows_behind_camera"] == 1 and rep["a"]["failed_rows"] == 1
    assert rep["b"]["detected_share"] == pytest.approx(1 - 1 / 144) and len(rep["a"]["per_camera"]) == 2 and set(rep["a"]["per_marker"]) == set(m.names)
    assert rep["a"]["accepted_share"] == pytest.approx(0.5) and "max_penetration" in rep["a"]


def test_fit_takes_keypoints_argument(o, tmp_path):
    """scripts/fit_takes.py --keypoints --cameras with a stub solver: uv, the confidences and the cameras reach the fit, the report has the
    reprojection columns, the output is AmassSingleDataset's schema"""
    import joblib
    from kinpoly_amd import fit
    spec = importlib.util.spec_from_file_location("fit_takes", os.path.join(ROOT, "scripts", "fit_takes.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    m = fit.MarkerSet.body_origins(); m.save(tmp_path / "set.json")
    rng = np.random.default_rng(0)
    uv = {"walk": {"uv": rng.uniform(0, 600, (4, 2, 24, 2)), "conf": rng.uniform(0.1, 1, (4, 2, 24))}, "sit": {"uv": rng.uniform(0, 600, (3, 2, 24, 2))}}
    uv["walk"]["uv"][1, 0, 3] = np.nan; uv["walk"]["conf"][2, 1, 4] = 0.0
    joblib.dump(uv, tmp_path / "uv.pkl")
    cams = np.stack([fit.Pinhole.from_camera([0, 0, 1, 3, 90 * i, -10, 45], 640, 480).pack() for i in range(2)])
    joblib.dump(cams, tmp_path / "cams.pkl")
    sim = StubSim(o)
    args = ["--keypoints", str(tmp_path / "uv.pkl"), "--cameras", str(tmp_path / "cams.pkl"), "--markers", str(tmp_path / "set.json"), "--out", str(tmp_path / "o" / "takes.pkl"), "--iters", "4"]
    takes, rep = mod.main(args + ["--floor", "10"], sim=sim)
    assert len(sim.calls) == 4 and sim.calls[0]["cfg"].scene.pts.w_floor == 10.0 and sim.calls[0]["cfg"].scene.pts.fit.n_iters == 4
    assert sim.calls[1]["uv_w"][0, 0, 3] == 0.0 and sim.calls[2]["uv_w"][0, 1, 4] == 0.0 and sim.calls[3]["uv_w"][1, 0, 0] == 1.0
    assert sim.calls[0]["cam"].shape == (2, 2, 16) and takes["walk"]["qpos"].shape == (4, 76) and takes["sit"]["qpos"].shape == (3, 76) and takes["sit"]["pose_aa"].shape == (3, 72)
    on_disk = json.load(open(tmp_path / "o" / "fit_report.json"))
    assert {"mean_px_err", "max_px_err", "px_err_p90", "detected_share", "rows_behind_camera", "max_penetration"} <= set(on_disk["walk"])
    joblib.dump({"walk": {"markers": rng.normal(size=(4, 24, 3))}, "sit": {"markers": rng.normal(size=(3, 24, 3))}}, tmp_path / "m.pkl")
    mod.main(args + ["--tracks", str(tmp_path / "m.pkl")], sim=sim)
    assert sim.calls[-1]["pt_tgt"].shape == (2, 24, 3), "combined with 3D marker tracks"
    joblib.dump({k: cams for k in uv}, tmp_path / "cams_by_take.pkl")
    mod.main([a if a != str(tmp_path / "cams.pkl") else str(tmp_path / "cams_by_take.pkl") for a in args], sim=sim)
    for bad in (args[:2] + args[4:], args[2:], args[:4] + args[6:]):
        with pytest.raises(SystemExit):
            mod.main(bad, sim=sim)
    joblib.dump(cams[:1], tmp_path / "one.pkl")
    with pytest.raises(ValueError, match="cameras must be"):
        mod.main([a if a != str(tmp_path / "cams.pkl") else str(tmp_path / "one.pkl") for a in args], sim=sim)
