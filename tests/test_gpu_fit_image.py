"""Pose fitting to 2D key points seen by calibrated cameras (kp_sim_fit_image) on a real MI355X: the kernel against the fp64
reference tests/fit_image_oracle.py on identical fp32 inputs, on the rows tests/test_fit_image_cpu.py has chosen; one step against the dense solve,
three iterations with equal accepted steps, convergence with two cameras and with one camera on the floor, bit-for-bit equality with kp_sim_fit_scene
where the term is absent, row independence, the edge rows (status 1 and 2, a trial that crosses z_near), the refusals, non-interference with the control
step, agreement with the egocentric renderer's flow, and scripts/fit_takes.py --keypoints end to end.

Tolerances not capped by sections 20 / 21 = 4 x the device's separation from the fp64 reference measured on the MI355X (run-to-run and marker-set
variation: the margin of sections 20 and 21); every figure is printed before it is asserted."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fit_image_oracle as FI  # noqa: E402
import fit_points_oracle as FT  # noqa: E402
import fit_pose_oracle as FP  # noqa: E402
import fit_scene_oracle as FS  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import render_oracle as RO  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

ROOT = H.ROOT
STD = H.STD
KPM = read_kpm(DEFAULT_KPM)
ROWS = FI.ROWS
ALL = ("qpos", "info", "dq", "pt_err", "uv_err")
SCENE = ("qpos", "info", "dq", "pt_err")
N = FI.N_DISTINCT

# caps sections 20 and 21 set for the same figures: one step against the dense solve (relative inf-norm), the normwise backward error of a step in the
# reference's system (n u, n = 75, u = 2^-24), the derived floor bound
CAP = {"dq": 2.8e-4, "dq_px": 2.8e-4, "backward_px": 75 * 2.0 ** -24, "floor_depth": FT.FLOOR_BOUND}
# 4 x the largest separation from the fp64 reference measured on the MI355X (measured value in the comment)
TOL = {
    "dq": 4 * 6.177e-05,                 # one step, unit cameras (w 1 on normalised coordinates), |dq - ref| / |ref|, worst row of the three shapes; measured 6.177e-05
    "cost": 4 * 1.049e-06,               # the same: first cost and cost after the step, relative to the first cost; measured 1.049e-06
    "backward_px": 4 * 2.223e-06,        # one step, 1000 px cameras at w = 1 px^-2: normwise backward error in the reference's system; measured 2.223e-06: 4 x that exceeds section 21's cap, which holds instead
    "cost_px": 4 * 5.670e-06,            # the same: first cost and cost after the step, relative to the first cost; measured 5.670e-06
    "it3_cost": 4 * 1.144e-07,           # three iterations, both camera configurations: final cost against the reference's, relative to the first cost; measured 1.144e-07
    "it3_qpos": 4 * 2.626e-05,           # the same: qpos against the reference's; measured 2.626e-05
    "it3_rms": 4 * 7.474e-06,            # the same: reprojection rms against the reference's, relative to the reference's first rms; measured 7.474e-06
    "conv_rms": 4 * 2.563e-05,           # thirty iterations, two cameras 90 degrees apart at 1000 px: final reprojection rms against the reference's [px], worst of four rows; measured 2.563e-05
    "cross_cost": 4 * 9.087e-07,         # the row whose first trial crosses z_near, six iterations: final cost against the reference's, relative to the first cost; measured 9.087e-07
    "dq_px": 4 * 5.647e-05,              # one step, 1000 px cameras: |dq - ref| / |ref|, under section 20\'s cap like the unit rows; measured 5.647e-05
    "it3_pt": 4 * 2.171e-07,                   # three iterations, the K = 24 rows that carry 3D targets too: max |e_k| (info 8) against the reference's [m]; measured 2.171e-07
    "floor3_cost": 4 * 5.265e-07,              # three iterations on the floor at w_floor 4, one unit camera: final cost against the reference's, relative to the first cost; measured 5.265e-07
    "floor3_depth": 4 * 1.334e-07,             # the same: deepest vertex below the floor against the reference's [m]; measured 1.334e-07
    "flow": 4 * 3.441e-06,               # Pinhole.from_head_camera against the renderer's flow on a 16 x 16 pair [px]; measured 3.441e-06
}
for _k, _c in CAP.items():
    if _k in TOL:
        TOL[_k] = min(TOL[_k], _c)
M = H.Measured()


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def oracle():
    return memo("oracle", lambda: FI.oracle(DEFAULT_KPM))


def truths():
    return memo("truths", lambda: FP.truth_poses(ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"]), ID.sweep_states(KPM, STD["qpos"])))


def compare(K, C, cname):
    """(body, off, the N distinct rows) of a shape and a camera configuration"""
    return memo(("rows", K, C, cname), lambda: FI.compare_rows(oracle(), truths(), K, C, **FI.CAMERA_CONFIGS[cname]["rows"]))


def reference(K, C, cname, iters):
    """the fp64 loop on the N distinct rows: computed once, shared by the row counts"""
    def make():
        body, off, rows = compare(K, C, cname)
        return [FI.lm(oracle(), r["q0"], FI.row_problem(KPM, body, off, r), dict(FI.CAMERA_CONFIGS[cname]["cfg"], n_iters=iters)) for r in rows]
    return memo(("ref", K, C, cname, iters), make)


def cfg(kp, z_near=0.05, w_obj=0.0, w_floor=0.0, floor_z=0.0, **kw):
    c = kp.KpFitImageCfg.default()
    c.z_near, c.scene.w_obj, c.scene.pts.w_floor, c.scene.pts.floor_z = z_near, w_obj, w_floor, floor_z
    for k, v in kw.items():
        setattr(c.scene.pts.fit, k, v)
    return c


def scfg(kp, w_obj=0.0, w_floor=0.0, **kw):
    c = kp.KpFitSceneCfg.default()
    c.w_obj, c.pts.w_floor = w_obj, w_floor
    for k, v in kw.items():
        setattr(c.pts.fit, k, v)
    return c


def native(kp, d):
    """a KpFitImageCfg from an oracle configuration"""
    d = {**FI.DEFAULT_CFG, **d}
    return cfg(kp, d["z_near"], d["w_obj"], d["w_floor"], d["floor_z"], **{k: d[k] for k in ("n_iters", "mu0", "mu_min", "mu_max", "mu_up", "mu_down")})


def stack(rs, key, R=None):
    R = len(rs) if R is None else R
    return dev(np.stack([rs[e % len(rs)][key] for e in range(R)]))


def bits(t):
    return t.contiguous().view(torch.int32)


def image(sim, body, off, rs, R, c, pelvis, want=ALL, shared_cam=False, uv_w=None, **kw):
    """kp_sim_fit_image on the first R rows (row e is distinct row e % N); pelvis: the rows' tgt_pos / w_pos go in"""
    extra = dict(tgt_pos=stack(rs, "tgt_pos", R), w_pos=stack(rs, "w_pos", R)) if pelvis else {}
    if "pt_tgt" in rs[0]:                 # the rows that carry 3D targets beside their observations
        extra.update(pt_tgt=stack(rs, "pt_tgt", R), pt_w=stack(rs, "pt_w", R))
    cam = dev(rs[0]["cams"]) if shared_cam else stack(rs, "cams", R)
    return sim.fit_image(stack(rs, "q0", R), body, off, cam, stack(rs, "uv", R), uv_w, cfg=c, want=want, **extra, **kw)


# ---------------------------------------------------------------- 1. one step against the dense solve

@pytest.mark.parametrize("cname", list(FI.CAMERA_CONFIGS))
@pytest.mark.parametrize("R", ROWS)
def test_one_step_against_the_dense_solve(kp, R, cname):
    """unit cameras (weights 1 on normalised coordinates): under section 20's cap on dq; 1000 px cameras at w = 1 px^-2 (pixel magnitudes of 1e3 in
    fp32, masses of 1e5): the normwise backward error in the reference's system under section 21's cap"""
    sim = handle(kp)
    worst = {}
    for K, C in FI.COMPARE_SHAPES:
        body, off, rs = compare(K, C, cname)
        ref = reference(K, C, cname, 1)
        out = image(sim, body, off, rs, R, native(kp, dict(FI.CAMERA_CONFIGS[cname]["cfg"], n_iters=1)), K == 1)
        dq, info = out["dq"].double().cpu().numpy(), out["info"].double().cpu().numpy()
        for e in range(R):
            r = ref[e % N]
            err = float(np.abs(dq[e] - r["dq"]).max() / np.abs(r["dq"]).max())
            eta = float(np.abs(r["A"] @ dq[e] - r["g"]).max() / (np.abs(r["A"]).sum(1).max() * np.abs(dq[e]).max() + np.abs(r["g"]).max()))
            c0, c1 = abs(info[e, 0] - r["info"][0]) / r["info"][0], abs(info[e, 1] - r["info"][1]) / r["info"][0]
            if e < N:
                print(f"one step ({cname}), R = {R}, K = {K}, C = {C}, row {e}: |dq - ref|/|ref| {err:.3e}, backward error {eta:.3e}, cond(A) 2^-23 {np.linalg.cond(r['A']) * 2.0 ** -23:.2e}, "
                      f"first cost {c0:.3e}, cost after {c1:.3e}, accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}")
            assert info[e, 7] == 0 and info[e, 2] == r["info"][2] and info[e, 18] == K * C, f"K {K} C {C} row {e}"
            if cname == "unit":
                M.note("dq", err, worst); M.note("cost", max(c0, c1), worst); M.note("backward unit (reported)", eta)
            else:
                M.note("backward_px", eta, worst); M.note("cost_px", max(c0, c1), worst); M.note("dq_px", err, worst)
    if cname == "unit":
        print(f"one step (unit), R = {R}: worst dq {worst['dq']:.3e} (tolerance {TOL['dq']:.3e}, cap {CAP['dq']:.3e}), worst cost {worst['cost']:.3e} (tolerance {TOL['cost']:.3e})")
        assert worst["dq"] <= TOL["dq"] <= CAP["dq"] and worst["cost"] <= TOL["cost"]
    else:
        print(f"one step (px1000), R = {R}: normwise backward error {worst['backward_px']:.3e} (tolerance {TOL['backward_px']:.3e}, cap {CAP['backward_px']:.3e}), cost {worst['cost_px']:.3e} ({TOL['cost_px']:.3e})")
        print(f"one step (px1000), R = {R}: worst dq {worst['dq_px']:.3e} (tolerance {TOL['dq_px']:.3e}, cap {CAP['dq_px']:.3e})")
        assert worst["backward_px"] <= TOL["backward_px"] <= CAP["backward_px"] and worst["cost_px"] <= TOL["cost_px"] and worst["dq_px"] <= TOL["dq_px"] <= CAP["dq_px"]


# ---------------------------------------------------------------- 2. three iterations with the reference's accepted steps

@pytest.mark.parametrize("R", ROWS)
def test_three_iterations(kp, R):
    sim = handle(kp)
    worst = {}
    for cname in FI.CAMERA_CONFIGS:
        for K, C in FI.COMPARE_SHAPES:
            body, off, rs = compare(K, C, cname)
            ref, ref0 = reference(K, C, cname, FI.COMPARE_ITERS), reference(K, C, cname, 0)
            out = image(sim, body, off, rs, R, native(kp, dict(FI.CAMERA_CONFIGS[cname]["cfg"], n_iters=FI.COMPARE_ITERS)), K == 1)
            q, info, ue = out["qpos"].double().cpu().numpy(), out["info"].double().cpu().numpy(), out["uv_err"].double().cpu().numpy()
            pe = out["pt_err"].double().cpu().numpy()
            for e in range(R):
                r = ref[e % N]
                dc, dqp = abs(info[e, 1] - r["info"][1]) / r["info"][0], float(np.abs(q[e] - r["qpos"]).max())
                drms = abs(info[e, 17] - r["info"][17]) / ref0[e % N]["info"][17]
                if e < N:
                    print(f"three iterations ({cname}), R = {R}, K = {K}, C = {C}, row {e}: cost {dc:.3e}, qpos {dqp:.3e}, rms {info[e, 17]:.4e} / {r['info'][17]:.4e} px ({drms:.3e}), "
                          f"accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}")
                M.note("it3_cost", dc, worst); M.note("it3_qpos", dqp, worst); M.note("it3_rms", drms, worst)
                assert info[e, 2] == r["info"][2] and info[e, 7] == 0 and info[e, 18] == r["info"][18], f"{cname} K {K} C {C} row {e}: accepted steps"
                assert abs(info[e, 16] - ue[e].max()) <= 1e-6 * max(1.0, info[e, 16]) and abs(info[e, 19] - r["info"][19]) < 1e-3
                if "pt_tgt" in rs[0]:
                    M.note("it3_pt", abs(info[e, 8] - r["info"][8]), worst)
                    assert info[e, 8] > 0 and info[e, 8] == np.float32(pe[e].max())
                else:
                    assert not pe[e].any() and not info[e, 8:10].any(), "without 3D targets pt_err and info 8 / 9 are zeros"
    print(f"three iterations, R = {R}: cost {worst['it3_cost']:.3e} (tolerance {TOL['it3_cost']:.3e}), qpos {worst['it3_qpos']:.3e} ({TOL['it3_qpos']:.3e}), rms {worst['it3_rms']:.3e} ({TOL['it3_rms']:.3e})")
    print(f"three iterations, R = {R}: max |e_k| of the rows with 3D targets {worst['it3_pt']:.3e} m (tolerance {TOL['it3_pt']:.3e})")
    assert worst["it3_cost"] <= TOL["it3_cost"] and worst["it3_qpos"] <= TOL["it3_qpos"] and worst["it3_rms"] <= TOL["it3_rms"] and worst["it3_pt"] <= TOL["it3_pt"]


# ---------------------------------------------------------------- 3. convergence

def test_two_cameras_converge(kp):
    """two cameras 90 degrees apart observe a reachable pose exactly: the reference ends below 0.05 px (chosen so in tests/test_fit_image_cpu.py); the
    device is held to the reference's figure.  One shared camera table per call here (camera_rows = 1)."""
    sim = handle(kp)
    body, off = FI.marker_choice(53)
    rs = memo("conv", lambda: FI.convergence_rows(oracle(), KPM, truths()))
    ref = memo("conv_ref", lambda: [FI.lm(oracle(), r["q0"], r["pb"], r["cfg"]) for r in rs])
    worst = {}
    for e, r in enumerate(rs):
        out = image(sim, body, off, [r], 5, native(kp, r["cfg"]), False, shared_cam=True)
        info = out["info"].double().cpu().numpy()
        d = float(np.abs(info[:, 17] - ref[e]["info"][17]).max())
        print(f"{r['name']}: reprojection rms {info[0, 17]:.3e} px (reference {ref[e]['info'][17]:.3e}), max {info[0, 16]:.3e} px, accepted {info[0, 2]:.0f} / {ref[e]['info'][2]:.0f}, "
              f"qpos against the truth {float(np.abs(out['qpos'][0].double().cpu().numpy() - FP.normalized(truths()[(0, 2, 4, 5)[e]])).max()):.3e}")
        M.note("conv_rms", d, worst)
        assert ref[e]["info"][17] < 0.05 and not info[:, 7].any() and torch.equal(bits(out["qpos"][0]), bits(out["qpos"][4]))
    print(f"two cameras: reprojection rms against the reference's {worst['conv_rms']:.3e} px (tolerance {TOL['conv_rms']:.3e})")
    assert worst["conv_rms"] <= TOL["conv_rms"]


def test_one_camera_on_the_floor(kp):
    """one camera, the floor term and the hinge prior, from a pose pushed 0.03 m into the floor: section 20's derived bound holds (the candidate
    'translate up by delta' costs less than section 20's, fit_image_oracle.floor_rows)"""
    sim = handle(kp)
    body, off = FI.marker_choice(53)
    rs = memo("floor", lambda: FI.floor_rows(oracle(), KPM, truths()))
    out = sim.fit_image(stack(rs, "q0"), body, off, stack(rs, "cams"), stack(rs, "uv"), q_prior=stack(rs, "q_prior"), w_prior=stack(rs, "w_prior"), cfg=native(kp, rs[0]["cfg"]), want=ALL)
    start = sim.fit_image(stack(rs, "q0"), body, off, stack(rs, "cams"), stack(rs, "uv"), q_prior=stack(rs, "q_prior"), w_prior=stack(rs, "w_prior"),
                          cfg=native(kp, dict(rs[0]["cfg"], n_iters=0)), want=ALL)
    info, i0 = out["info"].double().cpu().numpy(), start["info"].double().cpu().numpy()
    for e, r in enumerate(rs):
        print(f"{r['name']}: deepest vertex {i0[e, 10] * 1e3:.2f} -> {info[e, 10] * 1e3:.3f} mm (bound {CAP['floor_depth'] * 1e3:.1f}), cost {info[e, 0]:.4e} -> {info[e, 1]:.4e} "
              f"(candidate {r['cand_cost']:.4e}), rms {info[e, 17]:.3e}, accepted {info[e, 2]:.0f}")
        M.note("floor_depth (derived bound)", info[e, 10])
        assert info[e, 7] == 0 and i0[e, 10] >= 0.029 and info[e, 1] <= r["cand_cost"] and info[e, 10] <= CAP["floor_depth"], r["name"]


@pytest.mark.parametrize("R", ROWS)
def test_three_iterations_on_the_floor(kp, R):
    """the floor term active under one camera and the hinge prior, three iterations at w_floor 4 (section 20's comparison): the fp64 loop keeps every
    vertex 1e-5 m off the plane at every pose (tests/test_fit_image_cpu.py), so the device holds the reference's active sets and accepted steps"""
    sim = handle(kp)
    body, off = FI.marker_choice(53)
    rs = memo("floor3", lambda: FI.floor_compare_rows(oracle(), KPM, truths()))
    ref = memo("floor3_ref", lambda: [FI.lm(oracle(), r["q0"], r["pb"], r["cfg"]) for r in rs])
    out = sim.fit_image(stack(rs, "q0", R), body, off, stack(rs, "cams", R), stack(rs, "uv", R), q_prior=stack(rs, "q_prior", R), w_prior=stack(rs, "w_prior", R),
                        cfg=native(kp, rs[0]["cfg"]), want=ALL)
    info = out["info"].double().cpu().numpy()
    worst = {}
    for e in range(R):
        r = ref[e % N]
        dc, dd = abs(info[e, 1] - r["info"][1]) / r["info"][0], abs(info[e, 10] - r["info"][10])
        if e < N:
            print(f"three iterations on the floor, R = {R}, row {e} {rs[e % N]['name']}: cost {dc:.3e}, depth {info[e, 10] * 1e3:.4f} / {r['info'][10] * 1e3:.4f} mm ({dd:.3e} m), "
                  f"below {info[e, 11]:.0f} / {r['info'][11]:.0f}, accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}")
        M.note("floor3_cost", dc, worst); M.note("floor3_depth", dd, worst)
        assert info[e, 7] == 0 and info[e, 2] == r["info"][2] and info[e, 11] == r["info"][11] and info[e, 18] == 53, f"row {e}: accepted steps and vertices below the floor"
    print(f"three iterations on the floor, R = {R}: cost {worst['floor3_cost']:.3e} (tolerance {TOL['floor3_cost']:.3e}), depth {worst['floor3_depth']:.3e} m ({TOL['floor3_depth']:.3e})")
    assert worst["floor3_cost"] <= TOL["floor3_cost"] and worst["floor3_depth"] <= TOL["floor3_depth"]


# ---------------------------------------------------------------- 4. bit for bit

@pytest.mark.parametrize("R", ROWS)
def test_equals_fit_scene_where_the_term_is_absent(kp, R):
    sim, obj = handle(kp), handle(kp, STEP_KPM)
    body, off, rs = compare(53, 3, "px1000")
    q0 = stack(rs, "q0", R)
    tgt = dev(np.stack([FT.marker_positions(oracle(), r["q_true"], body, off) for r in rs]))[torch.arange(R, device="cuda") % N].contiguous()
    cam, uv = stack(rs, "cams", R), stack(rs, "uv", R)
    nan_uv = torch.full_like(uv, float("nan"))
    blk = dev(np.tile(FS.block(box=[0.3, 0.0, 0.2, 1, 0, 0, 0]), (R, 1)))
    for what, s, objs in (("floor blob", sim, None), ("object blob", obj, blk)):
        ref = s.fit_scene(q0, body, off, tgt, obj_qpos=objs, cfg=scfg(kp, 50.0, 50.0, n_iters=5), want=SCENE)
        assert bool((ref["info"][:, 2] > 0).all())
        c = cfg(kp, 0.05, 50.0, 50.0, n_iters=5)
        for name, kw in (("no cameras", dict()), ("every uv_w 0, uv NaN", dict(cam=cam, uv=nan_uv, uv_w=torch.zeros(R, 3, 53, device="cuda"))),
                         ("every uv_w negative", dict(cam=cam, uv=uv, uv_w=torch.full((R, 3, 53), -1.0, device="cuda")))):
            out = s.fit_image(q0, body, off, pt_tgt=tgt, obj_qpos=objs, cfg=c, want=ALL if "cam" in kw else SCENE, **kw)
            for k in ("qpos", "dq", "pt_err"):
                assert torch.equal(bits(out[k]), bits(ref[k])), f"{what}, {name}: {k}"
            assert torch.equal(bits(out["info"][:, :16]), bits(ref["info"])) and not out["info"][:, 16:].any(), f"{what}, {name}: info"
            assert "uv_err" not in out or not out["uv_err"].any()
        # a NULL obs pointer through the C ABI itself (the binding always passes a struct)
        P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        offc = np.ascontiguousarray(off, np.float32)
        ms = kp.KpMarkerSet(53, body.ctypes.data_as(ctypes.c_void_p), offc.ctypes.data_as(ctypes.c_void_p))
        raw = {k: torch.full((R, *shape), 7, dtype=dt, device="cuda") for k, (shape, dt) in kp.fit_image_outputs(53, 0).items() if k != "uv_err"}
        fout = kp.KpFitImageOut(P(raw["qpos"]), P(raw["info"]), P(raw["dq"]), P(raw["pt_err"]), None)
        rc = s.L.kp_sim_fit_image(s.h, R, ctypes.byref(ms), ctypes.byref(kp.KpFitPointsIn(P(q0), P(tgt))), None if objs is None else P(objs), None, ctypes.byref(c), ctypes.byref(fout))
        assert rc == 0, s.L.kp_last_error().decode()
        torch.cuda.synchronize()
        for k in ("qpos", "dq", "pt_err"):
            assert torch.equal(bits(raw[k]), bits(ref[k])), f"{what}, NULL obs: {k}"
        assert torch.equal(bits(raw["info"][:, :16]), bits(ref["info"])) and not raw["info"][:, 16:].any(), f"{what}, NULL obs: info"


def test_bitwise_consistency(kp, monkeypatch):
    sim = handle(kp)
    body, off, rs = compare(53, 3, "px1000")
    R = 67
    c = native(kp, dict(FI.CAMERA_CONFIGS["px1000"]["cfg"], n_iters=4))
    monkeypatch.delenv("KP_ROWS_CHUNK", raising=False)
    full = image(sim, body, off, rs, R, c, False)
    again = image(sim, body, off, rs, R, c, False)
    for k in ALL:
        assert torch.equal(bits(full[k]), bits(again[k])), f"a second call: {k}"
    q0, cam, uv = stack(rs, "q0", R), stack(rs, "cams", R), stack(rs, "uv", R)
    for e in (0, 41, 66):
        alone = sim.fit_image(q0[e:e + 1], body, off, cam[e:e + 1], uv[e:e + 1], cfg=c, want=ALL)
        for k in ALL:
            assert torch.equal(bits(full[k][e]), bits(alone[k][0])), f"row {e} of 67 against the row alone: {k}"
    monkeypatch.setenv("KP_ROWS_CHUNK", "64")
    chunked = image(sim, body, off, rs, R, c, False)
    monkeypatch.delenv("KP_ROWS_CHUNK")
    for k in ALL:
        assert torch.equal(bits(full[k]), bits(chunked[k])), f"KP_ROWS_CHUNK = 64: {k}"
    assert bool((full["info"][:, 2] > 0).all()) and bool(torch.isfinite(full["qpos"]).all()) and bool((full["info"][:, 18] == 159).all())
    # one camera table for all rows = the same record repeated R times
    shared = sim.fit_image(q0, body, off, cam[0].contiguous(), uv, cfg=c, want=ALL)
    repeated = sim.fit_image(q0, body, off, cam[0].expand(R, 3, 16).contiguous(), uv, cfg=c, want=ALL)
    for k in ALL:
        assert torch.equal(bits(shared[k]), bits(repeated[k])), f"camera_rows 1 against R equal records: {k}"
    # a NaN uv at weight 0 = the observation removed (here: camera 2 switched off against the call with two cameras)
    w = torch.ones(R, 3, 53, device="cuda"); w[:, 2] = 0.0
    uvn = uv.clone(); uvn[:, 2] = float("nan")
    off3 = sim.fit_image(q0, body, off, cam, uvn, w, cfg=c, want=ALL)
    two = sim.fit_image(q0, body, off, cam[:, :2].contiguous(), uv[:, :2].contiguous(), cfg=c, want=ALL)
    for k in ("qpos", "info", "dq", "pt_err"):
        assert torch.equal(bits(off3[k]), bits(two[k])), f"camera 2 at weight 0 with NaN uv against two cameras: {k}"
    assert torch.equal(bits(off3["uv_err"][:, :2]), bits(two["uv_err"])) and not off3["uv_err"][:, 2].any()
    # single observations dropped: the row's sums hold the bits of the call without them
    w = torch.ones(R, 3, 53, device="cuda"); w[:, 1, 7] = 0.0; w[:, 0, 40] = -2.0
    uvn = uv.clone(); uvn[:, 1, 7] = float("nan"); uvn[:, 0, 40] = float("inf")
    a, b = sim.fit_image(q0, body, off, cam, uvn, w, cfg=c, want=ALL), sim.fit_image(q0, body, off, cam, uv, w, cfg=c, want=ALL)
    for k in ALL:
        assert torch.equal(bits(a[k]), bits(b[k])), f"a skipped observation's uv is not read: {k}"
    assert bool((a["info"][:, 18] == 157).all()) and not a["uv_err"][:, 1, 7].any()
    lead = sim.fit_image(q0[:6].view(2, 3, 76), body, off, cam[:6].view(2, 3, 3, 16), uv[:6].view(2, 3, 3, 53, 2), cfg=c, want=ALL)
    assert lead["info"].shape == (2, 3, 20) and lead["uv_err"].shape == (2, 3, 3, 53) and torch.equal(bits(lead["qpos"].view(6, 76)), bits(full["qpos"][:6]))


# ---------------------------------------------------------------- 5. edge rows

def test_edge_rows(kp):
    sim = handle(kp)
    body, off, rs = compare(53, 3, "px1000")
    c = native(kp, dict(FI.CAMERA_CONFIGS["px1000"]["cfg"], n_iters=4))
    q0, cam, uv = stack(rs, "q0", 5), stack(rs, "cams", 5), stack(rs, "uv", 5)
    clean = sim.fit_image(q0, body, off, cam, uv, cfg=c, want=ALL)

    def check(out, status, what):
        for e in (0, 1, 3, 4):
            for k in ALL:
                assert torch.equal(bits(out[k][e]), bits(clean[k][e])), f"{what}: row {e}, {k}"
        assert out["info"][2, 7] == status and out["info"][2, 2] == 0 and not out["info"][2, 8:].any() and not out["dq"][2].any() and not out["uv_err"][2].any(), what
        assert torch.equal(bits(out["qpos"][2]), bits(q0[2])), f"{what}: the input comes back as given"

    for col in (2, 10, 13):
        bad = cam.clone(); bad[2, 1, col] = float("nan")
        check(sim.fit_image(q0, body, off, bad, uv, cfg=c, want=ALL), 1, f"NaN in camera column {col}")
    w = torch.ones(5, 3, 53, device="cuda"); w[2, 0, 9] = float("nan")
    check(sim.fit_image(q0, body, off, cam, uv, w, cfg=c, want=ALL), 1, "a NaN weight")
    w = torch.ones(5, 3, 53, device="cuda")
    bad = uv.clone(); bad[2, 2, 30, 1] = float("inf")
    out = sim.fit_image(q0, body, off, cam, bad, w, cfg=c, want=ALL)
    assert out["info"][2, 7] == 1 and torch.equal(bits(out["qpos"][2]), bits(q0[2])), "a uv that is not finite under a positive weight"
    # a weighted point behind the camera at the start: status 2, the input back; z_near is the configuration's
    r = memo("cross", lambda: FI.crossing_row(oracle(), KPM, truths()))
    ref = memo("cross_ref", lambda: FI.lm(oracle(), r["q0"], r["pb"], r["cfg"]))
    qs = dev(np.stack([r["q0"], r["q0"], r["q_behind"], r["q0"], r["q0"]]))
    cc = native(kp, r["cfg"])
    out = sim.fit_image(qs, body, off, dev(r["cams"]), dev(np.tile(r["uv"], (5, 1, 1, 1))), cfg=cc, want=ALL)
    info = out["info"].double().cpu().numpy()
    assert info[2, 7] == 2 and info[2, 2] == 0 and np.isinf(info[2, 0]) and not info[2, 8:].any() and torch.equal(bits(out["qpos"][2]), bits(qs[2])) and not out["uv_err"][2].any()
    # its neighbours: the first trial crosses z_near, the reference rejects it, and the accepted steps are the reference's
    dc = abs(info[0, 1] - ref["info"][1]) / ref["info"][0]
    print(f"crossing row: accepted {info[0, 2]:.0f} / {ref['info'][2]:.0f} (reference crossed {ref['crossed']}), cost {info[0, 0]:.4e} -> {info[0, 1]:.4e} (reference {ref['info'][1]:.4e}, {dc:.3e}), "
          f"smallest depth {info[0, 19]:.4f} (z_near {r['cfg']['z_near']})")
    M.note("cross_cost", dc)
    for e in (0, 1, 3, 4):
        assert info[e, 7] == 0 and info[e, 2] == ref["info"][2] and info[e, 2] < r["cfg"]["n_iters"] and info[e, 19] >= r["cfg"]["z_near"]
        assert torch.equal(bits(out["qpos"][e]), bits(out["qpos"][0]))
    one = sim.fit_image(qs[:1], body, off, dev(r["cams"]), dev(r["uv"][None]), cfg=native(kp, dict(r["cfg"], n_iters=1)), want=ALL)
    assert one["info"][0, 2] == 0 and one["info"][0, 1] == one["info"][0, 0] and torch.equal(bits(one["qpos"][0, 7:]), bits(qs[0, 7:])), "the first trial is the one that crosses"
    assert dc <= TOL["cross_cost"]


# ---------------------------------------------------------------- 6. refusals

def test_refusals(kp, tmp_path):
    from kinpoly_amd.model_compiler import write_kpm
    m = read_kpm(DEFAULT_KPM)
    m["obj_geoms"] = np.zeros((0, 18), m["obj_geoms"].dtype)
    write_kpm(m, str(tmp_path / "no_objects.kpm"))
    sim, lean = handle(kp), kp.KpSim(kp.KpModel(str(tmp_path / "no_objects.kpm")), 1)
    body, off, rs = compare(53, 3, "px1000")
    off = np.ascontiguousarray(off, np.float32)
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    q0, cam, uv = stack(rs, "q0", 5), stack(rs, "cams", 5), stack(rs, "uv", 5)
    bufs, fout = H.sentinel(kp.fit_image_outputs(53, 3), kp.KpFitImageOut)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ms = kp.KpMarkerSet(53, body.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p))
    fin = kp.KpFitPointsIn(P(q0))
    obs = lambda n=3, rows=5, c=P(cam), u=P(uv): kp.KpFitImageObs(n, rows, c, u, None)      # noqa: E731
    ok, f, B = cfg(kp), L.kp_sim_fit_image, ctypes.byref
    assert f(None, 5, B(ms), B(fin), None, B(obs()), B(ok), B(fout)) != 0 and "null handle" in err()
    assert f(sim.h, -1, B(ms), B(fin), None, B(obs()), B(ok), B(fout)) != 0 and "n_rows" in err()
    assert f(sim.h, 5, None, B(fin), None, B(obs()), B(ok), B(fout)) != 0 and "null markers" in err()
    assert f(sim.h, 5, B(ms), None, None, B(obs()), B(ok), B(fout)) != 0 and "null in" in err()
    assert f(sim.h, 5, B(ms), B(fin), None, B(obs()), None, B(fout)) != 0 and "null cfg" in err()
    assert f(sim.h, 5, B(ms), B(fin), None, B(obs()), B(ok), None) != 0 and "null out" in err()
    assert f(sim.h, 5, B(ms), B(fin), None, None, B(ok), B(fout)) != 0 and "nothing to fit" in err()
    assert f(sim.h, 5, B(ms), B(fin), None, B(obs(0)), B(ok), B(fout)) != 0 and "nothing to fit" in err()
    for n in (-1, 9):
        assert f(sim.h, 5, B(ms), B(fin), None, B(obs(n)), B(ok), B(fout)) != 0 and "n_cams" in err(), n
    for rows in (0, 2, 4, 6):
        assert f(sim.h, 5, B(ms), B(fin), None, B(obs(3, rows)), B(ok), B(fout)) != 0 and "camera_rows" in err(), rows
    assert f(sim.h, 5, B(ms), B(fin), None, B(obs(c=None)), B(ok), B(fout)) != 0 and "null cam" in err()
    assert f(sim.h, 5, B(ms), B(fin), None, B(obs(u=None)), B(ok), B(fout)) != 0 and "null uv" in err()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert f(sim.h, 5, B(ms), B(fin), None, B(obs()), B(cfg(kp, v)), B(fout)) != 0 and "z_near" in err(), v
    for v in (-1.0, float("nan")):
        assert f(sim.h, 5, B(ms), B(fin), None, B(obs()), B(cfg(kp, 0.05, v)), B(fout)) != 0 and "w_obj" in err(), v
        assert f(sim.h, 5, B(ms), B(fin), None, B(obs()), B(cfg(kp, 0.05, 0.0, v)), B(fout)) != 0 and "w_floor" in err(), v
    assert f(sim.h, 5, B(ms), B(fin), None, B(obs()), B(cfg(kp, n_iters=-1)), B(fout)) != 0 and "n_iters" in err()
    assert f(lean.h, 5, B(ms), B(fin), P(q0), B(obs()), B(ok), B(fout)) != 0 and "no object geoms" in err()
    wide = kp.KpSim(kp.KpModel(DEFAULT_KPM, threads_per_env=128), 5)
    assert f(wide.h, 5, B(ms), B(fin), None, B(obs()), B(ok), B(fout)) != 0 and "threads_per_env" in err()
    assert f(sim.h, 0, B(ms), B(fin), None, B(obs(3, 1)), B(ok), B(fout)) == 0, "n_rows == 0 does nothing"
    H.refused_calls_wrote_nothing(bufs)
    for call in (lambda: sim.fit_image(q0, body, off, cam[:4], uv), lambda: sim.fit_image(q0, body, off, cam.cpu(), uv), lambda: sim.fit_image(q0, body, off, cam, uv.double()),
                 lambda: sim.fit_image(q0, body, off), lambda: sim.fit_image(q0, body, off, cam, uv, cfg=cfg(kp, -1.0))):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()                                             # no sticky HIP error: the next launch works
    assert torch.isfinite(sim.fit_image(q0, body, off, cam, uv, cfg=cfg(kp, n_iters=1))["qpos"]).all()


# ---------------------------------------------------------------- 7. the control step

@pytest.mark.parametrize("scene_name", ["floor", "h_push"])
def test_the_control_step_is_bit_identical(kp, scene_name):
    body, off, rs = compare(53, 3, "px1000")

    def between(sim):
        objs = dev(np.tile(FS.block(box=[0.3, 0.0, 0.2, 1, 0, 0, 0]), (5, 1))) if scene_name == "h_push" else None
        out = sim.fit_image(stack(rs, "q0", 5), body, off, stack(rs, "cams", 5), stack(rs, "uv", 5), obj_qpos=objs,
                            cfg=native(kp, dict(FI.CAMERA_CONFIGS["px1000"]["cfg"], n_iters=3, w_floor=10.0, w_obj=10.0)), want=ALL)
        assert torch.isfinite(out["qpos"]).all() and not out["info"][:, 7].any()
        stored = sim.fit_image(sim.view("qpos"), body, off, dev(rs[0]["cams"]), stack(rs, "uv", 67), cfg=native(kp, dict(FI.CAMERA_CONFIGS["px1000"]["cfg"], n_iters=2)))      # on the stored rows too
        assert torch.isfinite(stored["qpos"]).all()
    H.control_step_untouched(kp, scene_name, between)


# ---------------------------------------------------------------- 8. the renderer's flow

def test_pinhole_agrees_with_the_egocentric_renderer(kp):
    """one 16 x 16 render_ego pair with equal poses and a second camera B: what pixel (px, py) of A shows lies at eye_A + depth dir; through
    Pinhole.from_head_camera(B) it lands at the pixel centre + flow wherever ok = 1"""
    from kinpoly_amd.fit import Pinhole
    sim = handle(kp)
    W = Hh = 16
    q = dev(np.asarray(STD["qpos"], np.float32)[None])
    camA = np.array([2.5, 0.3, 1.4, *FS._quat([0.0, 1.0, 0.0], -1.9), 60.0])
    camB = np.array([2.4, 0.5, 1.5, *FS._quat([0.1, 1.0, 0.05], -1.8), 50.0])
    out = sim.render_ego(q, None, dev(camA[None]), q, None, dev(camB[None]), width=W, height=Hh, want=("depth", "flow", "ok", "geom"))
    depth, flow, okm = out["depth"][0].double().cpu().numpy(), out["flow"][0].double().cpu().numpy(), out["ok"][0].cpu().numpy().astype(bool)
    Rm = RO.qmat(camA[3:7] / np.linalg.norm(camA[3:7]))
    th = np.tan(0.5 * np.radians(camA[7]))
    x, y = np.meshgrid(np.arange(W), np.arange(Hh))
    sx, sy = 2.0 * (x + 0.5) / W - 1.0, 1.0 - 2.0 * (y + 0.5) / Hh
    d = Rm[:, 2][None, None] + (sx * th * (W / Hh))[..., None] * (-Rm[:, 0])[None, None] + (sy * th)[..., None] * Rm[:, 1][None, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    hit = okm & np.isfinite(depth)
    assert hit.sum() > 60 and len(np.unique(out["geom"][0].cpu().numpy()[hit])) >= 2, "the floor and the figure are both in view"
    p = camA[:3] + depth[hit][:, None] * d[hit]
    got = Pinhole.from_head_camera(camB, W, Hh).project(p)
    want = np.stack([x[hit] + 0.5, y[hit] + 0.5], 1) + flow[hit]
    err = float(np.abs(got - want).max())
    print(f"Pinhole.from_head_camera against the renderer's flow on {hit.sum()} pixels: {err:.3e} px (tolerance {TOL['flow']:.1e}), flow up to {np.abs(flow[hit]).max():.2f} px")
    M.note("flow", err)
    assert err <= TOL["flow"]


# ---------------------------------------------------------------- 9. end to end

def test_keypoints_to_takes_end_to_end(kp, tmp_path):
    """A two-take synthetic track seen by two cameras: scripts/fit_takes.py --keypoints --cameras fits it, the reprojection error of the result is
    small, and AmassSingleDataset reads the pickle."""
    import joblib
    from kinpoly_amd import dataset, fit
    sim = handle(kp)
    body, off = FI.marker_choice(53)
    ms = fit.MarkerSet([f"m{k}" for k in range(53)], body, off)
    takes = dataset.synthetic_takes(sim, STD["qpos"], n_per_action=1, T_range=(40, 41), with_objects=False)
    names = sorted(takes)[:2]
    centre = np.asarray(takes[names[0]]["qpos"], np.float64)[0, :3]
    cams = [fit.Pinhole(c[:9].reshape(3, 3), c[9:12], *c[12:]) for c in FI.ring(centre, 2, dist=4.0)]
    tracks = {}
    rng = np.random.default_rng(9)
    for k in names:
        p = np.stack([FT.marker_positions(oracle(), q, body, off) for q in np.asarray(takes[k]["qpos"], np.float64)])      # [T, 53, 3]
        uv = np.stack([c.project(p) for c in cams], 1) + rng.normal(size=(len(p), 2, 53, 2)) * 0.5
        conf = rng.uniform(0.5, 1.0, uv.shape[:3])
        drop = rng.uniform(size=conf.shape) < 0.05
        uv[drop] = np.nan; conf[rng.uniform(size=conf.shape) < 0.03] = 0.0
        tracks[k] = {"uv": uv, "conf": conf}
    ms.save(tmp_path / "set.json")
    joblib.dump(tracks, tmp_path / "uv.pkl")
    joblib.dump(np.stack([c.pack() for c in cams]), tmp_path / "cams.pkl")
    spec = importlib.util.spec_from_file_location("fit_takes", os.path.join(ROOT, "scripts", "fit_takes.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    _, rep = mod.main(["--keypoints", str(tmp_path / "uv.pkl"), "--cameras", str(tmp_path / "cams.pkl"), "--markers", str(tmp_path / "set.json"), "--out", str(tmp_path / "takes.pkl"),
                       "--floor", "100"], sim=sim)
    ds = dataset.AmassSingleDataset({"file_path": str(tmp_path / "takes.pkl"), "t_min": 30}, "train")
    assert ds.data_keys == names and list(ds.lens) == [40, 40]
    for k, r in rep.items():
        print(f"{k}: reprojection mean {r['mean_px_err']:.3f} px, p90 {r['px_err_p90']:.3f}, max {r['max_px_err']:.3f}, detected {r['detected_share']:.3f}, accepted {r['accepted_share']:.3f}")
        # 0.5 px of noise per coordinate: |e| has mean 0.63 px; a fit that follows the track stays within a few of it
        assert r["failed_rows"] == 0 and r["rows_behind_camera"] == 0 and r["mean_px_err"] < 2.0 and "per_camera" in r


def test_zz_measured_figures():
    """the figures this run measured, beside the tolerances (runs last in the file)"""
    for k in sorted(M):
        print(f"measured {k}: {M[k]:.3e}" + (f"  (tolerance {TOL[k]:.3e})" if k in TOL else ""))
