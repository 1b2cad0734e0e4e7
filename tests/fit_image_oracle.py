"""fp64 reference of the pose fit to 2D key points seen by calibrated cameras (kp_sim_fit_image): test infrastructure.

fit_scene_oracle's loop with one more term: per camera c (16 floats: R_cw row-major, t, fx, fy, cx, cy) and point k of the marker set,
    1/2 w_ck |uv_ck - pi_c(p_k)|^2,   cam = R_cw p + t,   pi = (cx + fx cam_x / cam_z, cy + fy cam_y / cam_z)
The gradient is exact (J_p^T w J^T e with J = J_pi R_cw, 2 x 3); in the matrix an observation is the isotropic block m J_p^T J_p with m = w lambda,
lambda the largest eigenvalue of J_pi J_pi^T in the kernel's closed form.  A weighted observation with cam_z < z_near makes the cost +inf (at the
start: status 2, no iteration).  The solve is dense.
"""
import numpy as np

import fit_points_oracle as FT
import fit_pose_oracle as FP
import fit_scene_oracle as FS
import push_oracle as PO
from np_rigid import f32, oracle  # noqa: F401  (the tests reach them through this module)

NV, NB, NU, NQ = FS.NV, FS.NB, FS.NU, FS.NQ
DEFAULT_CFG = dict(FS.DEFAULT_CFG, z_near=0.05)


def problem(kpm, geoms=None, cams=None, uv=None, uv_w=None, **kw):
    """fit_scene_oracle.problem's row with its cameras [C, 16], observations uv [C, K, 2] and weights [C, K] (None: ones).  pt_tgt None with K > 0: no 3D
    term.  An observation with w <= 0 is skipped (its uv is never looked at)."""
    K = len(np.asarray(kw.get("pt_body", ()), int).reshape(-1))
    if kw.get("pt_tgt") is None and K:
        kw = dict(kw, pt_tgt=np.zeros((K, 3)), pt_w=np.zeros(K))
    pb = FS.problem(kpm, geoms, **kw)
    cams = np.zeros((0, 16)) if cams is None else np.asarray(cams, np.float64).reshape(-1, 16)
    C = len(cams)
    w = np.ones((C, K)) if uv_w is None else np.asarray(uv_w, np.float64).reshape(C, K)
    on = w > 0
    obs = np.zeros((C, K, 2))
    if C and K:
        obs[on] = np.asarray(uv, np.float64).reshape(C, K, 2)[on]
    bad = bool(pb["bad"] or np.isnan(w).any() or not np.isfinite(obs[on]).all() or not np.isfinite(cams).all())
    return dict(pb, cams=cams, uv=obs, uv_w=np.where(on, w, 0.0), uv_on=on, bad=bad)


def projection(cam, p):
    """(pixel [2], J [2, 3] = d pixel / d p in the world frame, lambda: the majoriser's eigenvalue in the kernel's closed form, cam_z) of world point p"""
    R, t, (fx, fy, cx, cy) = cam[:9].reshape(3, 3), cam[9:12], cam[12:16]
    c = R @ p + t
    a, b, z = c[0] / c[2], c[1] / c[2], c[2]
    Jpi = np.array([[fx / z, 0.0, -fx * a / z], [0.0, fy / z, -fy * b / z]])
    a11, a22, a12 = (fx / z) ** 2 * (1 + a * a), (fy / z) ** 2 * (1 + b * b), fx * fy * a * b / z ** 2
    lam = 0.5 * (a11 + a22) + np.sqrt((0.5 * (a11 - a22)) ** 2 + a12 ** 2)
    return np.array([cx + fx * a, cy + fy * b]), Jpi @ R, float(lam), float(z)


def image_terms(pb, p, cfg):
    """the weighted observations at the world points p [K, 3], in the kernel's order within a body (point, then camera):
    [dict(k, c, w, e [2], J [2, 3], lam, z)], and whether one of them lies in front of z_near"""
    terms, behind = [], False
    for k in range(len(p)):
        for c in range(len(pb["cams"])):
            if not pb["uv_on"][c, k]:
                continue
            px, J, lam, z = projection(pb["cams"][c], p[k])
            if z < float(cfg["z_near"]):
                behind = True
                continue
            terms.append(dict(k=k, c=c, w=float(pb["uv_w"][c, k]), e=pb["uv"][c, k] - px, J=J, lam=lam, z=z))
    return terms, behind


def residuals(pb, xpos, xquat, cfg):
    res = FS.residuals(pb, xpos, xquat, cfg)
    res["img"], res["behind"] = image_terms(pb, res["p"], cfg)
    return res


def image_cost(res):
    return np.inf if res["behind"] else 0.5 * sum(t["w"] * float(t["e"] @ t["e"]) for t in res["img"])


def cost_of(pb, q, res, cfg):
    return FS.cost_of(pb, q, res, cfg) + image_cost(res)


def evaluate(o, pb, q, cfg):
    xpos, xquat = FP.fk(o, q)
    res = residuals(pb, xpos, xquat, cfg)
    return cost_of(pb, q, res, cfg), res


def normal_system(o, pb, q, mu, cfg, exact=False):
    """fit_scene_oracle.normal_system with the image term: blocks m J_p^T J_p (exact: the Gauss-Newton blocks w J_p^T J^T J J_p instead), gradient
    J_p^T w J^T e"""
    A, g, H, _ = FS.normal_system(o, pb, q, mu, cfg)
    qn = FP.normalized(q)
    Jc, com, xpos, xquat = PO.body_jacobians(o, qn)
    res = residuals(pb, xpos, xquat, cfg)
    Hi = np.zeros((NV, NV))
    if res["img"]:
        ks = np.array([t["k"] for t in res["img"]])
        Jp = FT.point_jacobians(Jc, com, res["p"][ks], pb["body"][ks])
        for i, t in enumerate(res["img"]):
            JJ = t["J"] @ Jp[i]
            Hi += t["w"] * JJ.T @ JJ if exact else t["w"] * t["lam"] * Jp[i].T @ Jp[i]
            g = g + t["w"] * (JJ.T @ t["e"])
    return A + Hi, g, H + Hi, res


def image_figures(pb, res):
    """info 16..19 and uv_err [C, K]: max and rms reprojection error over the weighted observations, their number, the smallest cam_z"""
    err = np.zeros(pb["uv_on"].shape)
    for t in res["img"]:
        err[t["c"], t["k"]] = np.linalg.norm(t["e"])
    n = len(res["img"])
    return [float(err.max()) if n else 0.0, float(np.sqrt((err ** 2).sum() / n)) if n else 0.0, float(n), min(t["z"] for t in res["img"]) if n else 0.0], err


def z_margin(res, pb, cfg):
    """the smallest |cam_z - z_near| over the weighted observations of a pose (behind ones included)"""
    m = np.inf
    for k in range(len(res["p"])):
        for c in range(len(pb["cams"])):
            if pb["uv_on"][c, k]:
                m = min(m, abs(projection(pb["cams"][c], res["p"][k])[3] - float(cfg["z_near"])))
    return m


def lm(o, q0, pb, cfg=None, jnt_range=None, jnt_limited=None):
    """The kernel's loop in fp64.  Returns fit_scene_oracle.lm's dict with info [20], uv_err [C, K], z_margin (the smallest |cam_z - z_near| of a
    weighted observation over every pose the loop evaluated) and crossed (trial poses rejected because a point went behind a camera)."""
    cfg = {**DEFAULT_CFG, **(cfg or {})}
    q = FP.normalized(q0)
    c, res = evaluate(o, pb, q, cfg)
    cost0, mu, nacc, crossed = c, float(cfg["mu0"]), 0, 0
    dq = np.zeros(NV); A = g = None
    costs, margin, margins, zm = [], float(np.abs(res["depth"]).min()), {}, z_margin(res, pb, cfg)
    FS._fold(margins, res["margins"])
    clean = not pb["bad"] and bool(np.all(np.isfinite(q0)))
    status = 1.0 if not clean else 2.0 if res["behind"] else 0.0 if np.isfinite(c) else 1.0
    for it in range(int(cfg["n_iters"]) if status == 0 else 0):
        A, g, _, _ = normal_system(o, pb, q, mu, cfg)
        dq = np.linalg.solve(A, g)
        qt = FP.oplus(q, dq, *((jnt_range, jnt_limited) if cfg["clamp_limits"] else (None, None)))
        ct, rest = evaluate(o, pb, qt, cfg)
        margin = min(margin, float(np.abs(rest["depth"]).min()))
        zm = min(zm, z_margin(rest, pb, cfg))
        crossed += int(rest["behind"])
        FS._fold(margins, rest["margins"])
        if np.isfinite(ct) and ct < c:
            q, c, res = qt, ct, rest
            nacc += 1; mu = max(mu * cfg["mu_down"], cfg["mu_min"])
        else:
            mu = min(mu * cfg["mu_up"], cfg["mu_max"])
        costs.append(c)
    bad = status != 0
    ep, er = FP.errors(pb, res["e_pos"], res["e_rot"])
    fig, en = ([0.0] * 4, np.zeros(len(pb["body"]))) if bad else FT.point_figures(pb, res)
    sfig = [0.0] * 3 if bad else FS.scene_figures(res)
    ifig, uerr = ([0.0] * 4, np.zeros(pb["uv_on"].shape)) if bad else image_figures(pb, res)
    info = np.array([cost0, c, nacc, mu, ep, er, float(np.abs(dq).max()), status, *fig, *sfig, 0.0, *ifig])
    return dict(qpos=np.array(q0, np.float64) if bad else q, info=info, dq=dq, pt_err=en, uv_err=uerr, A=A, g=g, costs=costs, margin=margin, margins=margins,
                z_margin=zm, crossed=crossed)


# ---------------------------------------------------------------- cameras and the cases of the GPU tests (chosen in tests/test_fit_image_cpu.py)

ROWS = (1, 5, 67)
POINTS = (1, 24, 53)
CAMS = (1, 2, 3)
Z_MARGIN = 1e-3                # no weighted observation of a compared row comes this close to z_near at any pose the fp64 loop evaluates
PX_W = 1.0                     # w = 1 px^-2 at a 1000 px focal length
COMPARE_ITERS = 3
N_DISTINCT = 8                 # distinct rows of the comparisons; row e of a launch is row e % 8


def look_at(eye, target, f=1000.0, fy=None, cx=640.0, cy=360.0, up=(0.0, 0.0, 1.0), exact=False):
    """the 16 floats (fp32-representable; exact: as computed, R orthonormal to fp64) of a camera at eye looking at target, image x to the right, y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fw = target - eye; fw /= np.linalg.norm(fw)
    r = np.cross(fw, up); r /= np.linalg.norm(r)
    d = np.cross(fw, r)
    R = np.stack([r, d, fw])
    rec = np.concatenate([R.ravel(), -R @ eye, [f, f if fy is None else fy, cx, cy]])
    return rec if exact else f32(rec)


def ring(centre, n, dist=3.0, height=1.2, f=1000.0, start=0.0, step=90.0, cx=640.0, cy=360.0):
    """n cameras `step` degrees apart on a circle around centre, at `height`, looking at the point 0.9 m above centre's ground point"""
    c = np.asarray(centre, np.float64)
    tgt = np.array([c[0], c[1], 0.9])
    cams = []
    for i in range(n):
        a = np.radians(start + step * i)
        cams.append(look_at([c[0] + dist * np.cos(a), c[1] + dist * np.sin(a), height], tgt, f=f, fy=f * (1.0 if i % 2 == 0 else 1.1), cx=cx, cy=cy))
    return np.stack(cams)


def marker_choice(K):
    """(body, offset) of the GPU tests' marker sets: one point (the head), the 24 origins moved 3 cm, fit_points_oracle's 53"""
    if K == 1:
        return np.array([13], np.int32), f32(np.array([[0.0, 0.05, 0.1]]))
    if K == 24:
        return np.arange(NB, dtype=np.int32), f32(np.tile([0.03, 0.0, 0.0], (NB, 1)))
    return FT.marker_set(FT.counts_53(), FT.SEED_53)


def observe(o, q, body, off, cams):
    """uv [C, K, 2] (fp32-representable) of the markers of pose q, and their camera depths [C, K]"""
    p = FT.marker_positions(o, q, body, off)
    uv = np.zeros((len(cams), len(p), 2)); z = np.zeros((len(cams), len(p)))
    for c, cam in enumerate(cams):
        for k in range(len(p)):
            uv[c, k], _, _, z[c, k] = projection(np.asarray(cam, np.float64), p[k])
    return f32(uv), z


# Seeds of the compared rows (fit_pose_oracle.perturbed on the truth).  A row on which some weighted observation comes within Z_MARGIN of z_near in the
# fp64 loop, or on which the loop comes within section 21's margins of a discrete choice, is replaced by seed + 100 and listed here (none so far:
# the cameras stand 3 m away).  The truths are lifted LIFT above where they stand: as given, hull vertices of four of the first eight lie within
# VERTEX_MARGIN of the plane z = 0 at some evaluated pose (1.7e-6 m the nearest), which flips info 10 / 11 between fp32 and fp64 although the floor term
# is off on these rows; lifted, every row keeps section 21's vertex margin (tests/test_fit_image_cpu.py asserts it).
SEED0 = 700
SEED_OF = {}
LIFT = 0.5                     # 0.05 was tried first: truth 2 still brought a vertex within 4.2e-6 m of the plane at a trial pose
PT_W = 1.0                     # weight of the 3D targets the K = 24 rows carry beside their observations


def compare_rows(o, truths, K, C, f=1000.0, scale=0.5, cx=640.0, cy=360.0):
    """N_DISTINCT rows: truth i seen exactly by C cameras of the ring around its pelvis; init = the truth perturbed by `scale` x section 17's perturbation;
    all K points weighted PX_W, and with K == 1 the 24 origins as tgt_pos at weight 1 (one pixel pair does not fix a pose; the 2D and the 3D terms together).
    With K == 24 the rows carry the truth's markers as 3D targets too (pt_tgt, weight PT_W): the combination fit_takes.py --keypoints --tracks runs."""
    body, off = marker_choice(K)
    rows = []
    for i in range(N_DISTINCT):
        qt = FP.normalized(truths[i])
        qt[2] += LIFT
        qt = f32(qt); qt = FP.normalized(qt)
        cams = ring(qt[:3], C, f=f, start=30.0 * i, cx=cx, cy=cy)
        uv, z = observe(o, qt, body, off, cams)
        q0 = FP.oplus(qt, scale * _perturbation(SEED_OF.get(i, SEED0 + i)))
        xpos, _ = FP.fk(o, qt)
        rows.append(dict(name=f"truth{i}/K{K}/C{C}", q_true=qt, q0=f32(q0), cams=cams, uv=uv, z=z, tgt_pos=f32(xpos), w_pos=np.ones(NB)))
        if K == 24:
            rows[-1]["pt_tgt"] = f32(FT.marker_positions(o, qt, body, off))
            rows[-1]["pt_w"] = np.full(K, PT_W)
    return body, off, rows


def _perturbation(seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.2, 0.2, 3), rng.normal(size=NU) * 0.2])


def row_problem(kpm, body, off, r, uv_w=None, with_pelvis=None, **kw):
    pelvis = len(body) == 1 if with_pelvis is None else with_pelvis
    extra = dict(tgt_pos=r["tgt_pos"], w_pos=r["w_pos"]) if pelvis else {}
    if "pt_tgt" in r:
        extra.update(pt_tgt=r["pt_tgt"], pt_w=r["pt_w"])
    return problem(kpm, None, r["cams"], r["uv"], uv_w, pt_body=body, pt_offset=off, **extra, **kw)


# The (K, C) pairs the device is compared at, and the two camera configurations of the issue: weights 1 on normalised image coordinates (f = 1, principal
# point 0), and a 1000 px focal length with w = 1 px^-2.  The second one's damping is scaled with the problem: an observation's mass is w (f / z)^2, some
# 1e5 at 3 m, against 0.1 in the first; mu0 = 1e-2 under it would leave the weakly determined twists undamped (the fp64 loop then rejects its first steps).
COMPARE_SHAPES = ((1, 1), (24, 2), (53, 3))
CAMERA_CONFIGS = {"unit": dict(rows=dict(f=1.0, cx=0.0, cy=0.0), cfg=dict(mu0=1e-2)),
                  "px1000": dict(rows=dict(f=1000.0), cfg=dict(mu0=1e3, mu_min=1e-2, mu_max=1e11))}


def floor_rows(o, kpm, truths, which=(0, 1)):
    """The one-camera case with the floor term and the hinge prior, section 20's bound case seen by a camera: a pose standing ON the floor, moved
    FLOOR_DELTA down; the observations are the sunk pose's own (53 markers, one unit camera, w 1), the prior holds the hinges (weight 0.1), the init is the
    sunk pose.  'Translate up by delta' is feasible and costs only the reprojection error of that shift (cand_cost, below section 20's 1/2 24 delta^2),
    so 1/2 w_floor d_max^2 <= cand_cost gives section 20's bound a fortiori."""
    body, off = marker_choice(53)
    rows = []
    for i in which:
        q_on = FT.grounded(o, kpm, truths[i], 0.0)
        sunk = np.array(q_on); sunk[2] -= FT.FLOOR_DELTA
        sunk = f32(sunk)
        cams = ring(q_on[:3], 1, f=1.0, start=40.0 * i, cx=0.0, cy=0.0)
        uv, _ = observe(o, sunk, body, off, cams)
        cfg = dict(DEFAULT_CFG, n_iters=FT.FLOOR_ITERS, w_floor=FT.FLOOR_W)
        pb = problem(kpm, None, cams, uv, None, pt_body=body, pt_offset=off, q_prior=f32(q_on[7:]), w_prior=f32(np.full(NU, 0.1)))
        cand = evaluate(o, pb, q_on, cfg)[0]
        assert cand <= 0.5 * NB * FT.FLOOR_DELTA ** 2
        depth0 = -FT.lowest_vertex(o, kpm, sunk)
        rows.append(dict(name=f"floor/truth{i}", q0=sunk, cams=cams, uv=uv, q_prior=f32(q_on[7:]), w_prior=f32(np.full(NU, 0.1)), pb=pb, cfg=cfg, cand_cost=cand, depth0=depth0))
    return rows


# The floor rows compared with the device iteration by iteration, as section 20 compares its own: FLOOR_COMPARE_ITERS iterations at FLOOR_COMPARE_W, where
# the fp64 loop keeps every hull vertex VERTEX_MARGIN off the plane at every evaluated pose, so that the device holds the SAME active sets.  (Over the
# thirty iterations of floor_rows the sole's vertices settle micrometres around the plane -- 1.4e-6 m at the end -- which is why those rows are held to
# the derived bound and not to the reference's sets.)  Wanted were truths 0 .. 7; truth 1 comes within 9.9e-6 m and was replaced by truth 8.
FLOOR_COMPARE_TRUTHS = (0, 2, 3, 4, 5, 6, 7, 8)


def floor_compare_rows(o, kpm, truths):
    rows = floor_rows(o, kpm, truths, FLOOR_COMPARE_TRUTHS)
    for r in rows:
        r["cfg"] = dict(r["cfg"], n_iters=FT.FLOOR_COMPARE_ITERS, w_floor=FT.FLOOR_COMPARE_W)
        r["name"] += "/3it"
    return rows


CONVERGENCE_ITERS = 30


def convergence_rows(o, kpm, truths, which=(0, 2, 4, 5)):
    """two cameras 90 degrees apart (1000 px) observe a reachable pose exactly: 53 markers, init = the truth perturbed by half of section 17's perturbation"""
    body, off = marker_choice(53)
    rows = []
    for i in which:
        qt = FP.normalized(truths[i])
        cams = ring(qt[:3], 2, start=20.0 * i)
        uv, _ = observe(o, qt, body, off, cams)
        cfg = dict(DEFAULT_CFG, n_iters=CONVERGENCE_ITERS, **CAMERA_CONFIGS["px1000"]["cfg"])
        rows.append(dict(name=f"converge/truth{i}", q0=f32(FP.oplus(qt, 0.5 * _perturbation(900 + i))), cams=cams, uv=uv, cfg=cfg,
                         pb=problem(kpm, None, cams, uv, None, pt_body=body, pt_offset=off)))
    return rows


CROSS_Z_NEAR, CROSS_SHIFT = 2.5, 0.4


def crossing_row(o, kpm, truths):
    """One camera 3 m from the standing pose (its markers 2.70 .. 3.32 m deep) with z_near = 2.5 m: the observations are those of the pose moved 0.4 m
    towards the camera, where its nearest markers lie 2.30 m deep, in front of z_near.  The first trial goes most of the way and crosses; the accept rule rejects it.  q_behind: that pose itself, status 2."""
    body, off = marker_choice(53)
    qt = FP.normalized(truths[0])
    cams = ring(qt[:3], 1)
    R = cams[0][:9].reshape(3, 3)
    eye = -R.T @ cams[0][9:12]
    d = eye - qt[:3]; d[2] = 0.0; d /= np.linalg.norm(d)
    near = np.array(qt); near[:3] += CROSS_SHIFT * d
    near = f32(near)
    uv, z = observe(o, near, body, off, cams)
    assert z.min() < CROSS_Z_NEAR - 0.1 and observe(o, qt, body, off, cams)[1].min() > CROSS_Z_NEAR + 0.1
    cfg = dict(DEFAULT_CFG, **CAMERA_CONFIGS["px1000"]["cfg"])
    cfg.update(n_iters=6, z_near=CROSS_Z_NEAR, mu0=1.0)      # a first damping far below the observations' mass: the first step goes nearly all the way
    return dict(name="crossing", q0=f32(qt), q_behind=near, cams=cams, uv=uv, cfg=cfg, pb=problem(kpm, None, cams, uv, None, pt_body=body, pt_offset=off))
