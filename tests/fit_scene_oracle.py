"""fp64 reference of the pose fit that keeps the hulls out of the scene's static objects (kp_sim_fit_scene): test infrastructure.

fit_points_oracle's loop with one more term.  The row's geoms are built from the blob's obj_geoms table (18 floats per geom: object, type, size, pos,
mat) and the row's object poses by oracle.kpo.object_geoms -- the 17-float world records kp_sim_inverse_dynamics uses, at most MAXGEOM.  Per pair
(geom g in index order, hull b), after the cull sdf_g(xpos_b) - body_rbound[b] > 0:
    candidate planes (n, d)   box: (+-a_i, n.c + h_i) in the order +x -x +y -y +z -z; cylinder: the caps +-a_3, then, when the radial part of
                              xpos_b - c is longer than 1e-6, the tangent plane n = u, d = u.c + rho (u: unit radial direction towards xpos_b)
    D_f = max_v (d_f - n_f.x_v) over all vertices of the hull; some D_f <= 0: no term; otherwise f* = the first plane of least D_f
    footprint of f*           the primitive's extent in the directions other than n
    cost                      1/2 w_obj sum_{v in footprint} max(0, d - n.x_v)^2          (a vertex in two geoms' footprints counts in both: the SUM)
The gradient holds n fixed; the matrix counts every such vertex as an isotropic point mass w_obj; the solve is dense.
"""
import numpy as np

import fit_points_oracle as FT
import fit_pose_oracle as FP
import push_oracle as PO
from np_rigid import f32, oracle  # noqa: F401  (the tests reach them through this module)
from oracle.kpo import object_geoms

NV, NB, NU, NQ = FT.NV, FT.NB, FT.NU, FT.NQ
MAXGEOM = 8
DEFAULT_CFG = dict(FT.DEFAULT_CFG, w_obj=0.0)
BOX_FACES = ("+x", "-x", "+y", "-y", "+z", "-z")


def scene_geoms(kpm_obj, blk):
    """[n <= 8, 17] world records (type, size3, pos3, mat9, invweight) of the block's unparked objects; None or an all-parked block: none"""
    if blk is None:
        return np.zeros((0, 17))
    return object_geoms(kpm_obj, np.asarray(blk, np.float64))[:MAXGEOM]


def geom_sdf(g, x):
    """signed distance of world point x to a box (type 0) / z-axis cylinder (type 1) record"""
    R = g[7:16].reshape(3, 3)
    l = R.T @ (x - g[4:7])
    if g[0] == 0:
        q = np.abs(l) - g[1:4]
        return float(np.linalg.norm(np.maximum(q, 0.0)) + min(q.max(), 0.0))
    qr, qz = np.hypot(l[0], l[1]) - g[1], abs(l[2]) - g[2]
    return float(np.hypot(max(qr, 0.0), max(qz, 0.0)) + min(max(qr, qz), 0.0))


def candidate_planes(g, xb):
    """[(name, n_local, h, footprint)] of a geom for a body origin: depth of a local point l behind the plane = h - n_local.l; footprint: ("rect", t1, e1,
    t2, e2) or ("disc", rho), in the geom frame"""
    ex, ey, ez = np.eye(3)
    if g[0] == 0:
        hx, hy, hz = g[1:4]
        return [("+x", ex, hx, ("rect", ey, hy, ez, hz)), ("-x", -ex, hx, ("rect", ey, hy, ez, hz)), ("+y", ey, hy, ("rect", ex, hx, ez, hz)),
                ("-y", -ey, hy, ("rect", ex, hx, ez, hz)), ("+z", ez, hz, ("rect", ex, hx, ey, hy)), ("-z", -ez, hz, ("rect", ex, hx, ey, hy))]
    rho, h = g[1], g[2]
    out = [("+cap", ez, h, ("disc", rho)), ("-cap", -ez, h, ("disc", rho))]
    l = g[7:16].reshape(3, 3).T @ (xb - g[4:7])
    un = np.hypot(l[0], l[1])
    if un > 1e-6:
        u = np.array([l[0], l[1], 0.0]) / un
        out.append(("tangent", u, rho, ("rect", ez, h, np.cross(ez, u), rho)))
    return out


def footprint(fp, L):
    """(inside [n] bool, distance to the footprint's boundary [n]) of local points L [n, 3]"""
    if fp[0] == "disc":
        rr = np.hypot(L[:, 0], L[:, 1])
        return rr < fp[1], np.abs(rr - fp[1])
    _, t1, e1, t2, e2 = fp
    a, b = np.abs(L @ t1), np.abs(L @ t2)
    return (a < e1) & (b < e2), np.minimum(np.abs(a - e1), np.abs(b - e2))


def object_terms(pb, geoms, xpos, xquat, hp):
    """The pairs with a term at a pose, in the kernel's order (geom index, then body): [dict(g, b, face, n (world), idx (counted vertices, indices into
    the hull table), dep (their depths))], and the margins of the discrete choices: dict(cull: min |sdf - rbound|, sep: min |least D| over the pairs that
    passed the cull, runner: min (second least D - least D) over the pairs with a term, plane: min |depth| of a footprint vertex of a chosen plane,
    edge: min distance of a vertex behind a chosen plane to its footprint's boundary) -- inf where nothing was there to measure."""
    terms, m = [], dict(cull=np.inf, sep=np.inf, runner=np.inf, plane=np.inf, edge=np.inf)
    for gi, g in enumerate(geoms):
        R = g[7:16].reshape(3, 3)
        for b in range(NB):
            s = geom_sdf(g, xpos[b]) - pb["rbound"][b]
            m["cull"] = min(m["cull"], abs(s))
            if s > 0.0:
                continue
            idx = np.flatnonzero(pb["hb"] == b)
            L = (hp[idx] - g[4:7]) @ R                                  # R^T (x - c), row by row
            planes = candidate_planes(g, xpos[b])
            D = np.array([float((h - L @ n).max()) for _, n, h, _ in planes])
            m["sep"] = min(m["sep"], float(np.abs(D.min())))
            if D.min() <= 0.0:
                continue
            k = int(np.argmin(D))                                       # the first of the least
            m["runner"] = min(m["runner"], float(np.sort(D)[1] - D[k]))
            name, n, h, fp = planes[k]
            dep = h - L @ n
            inside, edge = footprint(fp, L)
            if inside.any():
                m["plane"] = min(m["plane"], float(np.abs(dep[inside]).min()))
            if (dep > 0.0).any():
                m["edge"] = min(m["edge"], float(edge[dep > 0.0].min()))
            cnt = inside & (dep > 0.0)
            terms.append(dict(g=gi, b=b, face=name, n=R @ n, idx=idx[cnt], dep=dep[cnt]))
    return terms, m


def problem(kpm, geoms=None, **kw):
    """fit_points_oracle.problem's row with its static geoms [n, 17] and the hull bounding radii"""
    pb = FT.problem(kpm, **kw)
    geoms = np.zeros((0, 17)) if geoms is None else np.asarray(geoms, np.float64).reshape(-1, 17)
    return dict(pb, geoms=geoms, rbound=np.asarray(kpm["body_rbound"], np.float64), bad=bool(pb["bad"] or not np.isfinite(geoms).all()))


def residuals(pb, xpos, xquat, cfg):
    res = FT.residuals(pb, xpos, xquat, cfg)
    res["terms"], res["margins"] = object_terms(pb, pb["geoms"], xpos, xquat, res["hp"])
    return res


def obj_cost(res, w):
    return 0.5 * float(w) * sum(float(t["dep"] @ t["dep"]) for t in res["terms"])


def cost_of(pb, q, res, cfg):
    return FT.cost_of(pb, q, res, cfg) + obj_cost(res, cfg["w_obj"])


def evaluate(o, pb, q, cfg):
    xpos, xquat = FP.fk(o, q)
    res = residuals(pb, xpos, xquat, cfg)
    return cost_of(pb, q, res, cfg), res


def normal_system(o, pb, q, mu, cfg):
    """fit_points_oracle.normal_system with the object term: isotropic blocks w_obj J_v^T J_v, gradient J_v^T w_obj dep n (n held fixed)"""
    A, g, H, _ = FT.normal_system(o, pb, q, mu, cfg)
    qn = FP.normalized(q)
    Jc, com, xpos, xquat = PO.body_jacobians(o, qn)
    res = residuals(pb, xpos, xquat, cfg)
    wo = float(cfg["w_obj"])
    Ho = np.zeros((NV, NV))
    if wo > 0.0:
        for t in res["terms"]:
            Jv = FT.point_jacobians(Jc, com, res["hp"][t["idx"]], pb["hb"][t["idx"]])
            for i in range(len(t["idx"])):
                Ho += wo * Jv[i].T @ Jv[i]
                g = g + wo * t["dep"][i] * (Jv[i].T @ t["n"])
    return A + Ho, g, H + Ho, res


def scene_figures(res):
    """info 12..14: the deepest counted vertex, the counted vertices, the pairs with a term"""
    deps = [t["dep"] for t in res["terms"] if len(t["dep"])]
    return [float(np.concatenate(deps).max()) if deps else 0.0, float(sum(len(t["dep"]) for t in res["terms"])), float(len(res["terms"]))]


def _fold(m, new):
    for k, v in new.items():
        m[k] = min(m.get(k, np.inf), v)


def lm(o, q0, pb, cfg=None, jnt_range=None, jnt_limited=None):
    """The kernel's loop in fp64.  Returns dict(qpos, info [16], dq, pt_err, A, g, costs, margin (the floor's, as fit_points_oracle.lm), margins: the
    smallest of object_terms' margins over every pose the loop evaluated, faces: the chosen planes at the result)."""
    cfg = {**DEFAULT_CFG, **(cfg or {})}
    q = FP.normalized(q0)
    c, res = evaluate(o, pb, q, cfg)
    cost0, mu, nacc = c, float(cfg["mu0"]), 0
    dq = np.zeros(NV); A = g = None
    costs, margin, margins = [], float(np.abs(res["depth"]).min()), {}
    _fold(margins, res["margins"])
    bad = pb["bad"] or not (np.isfinite(c) and np.all(np.isfinite(q0)))
    for it in range(0 if bad else int(cfg["n_iters"])):
        A, g, _, _ = normal_system(o, pb, q, mu, cfg)
        dq = np.linalg.solve(A, g)
        qt = FP.oplus(q, dq, *((jnt_range, jnt_limited) if cfg["clamp_limits"] else (None, None)))
        ct, rest = evaluate(o, pb, qt, cfg)
        margin = min(margin, float(np.abs(rest["depth"]).min()))
        _fold(margins, rest["margins"])
        if np.isfinite(ct) and ct < c:
            q, c, res = qt, ct, rest
            nacc += 1; mu = max(mu * cfg["mu_down"], cfg["mu_min"])
        else:
            mu = min(mu * cfg["mu_up"], cfg["mu_max"])
        costs.append(c)
    ep, er = FP.errors(pb, res["e_pos"], res["e_rot"])
    fig, en = ([0.0] * 4, np.zeros(len(pb["body"]))) if bad else FT.point_figures(pb, res)
    sfig = [0.0] * 3 if bad else scene_figures(res)
    info = np.array([cost0, c, nacc, mu, ep, er, float(np.abs(dq).max()), 1.0 if bad else 0.0, *fig, *sfig, 0.0])
    return dict(qpos=np.array(q0, np.float64) if bad else q, info=info, dq=dq, pt_err=en, A=A, g=g, costs=costs, margin=margin, margins=margins,
                faces=[(t["g"], t["b"], t["face"]) for t in res["terms"]])


# ---------------------------------------------------------------- the cases of the GPU tests (chosen in tests/test_fit_scene_cpu.py)

ROWS = (1, 5, 67)
OBJ_DELTA, OBJ_W, FLOOR_W = 0.03, 2400.0, 2400.0
OBJ_BOUND = OBJ_DELTA * np.sqrt(NB / OBJ_W)        # 3 mm: 1/2 w_obj d_max^2 <= 1/2 24 w_pos delta^2, FLOOR_BOUND's arithmetic
OBJ_ITERS = 30
COMPARE_ITERS, COMPARE_W, PARITY_W = 3, 4.0, 1.0
PEN_MARGIN = 0.003
# margins the discrete choices keep in the fp64 loop on every compared case: runner-up plane, and a vertex against a chosen plane / a footprint boundary
RUNNER_MARGIN, VERTEX_MARGIN = 1e-4, 1e-5
CHAIR, BOX, TABLE, CAN, STEP = 0, 1, 2, 3, 4      # the objects of the step blob, in its order


def parked_block():
    blk = np.zeros(35)
    for i in range(5):
        blk[7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    blk[3::7] = 1.0
    return blk


def block(**poses):
    """an object block with the named objects placed: block(chair=[x, y, z, qw, qx, qy, qz])"""
    blk = parked_block()
    for name, pose in poses.items():
        oi = dict(chair=CHAIR, box=BOX, table=TABLE, can=CAN, step=STEP)[name]
        blk[7 * oi: 7 * oi + 7] = pose
    return f32(blk)


def hull_points(o, kpm, q):
    hv, hb = FT.hull_table(kpm)
    xpos, xquat = FP.fk(o, q)
    return FT.world_points(xpos, xquat, hb, hv), hb, xpos


def pushed_case(o, q_free, blk, direction, delta=OBJ_DELTA):
    """The bound's case: q_free is a feasible pose (touching or clear of the objects); targets = its 24 origins moved delta along `direction` (a unit
    vector INTO the surface), w_pos 1; init = the pose translated with them.  'Translate back by delta' is feasible and costs 1/2 24 delta^2."""
    d = np.asarray(direction, np.float64) * delta
    xpos, _ = FP.fk(o, q_free)
    q0 = np.array(q_free, np.float64); q0[:3] += d
    return dict(q_free=f32(q_free), q0=f32(q0), tgt_pos=f32(xpos + d), blk=f32(blk), cand_cost=0.5 * NB * delta ** 2)


def touching(o, kpm, q, n, d, bodies=None):
    """q translated along the unit normal n until its lowest hull vertex (of `bodies`, default all) against the plane n.x = d sits ON the plane"""
    hp, hb, _ = hull_points(o, kpm, q)
    sel = np.ones(len(hb), bool) if bodies is None else np.isin(hb, bodies)
    q = np.array(q, np.float64)
    q[:3] += (d - float((hp[sel] @ n).min())) * np.asarray(n, np.float64)
    return f32(q)


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    return [float(np.cos(angle / 2)), *(np.sin(angle / 2) * a / np.linalg.norm(a))]


STEP_TOP = 0.14      # height of the step box's top face in the step cases (its origin lies 0.03 above the top)


def scene_cases(o, kpm, named):
    """name -> pushed_case dict (+ bodies: the hulls of the contact, walk: a face-type contact the pose-contact walk is asserted on) of the bound cases:
      step       a_standing on the step box, pushed 30 mm down into its top
      step_yaw   the same with the box turned 0.4 rad about z (quaternion not identity)
      sit        g_sit on the chair as the named states have it (hands and pelvis inside the chair to begin with), pushed 30 mm into the seat
      sit_moved  the same with the chair moved 0.1 m
      sit_open   g_sit with the arms spread (clear of the chair), pushed 30 mm into the seat
      can        a_standing beside the Can, pushed 30 mm towards its axis: a cylinder's tangent plane
      can_top    a_standing on the Can's top cap, pushed 30 mm down: a cylinder's cap
      slab_tilt  a_standing on the table's 2 cm top tilted 0.15 rad about x, pushed 30 mm along the top's inward normal"""
    by = {s["name"]: s for s in named}
    stand, sit = np.array(by["a_standing"]["q"], np.float64), by["g_sit"]
    og = np.asarray(kpm["obj_geoms"], np.float64).reshape(-1, 18)
    up, out = np.array([0.0, 0.0, 1.0]), {}
    for name, quat in (("step", [1.0, 0.0, 0.0, 0.0]), ("step_yaw", _quat(up, 0.4))):
        q = touching(o, kpm, stand, up, STEP_TOP)
        x = FP.fk(o, q)[0][0]
        out[name] = dict(pushed_case(o, q, block(step=[x[0], x[1], STEP_TOP + 0.03, *quat]), -up), walk=True)
    seat_top = float(sit["blk"][2]) + 0.02
    q = touching(o, kpm, sit["q"], up, seat_top, (0, 1, 5))
    out["sit"] = dict(pushed_case(o, q, sit["blk"], -up), walk=False)
    moved = np.array(sit["blk"], np.float64); moved[1] += 0.1
    out["sit_moved"] = dict(pushed_case(o, q, moved, -up), walk=False)
    qo = np.array(sit["q"], np.float64)
    for j in (14, 19):
        qo[7 + 3 * j: 10 + 3 * j] = [0.0, 0.0, np.pi / 2]
    out["sit_open"] = dict(pushed_case(o, touching(o, kpm, qo, up, seat_top, (0, 1, 5)), sit["blk"], -up), walk=False)
    # the Can's axis at the distance along +x at which the nearest hull vertex inside its height touches the wall
    g = og[8]
    rho, top = float(g[2]), 0.55
    lifted = np.array(stand); lifted[2] += 0.02        # as given a sole vertex of a_standing lies 9e-6 m from the floor plane: an edge of the floor term
    hp, hb, xpos = hull_points(o, kpm, lifted)
    sel = (hp[:, 2] < top) & (hp[:, 2] > top - 2 * float(g[3]))
    lo, hi = 0.0, 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if np.hypot(hp[sel, 0] - (xpos[0, 0] + mid), hp[sel, 1] - xpos[0, 1]).min() < rho:
            lo = mid
        else:
            hi = mid
    axis = np.array([xpos[0, 0] + hi, xpos[0, 1]])
    vmin = np.flatnonzero(sel)[np.argmin(np.hypot(*(hp[sel, :2] - axis).T))]
    u = xpos[hb[vmin], :2] - axis                      # the push runs along the tangent plane's normal of the hull that touches, towards the axis
    u /= np.linalg.norm(u)
    out["can"] = dict(pushed_case(o, lifted, block(can=[axis[0] - g[5], axis[1] - g[6], top, 1.0, 0.0, 0.0, 0.0]), [-u[0], -u[1], 0.0]), walk=False)
    # standing on the Can's top cap (the cap is the Can's origin plane)
    q = touching(o, kpm, stand, up, STEP_TOP)
    x = FP.fk(o, q)[0][0]
    out["can_top"] = dict(pushed_case(o, q, block(can=[x[0] - g[5], x[1] - g[6], STEP_TOP, 1.0, 0.0, 0.0, 0.0]), -up), walk=True)
    # the table: its top box is geom 3 (centre 0.1 below the origin, 1 cm half thickness)
    tilt = 0.15
    n = np.array([0.0, -np.sin(tilt), np.cos(tilt)])
    x = FP.fk(o, stand)[0][0]
    origin = np.array([x[0], x[1], STEP_TOP + 0.09])
    d = float(n @ origin) - 0.1 + 0.01                 # the top face: the centre moves with the tilt, 0.1 along -n from the origin
    out["slab_tilt"] = dict(pushed_case(o, touching(o, kpm, stand, n, d), block(table=[*origin, *_quat([1.0, 0.0, 0.0], tilt)]), -n), walk=True)
    return out


def compare_row(name, c, frac):
    """case c pushed frac * OBJ_DELTA instead of OBJ_DELTA: its init and targets moved back along the push"""
    back = (1.0 - frac) * (np.asarray(c["q0"], np.float64)[:3] - np.asarray(c["q_free"], np.float64)[:3])
    q0 = np.array(c["q0"], np.float64); q0[:3] -= back
    return dict(name=f"{name}@{frac:.2f}", q0=f32(q0), tgt_pos=f32(np.asarray(c["tgt_pos"], np.float64) - back), blk=c["blk"])


# The push fractions of the rows compared with the device iteration by iteration, two per case.  Wanted were 1.00 and 0.67 for every case; a fraction at
# which the fp64 loop comes within RUNNER_MARGIN / VERTEX_MARGIN of a discrete choice at some evaluated pose (tests/test_fit_scene_cpu.py asserts it) was
# replaced by the next one 0.01 below that keeps the margins.
COMPARE_FRACS = {"step": (0.99, 0.65), "step_yaw": (0.99, 0.65), "sit": (1.00, 0.66), "sit_moved": (0.99, 0.66), "sit_open": (1.00, 0.67), "can": (1.00, 0.66),
                 "can_top": (0.99, 0.65), "slab_tilt": (0.90, 0.67)}      # replaced: step / step_yaw / can_top 1.00, 0.67, 0.66; sit, can 0.67; sit_moved 1.00, 0.67; slab_tilt 1.00 .. 0.91


def compare_rows(cases):
    """the 16 distinct rows of the comparisons with the device; row e of a launch is row e % 16"""
    return [compare_row(name, cases[name], COMPARE_FRACS[name][k]) for k in (0, 1) for name in cases]


def compare_configs():
    """the configurations the device is compared at on the compared rows: three iterations at COMPARE_W; one step at PARITY_W (reported beside
    step_rows' figure)"""
    return (dict(n_iters=COMPARE_ITERS, w_obj=COMPARE_W, w_floor=COMPARE_W), dict(n_iters=1, mu0=1e-2, w_obj=PARITY_W, w_floor=PARITY_W))


def margins_hold(r):
    """the fp64 loop r kept every discrete choice clear: (ok, the margins with the floor's among them)"""
    m = dict(r["margins"], floor=r["margin"])
    return m["runner"] >= RUNNER_MARGIN and all(m[k] >= VERTEX_MARGIN for k in ("cull", "sep", "plane", "edge", "floor")), m


# The rows of the one-step comparison: the compared rows with section 20's init on top -- fit_pose_oracle.perturbed (N(0, 0.2 rad) on the hinges, +-0.1 m
# and +-0.2 rad on the root), seed STEP_SEED0 + row.  Section 20's cap on |dq - dq_ref| / |dq_ref| was taken on such inits, whose step is some 0.3 in
# the inf-norm; the compared rows themselves are a pure translation of 0.02 .. 0.03 m, a step ten times smaller against the same absolute error
# cond(A) eta |dq| leaves in the weakly determined twist dofs (DESIGN.md section 21 has both figures).  A seed at which the fp64 step comes within the
# margins of a discrete choice is replaced by seed + 16 (STEP_SEED_OF; tests/test_fit_scene_cpu.py asserts the margins).
STEP_SEED0 = 200
STEP_SEED_OF = {1: 217, 3: 219, 4: 220, 6: 286, 7: 271, 9: 257, 13: 229, 14: 278, 15: 231}      # also replaced: a seed whose init has fewer than 3 counted vertices


def step_rows(cases):
    rows = []
    for i, r in enumerate(compare_rows(cases)):
        rows.append(dict(r, name=r["name"] + "+p", q0=f32(FP.perturbed(np.asarray(r["q0"], np.float64), STEP_SEED_OF.get(i, STEP_SEED0 + i)))))
    return rows


def step_configs():
    """the one-step configurations: PARITY_W (held to the dq cap and to the reference's discrete choices) and OBJ_W (held to the backward error)"""
    return (dict(n_iters=1, mu0=1e-2, w_obj=PARITY_W, w_floor=PARITY_W), dict(n_iters=1, mu0=1e-2, w_obj=OBJ_W, w_floor=OBJ_W))
