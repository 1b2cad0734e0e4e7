"""Seeded scenes for the narrow phases under arbitrary object orientation (tests/test_collide_cases_cpu.py, tests/test_gpu_collide_sweep.py): host-only
numpy on the fp64 oracle, test infrastructure.

A scene is a dict(name, family, q [76], blk [35], slots (object indices of the dynamic route, ascending model order, at most MAXOBJ), routes (subset of
"dyn", "static", "pose"), tags, ...).  Every value of q and blk is rounded to fp32 before anything is computed from it, so the device and the oracle read
identical inputs.  Objects are the ones compiled into the step model: chair (2 boxes), box, table (slab + 4 cylinder legs), Can (cylinder), step (box).

Pairs "in contact" at random orientation are placed by bisection of the distance along a direction on the oracle's own single-pair narrow phase, until the
pair's smallest dist meets a seeded target in [-0.01, +0.0009] (the contact margin is 0.001).

conditioning() measures, on the oracle alone, how much a scene's contact list moves when every pose component of the objects and of the root moves by one
fp32 ulp (four seeded sign patterns): per reference contact the largest change of dist / pos / normal (the spread), and whether the set changed."""
from __future__ import annotations

import os

import numpy as np

from kinpoly_amd.model_compiler import STEP_KPM, read_kpm
from oracle import np_oracle as O
from oracle.kpo import OracleSim, narrowphase, object_geoms, shape_record

MARGIN = 0.001
MAXOBJ, MAXGEOM = 2, 8                    # oracle/kp_oracle.c; D_MAXOBJ, D_MAXGEOM on the device
CHAIR, BOX, TABLE, CAN, STEP = range(5)
KPM = read_kpm(STEP_KPM)
OG = KPM["obj_geoms"].reshape(-1, 18)      # object, type (0 box, 1 cylinder), size [3], pos [3], R [9], mass
STD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "standing_neutral.npz"))["qpos"].astype(np.float64)
GEOMS_OF = {oi: [g for g in range(len(OG)) if int(OG[g, 0]) == oi] for oi in range(5)}
SLAB, LEGS, CAN_GEOM = GEOMS_OF[TABLE][0], GEOMS_OF[TABLE][1:], GEOMS_OF[CAN][0]
AIR = np.array([STD[0] + 2.0, STD[1], 1.5])       # where the object - object pairs hang; the humanoid of those scenes stands 3 m up


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------- quaternions (w, x, y, z) and placed geoms

def qmat(q):
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def qaxis(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])


def qyaw(ang):
    return qaxis([0, 0, 1], ang)


def qrand(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def qalign(u, t):
    """the shortest rotation taking the unit vector u to the unit vector t"""
    c = float(np.dot(u, t))
    q = np.concatenate([[1.0 + c], np.cross(u, t)])
    return q / np.linalg.norm(q)


def horizontal(rng):
    a = rng.uniform(0, 2 * np.pi)
    return np.array([np.cos(a), np.sin(a), 0.0])


def placed(oi, pose7):
    """the world-frame geoms of object oi at pose7 (fp64 on the given values): list of dict(gi, type, size, pos, mat)"""
    pose7 = np.asarray(pose7, float)
    R = qmat(pose7[3:7])
    return [dict(gi=g, type=int(OG[g, 1]), size=OG[g, 2:5].copy(), pos=pose7[:3] + R @ OG[g, 5:8], mat=R @ OG[g, 8:17].reshape(3, 3)) for g in GEOMS_OF[oi]]


def shape(g):
    return shape_record("cylinder" if g["type"] else "box", size=g["size"], pos=g["pos"], mat=g["mat"])


def lowest(oi, pose7):
    """(lowest z, type of the geom it belongs to) of the object"""
    best = (np.inf, -1)
    for g in placed(oi, pose7):
        if g["type"] == 0:
            z = g["pos"][2] - np.abs(g["mat"][2] * g["size"]).sum()
        else:
            az = g["mat"][2, 2]
            z = g["pos"][2] - abs(az) * g["size"][1] - g["size"][0] * np.sqrt(max(0.0, 1.0 - az * az))
        if z < best[0]:
            best = (z, g["type"])
    return best


def pair_rows(ga, gb, margin=MARGIN):
    """narrow phase of two placed geoms as the scene runs it: geom 1 = the lower type (cylinder < box), then the earlier geom (ga).
    Returns (kind, rows [n, 7])"""
    if ga["type"] == 0 and gb["type"] == 0:
        return "box-box", narrowphase("box_box", a=shape(ga), b=shape(gb), margin=margin)
    a_first = not (ga["type"] == 0 and gb["type"] != 0)
    g1, g2 = (ga, gb) if a_first else (gb, ga)
    return ("cyl-cyl" if g2["type"] else "cyl-box"), narrowphase("convex", a=shape(g1), b=shape(g2), margin=margin)


def floor_rows(g, margin=MARGIN):
    return ("floor-cyl", narrowphase("plane_cylinder", a=shape(g), margin=margin)) if g["type"] else ("floor-box", narrowphase("plane_box", a=shape(g), margin=margin))


_FK = {}


def fk(q):
    key = np.asarray(q, np.float64).tobytes()
    if key not in _FK:
        _FK[key] = O.qpos_fk(np.asarray(q, np.float64), KPM["body_pos"].reshape(24, 3), KPM["body_ipos"].reshape(24, 3), KPM["body_parent"])
    return _FK[key]


def hull_parts(q, b):
    """(body origin, R, body-frame vertices, world vertices) of hull b at qpos q"""
    f = fk(q)
    R = O.quaternion_matrix3(f["wbquat"][b])
    vb = KPM["verts"].reshape(-1, 3)[KPM["vert_adr"][b]:KPM["vert_adr"][b + 1]]
    return f["wbpos"][b], R, vb, f["wbpos"][b] + vb @ R.T


def hull_rows(q, b, g, margin=MARGIN):
    """narrow phase of a placed geom (geom 1) and hull b (geom 2)"""
    xb, R, vb, _ = hull_parts(q, b)
    hull = shape_record("hull", pos=xb, mat=R, center=xb + R @ KPM["body_ipos"].reshape(24, 3)[b])
    return ("hull-cyl" if g["type"] else "hull-box"), narrowphase("convex", a=shape(g), b=hull, verts_b=vb, margin=margin)


# ---------------------------------------------------------------- scenes

def parked():
    blk = np.zeros(35)
    for i in range(5):
        blk[7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    blk[3::7] = 1.0
    return blk


def active(blk):
    return [oi for oi in range(5) if not np.linalg.norm(blk[7 * oi: 7 * oi + 3]) > 50.0]


def far_humanoid():
    q = STD.copy()
    q[2] += 3.0
    return q


def scene(name, family, q, poses, routes, tags=(), **extra):
    """poses: {object index: pose7}; everything rounded to fp32 here"""
    blk = parked()
    for oi, p in poses.items():
        blk[7 * oi: 7 * oi + 7] = p
    blk = f32(blk)
    return dict(name=name, family=family, q=f32(q), blk=blk, slots=tuple(active(blk)[:MAXOBJ]), routes=tuple(routes), tags=set(tags), **extra)


def object_pairs(sc):
    """[(kind, rows)] of every geom pair the dynamic route of the scene runs, humanoid excluded: each dynamic geom against the floor and against the
    geoms of the higher slots"""
    out = []
    geoms = [placed(oi, sc["blk"][7 * oi: 7 * oi + 7]) for oi in sc["slots"]]
    for k, ga_list in enumerate(geoms):
        for ga in ga_list:
            out.append(floor_rows(ga))
            for gb_list in geoms[k + 1:]:
                for gb in gb_list:
                    out.append(pair_rows(ga, gb))
    return out


def bisect(dist_fn, lo, hi, target, steps=40):
    """the largest t found in [lo, hi] with dist_fn(t) <= target, given dist_fn(lo) <= target < dist_fn(hi); dist_fn returns inf when nothing is within the margin"""
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if dist_fn(mid) > target:
            hi = mid
        else:
            lo = mid
    return lo


def min_dist(rows_list):
    return min([r[:, 0].min() for r in rows_list if len(r)], default=np.inf)


def on_floor(oi, quat, depth, xy=(0.0, 0.0)):
    """pose7 of object oi with its lowest point `depth` below the floor; (pose, type of the lowest geom)"""
    quat = f32(quat)
    pose = np.array([STD[0] + xy[0], STD[1] + xy[1], 0.0, *quat])
    z, typ = lowest(oi, pose)
    pose[2] = -z - depth
    return f32(pose), typ


def approach(rng, a, qa, b, qb, direction, target, ga_set=None, gb_set=None, lateral=(0.0, 0.0, 0.0)):
    """object a fixed at AIR with quaternion qa; object b with quaternion qb moved along `direction` from a's (first targeted) geom centre until the smallest
    dist over the targeted geom pairs meets `target`.  Returns (pose_a, pose_b) or None when the bisection did not land on the target."""
    qa, qb = f32(qa), f32(qb)
    pose_a = f32(np.concatenate([AIR, qa]))
    A = [g for g in placed(a, pose_a) if ga_set is None or g["gi"] in ga_set]
    gb0 = [g for g in GEOMS_OF[b] if gb_set is None or g in gb_set][0]
    off = qmat(qb) @ OG[gb0, 5:8]
    direction = np.asarray(direction, float) / np.linalg.norm(direction)

    def pose_b(t):
        return f32(np.concatenate([A[0]["pos"] + np.asarray(lateral) + t * direction - off, qb]))

    def dist(t):
        B = [g for g in placed(b, pose_b(t)) if gb_set is None or g["gi"] in gb_set]
        return min_dist([pair_rows(x, y)[1] if a < b else pair_rows(y, x)[1] for x in A for y in B])

    t = bisect(dist, 0.0, 3.0, target)
    if abs(dist(t) - target) > 2e-6:
        return None
    return pose_a, pose_b(t)


def _retry(rng, build, tries=60):
    """the first scene of build(rng) that exists and whose object pairs do not sink into each other by more than 2 cm"""
    for _ in range(tries):
        sc = build(rng)
        if sc is not None and min_dist([r for _, r in object_pairs(sc)] if sc["family"] in ("F3", "F4") else []) > -0.02:
            return sc
    raise RuntimeError("no admissible scene in %d tries" % tries)


def family_f1(seed=101):
    """object - floor, boxes: box, step, chair and the table's slab, at random orientation and exactly on a face, an edge and a corner"""
    rng = np.random.default_rng(seed)
    out = []
    for oi in (BOX, STEP, CHAIR, TABLE):
        flip = qaxis([1, 0, 0], np.pi)
        base = flip if oi == TABLE else np.array([1.0, 0, 0, 0])
        g0 = OG[GEOMS_OF[oi][0]]
        for k in range(10):
            xy = rng.uniform(-0.3, 0.3, 2)
            if k < 6 or (k == 9 and oi == TABLE):
                kind = "random"
                for _ in range(200):
                    pose, typ = on_floor(oi, qrand(rng), rng.uniform(-0.002, 0.01), xy)
                    if typ == 0:
                        break
            elif k < 8:
                kind = "face"
                b = base if (k == 6 or oi in (CHAIR, TABLE)) else flip
                pose, typ = on_floor(oi, qmul(qyaw(rng.uniform(0, 2 * np.pi)), b), rng.uniform(0.0, 0.01), xy)
            elif k == 8:
                kind = "edge"
                pose, typ = on_floor(oi, qmul(qyaw(rng.uniform(0, 2 * np.pi)), qmul(qaxis([1, 0, 0], rng.uniform(0.3, 0.6)), base)), rng.uniform(0.0, 0.01), xy)
            else:
                kind = "corner"
                u = g0[8:17].reshape(3, 3) @ (-g0[2:5] / np.linalg.norm(g0[2:5]))
                pose, typ = on_floor(oi, qmul(qyaw(rng.uniform(0, 2 * np.pi)), qalign(u, np.array([0, 0, -1.0]))), rng.uniform(0.0005, 0.004), xy)
            assert typ == 0 or (oi == TABLE and kind == "face"), (oi, kind, k)      # upside down, the table's leg caps lie flush with its slab: both touch
            out.append(scene(f"F1/{oi}/{kind}/{k}", "F1", far_humanoid(), {oi: pose}, ("dyn",), (kind,)))
    return out


def family_f2(seed=202):
    """object - floor, cylinders: the Can and the table's legs"""
    rng = np.random.default_rng(seed)
    out = []
    up = np.array([1.0, 0, 0, 0])

    def add(oi, kind, quat, depth):
        pose, _ = on_floor(oi, quat, depth, rng.uniform(-0.3, 0.3, 2))
        out.append(scene(f"F2/{oi}/{kind}/{len(out)}", "F2", far_humanoid(), {oi: pose}, ("dyn",), (kind,)))

    d = lambda: rng.uniform(-0.0005, 0.01)      # noqa: E731
    for oi in (CAN, TABLE):
        for _ in range(6 if oi == CAN else 5):
            for _ in range(200):
                q = qrand(rng)
                if oi == CAN or lowest(oi, np.array([0, 0, 0, *f32(q)]))[1] == 1:
                    break
            add(oi, "random", q, rng.uniform(-0.002, 0.01))
        add(oi, "upright", up, d())
        add(oi, "yaw", qyaw(rng.uniform(0, 2 * np.pi)), d())
        if oi == CAN:
            add(oi, "yaw", qyaw(rng.uniform(0, 2 * np.pi)), d())
        for tilt in (0.02, 0.1, 0.5, 1.2):
            add(oi, f"tilt{tilt}", qmul(qyaw(rng.uniform(0, 2 * np.pi)), qaxis(horizontal(rng), tilt)), d())
    for _ in range(2):           # upside down: the axis points up, the flip is taken
        add(CAN, "upside-down", qmul(qyaw(rng.uniform(0, 2 * np.pi)), qaxis(horizontal(rng), np.pi)), d())
    add(CAN, "upside-down", qaxis([1, 0, 0], np.pi), d())
    for tilt in (0.02, 0.1, 0.5, 1.2):
        add(CAN, f"upside-down-tilt{tilt}", qmul(qaxis(horizontal(rng), tilt), qaxis(horizontal(rng), np.pi)), d())
    for _ in range(3):           # lying at exactly pi / 2
        add(CAN, "lying", qmul(qyaw(rng.uniform(0, 2 * np.pi)), qaxis(horizontal(rng), np.pi / 2)), d())
    # the table on its long side, 0.05 rad short of lying and pressed 10 cm into the floor: its two lower legs lie in the floor with both caps inside the margin
    # and deeper than 1.5 radii, the four-contact branch.  (At exactly pi / 2 and that deep the reference itself is not comparable: the sign of the axis'
    # vertical component decides at which end the two extra contacts sit.)
    for s in (1.0, -1.0):
        add(TABLE, "lying-deep", qmul(qyaw(rng.uniform(0, 2 * np.pi)), qaxis([1, 0, 0], s * (np.pi / 2 - 0.05))), rng.uniform(0.10, 0.11))
    add(TABLE, "upside-down", qmul(qyaw(rng.uniform(0, 2 * np.pi)), qaxis([1, 0, 0], np.pi)), d())
    return out


def _target(rng):
    return rng.uniform(-0.01, 0.0009)


def family_f3(seed=303):
    """object - object, box - box: box - slab, box - step, box - chair, step - chair as two dynamic objects in the air"""
    rng = np.random.default_rng(seed)
    out = []
    box_geoms = {BOX: None, STEP: None, CHAIR: None, TABLE: {SLAB}}
    for a, b in ((BOX, TABLE), (BOX, STEP), (CHAIR, BOX), (CHAIR, STEP)):
        for k in range(5):
            fixed, moved = (a, b) if k % 2 == 0 else (b, a)          # which of the two is approached changes which one's face gets hit

            def build(rng, fixed=fixed, moved=moved, k=k):
                d = rng.normal(size=3)
                p = approach(rng, fixed, qrand(rng), moved, qrand(rng), d, _target(rng), box_geoms[fixed], box_geoms[moved])
                return None if p is None else scene(f"F3/{fixed}-{moved}/random/{k}", "F3", far_humanoid(), {fixed: p[0], moved: p[1]}, ("dyn",), ("random",))
            out.append(_retry(rng, build))
    # the box on the slab with its own tilt; then with the slab tilted too
    for k in range(6):
        def build(rng, k=k):
            qt = qmul(qaxis(horizontal(rng), rng.uniform(0.1, 0.5)), qyaw(rng.uniform(0, 2 * np.pi))) if k >= 3 else qyaw(rng.uniform(0, 2 * np.pi))
            qb = qmul(qt, qaxis(horizontal(rng), rng.uniform(0.05, 0.5)))
            p = approach(rng, TABLE, qt, BOX, qb, qmat(f32(qt))[:, 2], _target(rng), {SLAB}, None)
            return None if p is None else scene(f"F3/box-on-slab/{'both-tilted' if k >= 3 else 'tilted'}/{k}", "F3", far_humanoid(), {TABLE: p[0], BOX: p[1]}, ("dyn",), ("tilted",))
        out.append(_retry(rng, build))
    # face on face at relative yaws 0, exactly pi / 2, 0.3 and pi / 4, both index orders (upper object in the lower or the higher slot)
    for lower, upper in ((TABLE, BOX), (BOX, STEP), (STEP, BOX)):
        for yaw in (0.0, np.pi / 2, 0.3, np.pi / 4):
            def build(rng, lower=lower, upper=upper, yaw=yaw):
                q0 = qyaw(rng.uniform(0, 2 * np.pi)) if rng.uniform() < 0.5 else np.array([1.0, 0, 0, 0])
                lat = np.concatenate([rng.uniform(-0.02, 0.02, 2), [0.0]])
                p = approach(rng, lower, q0, upper, qmul(q0, qyaw(yaw)), [0, 0, 1], rng.uniform(-0.005, 0.0009), {SLAB} if lower == TABLE else None, None, lat)
                return None if p is None else scene(f"F3/{upper}-on-{lower}/yaw{yaw:.3f}", "F3", far_humanoid(), {lower: p[0], upper: p[1]}, ("dyn",), ("face",))
            out.append(_retry(rng, build))
    return out


def family_f4(seed=404):
    """object - object through the convex query: Can - step, Can - box, table leg - box (cylinder - box), Can - table leg (cylinder - cylinder)"""
    rng = np.random.default_rng(seed)
    out = []
    sets = {CAN: None, STEP: None, BOX: None, TABLE: set(LEGS)}
    for a, b in ((CAN, STEP), (BOX, CAN), (BOX, TABLE), (TABLE, CAN)):
        for k in range(8):
            fixed, moved = (a, b) if k % 2 == 0 else (b, a)

            def build(rng, fixed=fixed, moved=moved, k=k):
                fs = {LEGS[rng.integers(4)]} if fixed == TABLE else sets[fixed]
                ms = {LEGS[rng.integers(4)]} if moved == TABLE else sets[moved]
                p = approach(rng, fixed, qrand(rng), moved, qrand(rng), rng.normal(size=3), _target(rng), fs, ms)
                return None if p is None else scene(f"F4/{fixed}-{moved}/random/{k}", "F4", far_humanoid(), {fixed: p[0], moved: p[1]}, ("dyn",), ("random",))
            out.append(_retry(rng, build))
    for k in range(3):           # the Can standing on the step
        def build(rng, k=k):
            q0 = qyaw(rng.uniform(0, 2 * np.pi)) if k else np.array([1.0, 0, 0, 0])
            lat = np.concatenate([rng.uniform(-0.05, 0.05, 2), [0.0]])
            p = approach(rng, STEP, q0, CAN, qmul(q0, qyaw(rng.uniform(0, 2 * np.pi))), [0, 0, 1], rng.uniform(-0.005, 0.0009), None, None, lat)
            return None if p is None else scene(f"F4/can-standing-on-step/{k}", "F4", far_humanoid(), {STEP: p[0], CAN: p[1]}, ("dyn",), ("standing",))
        out.append(_retry(rng, build))
    # the Can lying against a side face of the box: a line contact, which the conditioning measure flags (the query's single point may sit anywhere along the
    # line: 0.2 m of spread in pos under a one-ulp change); it is the family's one such scene, its contact set is still compared
    def build(rng):
        q0 = qyaw(rng.uniform(0, 2 * np.pi))
        p = approach(rng, BOX, q0, CAN, qmul(q0, qaxis([1, 0, 0], np.pi / 2)), qmat(f32(q0))[:, 0], rng.uniform(-0.005, 0.0009))
        return None if p is None else scene("F4/can-lying-against-box", "F4", far_humanoid(), {BOX: p[0], CAN: p[1]}, ("dyn",), ("lying",))
    out.append(_retry(rng, build))
    return out


def humanoid(rng):
    q = STD.copy()
    q[7:] += rng.normal(size=69) * 0.3
    q[2] += 0.3
    return f32(q)


def surface_point(rng, g):
    """(point, outward unit normal) on a random face of a box geom / on the side or a cap of a cylinder geom (geom frame), away from the rims"""
    if int(g[1]) == 0:
        k, s = rng.integers(3), rng.choice([-1.0, 1.0])
        loc = rng.uniform(-0.8, 0.8, 3) * g[2:5]
        n = np.zeros(3)
        n[k] = s
        loc[k] = s * g[2 + k]
        return loc, n
    r, h, phi = g[2], g[3], rng.uniform(0, 2 * np.pi)
    if rng.uniform() < 0.6:
        n = np.array([np.cos(phi), np.sin(phi), 0.0])
        return r * n + np.array([0, 0, rng.uniform(-0.8, 0.8) * h]), n
    s, rho = rng.choice([-1.0, 1.0]), rng.uniform(0, 0.8) * r
    return np.array([rho * np.cos(phi), rho * np.sin(phi), s * h]), np.array([0, 0, s])


def vertex_on_surface(q, b, oi, quat, gi, loc, n, depth, vertex=None):
    """pose7 of object oi with quaternion quat such that a vertex of hull b (the one reaching farthest against the surface normal when vertex is None) lies
    `depth` inside the surface point loc (normal n) of its geom gi: pos = v - R (g_pos + R_g (loc - depth n))"""
    quat = f32(quat)
    R, Rg = qmat(quat), OG[gi, 8:17].reshape(3, 3)
    V = hull_parts(q, b)[3]
    v = V[np.argmin(V @ (R @ Rg @ n))] if vertex is None else V[vertex % len(V)]
    return f32(np.concatenate([v - R @ (OG[gi, 5:8] + Rg @ (loc - depth * n)), quat]))


def family_f5(seed=505):
    """hull - object: the humanoid at standing_neutral + N(0, 0.3) on the joints, lifted 0.3 m; one object at uniformly random orientation with a hull vertex
    at depth U(-0.001, 0.01) inside a face, side or cap of one of its geoms; then the cull-edge scenes (a), (b), (c)"""
    rng = np.random.default_rng(seed)
    out = []
    routes = ("dyn", "static", "pose")
    for oi in range(5):
        for k in range(7):
            q = humanoid(rng)
            b, gi = int(rng.integers(24)), int(rng.choice(GEOMS_OF[oi]))
            loc, n = surface_point(rng, OG[gi])
            pose = vertex_on_surface(q, b, oi, qrand(rng), gi, loc, n, rng.uniform(-0.001, 0.01), None if k % 2 else int(rng.integers(64)))
            out.append(scene(f"F5/{oi}/random/{k}", "F5", q, {oi: pose}, routes, ("random",), target=(b, gi)))
    # (a) the farthest-reaching vertex margin - U(1e-5, 8e-5) outside the surface: the contact lies just inside the margin and the culls' 1e-4 slack keeps it
    for k in range(8):
        oi = (CHAIR, BOX, TABLE, CAN, STEP, TABLE, CAN, CHAIR)[k]
        q = humanoid(rng)
        b, gi = int(rng.integers(24)), int(rng.choice(GEOMS_OF[oi]))
        loc, n = surface_point(rng, OG[gi])
        pose = vertex_on_surface(q, b, oi, qrand(rng), gi, loc, n, -(MARGIN - rng.uniform(1e-5, 8e-5)))
        out.append(scene(f"F5/a/{oi}/{k}", "F5", q, {oi: pose}, routes, ("a",), target=(b, gi)))
    # (b) a hull whose body origin lies on the Can's axis: the tangent-plane cull has no radial direction there
    for k, (b, tilted) in enumerate(((0, False), (3, False), (0, True), (7, True))):
        q = humanoid(rng)
        quat = f32(qmul(qaxis(horizontal(rng), 0.4), qyaw(rng.uniform(0, 2 * np.pi))) if tilted else (qyaw(rng.uniform(0, 2 * np.pi)) if k else np.array([1.0, 0, 0, 0])))
        R = qmat(quat)
        xb = hull_parts(q, b)[0]

        def pose_at(t, R=R, xb=xb, quat=quat):
            return f32(np.concatenate([xb - t * R[:, 2] - R @ OG[CAN_GEOM, 5:8], quat]))
        target = -rng.uniform(-0.0008, 0.008)
        t = bisect(lambda t: min_dist([hull_rows(q, b, placed(CAN, pose_at(t))[0])[1]]), 0.0, 2.0, target)
        pose = pose_at(t)
        g = placed(CAN, pose)[0]
        cb = xb - g["pos"]
        un = float(np.linalg.norm(cb - g["mat"][:, 2] * (cb @ g["mat"][:, 2])))
        out.append(scene(f"F5/b/{b}/{'tilted' if tilted else 'upright'}", "F5", q, {CAN: pose}, routes, ("b",), target=(b, CAN_GEOM), un=un))
    # (c) a hull over a box edge, its farthest-reaching vertex at a depth along the edge's diagonal: no face plane separates the two
    for k, depth in enumerate((-0.0006, 0.0005, 0.003, 0.008)):
        oi = (BOX, STEP)[k % 2]
        gi = GEOMS_OF[oi][0]
        q = humanoid(rng)
        b = int(rng.integers(24))
        sx, sy, sz = OG[gi, 2:5]
        loc, n = np.array([sx, rng.uniform(-0.6, 0.6) * sy, sz]), np.array([1.0, 0, 1.0]) / np.sqrt(2)
        pose = vertex_on_surface(q, b, oi, qrand(rng), gi, loc, n, depth)
        out.append(scene(f"F5/c/{oi}/{k}", "F5", q, {oi: pose}, routes, ("c",), target=(b, gi)))
    return out


def family_f6(f3, f5, seed=606):
    """placement edges: scenes of F5 and F3 with the object quaternions scaled by 0.5 and 2 and negated; three objects on the dynamic route (two slots);
    all five objects on the static route (ten geoms, room for eight)"""
    rng = np.random.default_rng(seed)
    out = []
    by = {s["name"]: s for s in f3 + f5}
    for base in ("F5/0/random/1", "F5/2/random/3", "F5/3/random/5", "F3/1-2/random/0", "F3/box-on-slab/both-tilted/4", "F3/1-on-2/yaw0.300"):
        s0 = by[base]
        for fac in (0.5, 2.0, -1.0):
            blk = s0["blk"].copy()
            for oi in active(blk):
                blk[7 * oi + 3: 7 * oi + 7] *= fac
            sc = dict(s0, name=f"F6/{base}*{fac}", family="F6", blk=f32(blk), tags={"scaled"}, base=base)
            out.append(sc)
    # three active objects, two slots: the box on the slab and the step on the box; the step has no slot and does not exist for the step kernel
    q0 = qyaw(0.4)
    p = approach(rng, TABLE, q0, BOX, qmul(q0, qyaw(0.3)), [0, 0, 1], -0.002, {SLAB}, None)
    box_top = placed(BOX, p[1])[0]["pos"] + np.array([0, 0, OG[GEOMS_OF[BOX][0], 4]])
    step_pose = f32(np.concatenate([box_top + np.array([0.0, 0.0, OG[GEOMS_OF[STEP][0], 4] - 0.003]) - OG[GEOMS_OF[STEP][0], 5:8], [1.0, 0, 0, 0]]))
    out.append(scene("F6/three-dynamic-objects", "F6", far_humanoid(), {TABLE: p[0], BOX: p[1], STEP: step_pose}, ("dyn",), ("overcap-dyn",)))
    # five active objects as static obstacles: chair, box and table fill the eight geom rows; the Can (touched by a hull) and the step fall off the end
    q = humanoid(rng)
    poses = {}
    for oi, b in ((CHAIR, 18), (CAN, 23)):
        gi = GEOMS_OF[oi][0]
        loc, n = surface_point(rng, OG[gi])
        poses[oi] = vertex_on_surface(q, b, oi, qrand(rng), gi, loc, n, 0.004)
    for oi, dx in ((BOX, 3.0), (TABLE, -3.0), (STEP, 6.0)):
        poses[oi] = np.concatenate([[STD[0] + dx, STD[1], 1.0], qrand(rng)])
    out.append(scene("F6/five-static-objects", "F6", q, poses, ("static",), ("overcap-static",), target=(23, CAN_GEOM)))
    return out


_SCENES = None


def all_scenes():
    """every scene, in a fixed order (cached)"""
    global _SCENES
    if _SCENES is None:
        f1, f2, f3, f4, f5 = family_f1(), family_f2(), family_f3(), family_f4(), family_f5()
        _SCENES = f1 + f2 + f3 + f4 + f5 + family_f6(f3, f5)
        assert len({s["name"] for s in _SCENES}) == len(_SCENES) <= 256
    return _SCENES


# ---------------------------------------------------------------- the oracle's contact list and its conditioning

def oracle_contacts(o: OracleSim, sc, route, q=None, blk=None):
    """contacts_full() of the scene on route "dyn" (the slots' objects as free bodies) or "static" (every active object's geoms frozen, the first MAXGEOM)"""
    q = sc["q"] if q is None else q
    blk = sc["blk"] if blk is None else blk
    o.clear_objects()
    if route == "dyn":
        o.set_geoms(np.zeros((0, 17)))
        for slot, oi in enumerate(sc["slots"]):
            o.set_object(slot, KPM, oi, blk[7 * oi: 7 * oi + 7])
    else:
        o.set_geoms(object_geoms(KPM, blk))
    o.reset(q, np.zeros(75))
    return {k: np.array(v) for k, v in o.contacts_full().items()}


def ulp_step(x, sign):
    x = np.float32(x)
    return float(np.nextafter(x, np.float32(np.inf) if sign > 0 else np.float32(-np.inf)))


def conditioning(o: OracleSim, sc, route, n_pert=4):
    """dict(ref = the scene's contact list, spread [ncon, 3] = largest change of dist / pos / normal per contact, changed = the set changed, ill) under
    n_pert one-ulp perturbations of the root's and the active objects' pose components (signs seeded by the scene's name)"""
    from contact_force_oracle import match_contacts
    ref = oracle_contacts(o, sc, route)
    rng = np.random.default_rng(sum(map(ord, sc["name"])) + (0 if route == "dyn" else 7))
    spread = np.zeros((len(ref["body"]), 3))
    changed = False
    for _ in range(n_pert):
        q, blk = sc["q"].copy(), sc["blk"].copy()
        for i in range(7):
            q[i] = ulp_step(q[i], rng.choice([-1, 1]))
        for oi in active(blk):
            for i in range(7 * oi, 7 * oi + 7):
                blk[i] = ulp_step(blk[i], rng.choice([-1, 1]))
        c = oracle_contacts(o, sc, route, q, blk)
        pairs, only_c, only_ref = match_contacts(c, ref)
        changed = changed or bool(only_c or only_ref)
        for i, j in pairs:
            spread[j] = np.maximum(spread[j], [abs(c["dist"][i] - ref["dist"][j]), np.abs(c["pos"][i] - ref["pos"][j]).max(), np.abs(c["normal"][i] - ref["normal"][j]).max()])
    ill = changed or bool(len(spread) and spread[:, :2].max() > 1e-5)
    return dict(ref=ref, spread=spread, changed=changed, ill=ill)


_COND = {}


def references(route):
    """{scene name: conditioning()} of every scene that takes the route (cached per process)"""
    if route not in _COND:
        o = OracleSim(kpm=STEP_KPM)
        _COND[route] = {s["name"]: conditioning(o, s, route) for s in all_scenes() if route in s["routes"]}
    return _COND[route]
