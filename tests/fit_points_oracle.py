"""fp64 reference of the pose fit to points at body offsets with a floor term (kp_sim_fit_points): test infrastructure.

Kinematics and Jacobians come from OracleSim through np_rigid.oracle and push_oracle (body_jacobians once per pose, then point_jacobian's formula for
every point of that pose).  The Levenberg-Marquardt loop is the kernel's -- fit_pose_oracle's residuals, q (+) dq, accept rule and mu schedule -- with a
dense numpy.linalg.solve of
    J^T W J + diag(mu damp + w_prior),   J^T W J = fit_pose's + sum_k w_k J_k^T J_k + w_floor sum_{v below} J_v^T J_v   (isotropic floor blocks)
and the exact gradient: J_k^T w_k e_k per point, J_v^T w_floor (0, 0, floor_z - z_v) per hull vertex below the floor.  The vertex table (verts,
vert_adr) is read from the model blob.
"""
import numpy as np

import fit_pose_oracle as FP
import push_oracle as PO
from np_rigid import f32, oracle  # noqa: F401  (the tests reach them through this module)

NV, NB, NU, NQ = FP.NV, FP.NB, FP.NU, FP.NQ
DEFAULT_CFG = dict(FP.DEFAULT_CFG, w_floor=0.0, floor_z=0.0)


def hull_table(kpm):
    """(verts [n, 3] in the body frames, body [n]) of the blob's hull vertices, in the blob's order"""
    adr = np.asarray(kpm["vert_adr"]).astype(int)
    verts = np.asarray(kpm["verts"], np.float64).reshape(-1, 3)[:adr[NB]]
    body = np.concatenate([np.full(adr[b + 1] - adr[b], b) for b in range(NB)])
    return verts, body


def problem(kpm, pt_body=(), pt_offset=(), pt_tgt=None, pt_w=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None):
    """the inputs of one row with the kernel's defaults filled in: fit_pose_oracle.problem's (no origin term without tgt_pos), null point weights are 1,
    a point with w <= 0 is skipped (its target is never looked at)"""
    body = np.asarray(pt_body, int).reshape(-1)
    K = len(body)
    pb = FP.problem(np.zeros((NB, 3)) if tgt_pos is None else tgt_pos, tgt_quat, np.zeros(NB) if tgt_pos is None else w_pos, w_rot, q_prior, w_prior)
    w = np.ones(K) if pt_w is None else np.asarray(pt_w, np.float64).reshape(K)
    on = w > 0
    tgt = np.zeros((K, 3))
    if K:
        tgt[on] = np.asarray(pt_tgt, np.float64).reshape(K, 3)[on]
    hv, hb = hull_table(kpm)
    bad = bool(np.isnan(w).any() or not np.isfinite(tgt[on]).all())
    return dict(pb, body=body, off=np.asarray(pt_offset, np.float64).reshape(K, 3), tgt=tgt, w=np.where(on, w, 0.0), on=on, hv=hv, hb=hb, bad=bad)


def world_points(xpos, xquat, body, off):
    """x_b + R_b o for every (body, offset)"""
    if len(body) == 0:
        return np.zeros((0, 3))
    R = np.stack([PO._rot(xquat[b]) for b in range(NB)])
    return xpos[body] + np.einsum("kij,kj->ki", R[body], off)


def residuals(pb, xpos, xquat, cfg):
    """dict(e_pos, e_rot (fit_pose's), p, e (points; zero where skipped), hp (hull vertices), depth (floor_z - z, > 0 below the floor))"""
    e_pos, e_rot = FP.residuals(pb, xpos, xquat)
    p = world_points(xpos, xquat, pb["body"], pb["off"])
    e = np.where(pb["on"][:, None], pb["tgt"] - p, 0.0)
    hp = world_points(xpos, xquat, pb["hb"], pb["hv"])
    return dict(e_pos=e_pos, e_rot=e_rot, p=p, e=e, hp=hp, depth=float(cfg["floor_z"]) - hp[:, 2])


def cost_of(pb, q, res, cfg):
    below = np.maximum(res["depth"], 0.0)
    return FP.cost_of(pb, q, res["e_pos"], res["e_rot"]) + 0.5 * float(pb["w"] @ (res["e"] ** 2).sum(1)) + 0.5 * float(cfg["w_floor"]) * float(below @ below)


def evaluate(o, pb, q, cfg):
    xpos, xquat = FP.fk(o, q)
    res = residuals(pb, xpos, xquat, cfg)
    return cost_of(pb, q, res, cfg), res


def point_jacobians(Jc, com, pts, body):
    """the velocity Jacobians [n, 3, 75] of world points pts rigidly attached to `body`, from push_oracle.body_jacobians' Jc and subtree_com"""
    out = np.zeros((len(body), 3, NV))
    for i, (b, r) in enumerate(zip(body, pts)):
        out[i] = Jc[b, 3:] - PO._skew(r - com) @ Jc[b, :3]
    return out


def normal_system(o, pb, q, mu, cfg):
    """A = J^T W J + diag(mu damp + w_prior) with the isotropic floor blocks, g = the exact gradient's negative, at q; also J^T W J alone and the residuals"""
    qn = FP.normalized(q)
    Jc, com, xpos, xquat = PO.body_jacobians(o, qn)
    res = residuals(pb, xpos, xquat, cfg)
    H = np.zeros((NV, NV)); g = np.zeros(NV)
    for b in range(NB):
        Jl = Jc[b, 3:] - PO._skew(xpos[b] - com) @ Jc[b, :3]
        H += pb["wp"][b] * Jl.T @ Jl + pb["wr"][b] * Jc[b, :3].T @ Jc[b, :3]
        g += pb["wp"][b] * Jl.T @ res["e_pos"][b] + pb["wr"][b] * Jc[b, :3].T @ res["e_rot"][b]
    idx = np.flatnonzero(pb["on"])
    Jp = point_jacobians(Jc, com, res["p"][idx], pb["body"][idx])
    for i, k in enumerate(idx):
        H += pb["w"][k] * Jp[i].T @ Jp[i]
        g += pb["w"][k] * Jp[i].T @ res["e"][k]
    wf = float(cfg["w_floor"])
    if wf > 0.0:
        act = np.flatnonzero(res["depth"] > 0.0)
        Jv = point_jacobians(Jc, com, res["hp"][act], pb["hb"][act])
        for i, v in enumerate(act):
            H += wf * Jv[i].T @ Jv[i]                                   # isotropic: a majoriser of wf J^T n n^T J
            g += wf * Jv[i, 2] * res["depth"][v]
    extra = mu * np.asarray(cfg["damp"], float)
    extra[6:] += pb["wq"]
    g[6:] += pb["wq"] * (pb["qp"] - np.asarray(qn, float)[7:])
    return H + np.diag(extra), g, H, res


def point_figures(pb, res):
    """info 8..11 and pt_err: max and rms |e_k| over the counted points, deepest vertex below the floor, vertices below it; |e_k| per point"""
    en = np.linalg.norm(res["e"], axis=1)
    n = int(pb["on"].sum())
    below = res["depth"] > 0.0
    return [float(en.max()) if n else 0.0, float(np.sqrt((en ** 2).sum() / n)) if n else 0.0, float(res["depth"][below].max()) if below.any() else 0.0, float(below.sum())], en


def lm(o, q0, pb, cfg=None, jnt_range=None, jnt_limited=None):
    """The kernel's loop in fp64.  Returns dict(qpos, info [12], dq [75], pt_err [K], A, g (last system), costs (after every iteration), margin: the
    smallest |z_v - floor_z| over every hull vertex at every pose the loop evaluated -- the init and every trial pose (equal active sets on the device
    need it above the device's rounding))."""
    cfg = {**DEFAULT_CFG, **(cfg or {})}
    q = FP.normalized(q0)
    c, res = evaluate(o, pb, q, cfg)
    cost0, mu, nacc = c, float(cfg["mu0"]), 0
    dq = np.zeros(NV); A = g = None
    costs, margin = [], float(np.abs(res["depth"]).min())
    bad = pb["bad"] or not (np.isfinite(c) and np.all(np.isfinite(q0)))
    for it in range(0 if bad else int(cfg["n_iters"])):
        A, g, _, _ = normal_system(o, pb, q, mu, cfg)
        dq = np.linalg.solve(A, g)
        qt = FP.oplus(q, dq, *((jnt_range, jnt_limited) if cfg["clamp_limits"] else (None, None)))
        ct, rest = evaluate(o, pb, qt, cfg)
        margin = min(margin, float(np.abs(rest["depth"]).min()))
        if np.isfinite(ct) and ct < c:
            q, c, res = qt, ct, rest
            nacc += 1; mu = max(mu * cfg["mu_down"], cfg["mu_min"])
        else:
            mu = min(mu * cfg["mu_up"], cfg["mu_max"])
        costs.append(c)
    ep, er = FP.errors(pb, res["e_pos"], res["e_rot"])
    fig, en = ([0.0] * 4, np.zeros(len(pb["body"]))) if bad else point_figures(pb, res)
    info = np.array([cost0, c, nacc, mu, ep, er, float(np.abs(dq).max()), 1.0 if bad else 0.0, *fig])
    return dict(qpos=np.array(q0, np.float64) if bad else q, info=info, dq=dq, pt_err=en, A=A, g=g, costs=costs, margin=margin)


# ---------------------------------------------------------------- the matrix identity the design rests on

def body_floats(xpos, pts, body, w, w_rot=None):
    """The ten floats per body the kernel writes into s.cinert [24, 10]: (Ixx Iyy Izz Ixy Ixz Iyz | m r | m) of the body's weighted points as point
    masses about the root origin xpos[0], plus w_rot on the diagonal"""
    ci = np.zeros((NB, 10))
    for b, p, m in zip(body, pts, w):
        r = p - xpos[0]; r2 = r @ r
        ci[b, 0:3] += m * (r2 - r * r)
        ci[b, 3] -= m * r[0] * r[1]; ci[b, 4] -= m * r[0] * r[2]; ci[b, 5] -= m * r[1] * r[2]
        ci[b, 6:9] += m * r; ci[b, 9] += m
    if w_rot is not None:
        ci[:, 0:3] += np.asarray(w_rot, float)[:, None]
    return ci


def inertia_from_floats(o, q, ci, dof_body, body_parent):
    """The joint-space inertia of the tree whose body b has the spatial inertia ci[b] about the root origin (composite-rigid-body algorithm, as
    fit_pose_oracle.pseudo_inertia_crba, which takes weights at the origins only).  Spatial vectors [ang; lin] about xpos[0], world axes."""
    Jc, com, xpos, _ = PO.body_jacobians(o, FP.normalized(q))
    Ic = np.zeros((NB, 6, 6))
    for b in range(NB):
        I = np.array([[ci[b, 0], ci[b, 3], ci[b, 4]], [ci[b, 3], ci[b, 1], ci[b, 5]], [ci[b, 4], ci[b, 5], ci[b, 2]]])
        S = PO._skew(ci[b, 6:9])
        Ic[b, :3, :3] = I; Ic[b, :3, 3:] = S; Ic[b, 3:, :3] = -S; Ic[b, 3:, 3:] = ci[b, 9] * np.eye(3)
    for b in range(NB - 1, 0, -1):
        Ic[body_parent[b]] += Ic[b]
    s = np.zeros((NV, 6))
    for d in range(NV):
        a, l = Jc[dof_body[d], :3, d], Jc[dof_body[d], 3:, d]
        s[d] = np.concatenate([a, l - PO._skew(xpos[0] - com) @ a])      # the axis' linear part moved from subtree_com to the root origin
    anc = []
    for b in range(NB):
        path = [b]
        while body_parent[path[-1]] >= 0:
            path.append(body_parent[path[-1]])
        anc.append(set(path))
    M = np.zeros((NV, NV))
    for i in range(NV):
        bi = dof_body[i]
        f = Ic[bi] @ s[i]
        for j in range(NV):
            if dof_body[j] in anc[bi] and (dof_body[j] != bi or j <= i):
                M[i, j] = M[j, i] = s[j] @ f
    return M


# ---------------------------------------------------------------- marker sets and cases of the GPU tests (chosen in tests/test_fit_points_cpu.py)

ROWS = (1, 5, 67)
OFFSET_RADIUS = 0.12
K_MARKERS = 53


def _offsets(rng, n):
    """n offsets within OFFSET_RADIUS of the body origin, at least 0.04 m apart and, from three on, at least 0.03 m off the line through the first two"""
    out = []
    while len(out) < n:
        v = rng.uniform(-1.0, 1.0, 3)
        nv = np.linalg.norm(v)
        if nv > 1.0 or nv < 1e-3:
            continue
        v = v * OFFSET_RADIUS * rng.uniform(0.4, 1.0) / nv
        if any(np.linalg.norm(v - u) < 0.04 for u in out):
            continue
        if len(out) >= 2:
            d = out[1] - out[0]
            if np.linalg.norm(np.cross(v - out[0], d)) / np.linalg.norm(d) < 0.03:
                continue
        out.append(v)
    return out


def marker_set(counts, seed):
    """(body int32 [K], offset [K, 3] fp32-representable) with counts[b] points on body b, in an order that interleaves the bodies (the entry point
    sorts them)"""
    rng = np.random.default_rng(seed)
    body, off = [], []
    for b, n in enumerate(counts):
        for v in _offsets(rng, n):
            body.append(b); off.append(v)
    order = rng.permutation(len(body))
    return np.asarray(body, np.int32)[order], f32(np.asarray(off).reshape(-1, 3)[order])


def counts_53():
    """53 markers: two on every body and a third on the pelvis, the torso, the head and the two feet (0, 3, 7, 9..: see BODIES_3).  Two markers and the
    joint that ties a body to its parent are three points off one line, which fixes the body; the pelvis has no parent and carries three."""
    c = [2] * NB
    for b in BODIES_3:
        c[b] += 1
    assert sum(c) == K_MARKERS
    return c


BODIES_3 = (0, 3, 7, 11, 13)      # Pelvis, L_Ankle, R_Ankle, Chest, Head in the blob's body order


def counts_67():
    """67 markers, 40 of them on the pelvis, nine bodies empty: lane wrap (more than 64 points) and a long per-body sum"""
    c = [0] * NB
    c[0] = 40
    carrying = [1, 2, 3, 5, 6, 7, 9, 11, 13, 15, 16, 18, 20, 21]      # 14 bodies, 27 points
    for i, b in enumerate(carrying):
        c[b] = 2 if i < 13 else 1
    assert sum(c) == 67 and sum(1 for n in c if n == 0) == 9
    return c


def marker_positions(o, q, body, off):
    xpos, xquat = FP.fk(o, q)
    return world_points(xpos, xquat, np.asarray(body, int), np.asarray(off, float))


def reachable_case(o, q_true, seed, body, off, exact=False):
    """targets = the markers of the truth (fp32 roundings unless exact), all weights 1, no orientations; init = fit_pose_oracle.perturbed(truth)"""
    p = marker_positions(o, q_true, body, off)
    return dict(q_true=FP.normalized(q_true), q0=f32(FP.perturbed(q_true, seed)), pt_tgt=p if exact else f32(p))


def lowest_vertex(o, kpm, q):
    hv, hb = hull_table(kpm)
    xpos, xquat = FP.fk(o, q)
    return float(world_points(xpos, xquat, hb, hv)[:, 2].min())


def grounded(o, kpm, q, height=0.0):
    """q moved along z so that its lowest hull vertex sits at `height` (fp32-representable; the rounding moves it by < 1e-7)"""
    q = np.array(q, np.float64)
    q[2] += height - lowest_vertex(o, kpm, q)
    return f32(q)


FLOOR_DELTA, FLOOR_W = 0.03, 2400.0
FLOOR_BOUND = FLOOR_DELTA * np.sqrt(NB / FLOOR_W)      # 3 mm: 1/2 w_floor d_max^2 <= 1/2 24 w_pos delta^2
FLOOR_ITERS = 30
# The comparison with the reference runs FLOOR_COMPARE_ITERS iterations, at two weights.  In the fp64 loop no hull vertex comes within 1e-5 m of the plane at
# any pose of those iterations, at either weight (asserted in tests/test_fit_points_cpu.py); near the minimum the sole's vertices hover micrometres around
# the plane (the deepest sits 3e-5 m below it), which is why the comparison stops early.
#   FLOOR_COMPARE_W (a vertex weighs like a few markers; cond(A) 2^-23 <= 6e-2 over the three iterations): the device follows the reference closely enough
#       to hold the SAME active sets, so the vertex counts are asserted equal and cost and depth carry tight measured tolerances.
#   FLOOR_W = 2400 (cond(A) 1e7 .. 1e8): the margin of the fp64 loop does NOT carry over -- the fp32 steps move the trajectory by up to 3e-4 m in depth, the
#       active sets differ (lying: 9 vertices below against 8) and cost and depth are held only to their loose measured figures.
FLOOR_COMPARE_ITERS = 3
FLOOR_COMPARE_W = 4.0
# depth of the sunk one-step cases; a case with a vertex within 1e-5 m of the plane at the init or the trial pose (at either weight below) gets its own
SUNK_DEPTH, SUNK_DEPTH_OF = 0.04, {20: 0.041, 51: 0.041}
# The floor weight of the one-step parity variant.  With w_floor = 2400 and some 50 vertices 4 cm deep the normal matrix has cond(A) up to 8e7
# (cond(A) 2^-23 up to 9.9: the floor's blocks against mu damp = 1e-2), so an fp32 step cannot be held to a 1e-4 figure against the fp64 solve, whatever the
# method.  The variant under the dq cap therefore weighs a vertex like a marker (w_floor = 1: cond(A) 2^-23 <= 5e-3, the order of the other variants);
# the 2400 variant is held to the conditioning bound cond(A) 2^-23 row by row, and to the cost tolerance.
FLOOR_PARITY_W = 1.0


def floor_case(o, kpm, q, floor_z=0.0):
    """The bound's case: a pose standing ON floor_z; targets = its 24 origins moved FLOOR_DELTA down (w_pos 1), init = the pose moved down with them.
    'Translate up by delta' is feasible and costs 1/2 24 delta^2 (cand_cost)."""
    qg = grounded(o, kpm, q, floor_z)
    xpos, _ = FP.fk(o, qg)
    sunk = np.array(qg); sunk[2] -= FLOOR_DELTA
    return dict(q_on=qg, q0=f32(sunk), tgt_pos=f32(xpos - np.array([0.0, 0.0, FLOOR_DELTA])), cand_cost=0.5 * NB * FLOOR_DELTA ** 2, floor_z=floor_z)


def floor_poses(named):
    """name -> (pose, floor_z) of the floor-bound cases: standing and lying on z = 0, the sitting pose on a floor at 0.05 m"""
    by = {s["name"]: s["q"] for s in named}
    return {"standing": (f32(by["a_standing"]), 0.0), "lying": (f32(by["d_lying"]), 0.0), "sit_z05": (f32(by["g_sit"]), 0.05)}


SEED_53, SEED_67 = 1, 2
# iterations of the reachable cases: what the fp64 loop needs on the worst of them to bring every |e_k| under 1e-5 m is asserted in
# tests/test_fit_points_cpu.py; a case that needs more gets its own entry here (the cap stays)
REACH_ITERS = 12
REACH_ITERS_OF = {}


def reach_iters(i):
    return REACH_ITERS_OF.get(i, REACH_ITERS)


def sunk_marker_case(o, kpm, q_true, i, body, off):
    """one-step parity with the floor on, case i: the markers of a truth whose lowest vertex lies SUNK_DEPTH below the floor, init = the perturbed truth"""
    seed = 100 + i
    qs = grounded(o, kpm, q_true, -SUNK_DEPTH_OF.get(i, SUNK_DEPTH))
    return dict(reachable_case(o, qs, seed, body, off), q_sunk=qs)


EQUIV_ITERS = 30


def equiv_reference(o, truths):
    """(qpos [67, 76], info [67, 8]) of the fp64 loop on the 24 body origins, positions only, EQUIV_ITERS iterations: what fit_points on
    MarkerSet.body_origins() and fit_pose are both measured against (tests/golden/fit_points_equiv_ref.npz)"""
    body, off = np.arange(NB), np.zeros((NB, 3))
    qs, infos = [], []
    for i, q in enumerate(truths):
        c = reachable_case(o, q, 100 + i, body, off)
        r = FP.lm(o, c["q0"], FP.problem(c["pt_tgt"]), dict(n_iters=EQUIV_ITERS))
        qs.append(r["qpos"]); infos.append(r["info"])
    return np.stack(qs), np.stack(infos)


if __name__ == "__main__":
    # rewrites tests/golden/fit_points_equiv_ref.npz (tests/test_fit_points_cpu.py checks the file against a fresh computation)
    import os
    import inverse_dynamics_oracle as ID
    from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    std = np.load(os.path.join(root, "tests", "golden", "standing_neutral.npz"))
    kpm = read_kpm(DEFAULT_KPM)
    truths = FP.truth_poses(ID.named_states(kpm, read_kpm(STEP_KPM), std["qpos"], std["qvel"]), ID.sweep_states(kpm, std["qpos"]))
    qpos, info = equiv_reference(oracle(DEFAULT_KPM), truths)
    np.savez(os.path.join(root, "tests", "golden", "fit_points_equiv_ref.npz"), qpos=qpos, info=info)
    print(f"{len(qpos)} fits written, final max |e_pos| up to {info[:, 4].max():.3e} m, last |dq| up to {info[:, 6].max():.3e}")
