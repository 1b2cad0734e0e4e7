"""The kinematic part of the reference's paper-metric script (scripts/eval_pose_all.py:113-197, kin_poly/utils/metrics.py) on the records
`evaluate.write_coverage` stores (`*_coverage_full.pkl`: per take `pred`, `target`, `obj_pose`, `percent`, `fail_safe`):

    root_dist   mean Frobenius norm of I - T_pred T_gt^-1 over the root's 4 x 4 transforms      (get_root_matrix, get_frobenious_norm)
    mpjpe       mean root-relative joint position error, mm                                      (:170-172)
    accel_dist  mean norm of the second-difference error of the joint positions, mm / frame^2    (compute_error_accel, :45-74)
    vel_dist    mean norm of the difference of the finite-difference generalised velocities      (get_joint_vels -> get_qvel_fd(.., 'heading'), get_mean_dist)
    head_dist   root_dist's measure on the head's transform against the data set's head_pose

numpy, host side (an analysis step after the roll-outs, as in the reference).  Joint positions come from the forward kinematics of the poses (the
reference reads MuJoCo's body_xpos after sim.forward: the same quantities).

The physical columns of compute_physcis_metris (:205-467), on every frame of the predicted and of the ground-truth trajectory:

    pen         penetration beyond 5 mm, summed over the hull - floor / hull - object contacts of a frame and over the frames, / T, x 1000
    slide       foot sliding of the two toes (compute_foot_sliding, :294-309), mean of L_Toe and R_Toe
    succ        the take's object interaction (compute_obj_interact, :337-467), by the action prefix of its name

The contact walk is one batched device query (KpSim.pose_contacts: kp_sim_pose_contacts on kp_sim_fk's body poses); the rules applied to its
per-frame results are restated here.  Reference geom ids: 1 + body index for the 24 hulls (1 Pelvis, 2 L_Hip, 4 L_Ankle, 5 L_Toe, 6 R_Hip,
8 R_Ankle, 9 R_Toe, 10 Torso, 11 Spine, 14 Head), 25 + g for object geom g of the model (25-26 chair, 27 box, 28-32 table, 33 Can, 34 step).
"""
from __future__ import annotations

import numpy as np


def _qmat(q):
    """Gohlke quaternion_matrix (rotation part), batched [T, 4] -> [T, 3, 3]; a near-zero quaternion gives the identity as there."""
    q = np.asarray(q, np.float64)
    n = (q * q).sum(-1)
    out = np.tile(np.eye(3), (q.shape[0], 1, 1))
    ok = n > np.finfo(float).eps * 4.0
    s = np.where(ok, np.sqrt(2.0 / np.where(ok, n, 1.0)), 0.0)
    w, x, y, z = (q * s[:, None]).T
    R = np.stack([np.stack([1 - y * y - z * z, x * y - z * w, x * z + y * w], -1),
                  np.stack([x * y + z * w, 1 - x * x - z * z, y * z - x * w], -1),
                  np.stack([x * z - y * w, y * z + x * w, 1 - x * x - y * y], -1)], -2)
    out[ok] = R[ok]
    return out


def _qmul(a, b):
    w1, x1, y1, z1 = a.T; w0, x0, y0, z0 = b.T
    return np.stack([-x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0, x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0,
                     -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0, x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0], -1)


def root_matrices(poses7):
    """get_root_matrix (metrics.py:15-24): [T, 4, 4] from rows (x, y, z, qw, qx, qy, qz)."""
    p = np.asarray(poses7, np.float64)
    M = np.tile(np.eye(4), (p.shape[0], 1, 1))
    M[:, :3, :3] = _qmat(p[:, 3:7])
    M[:, :3, 3] = p[:, :3]
    return M


def frobenius_dist(A, B):
    """get_frobenious_norm (metrics.py:64-72): mean over frames of || I - A_t B_t^-1 ||_F."""
    return float(np.linalg.norm(np.eye(4)[None] - A @ np.linalg.inv(B), axis=(1, 2)).mean())


def joint_vels(qpos, dt):
    """get_joint_vels (metrics.py:38-44) = get_qvel_fd(p_t, p_t+1, dt, 'heading') of kin_poly/utils/math_utils.py:26-43 for every frame pair -> [T - 1, 75]."""
    q = np.asarray(qpos, np.float64)
    cur, nxt = q[:-1], q[1:]
    v = (nxt[:, :3] - cur[:, :3]) / dt
    cq = cur[:, 3:7]
    inv = np.concatenate([cq[:, :1], -cq[:, 1:]], 1) / (cq * cq).sum(1, keepdims=True)
    qrel = _qmul(nxt[:, 3:7], inv)
    w = qrel[:, 0]
    none = (np.abs(1.0 - w) < 1e-6) | (np.abs(1.0 + w) < 1e-6)                       # rotation_from_quaternion (transformation.py:362-372)
    angle = np.where(none, 0.0, 2.0 * np.arccos(np.clip(w, -1.0, 1.0)))
    ax = qrel[:, 1:] / np.where(none, 1.0, np.sin(angle / 2.0))[:, None]
    ax = ax / np.where(none, 1.0, np.linalg.norm(ax, axis=1))[:, None]
    ax[none] = [1.0, 0.0, 0.0]
    angle = np.where(angle > np.pi, angle - 2 * np.pi, angle)
    rv = np.einsum("tji,tj->ti", _qmat(cq), ax * angle[:, None] / dt)               # transform_vec(., cur, 'root'): R^T rv
    hq = cq.copy(); hq[:, 1:3] = 0.0; hq /= np.linalg.norm(hq, axis=1, keepdims=True)
    v = np.einsum("tji,tj->ti", _qmat(hq), v)                                        # root velocity into the heading frame
    return np.concatenate([v, rv, (nxt[:, 7:] - cur[:, 7:]) / dt], 1)


def accel_error(jpos_gt, jpos_pred):
    """compute_error_accel (eval_pose_all.py:45-74, vis=None): per frame triple, mean over joints of || (second difference of pred) - (of gt) ||."""
    a_gt = jpos_gt[:-2] - 2 * jpos_gt[1:-1] + jpos_gt[2:]
    a_pr = jpos_pred[:-2] - 2 * jpos_pred[1:-1] + jpos_pred[2:]
    return np.linalg.norm(a_pr - a_gt, axis=2).mean(1)


def sequence_metrics(pred_qpos, gt_qpos, jpos_pred, jpos_gt, head_pred=None, head_gt=None, dt=1.0 / 30.0) -> dict:
    """One take: pred / gt qpos [T, 76], their joint positions [T, 24, 3] (forward kinematics), optional head poses [T, 7]."""
    pred_qpos, gt_qpos = np.asarray(pred_qpos, np.float64), np.asarray(gt_qpos, np.float64)
    jp, jg = np.asarray(jpos_pred, np.float64).reshape(-1, 24, 3), np.asarray(jpos_gt, np.float64).reshape(-1, 24, 3)
    out = {"root_dist": frobenius_dist(root_matrices(pred_qpos[:, :7]), root_matrices(gt_qpos[:, :7])),
           "vel_dist": float(np.linalg.norm(joint_vels(pred_qpos, dt) - joint_vels(gt_qpos, dt), axis=1).mean()),
           "accel_dist": float(accel_error(jp, jg).mean() * 1000.0),                 # the reference passes (pred, gt) into (gt, pred): symmetric
           "mpjpe": float(np.linalg.norm((jp - jp[:, :1]) - (jg - jg[:, :1]), axis=2).mean() * 1000.0)}
    if head_pred is not None and head_gt is not None:
        out["head_dist"] = frobenius_dist(root_matrices(head_pred), root_matrices(head_gt))
    return out


def coverage_metrics(results: dict, gt: dict, fk, dt=1.0 / 30.0) -> dict:
    """compute_metrics (:113-197) over a `*_coverage_full.pkl` dict.  gt: {take: {'qpos' [T, 76], 'head_pose' [T, 7]}} (the feature file's entries);
    fk(qpos [T, 76]) -> (joint positions [T, 24, 3], body quaternions [T, 24, 4]) -- e.g. supervised.TorchFK.chain_torch.  A take whose roll-out is one
    frame shorter than its clip is compared with the clip's first T - 1 frames, as the reference does (:683-688).  Returns the means over the takes
    + 'succ' = share of takes played to their end without the fail-safe, + 'per_take'."""
    per = {}
    for k, r in results.items():
        if k not in gt:
            continue
        pred = np.asarray(r["pred"], np.float64)
        g, hp = np.asarray(gt[k]["qpos"], np.float64), np.asarray(gt[k]["head_pose"], np.float64)
        n = min(len(pred), len(g))
        if n < 3:
            continue
        pred, g, hp = pred[:n], g[:n], hp[:n]
        jp, qp = fk(pred); jg, _ = fk(g)
        jp, qp, jg = np.asarray(jp, np.float64), np.asarray(qp, np.float64), np.asarray(jg, np.float64)
        m = sequence_metrics(pred, g, jp, jg, np.concatenate([jp[:, 13], qp[:, 13]], 1), hp, dt)
        m["succ"] = float(r.get("percent", 0.0) == 1 and not r.get("fail_safe", False))
        per[k] = m
    keys = sorted({kk for m in per.values() for kk in m})
    return {**{kk: float(np.mean([m[kk] for m in per.values() if kk in m])) for kk in keys}, "per_take": per}


PEN_MARGIN = 0.005                                    # compute_physcis_metris: margin
L_TOE, R_TOE, HEAD = 4, 8, 13                         # body indices (reference body / geom id - 1)
_SIT_BODIES = sum(1 << b for b in (0, 1, 5, 9, 10))   # geoms 1, 2, 6, 10, 11
_AVOID_BODIES = (1 << 12) - 1                         # geoms 1..12
_STEP_BODIES = sum(1 << b for b in (3, 4, 7, 8))      # geoms 4, 5, 8, 9
_CHAIR, _CAN, _STEP = (0, 1), 8, 9                    # object geoms 25-26, 33, 34


def pen_metric(frame_pen) -> float:
    """seq_pen (:229-285): the frames' penetration sums (frames without penetration add nothing), / T, x 1000."""
    p = np.asarray(frame_pen, np.float64)
    return float(np.sum(p[p > 0]) / len(p) * 1000) if np.any(p > 0) else 0.0


def foot_sliding(toe_xyz, root_z) -> float:
    """compute_foot_sliding (:294-309): toe positions [T, 3] (body_xpos), root heights qpos[:, 2] [T]."""
    H, z_threshold = 0.033, 0.65
    seq_len = len(root_z)
    z = np.asarray(root_z, np.float64)[1:]
    foot = np.array(toe_xyz, np.float64)
    foot[:, -1] -= np.mean(foot[:3, -1])
    disp = np.linalg.norm(foot[1:, :2] - foot[:-1, :2], axis=1)
    avg = (foot[:-1, -1] + foot[1:, -1]) / 2
    subset = np.logical_and(avg < H, z > z_threshold)
    return float(np.sum(np.abs(disp * (2 - 2 ** (avg / H)))[subset]) / seq_len * 1000)


def interaction_success(action, hits, root_z, obj_pose, head_pos, head_pos_gt, fail_safe=None) -> bool:
    """compute_obj_interact (:337-467) on the per-frame hit masks hits [T, n_obj_geoms] (bit b: hull b touches object geom g).  root_z = qpos[:, 2];
    obj_pose [T, 35]; head_pos / head_pos_gt [T, 3].  fail_safe (the predicted run only): succ &= not fail_safe.  An action the reference does not
    know is a success here (the reference's compute_metrics raises KeyError on it)."""
    h = np.asarray(hits, np.int64)
    if action == "sit":
        succ = bool(np.any((h[:, _CHAIR[0]] | h[:, _CHAIR[1]]) & _SIT_BODIES))
    elif action == "avoid":
        diff = np.linalg.norm(np.asarray(head_pos, np.float64)[-1] - np.asarray(head_pos_gt, np.float64)[-1])
        succ = not (bool(np.any(h[:, _CAN] & _AVOID_BODIES)) or diff > 0.5)
    elif action == "push":
        box = np.asarray(obj_pose, np.float64)[:, 7:10]
        succ = bool(np.max(np.linalg.norm(box[0] - box, axis=1)) > 0.1)
    elif action == "step":
        z = np.asarray(root_z, np.float64)
        succ = bool(np.any(h[:, _STEP] & _STEP_BODIES)) and bool(np.any(z - z[0] > 0.1))
    else:
        succ = True
    if fail_safe is not None:
        succ = succ and not fail_safe
    return succ


def coverage_physics_metrics(results: dict, gt: dict, sim, chunk_rows: int = 65536) -> dict:
    """compute_physcis_metris (:205-292) for the predicted and the ground-truth trajectory of every take of a `*_coverage_full.pkl` dict.  gt as in
    coverage_metrics ({take: {'qpos', 'head_pose'}}); sim: a KpSim on the scene the run used.  Takes are cut to n = min(len(pred), len(gt qpos)) as
    coverage_metrics does; the ground truth is played with the predicted run's obj_pose (:146-147).  All frames of all takes go to the device in one
    query per chunk of chunk_rows rows.  Returns the means of pen_pred, pen_gt, slide_pred, slide_gt and succ, 'succ_by_action' and 'per_take'."""
    import torch
    takes, q_rows, o_rows = [], [], []
    for k, r in results.items():
        if k not in gt:
            continue
        pred, g = np.asarray(r["pred"], np.float64), np.asarray(gt[k]["qpos"], np.float64)
        n = min(len(pred), len(g))
        if n < 3:
            continue
        obj = np.asarray(r["obj_pose"], np.float64)[:n]
        if obj.shape != (n, 35):
            raise ValueError(f"{k}: obj_pose must hold the 35-float object block of every frame")
        takes.append((k, n, r))
        q_rows += [pred[:n], g[:n]]; o_rows += [obj, obj]
    if not takes:
        return {"per_take": {}, "succ_by_action": {}}
    Q, O = np.concatenate(q_rows).astype(np.float32), np.concatenate(o_rows).astype(np.float32)
    pen, hits, xpos = np.empty(len(Q), np.float64), None, np.empty((len(Q), 24, 3), np.float64)
    for a in range(0, len(Q), chunk_rows):
        out = sim.pose_contacts(torch.from_numpy(Q[a:a + chunk_rows]).to(sim.device), torch.from_numpy(O[a:a + chunk_rows]).to(sim.device))
        pen[a:a + chunk_rows] = out["pen"].double().cpu().numpy()
        hc = out["hits"].cpu().numpy().astype(np.int64)
        hits = np.empty((len(Q), hc.shape[1]), np.int64) if hits is None else hits
        hits[a:a + chunk_rows] = hc
        xpos[a:a + chunk_rows] = out["xpos"].double().cpu().numpy().reshape(-1, 24, 3)
    per, row = {}, 0
    for k, n, r in takes:
        hp_gt = np.asarray(gt[k]["head_pose"], np.float64)[:n, :3]
        m = {}
        for side, qp, fs in (("pred", Q[row:row + n], r.get("fail_safe")), ("gt", Q[row + n:row + 2 * n], None)):
            sl = slice(row, row + n) if side == "pred" else slice(row + n, row + 2 * n)
            z = qp[:, 2].astype(np.float64)
            m["pen_" + side] = pen_metric(pen[sl])
            m["slide_" + side] = (foot_sliding(xpos[sl, L_TOE], z) + foot_sliding(xpos[sl, R_TOE], z)) / 2
            s = interaction_success(k.split("-")[0], hits[sl], z, O[row:row + n], xpos[sl, HEAD], hp_gt, fs)
            m["succ" if side == "pred" else "succ_gt"] = float(s)
        per[k] = m
        row += 2 * n
    keys = ("pen_pred", "pen_gt", "slide_pred", "slide_gt", "succ")
    by_action = {}
    for k, m in per.items():
        by_action.setdefault(k.split("-")[0], []).append(m["succ"])
    return {**{kk: float(np.mean([m[kk] for m in per.values()])) for kk in keys},
            "succ_by_action": {a: float(np.mean(v)) for a, v in by_action.items()}, "per_take": per}


DYNAMICS_KEYS = ("resid_force", "resid_torque", "torque_rms", "over_limit", "power")


def coverage_dynamics_metrics(results: dict, gt: dict, sim, dt=1.0 / 30.0, kpm=None, chunk_rows: int = 65536, contacts: str = "soft", estimate_cfg=None) -> dict:
    """Dynamics score of pose sequences that were never simulated: inverse dynamics (KpSim.inverse_dynamics on
    dynamics.motion_derivatives' finite differences) of the predicted (`pred`, its first 76 columns) and the ground-truth trajectory of every take of a
    `*_coverage_full.pkl` dict, with the take's object block (`obj_pose` [T, 35], static obstacles) where the pickle has one and sim's blob has object
    geoms.  gt as in coverage_metrics; takes are cut to n = min(len(pred), len(gt qpos)), n >= 3.  kpm: the blob (path or read_kpm dict) whose
    torque_lim and body masses are used; default: the blob sim's model was loaded from.  Per side (pred / gt), means over a take's frames of
    dynamics.plausibility: resid_force_* (root residual force / body weight), resid_torque_* (N m), torque_rms_* (N m), over_limit_* (share of
    joint-frames beyond torque_lim), power_* (W).  Returns their means over the takes, 'by_action' (the same per action prefix) and 'per_take'.
    contacts: "soft" (the default: the soft-constraint contact forces of inverse dynamics, the keys above and nothing else), "estimated" (the contact
    forces estimated from kinematics, DESIGN.md section 18: the same scores from KpSim.estimate_contacts under the keys `<name>_<side>_est`, plus
    support_share_<side>_est, the share of frames with a candidate, and grf_z_<side>_est, the estimated vertical ground reaction / body weight) or
    "both".  estimate_cfg: a dynamics.EstimateConfig (None: the defaults)."""
    if contacts not in ("soft", "estimated", "both"):
        raise ValueError(f'coverage_dynamics_metrics: contacts must be "soft", "estimated" or "both", got {contacts!r}')
    import torch
    from . import dynamics
    from .contact import body_weight
    from .model_compiler import DEFAULT_KPM, read_kpm
    kpm = kpm if kpm is not None else (getattr(sim.model, "kpm_path", None) or DEFAULT_KPM)
    kpm = read_kpm(kpm) if isinstance(kpm, str) else kpm
    weight, lim = body_weight(kpm), torch.tensor(np.asarray(kpm["torque_lim"], np.float32), device=sim.device)
    has_geoms = int(sim.model.get_option("n_obj_geoms")) > 0
    takes, q_rows, o_rows, off = [], [], [], [0]
    for k, r in results.items():
        if k not in gt:
            continue
        pred, g = np.asarray(r["pred"], np.float64)[:, :76], np.asarray(gt[k]["qpos"], np.float64)[:, :76]
        n = min(len(pred), len(g))
        if n < 3:
            continue
        obj = np.asarray(r["obj_pose"], np.float64)[:n] if has_geoms and r.get("obj_pose") is not None else None
        if obj is not None and obj.shape != (n, 35):
            raise ValueError(f"{k}: obj_pose must hold the 35-float object block of every frame")
        takes.append((k, n))
        for side in (pred[:n], g[:n]):
            q_rows.append(side); o_rows.append(obj); off.append(off[-1] + n)
    if not takes:
        return {"per_take": {}, "by_action": {}}
    if any(o is None for o in o_rows) and not all(o is None for o in o_rows):      # a pickle that mixes takes with and without a block: parked where there is none
        park = np.zeros(35); park[3::7] = 1.0; park[0::7] = 100.0 * np.arange(1, 6); park[1::7] = 100.0
        o_rows = [np.tile(park, (len(q), 1)) if o is None else o for q, o in zip(q_rows, o_rows)]
    Q = torch.from_numpy(np.concatenate(q_rows).astype(np.float32))
    Ob = None if o_rows[0] is None else torch.from_numpy(np.concatenate(o_rows).astype(np.float32))
    names = ("resid_force", "resid_torque", "joint_torque_rms", "over_limit", "power")
    frames, keys = {}, []
    if contacts in ("soft", "both"):
        out = dynamics.inverse_dynamics_sequence(sim, Q, dt, Ob, chunk_rows, take_off=off, want=("qfrc_inverse",))
        p = dynamics.plausibility(out["qfrc_inverse"], Q.to(sim.device), out["qvel"], lim, weight)
        frames.update({(a, ""): p[b].double().cpu().numpy() for a, b in zip(DYNAMICS_KEYS, names)})
        keys += [f"{a}_{b}" for a in DYNAMICS_KEYS for b in ("pred", "gt")]
    if contacts in ("estimated", "both"):
        est = dynamics.estimate_contacts_sequence(sim, Q, dt, Ob, chunk_rows, take_off=off, cfg=estimate_cfg, want=("qfrc_inverse", "net_wrench", "ncon"))
        p = dynamics.plausibility_estimated(est, Q.to(sim.device), lim, weight)
        frames.update({(a, "_est"): p[b].double().cpu().numpy() for a, b in zip(DYNAMICS_KEYS, names)})
        frames[("support_share", "_est")] = (est["ncon"] > 0).double().cpu().numpy()
        frames[("grf_z", "_est")] = p["grf"][:, 2].double().cpu().numpy()
        keys += [f"{a}_{b}_est" for a in DYNAMICS_KEYS + ("support_share", "grf_z") for b in ("pred", "gt")]
    per = {}
    for i, (k, n) in enumerate(takes):
        per[k] = {f"{a}_{side}{sfx}": float(fr[off[2 * i + j]:off[2 * i + j + 1]].mean()) for (a, sfx), fr in frames.items() for j, side in enumerate(("pred", "gt"))}
    by_action = {}
    for k, m in per.items():
        by_action.setdefault(k.split("-")[0], []).append(m)
    return {**{kk: float(np.mean([m[kk] for m in per.values()])) for kk in keys},
            "by_action": {a: {kk: float(np.mean([m[kk] for m in v])) for kk in keys} for a, v in by_action.items()}, "per_take": per}


def write_dynamics_metrics(results: dict, gt: dict, sim, result_dir: str, iter_num: int, data_file: str, dt=1.0 / 30.0, contacts: str = "soft") -> dict:
    """coverage_dynamics_metrics as `<result_dir>/dynamics_metrics_<iter>_<data_file>.json`; returns them.  contacts: "soft" | "estimated" | "both"."""
    import json
    import os
    m = coverage_dynamics_metrics(results, gt, sim, dt, contacts=contacts)
    os.makedirs(result_dir, exist_ok=True)
    with open(os.path.join(result_dir, f"dynamics_metrics_{iter_num}_{data_file}.json"), "w") as f:
        json.dump(m, f, indent=1)
    return m


BALANCE_KEYS = ("com_margin", "xcom_margin", "zmp_margin", "stable_frac", "airborne_frac", "zmp_out_mean")


def coverage_balance_metrics(results: dict, gt: dict, sim, dt=1.0 / 30.0) -> dict:
    """Balance score of pose sequences that were never simulated: balance.balance_sequence (one KpSim.body_motion and one
    KpSim.inverse_dynamics call over all rows; dynamics.motion_derivatives inside the takes) of the predicted (`pred`, its first 76 columns) and the
    ground-truth trajectory of every take of a `*_coverage_full.pkl` dict, on the FLOOR scene (the support polygon is the hull of the floor contacts; a
    seat carries nothing here).  Takes are cut to n = min(len(pred), len(gt qpos)), n >= 3.  Per side (pred / gt) and take: the means over the frames
    with floor contact of com_margin_*, xcom_margin_*, zmp_margin_* (m, positive inside the polygon), and stable_frac_*, airborne_frac_*,
    zmp_out_mean_* (balance.balance).  Returns their means over the takes (NaN-aware), 'by_action' (the same per action prefix) and 'per_take'."""
    from . import balance
    takes, q_rows, off = [], [], [0]
    for k, r in results.items():
        if k not in gt:
            continue
        pred, g = np.asarray(r["pred"], np.float64)[:, :76], np.asarray(gt[k]["qpos"], np.float64)[:, :76]
        n = min(len(pred), len(g))
        if n < 3:
            continue
        takes.append((k, n))
        for side in (pred[:n], g[:n]):
            q_rows.append(side); off.append(off[-1] + n)
    keys = [f"{a}_{b}" for a in BALANCE_KEYS for b in ("pred", "gt")]
    if not takes:
        return {"per_take": {}, "by_action": {}}
    fr = balance.balance_sequence(sim, np.concatenate(q_rows).astype(np.float32), dt, take_off=off)

    def nanmean(x):
        x = np.asarray(x, np.float64)
        x = x[np.isfinite(x)]
        return float(x.mean()) if len(x) else float("nan")

    per = {}
    for i, (k, n) in enumerate(takes):
        m = {}
        for j, side in enumerate(("pred", "gt")):
            rows = slice(off[2 * i + j], off[2 * i + j + 1])
            m.update({f"{a}_{side}": nanmean(fr[a][rows]) for a in BALANCE_KEYS[:3]})
            m.update({f"{a}_{side}": v for a, v in balance.summary(fr, rows).items()})
        per[k] = m
    by_action = {}
    for k, m in per.items():
        by_action.setdefault(k.split("-")[0], []).append(m)
    return {**{kk: nanmean([m[kk] for m in per.values()]) for kk in keys},
            "by_action": {a: {kk: nanmean([m[kk] for m in v]) for kk in keys} for a, v in by_action.items()}, "per_take": per}


def write_balance_metrics(results: dict, gt: dict, sim, result_dir: str, iter_num: int, data_file: str, dt=1.0 / 30.0) -> dict:
    """coverage_balance_metrics as `<result_dir>/balance_metrics_<iter>_<data_file>.json`; returns them"""
    import json
    import os
    m = coverage_balance_metrics(results, gt, sim, dt)
    os.makedirs(result_dir, exist_ok=True)
    with open(os.path.join(result_dir, f"balance_metrics_{iter_num}_{data_file}.json"), "w") as f:
        json.dump(m, f, indent=1)
    return m


def grf_metrics(results: dict, weight: float) -> dict:
    """Ground-reaction summary of an evaluation run with grf=True (kinpoly_amd.evaluate): over all recorded frames of all sequences,
        grf_mean_bw / grf_peak_bw   mean and peak of the feet's total vertical force sum_feet F_z / weight (weight = m g in N, contact.body_weight)
        no_support / double_support share of frames with no foot / both feet in contact (foot_contact)
        frames                      frames counted
    Sequences recorded without grf are refused."""
    fz, sup = [], []
    for k, r in results.items():
        if "grf" not in r or "foot_contact" not in r:
            raise KeyError(f"grf_metrics: sequence {k!r} has no grf record (run the evaluation with grf=True)")
        fz.append(np.asarray(r["grf"], np.float64)[:, :, 2].sum(1)); sup.append(np.asarray(r["foot_contact"], bool))
    fz, sup = np.concatenate(fz) if fz else np.zeros(0), np.concatenate(sup) if sup else np.zeros((0, 2), bool)
    if len(fz) == 0:
        return {"grf_mean_bw": float("nan"), "grf_peak_bw": float("nan"), "no_support": float("nan"), "double_support": float("nan"), "frames": 0}
    return {"grf_mean_bw": float(fz.mean() / weight), "grf_peak_bw": float(fz.max() / weight), "no_support": float((~sup.any(1)).mean()),
            "double_support": float(sup.all(1).mean()), "frames": int(len(fz))}


def write_grf_metrics(results: dict, weight: float, result_dir: str, iter_num: int, data_file: str) -> dict:
    """grf_metrics as `<result_dir>/grf_metrics_<iter>_<data_file>.json`; returns them"""
    import json
    import os
    m = grf_metrics(results, weight)
    os.makedirs(result_dir, exist_ok=True)
    with open(os.path.join(result_dir, f"grf_metrics_{iter_num}_{data_file}.json"), "w") as f:
        json.dump(m, f, indent=1)
    return m
