"""fp64 reference of the contact-force read-out (kp_sim_contact_forces), composed from OracleSim's own forward pass: test infrastructure.

oracle_contact_forces(osim, mode, act, target_qpos) sets the actuation up, calls osim.forward() and derives what the kernel reports from efc_force, the
contact list and the solve.  The caller puts the state in first: for the stale controller (mode 2 on a default handle) with
`osim.reset(qpos_d, qvel_d); osim.set_state_raw(qpos, qvel)`, the counterpart of kp_sim_set_full_state.
"""
import numpy as np

from np_rigid import make_frame  # noqa: F401  (the tests reach it through this module)

NB, NV, NU, MAXOBJ = 24, 75, 69, 2


def contact_forces_from_efc(efc_force, contacts, mu):
    """f_c [ncon, 3] (world, on the entity carrying the vertex) from the pyramid rows: limit rows first, then 4 rows per contact in contact order
    (kpo_make_constraint); row e of a contact pushes along n + sgn mu t with t = t1 (e < 2) or t2, sgn = + (e even) / - (e odd)"""
    ncon = len(contacts["body"])
    nlim = len(efc_force) - 4 * ncon
    f = np.zeros((ncon, 3))
    for c in range(ncon):
        fr = make_frame(contacts["normal"][c])
        for e in range(4):
            f[c] += efc_force[nlim + 4 * c + e] * (fr[0] + (-1.0 if e & 1 else 1.0) * mu * fr[1 + e // 2])
    return f, nlim


def entity_wrenches(contacts, f):
    """[26, 6]: force and torque about the world origin per entity; + on A, - on an object-slot B"""
    w = np.zeros((NB + MAXOBJ, 6))
    for c in range(len(f)):
        a, b = int(contacts["body"][c]), int(contacts["b2"][c])
        w[a, :3] += f[c]; w[a, 3:] += np.cross(contacts["pos"][c], f[c])
        if b >= NB:
            w[b, :3] -= f[c]; w[b, 3:] -= np.cross(contacts["pos"][c], f[c])
    return w


def oracle_contact_forces(osim, mode, act, target_qpos, kpm=None):
    """mode 0: no actuation; 1: act [75] = qfrc_applied[0:6] ++ ctrl[69]; 2: act = a cc_action row [75] of the default controller, target_qpos [76] its
    PD base pose.  kpm: the dict of the blob osim runs (torque limits, friction; default: the shipped one).  Returns dict(contacts, force [ncon,3], wrench [26,6], qfrc_constraint [75], qacc [75],
    torque [75], obj_qacc [2,6], nlim, efc_force, J)."""
    if kpm is None:
        from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
        kpm = read_kpm(DEFAULT_KPM)
    if mode == 0:
        osim.set_ctrl(np.zeros(NU), np.zeros(6))
    elif mode == 1:
        act = np.asarray(act, float)
        osim.set_ctrl(act[6:NV], act[:6])
    else:
        act = np.asarray(act, float)
        tau = osim.compute_torque(act[:NU], target_qpos)
        lim = np.asarray(kpm["torque_lim"], float)
        osim.set_ctrl(np.clip(tau, -lim, lim))
        osim.rfc_implicit(act[NU:NU + 6])
    return oracle_forward_forces(osim, kpm)


def oracle_forward_forces(osim, kpm):
    """forward() on the actuation osim holds, then the derived quantities"""
    osim.forward()
    efc_force = osim.efc()[0]
    con = osim.contacts_full()
    f, nlim = contact_forces_from_efc(efc_force, con, float(kpm["opt"][11]))
    return dict(contacts=con, force=f, wrench=entity_wrenches(con, f), qfrc_constraint=osim.get("qfrc_constraint"), qacc=osim.get("qacc"),
                torque=np.concatenate([osim.get("qfrc_applied")[:6], osim.get("ctrl")]), obj_qacc=osim.qacc_full()[NV:NV + 6 * MAXOBJ].reshape(MAXOBJ, 6),
                nlim=nlim, efc_force=efc_force, J=osim.efc_J_full())


def match_contacts(got, ref):
    """pairs (i_got, i_ref) matched by (A, B) and nearest point, each contact used once; the unmatched indices of both sides.
    got / ref: dict(body, b2, pos)"""
    pairs, used = [], set()
    for i in range(len(got["body"])):
        best, bd = -1, np.inf
        for j in range(len(ref["body"])):
            if j in used or int(ref["body"][j]) != int(got["body"][i]) or int(ref["b2"][j]) != int(got["b2"][i]):
                continue
            d = np.linalg.norm(np.asarray(ref["pos"][j]) - np.asarray(got["pos"][i]))
            if d < bd:
                best, bd = j, d
        if best >= 0:
            pairs.append((i, best)); used.add(best)
    gi = {p[0] for p in pairs}
    return pairs, [i for i in range(len(got["body"])) if i not in gi], [j for j in range(len(ref["body"])) if j not in used]


# ---------------------------------------------------------------- the named states of the GPU tests (built on the host, checked on the oracle side)

def hull_world_verts(kpm, qpos, bodies):
    """world vertices of the hulls of `bodies` at qpos (oracle FK)"""
    from oracle import np_oracle as O
    fk = O.qpos_fk(qpos, kpm["body_pos"].reshape(24, 3), kpm["body_ipos"].reshape(24, 3), kpm["body_parent"])
    verts, vadr = kpm["verts"].reshape(-1, 3), kpm["vert_adr"]
    return np.concatenate([fk["wbpos"][b] + verts[vadr[b]:vadr[b + 1]] @ O.quaternion_matrix3(fk["wbquat"][b]).T for b in bodies])


def floor_states(kpm, std_qpos, std_qvel):
    """name -> (qpos, qvel) of the object-free states (a), (c), (d), (e), (f); (b) comes from the device.  fp64 here, rounded to fp32 by the caller."""
    from oracle import np_oracle as O
    out = {"a_standing": (np.array(std_qpos, float), np.array(std_qvel, float))}
    q = np.array(std_qpos, float); q[2] += 1.0
    out["c_airborne"] = (q, np.array(std_qvel, float))
    q = np.array(std_qpos, float)
    q[3:7] = O.quaternion_multiply(np.array([np.cos(np.pi / 4), np.sin(np.pi / 4), 0.0, 0.0]), q[3:7])          # root rotated 90 degrees about x
    q[2] = 0.0
    lows = np.sort([hull_world_verts(kpm, q, (b,))[:, 2].min() for b in range(24)])
    q[2] = -lows[9]                                                          # the tenth-lowest hull just reaches the floor: the lower ones press into it
    out["d_lying"] = (q, np.zeros(75))
    q = np.array(std_qpos, float); q[7 + 48] = np.pi + 0.2                   # an arm joint 0.2 rad past its +-pi limit
    out["e_limit"] = (q, np.array(std_qvel, float))
    rng = np.random.default_rng(77)
    q = np.array(std_qpos, float); q[7:] += rng.normal(size=69) * 0.2
    tilt = np.array([np.cos(0.35), np.sin(0.35) * 0.8, np.sin(0.35) * 0.6, 0.0])
    q[3:7] = O.quaternion_multiply(tilt, q[3:7])
    q[2] = 0.0
    q[2] = -0.003 - hull_world_verts(kpm, q, range(24))[:, 2].min()
    v = rng.uniform(-5.0, 5.0, 75); v[:3] = [0.4, -0.3, -1.5]
    out["f_falling"] = (q, v)
    return out


def parked_block():
    blk = np.zeros(35)
    for i in range(5):
        blk[7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    blk[3::7] = 1.0
    return blk


def object_scenes(kpm, std_qpos):
    """name -> (qpos, qvel, obj block [35], {slot: object index}) of the scenes (g) sit and (h) push"""
    out = {}
    # (g) hips flexed by 90 degrees, the pelvis and thigh hulls 4 mm into the chair's seat (top = chair origin + 0.02)
    q = np.array(std_qpos, float)
    q[7 + 2] = -np.pi / 2; q[7 + 12 + 2] = -np.pi / 2
    q[7 + 3 * 14 + 2] = np.pi / 2; q[7 + 3 * 19 + 2] = np.pi / 2          # arms raised forward, clear of the seat
    q[2] = 0.0
    low = hull_world_verts(kpm, q, (0, 1, 5))
    q[2] = 0.41 - 0.004 - low[:, 2].min()
    blk = parked_block(); blk[0:7] = [q[0], q[1] + 0.08, 0.39, 1, 0, 0, 0]   # 1 cm above the floor: the 100 t chair's own weight stays out of the forces
    out["g_sit"] = (q, np.zeros(75), blk, {0: 0})
    # (h) the box on the table (the push scene's heights), its near face 3 mm into the left hand's outermost vertex; the table shifted outwards so that
    # its slab stays clear of the hand
    q = np.array(std_qpos, float)
    hand = hull_world_verts(kpm, q, (18,))
    tipv = hand[np.argmin(hand[:, 0])]                                       # the left hand's outermost vertex (the humanoid's left is -x)
    blk = parked_block()
    bx = tipv[0] + 0.003 - 0.15
    blk[7:14] = [bx, tipv[1], 0.921, 1, 0, 0, 0]
    blk[14:21] = [bx - 0.39, tipv[1], 0.7905, 1, 0, 0, 0]
    out["h_push"] = (q, np.zeros(75), blk, {0: 1, 1: 2})
    return out
