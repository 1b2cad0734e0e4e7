"""fp64 reference of the inverse dynamics (kp_sim_inverse_dynamics), composed from OracleSim's own forward pass: test infrastructure.

For a state (qpos, qvel, optional object block whose unparked objects are STATIC geoms) the oracle's forward() leaves the constraint rows (J, D, aref), the
mass matrix and the bias force.  For a given qacc the soft-constraint inverse is closed form:
    jar = J qacc - aref,   fr = -D min(jar, 0),   qfrc_inverse = M qacc + qfrc_bias - J^T fr.
tests/test_inverse_dynamics_cpu.py shows that this is an inverse of the oracle's own forward (feeding qfrc_inverse back returns qacc).
"""
import numpy as np

import contact_force_oracle as CF
from np_rigid import f32  # noqa: F401  (the tests reach it through this module)
from oracle.kpo import OracleSim, object_geoms

NV, NU = 75, 69


def prepared(kpm_path, kpm, qpos, qvel, blk=None):
    """an OracleSim holding the state, the block's unparked objects as static geoms, no actuation, forward() done"""
    o = OracleSim(kpm=kpm_path, ls_exact=True)
    if blk is not None:
        o.set_geoms(object_geoms(kpm, blk))
    o.set_ctrl(np.zeros(NU), np.zeros(6))
    o.reset(qpos, qvel)                      # keeps the geoms; ends with forward()
    return o


def compose(o, kpm, qacc):
    """the inverse at `qacc` [75] from the rows forward() left in `o`.  Returns dict(qfrc_inverse, qfrc_constraint, qfrc_bias [75], contacts, force
    [ncon, 3], net_wrench [6], ncon, nlim, fr, jar, D)."""
    qacc = np.asarray(qacc, float)
    _, D, aref, J = o.efc()
    M, bias = o.fullM(), o.get("qfrc_bias")
    jar = J @ qacc - aref
    fr = -D * np.minimum(jar, 0.0)
    qc = J.T @ fr if len(fr) else np.zeros(NV)
    con = o.contacts_full()
    f, nlim = CF.contact_forces_from_efc(fr, con, float(kpm["opt"][11]))
    net = np.zeros(6)
    for c in range(len(f)):
        net[:3] += f[c]; net[3:] += np.cross(con["pos"][c], f[c])
    return dict(qfrc_inverse=M @ qacc + bias - qc, qfrc_constraint=qc, qfrc_bias=bias, contacts=con, force=f, net_wrench=net, ncon=len(f), nlim=nlim,
                fr=fr, jar=jar, D=D)


def qacc_choices(o, name):
    """the three accelerations of a state: zero, the state's own forward qacc (no actuation), seeded N(0, 30^2)"""
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    return {"zero": np.zeros(NV), "forward": o.get("qacc").copy(), "random": rng.normal(size=NV) * 30.0}


def falling_state(kpm, std_qpos, seed):
    """f_falling's recipe (contact_force_oracle.floor_states) with another seed"""
    from oracle import np_oracle as O
    rng = np.random.default_rng(seed)
    q = np.array(std_qpos, float); q[7:] += rng.normal(size=69) * 0.2
    tilt = np.array([np.cos(0.35), np.sin(0.35) * 0.8, np.sin(0.35) * 0.6, 0.0])
    q[3:7] = O.quaternion_multiply(tilt, q[3:7])
    q[2] = 0.0
    q[2] = -0.003 - CF.hull_world_verts(kpm, q, range(24))[:, 2].min()
    v = rng.uniform(-5.0, 5.0, 75); v[:3] = [0.4, -0.3, -1.5]
    return q, v


SWEEP_SEEDS = tuple(range(1000, 1064))       # the 64 falling states of the GPU sweep
MARGIN_OPT = 14                              # kpm["opt"] index of the contact margin (model_compiler.OPT_FIELDS)


def named_states(kpm_floor, kpm_step, std_qpos, std_qvel):
    """list of dict(name, q, v, blk, step) with fp32-representable values: contact_force_oracle's floor states and g_sit with the chair (static);
    step: the state needs the object blob"""
    out = [dict(name=k, q=f32(q), v=f32(v), blk=None, step=False) for k, (q, v) in CF.floor_states(kpm_floor, std_qpos, std_qvel).items()]
    q, v, blk, _ = CF.object_scenes(kpm_step, std_qpos)["g_sit"]
    q = q.copy(); q[2] -= 0.001              # as given, the left thigh sits 0.995 mm above the seat: 5e-6 from the 1 mm margin, an edge (on_edge); 1 mm deeper it is not
    out.append(dict(name="g_sit", q=f32(q), v=f32(v), blk=f32(blk), step=True))
    return out


def sweep_states(kpm_floor, std_qpos):
    out = []
    for seed in SWEEP_SEEDS:
        q, v = falling_state(kpm_floor, std_qpos, seed)
        out.append(dict(name=f"sweep_{seed}", q=f32(q), v=f32(v), blk=None, step=False))
    return out


def on_edge(o, kpm, res, margin):
    """Edge classification of a case (state + qacc): a fp32 kernel may legitimately land on the other side of a switch when
      * some row has |D jar| < 1e-3 N (a row about to switch on or off),
      * a contact's dist lies within 1e-5 of the margin (a contact about to appear or vanish),
      * two vertices of one hull tie in depth to 1e-6 (the plane-mesh contact may pick the other vertex).
    res: compose()'s result for the case."""
    if len(res["fr"]) and np.any(np.abs(res["D"] * res["jar"]) < 1e-3):
        return True
    con = res["contacts"]
    if len(con["dist"]) and np.any(np.abs(con["dist"] - margin) < 1e-5):
        return True
    q = o.get("qpos")
    for b in range(24):
        z = np.sort(CF.hull_world_verts(kpm, q, (b,))[:, 2])
        if z[0] <= margin + 1e-5 and len(z) > 1 and z[1] - z[0] < 1e-6:
            return True
    return False
