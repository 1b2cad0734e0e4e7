"""The fp64 oracle's answer to the per-frame contact walk of compute_physcis_metris (scripts/eval_pose_all.py:205-260), for the pose-contact
tests and tools/make_golden_physics.py: OracleSim.reset (sim.forward) on the frame's qpos with the frame's object geoms, then its contact list.

The oracle marks every static geom's contact with the same entity (-1, as the floor), so the geom behind a contact is recovered from the
order of the list: per hull the floor contacts come first, then at most one contact per object geom in geom order (kpo_collide).  A run with
the floor alone and one run per active geom give those counts.
"""
from __future__ import annotations

import numpy as np

from oracle.kpo import OracleSim, object_geoms


def live_geoms(kpm: dict, blk35, max_dist=50.0):
    """model geom indices that object_geoms() places for this object block (objects parked past max_dist have none), in its order"""
    og = kpm["obj_geoms"].reshape(-1, 18)
    return [g for g in range(og.shape[0]) if np.linalg.norm(np.asarray(blk35, float)[7 * int(og[g, 0]): 7 * int(og[g, 0]) + 3]) <= max_dist]


def _per_body(o: OracleSim, geoms, qpos):
    o.set_geoms(geoms)
    o.reset(np.asarray(qpos, np.float64), np.zeros(75))
    c = o.contacts_full()
    return c, np.bincount(c["body"], minlength=24)


def oracle_frame(o: OracleSim, kpm: dict, qpos, blk35=None, pen_margin=0.005) -> dict:
    """dict(ncon, pen, hits [n_obj_geoms] (bit b: hull b touches geom g), contacts [(geom1, geom2, dist)] in the reference's geom ids
    (0 floor, 1 + body, 25 + geom), xpos [24, 3], xquat [24, 4]) of one frame."""
    n_og = kpm["obj_geoms"].reshape(-1, 18).shape[0]
    blk = np.zeros(35) if blk35 is None else np.asarray(blk35, np.float64)
    live = [] if blk35 is None else live_geoms(kpm, blk)
    allg = object_geoms(kpm, blk) if live else np.zeros((0, 17))
    assert len(allg) == len(live)
    _, nfloor = _per_body(o, np.zeros((0, 17)), qpos)
    hit = np.zeros((len(live), 24), bool)
    for j in range(len(live)):
        _, n = _per_body(o, allg[j:j + 1], qpos)
        assert np.all((n - nfloor == 0) | (n - nfloor == 1))
        hit[j] = n - nfloor == 1
    c, n = _per_body(o, allg, qpos)
    assert len(c["body"]) < 64, "the oracle keeps at most 64 contacts (MAXCON): this frame may have lost some"
    assert np.array_equal(n, nfloor + hit.sum(0))
    geom1 = np.zeros(len(c["body"]), int)
    for b in range(24):
        idx = np.nonzero(c["body"] == b)[0]
        geom1[idx[nfloor[b]:]] = [25 + live[j] for j in np.nonzero(hit[:, b])[0]]
    hits = np.zeros(n_og, np.uint32)
    for j, g in enumerate(live):
        hits[g] = sum(1 << b for b in np.nonzero(hit[j])[0])
    pen = float(np.sum(np.maximum(0.0, -c["dist"] - pen_margin))) if len(c["dist"]) else 0.0
    return dict(ncon=len(c["body"]), pen=pen, hits=hits, contacts=[(int(geom1[i]), int(c["body"][i]) + 1, float(c["dist"][i])) for i in range(len(geom1))],
                xpos=o.get("xpos").reshape(24, 3), xquat=o.get("xquat").reshape(24, 4))
