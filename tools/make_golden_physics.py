"""Generate tests/golden/physics_metrics.npz by RUNNING the reference's own physics metrics (needs a checkout of the reference KinPoly tree).

The text of compute_physcis_metris, compute_foot_sliding, contiguous_regions and compute_obj_interact (with their helper get_body_part) is read
from scripts/eval_pose_all.py and executed here; nothing of it is stored.  Their `env` is a stub whose sim.forward() runs this repo's fp64
OracleSim on the frame (reset(qpos[:76], 0) with set_geoms(object_geoms(kpm, qpos[76:]))) and fills data.contact with the oracle's contacts in
the reference's geom ids (tests/pose_oracle.py), body_xpos / body_xquat with the oracle's body poses.

    python tools/make_golden_physics.py <path of the reference KinPoly checkout>

The fixture (data only, 13 takes of 30 frames: sit, push, avoid, step, None, a fail-safe take, a sunk / sliding take, an unknown action) holds
the takes' inputs, the oracle's per-frame pen / ncon / hit masks / toe and head positions, and the reference's pen, slide and succ of the
predicted and the ground-truth run; tests/test_physics_metrics_cpu.py and tests/test_gpu_pose_contacts.py read it.
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "physics_metrics.npz")
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from kinpoly_amd.model_compiler import STEP_KPM, read_kpm  # noqa: E402
from oracle import np_oracle as O  # noqa: E402
from oracle.kpo import OracleSim  # noqa: E402
from tests.pose_oracle import oracle_frame  # noqa: E402

T = 30
BODY_IDS = {"Pelvis": 1, "L_Toe": 5, "R_Toe": 9, "Head": 14}     # MuJoCo body ids of the reference's model (world = 0)


class StubEnv:
    qpos_lim = 76

    def __init__(self, kpm):
        self.kpm, self.o = kpm, OracleSim(kpm=STEP_KPM)
        self.model = types.SimpleNamespace(_body_name2id=BODY_IDS)
        self.data = types.SimpleNamespace(qpos=np.zeros(111), contact=[], ncon=0, body_xpos=np.zeros((25, 3)), body_xquat=np.zeros((25, 4)))
        self.sim = types.SimpleNamespace(forward=self._forward)
        self.frames = []

    def reset(self):
        pass

    def _forward(self):
        f = oracle_frame(self.o, self.kpm, self.data.qpos[:76].copy(), self.data.qpos[76:].copy())
        self.data.contact = [types.SimpleNamespace(geom1=g1, geom2=g2, dist=d) for g1, g2, d in f["contacts"]]
        self.data.ncon = len(self.data.contact)
        self.data.body_xpos = np.concatenate([np.zeros((1, 3)), f["xpos"]])
        self.data.body_xquat = np.concatenate([[[1.0, 0, 0, 0]], f["xquat"]])
        self.frames.append(f)

    def get_wbody_pos(self):
        return self.data.body_xpos[1:].reshape(-1).copy()


def parked():
    blk = np.zeros(35)
    for i in range(5):
        blk[7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    return blk


def takes(std, kpm, rng):
    x0, y0 = std[0], std[1]
    fk = O.qpos_fk(std, kpm["body_pos"].reshape(24, 3), kpm["body_ipos"].reshape(24, 3), kpm["body_parent"])
    verts, vadr = kpm["verts"].reshape(-1, 3), kpm["vert_adr"]
    hull = lambda b: fk["wbpos"][b] + verts[vadr[b]:vadr[b + 1]] @ O.quaternion_matrix3(fk["wbquat"][b]).T  # noqa: E731
    tip = max(hull(b)[:, 0].max() for b in (4, 8))
    hip_z = min(hull(b)[:, 2].min() for b in (0,))
    out = []

    def take(name, obj=None, lift=0.0, rise=0.0, dx=0.0, sink=None, fail_safe=False, head_off=0.0, moving=None):
        q = np.tile(std, (T, 1))
        q[:, 2] += lift + np.linspace(0.0, rise, T)
        q[:, 0] += np.arange(T) * dx
        if sink is not None:
            q[sink, 2] -= 0.04
        blk = np.tile(parked(), (T, 1))
        for oi, pose in (obj or {}).items():
            blk[:, 7 * oi: 7 * oi + 7] = pose
        if moving is not None:
            blk[:, 7:10] += np.linspace(0.0, 1.0, T)[:, None] * moving
        g = q.copy()
        g[:, 7:] += rng.normal(size=(T, 69)) * 0.02
        out.append(dict(name=name, pred=q.astype(np.float32), gt=g.astype(np.float32), obj=blk.astype(np.float32), fail_safe=fail_safe, head_off=head_off))

    take("sit-seat", {0: [x0, y0, hip_z - 0.02 + 0.18 - 0.2 + 0.2, 1, 0, 0, 0]})                 # seat block 2 cm into the pelvis / thighs
    take("sit-brush", {0: [tip + 0.209 - 0.004, y0, 0.38, 1, 0, 0, 0]})                          # seat block 4 mm into the toe tips only
    take("push-moved", {1: [x0 + 1.0, y0, 0.22, 1, 0, 0, 0]}, moving=[0.15, 0, 0])
    take("push-nudged", {1: [x0 + 1.0, y0, 0.22, 1, 0, 0, 0]}, moving=[0.05, 0, 0])
    take("avoid-legs", {3: [x0 + 0.36, y0 + 0.05, 0.69, 1, 0, 0, 0]})                           # Can against the legs
    take("avoid-headoff", {3: [x0 + 3.0, y0, 0.69, 1, 0, 0, 0]}, head_off=0.6)
    take("avoid-clear", {3: [x0 + 3.0, y0, 0.69, 1, 0, 0, 0]})
    take("step-up", {4: [x0, y0, 0.3705, 1, 0, 0, 0]}, lift=0.341 - 0.004, rise=0.15)            # on the step box (top at 0.3405), pelvis rising
    take("step-flat", {4: [x0, y0, 0.3705, 1, 0, 0, 0]}, lift=0.341 - 0.004)
    take("None-standing")
    take("push-failsafe", {1: [x0 + 1.0, y0, 0.22, 1, 0, 0, 0]}, moving=[0.15, 0, 0], fail_safe=True)
    take("None-sunk", dx=0.01, sink=slice(10, 20))                                               # sliding feet, ten frames 4 cm into the floor
    take("dance-1")                                                                               # an action prefix the reference does not know
    return out


def main():
    kpm = read_kpm(STEP_KPM)
    std = np.load(os.path.join(REPO, "tests", "golden", "standing_neutral.npz"))["qpos"].astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(4321)
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    src = open(os.path.join(sys.argv[1], "scripts", "eval_pose_all.py")).read()
    env = StubEnv(kpm)
    ns = {"np": np, "env": env}
    exec(src[src.index("def get_body_part"):src.index("class kin_polyVisulizer")], ns)          # the functions' own text, run here, nothing of it is stored
    rec = {k: [] for k in ("pen_pred", "pen_gt", "slide_pred", "slide_gt", "succ_pred", "succ_gt")}
    frames = {"pred": [], "gt": []}
    tk = takes(std, kpm, rng)
    head_gt_all = []
    for t in tk:
        env.frames = []
        # the data set's head pose: the ground truth's own head (its body_xpos / body_xquat), shifted on the take that must fail on it
        for fr in range(T):
            env.data.qpos[:76] = t["gt"][fr]; env.data.qpos[76:] = t["obj"][fr]; env.sim.forward()
        head_gt = np.stack([np.concatenate([f["xpos"][13], f["xquat"][13]]) for f in env.frames])
        head_gt[:, 0] += t["head_off"]
        head_gt_all.append(head_gt)
        env.frames = []
        res = {"fail_safe": t["fail_safe"]}
        obj = t["obj"].astype(np.float64)
        pp, sp, _, _, cp = ns["compute_physcis_metris"](t["pred"].astype(np.float64), obj, head_pose_gt=head_gt, take=t["name"], res=res)
        frames["pred"] += env.frames; env.frames = []
        pg, sg, _, _, cg = ns["compute_physcis_metris"](t["gt"].astype(np.float64), obj, head_pose_gt=head_gt, take=t["name"], res=None)
        frames["gt"] += env.frames; env.frames = []
        for k, v in zip(rec, (pp, pg, sp, sg, cp, cg)):
            rec[k].append(float(v))
        print(f"{t['name']:14s} pen {pp:8.3f} {pg:8.3f} slide {sp:7.3f} {sg:7.3f} succ {cp} {cg} ncon max {max(f['ncon'] for f in frames['pred'][-T:])}")
    per = {}
    for side in ("pred", "gt"):
        fs = frames[side]
        per[f"frame_pen_{side}"] = np.array([f["pen"] for f in fs])
        per[f"frame_ncon_{side}"] = np.array([f["ncon"] for f in fs], np.int32)
        per[f"frame_hits_{side}"] = np.stack([f["hits"] for f in fs]).astype(np.uint32)
        per[f"frame_toes_{side}"] = np.stack([f["xpos"][[4, 8]] for f in fs])
        per[f"frame_head_{side}"] = np.stack([f["xpos"][13] for f in fs])
    np.savez_compressed(OUT, names=np.array([t["name"] for t in tk]), T=T, kpm="step",
                        qpos_pred=np.concatenate([t["pred"] for t in tk]), qpos_gt=np.concatenate([t["gt"] for t in tk]),
                        obj_pose=np.concatenate([t["obj"] for t in tk]), head_pose_gt=np.concatenate(head_gt_all),
                        fail_safe=np.array([t["fail_safe"] for t in tk]), **per, **{k: np.array(v) for k, v in rec.items()})
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
