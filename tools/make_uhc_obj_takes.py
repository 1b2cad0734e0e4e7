"""Write tests/golden/uhc_obj_takes_small.pkl: a small take pickle in the schema DatasetSMPLObj reads ({take: {qpos [T,76], obj_pose [T,7] or
[T,14], action_one_hot [T,4]}}), from this project's own synthetic_takes(with_objects=True): one take per action, a second push take and one take
without an action, 95 to 130 frames, joint amplitude at most 0.05 rad (a standing controller survives a few control steps on them).

Two edits on top of synthetic_takes, both so that a wrongly placed object shows in a test after one control step:
  - every object is lifted 2 cm above its rest height, so it falls (and has a velocity) in the first control step;
  - the avoid take's can stands beside the left shin at frame 0, its wall 1.1 cm short of the shin's axis, so the first collision pass finds a
    contact between the leg and the can.

synthetic_takes asks its simulator for forward kinematics only; here that is the fp64 oracle's (oracle/np_oracle.py) on the host, so the tool needs no
GPU.  Arrays, names and numbers only.

    python tools/make_uhc_obj_takes.py [--out PATH]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "uhc_obj_takes_small.pkl")
LIFT = 0.02
CAN_RADIUS, CAN_GEOM_XY = 0.279, (-0.031, 0.004)     # the Can's cylinder in its body frame (humanoid_smpl_neutral_mesh_all.xml)
CAN_AXIS_TO_SHIN = 0.29
L_KNEE, L_ANKLE, R_KNEE = 2, 3, 6


class HostFk:
    """what synthetic_takes needs of a KpSim: `device` and `fk(qpos_rows)`, the latter from the fp64 oracle"""

    def __init__(self):
        import torch
        from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
        kpm = read_kpm(DEFAULT_KPM)
        self.device = torch.device("cpu")
        self.body_pos, self.body_ipos = np.asarray(kpm["body_pos"], float).reshape(24, 3), np.asarray(kpm["body_ipos"], float).reshape(24, 3)
        self.parent = [int(p) for p in np.asarray(kpm["body_parent"]).reshape(-1)]

    def fk(self, qpos_rows):
        import torch
        from oracle.np_oracle import qpos_fk
        rows = [qpos_fk(r, self.body_pos, self.body_ipos, self.parent) for r in qpos_rows.double().numpy()]
        return {k: torch.tensor(np.stack([r[k].reshape(-1) for r in rows]), dtype=torch.float32) for k in ("qpos", "wbpos", "wbquat", "bquat", "body_com")}


def make_takes():
    from kinpoly_amd.dataset import synthetic_takes
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))["qpos"].reshape(-1)[:76].astype(np.float64)
    sim = HostFk()
    with_obj = synthetic_takes(sim, std, n_per_action=2, T_range=(95, 131), seed=7, with_objects=True, amp_max=0.05)
    without = synthetic_takes(sim, std, n_per_action=1, T_range=(95, 131), seed=8, with_objects=False, amp_max=0.05)
    picked = {k: with_obj[k] for k in ("sit-synthetic-00", "push-synthetic-00", "avoid-synthetic-00", "step-synthetic-00", "push-synthetic-01")}
    picked["none-synthetic-sit-00"] = without["none-synthetic-sit-00"]
    takes = {}
    for name, f in picked.items():
        obj = np.array(f["obj_pose"], np.float64)
        if name.startswith("avoid"):
            wb = np.asarray(f["wbpos"], np.float64)[0].reshape(24, 3)
            lat = wb[L_KNEE, :2] - wb[R_KNEE, :2]
            lat /= np.linalg.norm(lat)
            axis = 0.5 * (wb[L_KNEE, :2] + wb[L_ANKLE, :2]) + CAN_AXIS_TO_SHIN * lat          # the cylinder's axis, outside the left leg
            yaw = 2.0 * np.arctan2(obj[0, 6], obj[0, 3])
            c, s = np.cos(yaw), np.sin(yaw)
            gx, gy = CAN_GEOM_XY
            obj[:, 0], obj[:, 1] = axis[0] - (c * gx - s * gy), axis[1] - (s * gx + c * gy)
        if not name.startswith("none"):
            obj[:, 2::7] += LIFT
        takes[name] = {"qpos": np.asarray(f["qpos"], np.float32), "obj_pose": obj.astype(np.float32), "action_one_hot": np.asarray(f["action_one_hot"], np.float32)}
    return takes


if __name__ == "__main__":
    import joblib
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    takes = make_takes()
    joblib.dump(takes, out, compress=3)
    for k, v in takes.items():
        print(k, v["qpos"].shape, v["obj_pose"].shape, v["action_one_hot"][0])
    print(os.path.getsize(out), "bytes")
