"""Write tests/golden/uhc_obj_takes.npz: what the reference's DatasetSMPLObj (uhc/data_loaders/dataset_smpl_obj.py) makes of
tests/golden/uhc_obj_takes_small.pkl.  The reference's class is IMPORTED from a reference checkout (the build container only, as tools/make_golden.py
does, with stub modules for what it imports but does not need); only recorded arrays and names are written.

    python tools/make_golden_uhc_obj.py [/path/to/reference]

The reference's argmax calls the all-zero action_one_hot of the one take without an action a sit take and puts its placeholder obj_pose (a chair at
the origin) into the block; SmplObjDataset parks everything for such a take instead.  iter_seq's records are the reference's as they come; for that take
`conv_<take>` records the reference's convert_obj_qpos with an action outside the four (everything parked), which is what SmplObjDataset is held to.
"""
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
PKL = os.path.join(OUT, "uhc_obj_takes_small.pkl")
sys.dont_write_bytecode = True


class Pkg(MagicMock):
    __path__ = []


def main():
    import joblib
    for m in ("cv2", "OpenGL", "OpenGL.GL", "gym", "gym.envs", "gym.envs.mujoco", "gym.envs.mujoco.mujoco_env", "gym.utils", "gym.spaces", "glfw", "torchvision",
              "torchvision.models", "torchvision.transforms", "skimage", "skimage.util", "skimage.util.shape", "mujoco_py", "mujoco_py.builder",
              "mujoco_py.generated", "mujoco_py.generated.const", "mujoco_py.utils", "mujoco_py.functions", "wandb", "lxml", "lxml.etree", "ipdb",
              "torchgeometry", "smplx", "imageio", "PIL", "tqdm", "uhc.smpllib.smpl_mujoco", "uhc.utils.transform_utils"):
        try:
            __import__(m)
        except Exception:
            sys.modules[m] = Pkg()
    sys.path.insert(0, REF)
    import uhc.data_loaders.dataset_smpl_obj as mod
    mod.tqdm = lambda it, *a, **k: it
    takes = joblib.load(PKL)
    no_action = [k for k, v in takes.items() if not np.any(np.asarray(v["action_one_hot"])[0] != 0)]
    out = {"take_names": np.array(list(takes.keys())), "no_action_takes": np.array(no_action)}
    with tempfile.TemporaryDirectory() as tmp:
        pkl, neutral = os.path.join(tmp, "takes.pkl"), os.path.join(tmp, "standing_neutral.pkl")
        joblib.dump(takes, pkl)
        joblib.dump({}, neutral)                       # the constructor loads the neutral-pose pickle and never reads it
        specs = {"file_path": pkl, "test_file_path": pkl, "has_smpl_root": True, "flip_cnd": 0, "flip_time": False, "neutral_path": neutral, "mode": "all"}
        for t_min in (90, 120):
            ds = mod.DatasetSMPLObj({**specs, "t_min": t_min}, data_mode="test")
            out[f"data_keys_tmin{t_min}"] = np.array(list(ds.data_keys))
        ds = mod.DatasetSMPLObj({**specs, "t_min": 90}, data_mode="train")
        for k in ds.data_keys:
            action = "none" if k in no_action else ds.data["action"][k]
            out[f"conv_{k}"] = np.asarray(ds.convert_obj_qpos(ds.data["obj_pose"][k], action), np.float64)
            out[f"action_{k}"] = np.array(action)
        order = []
        for i in range(len(ds.data_keys) + 2):            # once round and two takes more: the counter wraps
            s = ds.iter_seq()
            order.append(s["seq_name"])
            out[f"iter{i}_qpos"], out[f"iter{i}_obj_pose"] = np.asarray(s["qpos"], np.float64), np.asarray(s["obj_pose"], np.float64)
            out[f"iter{i}_has_obj"], out[f"iter{i}_num_obj"] = np.array(bool(s["has_obj"])), np.array(int(s["num_obj"]))
        out["iter_order"] = np.array(order)
    path = os.path.join(OUT, "uhc_obj_takes.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes;", order)


if __name__ == "__main__":
    main()
