"""What the cost tools of the rows kernels share (inverse_dynamics_bench, estimate_contacts_bench, body_motion_bench, fit_pose_bench,
contact_force_bench, push_bench): event-timed blocks of calls, the printed line, and the scenes the rows are taken from."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from kinpoly_amd import sim as kpsim  # noqa: E402

std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
dev = torch.device("cuda", 0)
t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731


def blocks(fn, reps, nblocks=5):
    """(median, min, max) over nblocks of (event time of reps calls) / reps, in ms"""
    out = []
    for _ in range(nblocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out), max(out)


def timed(label, fn, rows, reps, base=None, of="inverse_dynamics", width=58, wide=0, warm=5):
    """warm-up, blocks(), one printed line (label padded to `width`; wide: one more column in every number, as fit_pose_bench prints) -> the median.
    base: the median the line is compared with, `of` its name."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    med, lo, hi = blocks(fn, reps)
    tail = "" if base is None else f"   = {med / base:{5 + wide}.2f} x {of}"
    print(f"{label:{width}s} {med:{8 + wide}.4f} ms   ({lo:.4f} .. {hi:.4f})   {rows / med * 1e3 / 1e6:7.{2 + wide}f} M rows/s{tail}")
    return med


def settled_floor(n, rng, blob=None, blk=None):
    """n standing poses with joint noise under a random action, settled by 10 control steps -> (handle, action).  blk: object rows [n, 35] to set first."""
    qpos = np.tile(std["qpos"], (n, 1)); qpos[:, 7:] += rng.normal(size=(n, 69)) * 0.1
    sim = kpsim.KpSim(kpsim.KpModel(kpsim.DEFAULT_KPM if blob is None else blob), n)
    if blk is not None:
        sim.set_objects(t(blk))
    sim.set_state(t(qpos), t(rng.normal(size=(n, 75)) * 0.3)); sim.set_target(t(np.tile(std["qpos"], (n, 1))))
    act = t(rng.normal(size=(n, 75)) * 0.2)
    for _ in range(10):
        sim.step_ctrl(act, 15)
    return sim, act


def motion_scene(scene, n, rng):
    """(handle holding n states, obj_qpos rows or None).  floor: settled_floor; sit: the sit pose of tests/contact_force_oracle.py with joint noise, the chair
    a static obstacle under the pelvis (static in the read-out too: the same problem)."""
    if scene == "floor":
        return settled_floor(n, rng)[0], None
    import contact_force_oracle as CF
    from kinpoly_amd.model_compiler import read_kpm
    q, v, blk, _ = CF.object_scenes(read_kpm(kpsim.STEP_KPM), std["qpos"])["g_sit"]
    qpos = np.tile(q, (n, 1)); qpos[:, 7 + 12:] += rng.normal(size=(n, 57)) * 0.05          # the legs stay as they sit
    sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM, dynamic_objects=0), n)
    obj = t(np.tile(blk, (n, 1)))
    sim.set_objects(obj)
    sim.set_state(t(qpos), t(rng.normal(size=(n, 75)) * 0.3))
    return sim, obj
