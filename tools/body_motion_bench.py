"""What the body-motion read-out costs: rows/s of kp_sim_body_motion at R = 4096 and R = 65536, `centroid` alone and all four
outputs, next to kp_sim_inverse_dynamics (floor, qfrc_inverse alone) on the SAME rows in the same run.  body_motion does a strict subset of that kernel's
work (the forward pass and one spatial_accumulate; no collide, no make_constraint, no row evaluation, no projection) on a smaller LDS block, so it
should not be the slower one.  Device events around blocks of calls, medians of 5 blocks after a warm-up.  States: standing poses with joint noise,
settled by 10 control steps; qacc = the accelerations the contact read-out solved for.
    python tools/body_motion_bench.py"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from kinpoly_amd import sim as kpsim  # noqa: E402

N = 4096
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


def timed(label, fn, rows, reps, base=None):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    med, lo, hi = blocks(fn, reps)
    tail = "" if base is None else f"   = {med / base:5.2f} x inverse_dynamics"
    print(f"{label:58s} {med:8.4f} ms   ({lo:.4f} .. {hi:.4f})   {rows / med * 1e3 / 1e6:7.2f} M rows/s{tail}")
    return med


print("# ms per call, median (min .. max) of 5 blocks; the same rows for every line of a size")
rng = np.random.default_rng(0)
qpos = np.tile(std["qpos"], (N, 1)); qpos[:, 7:] += rng.normal(size=(N, 69)) * 0.1
sim = kpsim.KpSim(kpsim.KpModel(kpsim.DEFAULT_KPM), N)
sim.set_state(t(qpos), t(rng.normal(size=(N, 75)) * 0.3)); sim.set_target(t(np.tile(std["qpos"], (N, 1))))
act = t(rng.normal(size=(N, 75)) * 0.2)
for _ in range(10):
    sim.step_ctrl(act, 15)
q, v = sim.get("qpos").clone(), sim.get("qvel").clone()
a = sim.contact_forces(want=("qacc",))["qacc"].clone()
for mult, reps in ((1, 20), (16, 5)):
    R = mult * N
    qr, vr, ar = (x.repeat(mult, 1) for x in (q, v, a))
    base = timed(f"inverse_dynamics, floor, qfrc_inverse only, R = {R}", lambda: sim.inverse_dynamics(qr, vr, ar), R, reps)
    timed(f"body_motion, centroid only, R = {R}", lambda: sim.body_motion(qr, vr, ar, outputs=("centroid",)), R, reps, base)
    timed(f"body_motion, all outputs, R = {R}", lambda: sim.body_motion(qr, vr, ar), R, reps, base)
    timed(f"body_motion, body_vel only (no qacc), R = {R}", lambda: sim.body_motion(qr, vr, outputs=("body_vel",)), R, reps, base)
