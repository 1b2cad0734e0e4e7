"""What inverse dynamics costs: rows/s of kp_sim_inverse_dynamics at R = 4096 and R = 65536 on the floor scene and at R = 4096
on the sit scene (the chair a static obstacle under the pelvis), next to kp_sim_contact_forces mode 0 on the SAME 4096 states in the same run: both do
the same forward pass, collide and make_constraint on the same layout; the read-out then runs the Newton solve, the inverse one gradient evaluation.
Device events around blocks of calls, medians of 5 blocks after a warm-up.  Floor states: standing poses with joint noise, settled by 10 control steps;
qacc = the accelerations the read-out solved for.  Sit states: the sit pose of tests/contact_force_oracle.py with joint noise.
    python tools/inverse_dynamics_bench.py"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import contact_force_oracle as CF  # noqa: E402
from kinpoly_amd import sim as kpsim  # noqa: E402
from kinpoly_amd.model_compiler import read_kpm  # noqa: E402

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
    tail = "" if base is None else f"   = {med / base:5.2f} x the read-out"
    print(f"{label:58s} {med:8.4f} ms   ({lo:.4f} .. {hi:.4f})   {rows / med * 1e3 / 1e6:7.2f} M rows/s{tail}")
    return med


print(f"# ms per call, median (min .. max) of 5 blocks; {N} states per scene")
rng = np.random.default_rng(0)
for scene in ("floor", "sit"):
    if scene == "floor":
        qpos = np.tile(std["qpos"], (N, 1)); qpos[:, 7:] += rng.normal(size=(N, 69)) * 0.1
        sim = kpsim.KpSim(kpsim.KpModel(kpsim.DEFAULT_KPM), N)
        sim.set_state(t(qpos), t(rng.normal(size=(N, 75)) * 0.3)); sim.set_target(t(np.tile(std["qpos"], (N, 1))))
        act = t(rng.normal(size=(N, 75)) * 0.2)
        for _ in range(10):
            sim.step_ctrl(act, 15)
        obj = None
    else:
        q, v, blk, _ = CF.object_scenes(read_kpm(kpsim.STEP_KPM), std["qpos"])["g_sit"]
        qpos = np.tile(q, (N, 1)); qpos[:, 7 + 12:] += rng.normal(size=(N, 57)) * 0.05          # the legs stay as they sit
        sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM, dynamic_objects=0), N)                   # the chair static in the read-out too: the same problem
        obj = t(np.tile(blk, (N, 1)))
        sim.set_objects(obj)
        sim.set_state(t(qpos), t(rng.normal(size=(N, 75)) * 0.3))
    q, v = sim.get("qpos").clone(), sim.get("qvel").clone()
    fwd = sim.contact_forces(want=("qacc", "ncon"))
    a = fwd["qacc"].clone()
    print(f"{scene}: mean contacts per state {fwd['ncon'].float().mean().item():.1f}")
    base = timed(f"{scene:6s} contact_forces mode 0, qacc only, R = {N}", lambda: sim.contact_forces(want=("qacc",)), N, 20)
    timed(f"{scene:6s} inverse_dynamics, qfrc_inverse only, R = {N}", lambda: sim.inverse_dynamics(q, v, a, obj), N, 20, base)
    timed(f"{scene:6s} inverse_dynamics, all outputs, R = {N}", lambda: sim.inverse_dynamics(q, v, a, obj, want=tuple(kpsim.INVDYN_OUTPUTS)), N, 20, base)
    if scene == "floor":
        q16, v16, a16 = (x.repeat(16, 1) for x in (q, v, a))
        timed(f"{scene:6s} inverse_dynamics, qfrc_inverse only, R = {16 * N}", lambda: sim.inverse_dynamics(q16, v16, a16), 16 * N, 5)
    del sim
