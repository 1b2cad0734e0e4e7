"""What the contact-force estimate costs: rows/s of kp_sim_estimate_contacts at R = 4096 and R = 65536 on the floor scene and on
the sit scene (the chair a static obstacle under the pelvis), next to kp_sim_inverse_dynamics on the SAME rows in the same run: both do the same forward
pass and collision pass (the estimate with the margin at the reach, so with more contacts) on the same layout; inverse dynamics then evaluates the
constraint rows once, the estimate runs its Newton iterations on the 6-vector.  Device events around blocks of calls, medians of 5 blocks after a
warm-up.  Floor rows: standing poses with joint noise, settled by 10 control steps, qacc = the accelerations the read-out solved for.  Sit rows: the sit
pose of tests/contact_force_oracle.py with joint noise.
    python tools/estimate_contacts_bench.py"""
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
    tail = "" if base is None else f"   = {med / base:5.2f} x inverse_dynamics"
    print(f"{label:62s} {med:8.4f} ms   ({lo:.4f} .. {hi:.4f})   {rows / med * 1e3 / 1e6:7.2f} M rows/s{tail}")
    return med


print(f"# ms per call, median (min .. max) of 5 blocks; {N} distinct states per scene, repeated 16 times for R = {16 * N}")
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
        sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM, dynamic_objects=0), N)
        obj = t(np.tile(blk, (N, 1)))
        sim.set_objects(obj)
        sim.set_state(t(qpos), t(rng.normal(size=(N, 75)) * 0.3))
    q, v = sim.get("qpos").clone(), sim.get("qvel").clone()
    a = sim.contact_forces(want=("qacc",))["qacc"].clone()
    est = sim.estimate_contacts(q, v, a, obj, want=("ncon", "info"))
    soft = sim.inverse_dynamics(q, v, a, obj, want=("ncon",))
    info = est["info"]
    print(f"{scene}: mean candidates per row {est['ncon'].float().mean().item():.1f} (soft contacts {soft['ncon'].float().mean().item():.1f}), Newton iterations mean "
          f"{info[:, 2].mean().item():.2f} max {int(info[:, 2].max())}, rows with a line search {(info[:, 5] > 0).float().mean().item():.3f}, status != 0 on {int((info[:, 7] != 0).sum())} rows")
    for rep, reps in ((1, 20), (16, 5)):
        R = rep * N
        qr, vr, ar = (x.repeat(rep, 1) for x in (q, v, a))
        objr = None if obj is None else obj.repeat(rep, 1)
        base = timed(f"{scene:6s} inverse_dynamics, qfrc_inverse only, R = {R}", lambda: sim.inverse_dynamics(qr, vr, ar, objr), R, reps)
        timed(f"{scene:6s} estimate_contacts, qfrc_inverse only, R = {R}", lambda: sim.estimate_contacts(qr, vr, ar, objr), R, reps, base)
        timed(f"{scene:6s} estimate_contacts, all outputs, R = {R}", lambda: sim.estimate_contacts(qr, vr, ar, objr, want=tuple(kpsim.ESTIMATE_OUTPUTS)), R, reps, base)
    del sim
