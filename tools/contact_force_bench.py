"""What the contact-force read-out costs: ms per kp_sim_contact_forces call at 4096 envs -- floor scene and object scene (the push
scene: box on the table next to the humanoid), modes 0 (no actuation) and 2 (controller), with one output (wrench) and with all outputs -- next to one
substep of a control step of the same handle (kp_sim_last_step_seconds() / 15) in the same run.  Device events around blocks of calls, medians of 5
blocks after a warm-up; the states are standing poses with joint noise, settled by 10 control steps.
    python tools/contact_force_bench.py [n_envs]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kinpoly_amd import sim as kpsim  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
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


print(f"# {n} envs; ms per call, median (min .. max) of 5 blocks of 20 calls; substep = kp_sim_last_step_seconds() / 15 of the same handle")
for scene in ("floor", "objects"):
    rng = np.random.default_rng(0)
    qpos = np.tile(std["qpos"], (n, 1)); qpos[:, 7:] += rng.normal(size=(n, 69)) * 0.1
    sim = kpsim.KpSim(kpsim.KpModel(kpsim.DEFAULT_KPM if scene == "floor" else kpsim.STEP_KPM), n)
    if scene == "objects":
        blk = np.zeros((n, 35)); blk[:, 3::7] = 1.0
        for i in range(5):
            blk[:, 7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
        x0, y0 = std["qpos"][0], std["qpos"][1]
        blk[:, 7:14] = [x0 + 1.2, y0, 0.921, 1, 0, 0, 0]; blk[:, 14:21] = [x0 + 1.2, y0, 0.7905, 1, 0, 0, 0]
        sim.set_objects(t(blk))
    sim.set_state(t(qpos), t(rng.normal(size=(n, 75)) * 0.3)); sim.set_target(t(np.tile(std["qpos"], (n, 1))))
    act = t(rng.normal(size=(n, 75)) * 0.2)
    sub = []
    for _ in range(10):
        sim.step_ctrl(act, 15)
    for _ in range(5):
        sim.step_ctrl(act, 15); torch.cuda.synchronize(); sub.append(sim.last_step_seconds() * 1e3 / 15)
    ncon = sim.contact_forces(want=("ncon",))["ncon"].float().mean().item()
    print(f"{scene:8s} one substep of the control step      {statistics.median(sub):8.4f} ms   ({min(sub):.4f} .. {max(sub):.4f}); mean contacts per env {ncon:.1f}")
    for mode, kw in ((0, {}), (2, {"action": act})):
        for label, want in (("wrench only", ("wrench",)), ("all outputs", tuple(kpsim.CONTACT_OUTPUTS))):
            fn = lambda: sim.contact_forces(want=want, **kw)      # noqa: E731
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = blocks(fn, 20)
            print(f"{scene:8s} contact_forces mode {mode}, {label:12s}     {med:8.4f} ms   ({lo:.4f} .. {hi:.4f})   = {med / statistics.median(sub):5.2f} substeps")
    del sim
