"""What the contact-force read-out costs: ms per kp_sim_contact_forces call at 4096 envs -- floor scene and object scene (the push
scene: box on the table next to the humanoid), modes 0 (no actuation) and 2 (controller), with one output (wrench) and with all outputs -- next to one
substep of a control step of the same handle (kp_sim_last_step_seconds() / 15) in the same run.  Device events around blocks of calls, medians of 5
blocks after a warm-up; the states are standing poses with joint noise, settled by 10 control steps.
    python tools/contact_force_bench.py [n_envs]"""
import statistics
import sys

import numpy as np
import torch

from _rows_bench import blocks, kpsim, settled_floor, std

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096

print(f"# {n} envs; ms per call, median (min .. max) of 5 blocks of 20 calls; substep = kp_sim_last_step_seconds() / 15 of the same handle")
for scene in ("floor", "objects"):
    rng = np.random.default_rng(0)
    blk = None
    if scene == "objects":
        blk = np.zeros((n, 35)); blk[:, 3::7] = 1.0
        for i in range(5):
            blk[:, 7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
        x0, y0 = std["qpos"][0], std["qpos"][1]
        blk[:, 7:14] = [x0 + 1.2, y0, 0.921, 1, 0, 0, 0]; blk[:, 14:21] = [x0 + 1.2, y0, 0.7905, 1, 0, 0, 0]
    sim, act = settled_floor(n, rng, None if scene == "floor" else kpsim.STEP_KPM, blk)
    sub = []
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
