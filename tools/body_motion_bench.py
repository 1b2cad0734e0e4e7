"""What the body-motion read-out costs: rows/s of kp_sim_body_motion at R = 4096 and R = 65536, `centroid` alone and all four
outputs, next to kp_sim_inverse_dynamics (floor, qfrc_inverse alone) on the SAME rows in the same run.  body_motion does a strict subset of that kernel's
work (the forward pass and one spatial_accumulate; no collide, no make_constraint, no row evaluation, no projection) on a smaller LDS block, so it
should not be the slower one.  Device events around blocks of calls, medians of 5 blocks after a warm-up.  States: standing poses with joint noise,
settled by 10 control steps; qacc = the accelerations the contact read-out solved for.
    python tools/body_motion_bench.py"""
import numpy as np

from _rows_bench import settled_floor, timed

N = 4096

print("# ms per call, median (min .. max) of 5 blocks; the same rows for every line of a size")
rng = np.random.default_rng(0)
sim, _ = settled_floor(N, rng)
q, v = sim.get("qpos").clone(), sim.get("qvel").clone()
a = sim.contact_forces(want=("qacc",))["qacc"].clone()
for mult, reps in ((1, 20), (16, 5)):
    R = mult * N
    qr, vr, ar = (x.repeat(mult, 1) for x in (q, v, a))
    base = timed(f"inverse_dynamics, floor, qfrc_inverse only, R = {R}", lambda: sim.inverse_dynamics(qr, vr, ar), R, reps)
    timed(f"body_motion, centroid only, R = {R}", lambda: sim.body_motion(qr, vr, ar, outputs=("centroid",)), R, reps, base)
    timed(f"body_motion, all outputs, R = {R}", lambda: sim.body_motion(qr, vr, ar), R, reps, base)
    timed(f"body_motion, body_vel only (no qacc), R = {R}", lambda: sim.body_motion(qr, vr, outputs=("body_vel",)), R, reps, base)
