"""What the contact-force estimate costs: rows/s of kp_sim_estimate_contacts at R = 4096 and R = 65536 on the floor scene and on
the sit scene (the chair a static obstacle under the pelvis), next to kp_sim_inverse_dynamics on the SAME rows in the same run: both do the same forward
pass and collision pass (the estimate with the margin at the reach, so with more contacts) on the same layout; inverse dynamics then evaluates the
constraint rows once, the estimate runs its Newton iterations on the 6-vector.  Device events around blocks of calls, medians of 5 blocks after a
warm-up.  Floor rows: standing poses with joint noise, settled by 10 control steps, qacc = the accelerations the read-out solved for.  Sit rows: the sit
pose of tests/contact_force_oracle.py with joint noise.
    python tools/estimate_contacts_bench.py"""
import functools

import numpy as np

from _rows_bench import kpsim, motion_scene, timed

N = 4096
timed = functools.partial(timed, width=62)

print(f"# ms per call, median (min .. max) of 5 blocks; {N} distinct states per scene, repeated 16 times for R = {16 * N}")
rng = np.random.default_rng(0)
for scene in ("floor", "sit"):
    sim, obj = motion_scene(scene, N, rng)
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
