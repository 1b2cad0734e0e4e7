"""What inverse dynamics costs: rows/s of kp_sim_inverse_dynamics at R = 4096 and R = 65536 on the floor scene and at R = 4096
on the sit scene (the chair a static obstacle under the pelvis), next to kp_sim_contact_forces mode 0 on the SAME 4096 states in the same run: both do
the same forward pass, collide and make_constraint on the same layout; the read-out then runs the Newton solve, the inverse one gradient evaluation.
Device events around blocks of calls, medians of 5 blocks after a warm-up.  Floor states: standing poses with joint noise, settled by 10 control steps;
qacc = the accelerations the read-out solved for.  Sit states: the sit pose of tests/contact_force_oracle.py with joint noise.
    python tools/inverse_dynamics_bench.py"""
import functools

import numpy as np

from _rows_bench import kpsim, motion_scene, timed

N = 4096
timed = functools.partial(timed, of="the read-out")

print(f"# ms per call, median (min .. max) of 5 blocks; {N} states per scene")
rng = np.random.default_rng(0)
for scene in ("floor", "sit"):
    sim, obj = motion_scene(scene, N, rng)
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
