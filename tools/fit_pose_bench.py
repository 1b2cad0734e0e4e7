"""What the pose fit costs: kp_sim_fit_pose at R = 4096 and R = 65536, the whole fit at the default n_iters and per iteration
(the difference of a fit of n_iters and one of 0 iterations, divided by n_iters), kp_sim_point_jacobian, and kp_sim_inverse_dynamics (floor,
qfrc_inverse alone) on the SAME rows in the same run as the yardstick.  Device events around blocks of calls, medians of 5 blocks after a warm-up.
Rows: standing poses with joint noise as the truth, their FK as targets (positions and orientations), the fit starts 0.2 rad of joint noise away.
    python tools/fit_pose_bench.py"""
import functools

import numpy as np
import torch

from _rows_bench import dev, kpsim, std, t, timed

N = 4096
timed = functools.partial(timed, width=64, wide=1, warm=3)

def cfg(n_iters):
    c = kpsim.KpFitCfg.default()
    c.n_iters = n_iters
    return c


print("# ms per call, median (min .. max) of 5 blocks; the same rows for every line of a size")
rng = np.random.default_rng(0)
truth = np.tile(std["qpos"], (N, 1)); truth[:, 7:] += rng.normal(size=(N, 69)) * 0.2
start = truth.copy(); start[:, 7:] += rng.normal(size=(N, 69)) * 0.2; start[:, :3] += rng.uniform(-0.1, 0.1, (N, 3))
sim = kpsim.KpSim(kpsim.KpModel(kpsim.DEFAULT_KPM), 1)
fk = sim.fk(t(truth))
n_def = kpsim.KpFitCfg.default().n_iters
for mult, reps in ((1, 40), (16, 8)):
    R = mult * N
    q0, tp, tq = t(start).repeat(mult, 1), fk["wbpos"].view(N, 24, 3).repeat(mult, 1, 1), fk["wbquat"].view(N, 24, 4).repeat(mult, 1, 1)
    wr = torch.ones(R, 24, device=dev)
    body = t(np.arange(R) % 24, torch.int32)
    base = timed(f"inverse_dynamics, floor, qfrc_inverse only, R = {R}", lambda: sim.inverse_dynamics(q0), R, reps)
    timed(f"point_jacobian, R = {R}", lambda: sim.point_jacobian(q0, body), R, reps, base)
    t0 = timed(f"fit_pose, n_iters = 0 (load, one forward pass, costs), R = {R}", lambda: sim.fit_pose(q0, tp, tq, w_rot=wr, cfg=cfg(0)), R, reps, base)
    tn = timed(f"fit_pose, positions + orientations, n_iters = {n_def}, R = {R}", lambda: sim.fit_pose(q0, tp, tq, w_rot=wr, cfg=cfg(n_def)), R, reps, base)
    tpn = timed(f"fit_pose, positions only, n_iters = {n_def}, R = {R}", lambda: sim.fit_pose(q0, tp, cfg=cfg(n_def)), R, reps, base)
    out = sim.fit_pose(q0, tp, tq, w_rot=wr, cfg=cfg(n_def))["info"]
    print(f"{'  per iteration (positions + orientations)':64s} {(tn - t0) / n_def:9.4f} ms   = {(tn - t0) / n_def / base:6.2f} x inverse_dynamics;  positions only "
          f"{(tpn - t0) / n_def:.4f} ms;  accepted steps per row {float(out[:, 2].mean()):.1f} of {n_def}, final max |e_pos| {float(out[:, 4].max()):.2e} m")
