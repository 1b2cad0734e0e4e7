"""What the pose fit to points costs: kp_sim_fit_points at R = 4096 and R = 65536 with the 24 body origins as points, with 53
markers and with 53 markers and the floor term on, each against kp_sim_fit_pose on the SAME rows in the same run.  Device events around blocks of
calls, medians of 5 blocks after a warm-up.  Rows: standing poses with joint noise as the truth (feet near z = 0, so the floor term has vertices to
hold), their markers as targets, the fit starts 0.2 rad of joint noise away.  The marker set is the tests' (tests/fit_points_oracle.py).
    python tools/fit_points_bench.py"""
import functools

import numpy as np
import torch

from _rows_bench import dev, kpsim, std, t, timed

import fit_points_oracle as FT  # noqa: E402

N = 4096
timed = functools.partial(timed, width=72, wide=1, warm=3, of="fit_pose")


def cfg(n_iters, w_floor=0.0):
    c = kpsim.KpFitPointsCfg.default()
    c.fit.n_iters, c.w_floor = n_iters, w_floor
    return c


def pose_cfg(n_iters):
    c = kpsim.KpFitCfg.default()
    c.n_iters = n_iters
    return c


def marker_targets(fk, body, off):
    """x_b + R_b o of every marker on the rows of a kp_sim_fk result: [N, K, 3]"""
    b = torch.as_tensor(body.astype(np.int64), device=dev)
    x, q, o = fk["wbpos"].view(-1, 24, 3)[:, b], fk["wbquat"].view(-1, 24, 4)[:, b], t(off)[None]
    u = q[..., 1:]
    c = 2.0 * torch.cross(u, o.expand_as(u), dim=-1)
    return (x + o + q[..., :1] * c + torch.cross(u, c, dim=-1)).contiguous()


print("# ms per call, median (min .. max) of 5 blocks; the same rows for every line of a size")
rng = np.random.default_rng(0)
truth = np.tile(std["qpos"], (N, 1)); truth[:, 7:] += rng.normal(size=(N, 69)) * 0.2
start = truth.copy(); start[:, 7:] += rng.normal(size=(N, 69)) * 0.2; start[:, :3] += rng.uniform(-0.1, 0.1, (N, 3))
sim = kpsim.KpSim(kpsim.KpModel(kpsim.DEFAULT_KPM), 1)
fk = sim.fk(t(truth))
b24, o24 = np.arange(24, dtype=np.int32), np.zeros((24, 3), np.float32)
b53, o53 = FT.marker_set(FT.counts_53(), FT.SEED_53)
m53 = marker_targets(fk, b53, o53)
n_def = kpsim.KpFitCfg.default().n_iters
for mult, reps in ((1, 40), (16, 8)):
    R = mult * N
    q0, tp, t53 = t(start).repeat(mult, 1), fk["wbpos"].view(N, 24, 3).repeat(mult, 1, 1), m53.repeat(mult, 1, 1)
    base = timed(f"fit_pose, positions only, n_iters = {n_def}, R = {R}", lambda: sim.fit_pose(q0, tp, cfg=pose_cfg(n_def)), R, reps)
    z0 = timed(f"fit_points, K = 53, n_iters = 0 (load, one forward pass, one walk), R = {R}", lambda: sim.fit_points(q0, b53, o53, t53, cfg=cfg(0)), R, reps, base)
    lines = (("K = 24, the body origins as points", lambda: sim.fit_points(q0, b24, o24, tp, cfg=cfg(n_def))),
             ("K = 53", lambda: sim.fit_points(q0, b53, o53, t53, cfg=cfg(n_def))),
             ("K = 53, floor on (w_floor 2400)", lambda: sim.fit_points(q0, b53, o53, t53, cfg=cfg(n_def, FT.FLOOR_W))))
    for label, fn in lines:
        tn = timed(f"fit_points, {label}, n_iters = {n_def}, R = {R}", fn, R, reps, base)
        info = fn()["info"]
        print(f"{'  per iteration':72s} {(tn - z0) / n_def:9.4f} ms;  accepted steps per row {float(info[:, 2].mean()):.1f} of {n_def}, final max |e_k| {float(info[:, 8].max()):.2e} m, "
              f"deepest vertex {float(info[:, 10].max()) * 1e3:.3f} mm, rows with a vertex below the floor {int((info[:, 11] > 0).sum())}")
