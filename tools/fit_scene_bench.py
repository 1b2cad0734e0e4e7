"""What keeping the hulls out of the scene's objects costs: kp_sim_fit_scene at R = 4096 and R = 65536 on three kinds of rows --
the floor scene (every object parked), the sit pose on the chair (2 geoms), a standing pose on the table (5 geoms) -- each against kp_sim_fit_points
(K = 53, floor on) on the SAME rows in the same run.  Device events around blocks of calls, medians of 5 blocks after a warm-up.  Rows: poses with joint
noise as the truth, their 53 markers (tests/fit_points_oracle.py's set) as targets; the fit starts 0.2 rad of joint noise away and 3 cm lower (into
the seat, into the table top).  Both terms at weight 2400.
    python tools/fit_scene_bench.py"""
import functools

import numpy as np
import torch

from _rows_bench import dev, kpsim, std, t, timed

import contact_force_oracle as CF  # noqa: E402
import fit_points_oracle as FT  # noqa: E402
import fit_scene_oracle as FS  # noqa: E402
from kinpoly_amd.model_compiler import read_kpm  # noqa: E402

N = 4096
W = 2400.0
timed = functools.partial(timed, width=76, wide=1, warm=3, of="fit_points")


def scene_cfg(n_iters, w_obj):
    c = kpsim.KpFitSceneCfg.default()
    c.pts.fit.n_iters, c.pts.w_floor, c.w_obj = n_iters, W, w_obj
    return c


def points_cfg(n_iters):
    c = kpsim.KpFitPointsCfg.default()
    c.fit.n_iters, c.w_floor = n_iters, W
    return c


def marker_targets(fk, body, off):
    """x_b + R_b o of every marker on the rows of a kp_sim_fk result: [N, K, 3]"""
    b = torch.as_tensor(body.astype(np.int64), device=dev)
    x, q, o = fk["wbpos"].view(-1, 24, 3)[:, b], fk["wbquat"].view(-1, 24, 4)[:, b], t(off)[None]
    u = q[..., 1:]
    c = 2.0 * torch.cross(u, o.expand_as(u), dim=-1)
    return (x + o + q[..., :1] * c + torch.cross(u, c, dim=-1)).contiguous()


def scenes(rng):
    """name -> (truth [N, 76], object rows [N, 35])"""
    kpm = read_kpm(kpsim.STEP_KPM)
    stand = np.tile(std["qpos"], (N, 1)); stand[:, 7:] += rng.normal(size=(N, 69)) * 0.2
    out = {"floor scene (objects parked)": (stand, np.tile(FS.parked_block(), (N, 1)))}
    q, _, blk, _ = CF.object_scenes(kpm, std["qpos"])["g_sit"]
    sit = np.tile(q, (N, 1)); sit[:, 7 + 12:] += rng.normal(size=(N, 57)) * 0.05      # the legs stay as they sit
    out["chair (2 geoms)"] = (sit, np.tile(blk, (N, 1)))
    on = stand.copy(); on[:, 2] += FS.STEP_TOP
    tab = np.tile(FS.parked_block(), (N, 1))
    tab[:, 7 * FS.TABLE: 7 * FS.TABLE + 3] = on[:, :3] * [1, 1, 0] + [0, 0, FS.STEP_TOP + 0.09]      # the top's upper face at STEP_TOP, under the feet
    out["table (5 geoms)"] = (on, tab)
    return out


print("# ms per call, median (min .. max) of 5 blocks; the same rows for both lines of a scene")
rng = np.random.default_rng(0)
sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), 1)
b53, o53 = FT.marker_set(FT.counts_53(), FT.SEED_53)
n_def = kpsim.KpFitCfg.default().n_iters
for name, (truth, blk) in scenes(rng).items():
    start = truth.copy(); start[:, 7:] += rng.normal(size=(N, 69)) * 0.2; start[:, 2] -= 0.03
    m53 = marker_targets(sim.fk(t(truth)), b53, o53)
    for mult, reps in ((1, 40), (16, 8)):
        R = mult * N
        q0, t53, ob = t(start).repeat(mult, 1), m53.repeat(mult, 1, 1), t(blk).repeat(mult, 1)
        base = timed(f"fit_points, K = 53, floor on, n_iters = {n_def}, R = {R}: {name}", lambda: sim.fit_points(q0, b53, o53, t53, cfg=points_cfg(n_def)), R, reps)
        fn = lambda: sim.fit_scene(q0, b53, o53, t53, obj_qpos=ob, cfg=scene_cfg(n_def, W))      # noqa: E731
        tn = timed(f"fit_scene,  K = 53, floor on, w_obj {W:g}, n_iters = {n_def}, R = {R}: {name}", fn, R, reps, base)
        z0 = sim.fit_scene(q0, b53, o53, t53, obj_qpos=ob, cfg=scene_cfg(0, W))["info"]
        info = fn()["info"]
        print(f"{'  per iteration over fit_points':76s} {(tn - base) / n_def:9.4f} ms;  accepted steps per row {float(info[:, 2].mean()):.1f} of {n_def}, rows with a pair {int((z0[:, 14] > 0).sum())} -> "
              f"{int((info[:, 14] > 0).sum())}, deepest counted vertex {float(z0[:, 12].max()) * 1e3:.2f} -> {float(info[:, 12].max()) * 1e3:.3f} mm (median {float(info[:, 12].median()) * 1e3:.3f}), "
              f"final max |e_k| {float(info[:, 8].median()):.2e} m (median)")
