"""What the reprojection term costs: kp_sim_fit_image at R = 4096 and R = 65536, K = 53 markers seen by C = 1 and C = 3 cameras
(1000 px, w = 1 px^-2, the damping scaled as in tests/fit_image_oracle.py), 30 iterations, against kp_sim_fit_scene on the SAME rows in the same run
(its 53 markers as 3D targets, floor on, no objects).  Device events around blocks of calls, medians of 5 blocks after a warm-up.  Rows: standing poses
with joint noise as the truth, observed exactly by cameras 3 m away; the fit starts 0.2 rad of joint noise away.
    python tools/fit_image_bench.py"""
import functools

import numpy as np
import torch

from _rows_bench import dev, kpsim, std, t, timed

import fit_image_oracle as FI  # noqa: E402
import fit_points_oracle as FT  # noqa: E402

N = 4096
W = 2400.0
ITERS = 30
timed = functools.partial(timed, width=84, wide=1, warm=3, of="fit_scene")


def scene_cfg():
    c = kpsim.KpFitSceneCfg.default()
    c.pts.fit.n_iters, c.pts.w_floor = ITERS, W
    return c


def image_cfg():
    c = kpsim.KpFitImageCfg.default()
    f = c.scene.pts.fit
    f.n_iters, c.scene.pts.w_floor = ITERS, W
    px = FI.CAMERA_CONFIGS["px1000"]["cfg"]
    f.mu0, f.mu_min, f.mu_max = px["mu0"], px["mu_min"], px["mu_max"]
    return c


def marker_targets(fk, body, off):
    """x_b + R_b o of every marker on the rows of a kp_sim_fk result: [N, K, 3]"""
    b = torch.as_tensor(body.astype(np.int64), device=dev)
    x, q, o = fk["wbpos"].view(-1, 24, 3)[:, b], fk["wbquat"].view(-1, 24, 4)[:, b], t(off)[None]
    u = q[..., 1:]
    c = 2.0 * torch.cross(u, o.expand_as(u), dim=-1)
    return (x + o + q[..., :1] * c + torch.cross(u, c, dim=-1)).contiguous()


def project(cams, p):
    """uv [N, C, K, 2] of world points p [N, K, 3] through the records cams [C, 16] (torch, fp32 from fp64 arithmetic)"""
    cams, p = cams.double(), p.double()
    Rm, tr = cams[:, :9].view(-1, 3, 3), cams[:, 9:12]
    c = torch.einsum("cij,nkj->ncki", Rm, p) + tr[None, :, None, :]
    return torch.stack([cams[None, :, None, 14] + cams[None, :, None, 12] * c[..., 0] / c[..., 2], cams[None, :, None, 15] + cams[None, :, None, 13] * c[..., 1] / c[..., 2]], -1).float().contiguous()


print("# ms per call, median (min .. max) of 5 blocks; the same rows for every line of a row count")
rng = np.random.default_rng(0)
sim = kpsim.KpSim(kpsim.KpModel(), 1)
b53, o53 = FT.marker_set(FT.counts_53(), FT.SEED_53)
truth = np.tile(std["qpos"], (N, 1)); truth[:, 7:] += rng.normal(size=(N, 69)) * 0.2
start = truth.copy(); start[:, 7:] += rng.normal(size=(N, 69)) * 0.2
m53 = marker_targets(sim.fk(t(truth)), b53, o53)
cams3 = t(FI.ring(std["qpos"][:3], 3))
for mult, reps in ((1, 40), (16, 8)):
    R = mult * N
    q0, t53 = t(start).repeat(mult, 1), m53.repeat(mult, 1, 1)
    base = timed(f"fit_scene, K = 53 3D targets, floor on, n_iters = {ITERS}, R = {R}", lambda: sim.fit_scene(q0, b53, o53, t53, cfg=scene_cfg()), R, reps)
    for C in (1, 3):
        cam = cams3[:C].contiguous()
        uv = project(cam, t53)
        fn = lambda: sim.fit_image(q0, b53, o53, cam, uv, cfg=image_cfg())      # noqa: E731
        tn = timed(f"fit_image, K = 53 seen by C = {C}, no 3D targets, floor on, n_iters = {ITERS}, R = {R}", fn, R, reps, base)
        info = fn()["info"]
        print(f"{'  per iteration over fit_scene':84s} {(tn - base) / ITERS:9.4f} ms;  accepted steps per row {float(info[:, 2].mean()):.1f} of {ITERS}, rows with status != 0 "
              f"{int((info[:, 7] != 0).sum())}, reprojection rms {float(info[:, 17].median()):.3e} px (median), {float(info[:, 17].max()):.3e} (max)")
    uv3 = project(cams3, t53)
    fn = lambda: sim.fit_image(q0, b53, o53, cams3, uv3, pt_tgt=t53, cfg=image_cfg())      # noqa: E731
    timed(f"fit_image, K = 53 seen by C = 3 AND as 3D targets, floor on, n_iters = {ITERS}, R = {R}", fn, R, reps, base)
