"""Frames per second and launch time of the offscreen renderer (kp_sim_render) at the two shapes it is used at: many small frames (4096 rows x
128 x 128, an env batch) and few large ones (64 rows x 640 x 480, a take for a video); two figures per row (simulated and expert) with one active
object each.  Device time by events around blocks of launches after a warm-up, median over the blocks; the launch alone (body poses given) and
KpSim.render as a caller uses it (fk of both figures, then the launch).  Next to the times: how many plane tests a ray costs at most after the
bounding-sphere cull (a tile enters a body when any of its 64 rays passes the cull; the early exit inside a body only lowers this), from a host
restatement of the cull on a sample of rows -- that product is what bounds the kernel.

    python tools/render_bench.py [--blocks 7] [--launches 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pose_contacts_bench import synthetic_rows  # noqa: E402


def plane_tests_per_ray(xpos, rbound, counts, cams, W, H):
    """mean over the rays of the sample rows of sum over the bodies its 8 x 8 tile enters of the body's plane count (xpos [S, K, 24, 3])"""
    from kinpoly_amd.render import Camera
    total = 0.0
    for r in range(len(xpos)):
        o, d = Camera(tuple(cams[r, :3]), *cams[r, 3:]).rays(W, H)
        Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
        tests = np.zeros((Hp // 8, Wp // 8))
        for k in range(xpos.shape[1]):
            for b in range(24):
                oc = xpos[r, k, b] - o
                tca = d @ oc
                ok = (oc @ oc - tca * tca <= rbound[b] ** 2) & ((tca > 0) | (oc @ oc <= rbound[b] ** 2))
                pad = np.zeros((Hp, Wp), bool); pad[:H, :W] = ok
                tests += counts[b] * pad.reshape(Hp // 8, 8, Wp // 8, 8).any((1, 3))
        total += tests.mean()
    return total / len(xpos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: no HIP device visible (the renderer has no CPU path)")
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.model_compiler import STEP_KPM, read_kpm
    from kinpoly_amd.render import follow
    model = kpsim.KpModel(STEP_KPM)
    s = kpsim.KpSim(model, 1)
    planes, adr = model.hull_planes()
    rbound = read_kpm(STEP_KPM)["body_rbound"]
    out = {"device": torch.cuda.get_device_name(0), "planes": int(len(planes)), "shapes": []}
    for R, W, H in ((4096, 128, 128), (64, 640, 480)):
        q, blk = synthetic_rows(R, seed=1)
        q2 = q.copy(); q2[:, 1] += 0.4                                   # the expert, 0.4 m beside
        qd = torch.tensor(np.stack([q, q2], 1), dtype=torch.float32, device="cuda").contiguous()
        bd = torch.tensor(blk, dtype=torch.float32, device="cuda")
        cam = follow(qd[:, 0])
        cam[:, 4] = torch.linspace(0.0, 350.0, R, device="cuda")          # every row from another side
        f = s.fk(qd.reshape(2 * R, 76))
        xp, xq = f["wbpos"].view(R, 2, 72), f["wbquat"].view(R, 2, 96)
        for _ in range(2):                                                # warm-up: code object, plane upload, allocator
            s.render_poses(xp, xq, bd, cam, W, H); s.render(qd, bd, cam, W, H)
        torch.cuda.synchronize()
        res = {"rows": R, "width": W, "height": H}
        for name, call in (("launch", lambda: s.render_poses(xp, xq, bd, cam, W, H)), ("render", lambda: s.render(qd, bd, cam, W, H))):
            ms = []
            for _ in range(args.blocks):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    call()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / args.launches)
            res[name + "_ms_median"] = float(np.median(ms)); res[name + "_ms_blocks"] = [round(x, 4) for x in ms]
            res[name + "_frames_per_s"] = R / (float(np.median(ms)) * 1e-3)
        res["rays_per_s_launch"] = R * W * H / (res["launch_ms_median"] * 1e-3)
        sample = np.linspace(0, R - 1, 8).astype(int)
        res["plane_tests_per_ray_upper_bound"] = plane_tests_per_ray(xp[sample].double().cpu().numpy().reshape(-1, 2, 24, 3), rbound, np.diff(adr),
                                                                     cam[sample].double().cpu().numpy(), W, H)
        g = s.render_poses(xp[:8].contiguous(), xq[:8].contiguous(), bd[:8].contiguous(), cam[:8].contiguous(), W, H, want=("geom",))["geom"]
        res["figure_pixel_share_first_rows"] = float(((g > 0) & ((g < 25) | (g > 100))).float().mean())
        out["shapes"].append(res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
