"""Launch time of the egocentric renderer (kp_sim_render_ego) and frames per second of the flow features built on it.

Launches: R rows x 128 x 128 from a camera on every row's head (fovy 90), one figure and one active object per row -- k_render_ego without a B side
(rgba only), with a B side writing every output, and with a B side writing `cells` alone (what ego_flow_features asks for) -- against k_render
(kp_sim_render, the viewer's free camera at 5 m) at the same size in the same process, and k_render_ego on that same view (the free camera as pose
rows), which separates what the kernel costs from what the head's view costs.  Device time by events around blocks of launches after a warm-up, the median
of the blocks.  Features: kinpoly_amd.render.ego_flow_features on a take of --frames frames (host wall clock, upload and download included).

    python tools/ego_flow_bench.py [--rows 1024] [--blocks 3] [--launches 5] [--frames 1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pose_contacts_bench import synthetic_rows  # noqa: E402


def pose_rows(cam7):
    """the pose-camera rows [R, 8] that see what the free-camera rows [R, 7] see (zero roll): the same view through both kernels"""
    c = np.asarray(cam7, np.float64)
    az, el = np.radians(c[:, 4]), np.radians(c[:, 5])
    f = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    r = np.cross(f, [0.0, 0.0, 1.0]); r /= np.linalg.norm(r, axis=1, keepdims=True)
    u = np.cross(r, f)
    M = np.stack([-r, u, f], 2)                               # world from camera: columns e_x, e_y, e_z
    q = np.zeros((len(c), 4))
    for n, R in enumerate(M):                                 # matrix -> quaternion through the largest of w, x, y, z: none of the four divisions is by a small number
        d = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]]
        i = int(np.argmax(d))
        h = 0.5 * np.sqrt(1.0 + d[i])
        if i == 0:
            q[n] = [h, (R[2, 1] - R[1, 2]) / (4 * h), (R[0, 2] - R[2, 0]) / (4 * h), (R[1, 0] - R[0, 1]) / (4 * h)]
        elif i == 1:
            q[n] = [(R[2, 1] - R[1, 2]) / (4 * h), h, (R[0, 1] + R[1, 0]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h)]
        elif i == 2:
            q[n] = [(R[0, 2] - R[2, 0]) / (4 * h), (R[0, 1] + R[1, 0]) / (4 * h), h, (R[1, 2] + R[2, 1]) / (4 * h)]
        else:
            q[n] = [(R[1, 0] - R[0, 1]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h), (R[1, 2] + R[2, 1]) / (4 * h), h]
    return np.concatenate([c[:, :3] - c[:, 3:4] * f, q, c[:, 6:7]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ego_flow_bench: no HIP device visible (the renderer has no CPU path)")
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.model_compiler import STEP_KPM
    from kinpoly_amd.render import HeadCamera, ego_flow_features, follow
    s = kpsim.KpSim(kpsim.KpModel(STEP_KPM), 1)
    R, W, H = args.rows, 128, 128
    q, blk = synthetic_rows(R, seed=1)
    rng = np.random.default_rng(2)
    q2 = q.copy(); q2[:, 7:] += rng.uniform(-0.05, 0.05, (R, 69)); q2[:, :2] += 0.02          # the next frame
    fa, fb = (s.fk(torch.tensor(x, dtype=torch.float32, device="cuda").contiguous()) for x in (q, q2))
    xa, qa, xb, qb = (t.view(R, 1, -1) for t in (fa["wbpos"], fa["wbquat"], fb["wbpos"], fb["wbquat"]))
    bd = torch.tensor(blk, dtype=torch.float32, device="cuda")
    head = HeadCamera(pitch=20.0)
    ca, cb = head.rows(fa["wbpos"], fa["wbquat"]), head.rows(fb["wbpos"], fb["wbquat"])
    free = follow(torch.tensor(q, dtype=torch.float32, device="cuda"))
    free[:, 4] = torch.linspace(0.0, 350.0, R, device="cuda")         # every row from another side
    free8 = torch.tensor(pose_rows(free.cpu().numpy()), dtype=torch.float32, device="cuda")
    calls = {
        "k_render": lambda: s.render_poses(xa, qa, bd, free, W, H),
        "k_render_ego_same_view": lambda: s.render_ego_poses(xa, qa, bd, free8, width=W, height=H),
        "k_render_ego": lambda: s.render_ego_poses(xa, qa, bd, ca, width=W, height=H),
        "k_render_ego_pair_all": lambda: s.render_ego_poses(xa, qa, bd, ca, xb, qb, bd, cb, width=W, height=H, want=("rgba", "geom", "depth", "flow", "ok", "cells"), grid=16),
        "k_render_ego_pair_cells": lambda: s.render_ego_poses(xa, qa, bd, ca, xb, qb, bd, cb, width=W, height=H, want=("cells",), grid=16),
    }
    ga = s.render_poses(xa, qa, bd, free, W, H, ("geom",))["geom"]
    differ = float((ga != s.render_ego_poses(xa, qa, bd, free8, width=W, height=H, want=("geom",))["geom"]).float().mean())      # silhouette pixels: the two cameras round differently
    out = {"device": torch.cuda.get_device_name(0), "same_view_geom_differs_share": differ, "same_view_figure_share": float(((ga > 0) & ((ga < 25) | (ga > 100))).float().mean()),
           "rows": R, "width": W, "height": H, "launch_ms_median": {}, "launch_ms_blocks": {}}
    for call in calls.values():
        call(); call()
    torch.cuda.synchronize()
    for name, call in calls.items():
        ms = []
        for _ in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.launches)
        out["launch_ms_median"][name] = float(np.median(ms))
        out["launch_ms_blocks"][name] = [round(x, 4) for x in ms]
    T = args.frames
    take = np.tile(q[:1], (T, 1))
    take[:, 7:] += np.cumsum(rng.uniform(-0.01, 0.01, (T, 69)), 0)
    take[:, 1] += 0.01 * np.arange(T)
    obj = np.tile(blk[:1], (T, 1))
    ego_flow_features(s, take[:8], obj[:8], camera=head)
    torch.cuda.synchronize()
    secs = []
    for _ in range(args.blocks):
        t0 = time.perf_counter()
        feat = ego_flow_features(s, take, obj, camera=head)
        secs.append(time.perf_counter() - t0)
    out["features"] = {"frames": T, "dim": int(feat.shape[1]), "size": 128, "seconds_median": float(np.median(secs)), "seconds_blocks": [round(x, 4) for x in secs],
                       "frames_per_s": T / float(np.median(secs))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
