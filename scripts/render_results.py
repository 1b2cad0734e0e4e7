#!/usr/bin/env python
"""Frames of an evaluation: what the reference shows with `eval_uhc.py --mode vis / --record` (scripts/eval_uhc.py:85-131) and
`eval_pose_all.py --mode vis` (:468-531) through MuJoCo's viewer, drawn by this engine's own ray-caster (KpSim.render; kinpoly_amd/render.py).

    python scripts/render_results.py --results out/0002_usr_coverage_full.pkl --video_dir out/videos
    python scripts/render_results.py --results results/.../1000_test_coverage_full.pkl --takes sit-1,push-3 --every 3 --hide_expert

Reads either evaluation pickle: eval_ar_policy.py's `*_coverage_full.pkl` (per take `pred` / `target` / `obj_pose`) or eval_uhc.py's (`pred`, 76 or 111 wide,
/ `gt`; columns 76..110 of a 111-wide `pred` are the object block).  Writes `<video_dir>/<take>/%04d.png` (characters of a take name other than letters, digits, `-`, `_`, `.` become `_`): the simulated figure in grey, the expert / kinematic
target in red (unless --hide_expert), the take's objects, a checkered floor.  A take whose `pred` and expert lengths differ is cut to the shorter
(eval_pose_all.py:687-692).  The frames show the collision geometry (the convex hulls), not the visual mesh.  --video assembles an mp4 per take with
ffmpeg when it is on PATH.  --ego also writes what the simulated figure sees from its head (KpSim.render_ego through kinpoly_amd.render.HeadCamera) as
`<video_dir>/<take>/ego_%04d.png`, --ego_size pixels square.
"""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--results", required=True, help="a *_coverage_full.pkl of eval_ar_policy.py or eval_uhc.py")
    p.add_argument("--video_dir", default="out/videos/render")
    p.add_argument("--takes", default="", help="comma-separated take names (default: all)")
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--azimuth", type=float, default=45.0)
    p.add_argument("--distance", type=float, default=5.0)
    p.add_argument("--hide_expert", action="store_true", default=False)
    p.add_argument("--no_focus", action="store_true", default=False, help="keep the camera on the origin instead of following the simulated root")
    p.add_argument("--every", type=int, default=1, help="render every N-th frame")
    p.add_argument("--kpm", default="", help="model blob (default: the shipped smpl_humanoid.kpm)")
    p.add_argument("--video", action="store_true", default=False, help="also assemble <video_dir>/<take>.mp4 with ffmpeg, when it is on PATH")
    p.add_argument("--ego", action="store_true", default=False, help="also write ego_%%04d.png beside the frames: the simulated figure's own view from its head")
    p.add_argument("--ego_size", type=int, default=256, help="width = height of the --ego frames")
    p.add_argument("--ego_fovy", type=float, default=90.0)
    p.add_argument("--ego_pitch", type=float, default=0.0, help="degrees the head camera looks down from the head's forward axis")
    return p


def load_results(path):
    """{take: dict(pred [T,76], expert [T,76] or None, obj_pose [T,35] or None)} of either pickle layout, pred and expert cut to the shorter"""
    if not os.path.isfile(path):
        raise SystemExit(f"render_results.py: no such results file: {path}")
    try:
        import joblib
        res = joblib.load(path)
    except ImportError:
        import pickle
        with open(path, "rb") as f:
            res = pickle.load(f)
    if not isinstance(res, dict) or not res or not all(isinstance(r, dict) and "pred" in r for r in res.values()):
        raise SystemExit(f"render_results.py: {path} is not a *_coverage_full.pkl (a dict take -> {{pred, target | gt, ...}})")
    out = {}
    for take, r in res.items():
        pred = np.asarray(r["pred"], np.float64)
        if pred.ndim != 2 or pred.shape[1] not in (76, 111):
            raise SystemExit(f"render_results.py: take {take}: pred rows are {pred.shape[1:]} wide, expected 76 or 111")
        expert = r.get("target", r.get("gt"))
        expert = None if expert is None else np.asarray(expert, np.float64)[:, :76]
        obj = np.asarray(r["obj_pose"], np.float64) if r.get("obj_pose") is not None else (pred[:, 76:111] if pred.shape[1] == 111 else None)
        if obj is not None and (obj.ndim != 2 or obj.shape[1] != 35):
            raise SystemExit(f"render_results.py: take {take}: obj_pose rows are {obj.shape[1:]} wide, expected the 35-float object block")
        T = min(len(pred), len(expert) if expert is not None else len(pred), len(obj) if obj is not None else len(pred))
        out[take] = dict(pred=pred[:T, :76], expert=None if expert is None else expert[:T], obj_pose=None if obj is None else obj[:T])
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.every < 1:
        raise SystemExit("render_results.py: --every must be >= 1")
    takes = load_results(args.results)
    names = [t for t in args.takes.split(",") if t] or list(takes)
    missing = [t for t in names if t not in takes]
    if missing:
        raise SystemExit(f"render_results.py: takes not in {args.results}: {', '.join(missing)} (it has {', '.join(list(takes)[:8])} ...)")
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.render import Camera, HeadCamera, ego_sequence, render_sequence, write_png
    sim = kpsim.KpSim(kpsim.KpModel(args.kpm or kpsim.DEFAULT_KPM), 1)
    if int(sim.model.get_option("n_obj_geoms")) == 0:
        for t in takes.values():
            t["obj_pose"] = None
    cam = Camera(azimuth=args.azimuth, distance=args.distance)
    ffmpeg = shutil.which("ffmpeg") if args.video else None
    if args.video and not ffmpeg:
        print("render_results.py: ffmpeg is not on PATH: the frames are left as PNG files")
    for name in names:
        t = takes[name]
        sl = slice(None, None, args.every)
        figs = [t["pred"][sl]] + ([] if args.hide_expert or t["expert"] is None else [t["expert"][sl]])
        frames = render_sequence(sim, figs, None if t["obj_pose"] is None else t["obj_pose"][sl], cam, args.width, args.height, focus=not args.no_focus)
        safe = "".join(c if c.isalnum() or c in "-_." else "_" for c in str(name)).lstrip(".") or "take"      # a take key is data: never a path
        d = os.path.join(args.video_dir, safe)
        for i, fr in enumerate(frames):
            write_png(os.path.join(d, "%04d.png" % i), fr)
        if args.ego:
            ego = ego_sequence(sim, t["pred"][sl], None if t["obj_pose"] is None else t["obj_pose"][sl], HeadCamera(fovy=args.ego_fovy, pitch=args.ego_pitch),
                               args.ego_size, args.ego_size)
            for i, fr in enumerate(ego):
                write_png(os.path.join(d, "ego_%04d.png" % i), fr)
        print(f"{name}: {len(frames)} frames{' and their ego views' if args.ego else ''} -> {d}")
        if ffmpeg:
            subprocess.check_call([ffmpeg, "-y", "-loglevel", "error", "-framerate", str(max(1, round(30 / args.every))), "-i", os.path.join(d, "%04d.png"),
                                   "-pix_fmt", "yuv420p", os.path.join(args.video_dir, f"{safe}.mp4")])


if __name__ == "__main__":
    main()
