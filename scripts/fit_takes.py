#!/usr/bin/env python
"""Body-position tracks -> a take library the UHC pipeline reads (kinpoly_amd/fit.py).  No reference counterpart: the
reference gets qpos from SMPL axis-angles offline (uhc/data_process); this is the way in for marker or key-point tracks.

    python scripts/fit_takes.py --tracks in.pkl --out takes.pkl [--mode chained|independent] [--iters N] [--smooth W] [--limits]
                                [--markers set.json] [--floor W [--floor_z Z]] [--objects W]
    python scripts/fit_takes.py --keypoints uv.pkl --cameras cams.pkl --markers set.json --out takes.pkl [--tracks in.pkl] [--floor W] [--objects W] ...

in.pkl:  {take: {"wbpos": [T, 24, 3], optional "wbquat": [T, 24, 4], optional "obj_pose"}} (joblib or pickle).
         With --markers set.json (a kinpoly_amd.fit.MarkerSet: names, body, offset): {take: {"markers": [T, K, 3], optional "obj_pose"}}, NaN where a
         marker is occluded.  --floor W (> 0; 0 switches the term off) keeps the hull vertices above floor_z with weight W, with
         either kind of input; the report then gains the penetration columns, and with --markers the per-marker error percentiles.
         --objects W (> 0) reads each take's "obj_pose" [T, 35] (five object poses, as the take library carries them) and keeps the hull vertices out
         of those objects, static boxes and cylinders, with weight W (the object blob is loaded); a take without obj_pose has
         every object parked.  The report gains the object-penetration columns.  Without the flag the code path and the output are the old ones.
         --keypoints uv.pkl --cameras cams.pkl: 2D key points detected in video, {take: {"uv": [T, C, K, 2] pixels, optional
         "conf": [T, C, K], optional "obj_pose"}} for the K points of --markers (required) seen by C calibrated cameras; confidence <= 0 or a NaN uv
         means undetected, otherwise the confidence is the weight (px^-2).  cams.pkl: an array [C, 16] for every take, or {take: [C, 16] or [T, C, 16]};
         a record is R_cw (9, row-major), t, fx, fy, cx, cy (kinpoly_amd.fit.Pinhole.pack).  No triangulation: a point seen by one camera counts.
         --tracks then is optional and carries the same takes' 3D "markers" [T, K, 3]; --floor and --objects combine as above.  The report has the
         reprojection columns in pixels.
out:     {take: {"qpos": [T, 76], "pose_aa": zeros [T, 72], "trans": zeros [T, 3], (obj_pose as given)}}: the schema AmassSingleDataset reads (of pose_aa
         and trans only the length is read, by its length filter), and next to it fit_report.json (per take: mean / max position error, share of
         accepted steps, failed rows).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_marker_tracks(path, markers):
    """{take: {"markers": [T, K, 3], ...}} for the K points of `markers`"""
    import joblib
    tracks = joblib.load(path)
    K = len(markers)
    if not isinstance(tracks, dict) or not tracks:
        raise ValueError(f"{path}: expected a non-empty dict take -> {{'markers': [T, {K}, 3], ...}}")
    for k, v in tracks.items():
        if "markers" not in v:
            raise ValueError(f"take '{k}': no 'markers' (--markers reads marker tracks, not wbpos)")
        m = np.asarray(v["markers"])
        if m.ndim != 3 or m.shape[1:] != (K, 3) or m.shape[0] < 1:
            raise ValueError(f"take '{k}': markers must be [T, {K}, 3] for the {K} points of the marker set, got {m.shape}")
    return tracks


def parked_objects(T):
    """[T, 35]: every object parked where convert_obj_qpos parks the inactive ones (beyond the 50 m within which an object counts)"""
    blk = np.zeros((T, 35), np.float32)
    for i in range(5):
        blk[:, 7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    blk[:, 3::7] = 1.0
    return blk


def object_rows(sim, tracks, names, lens, Tm):
    """obj_pose of the takes as [B, Tm, 35] device rows, padded with the last frame like the tracks; a take without obj_pose: parked"""
    rows = []
    for k, T in zip(names, lens):
        a = tracks[k].get("obj_pose")
        a = parked_objects(T) if a is None else np.asarray(a, np.float32)
        if a.shape != (T, 35):
            raise ValueError(f"take '{k}': obj_pose must be [{T}, 35], got {a.shape}")
        rows.append(np.concatenate([a, np.repeat(a[-1:], Tm - T, 0)], 0))
    return torch.as_tensor(np.stack(rows), device=sim.device)


def fit_marker_tracks(sim, tracks: dict, markers, mode="chained", iters=30, smooth=1e-2, limits=False, w_floor=0.0, floor_z=0.0, w_obj=0.0):
    """fit_tracks for points of a marker set (tracks[take]["markers"] [T, K, 3], NaN: occluded) through fit_sequence_points; the floor term with w_floor > 0,
    the takes' objects as obstacles with w_obj > 0"""
    from kinpoly_amd import fit
    names = list(tracks)
    K = len(markers)
    arrs = [np.asarray(tracks[k]["markers"], np.float32).reshape(-1, K, 3) for k in names]
    lens = [a.shape[0] for a in arrs]
    Tm = max(lens)
    tgt = torch.as_tensor(np.stack([np.concatenate([a, np.repeat(a[-1:], Tm - a.shape[0], 0)], 0) for a in arrs]), device=sim.device)
    cfg = fit.FitConfig(n_iters=iters, clamp_limits=limits, w_floor=w_floor, floor_z=floor_z, w_obj=w_obj)
    objs = dict(obj_qpos=object_rows(sim, tracks, names, lens, Tm)) if w_obj > 0.0 else {}
    out = fit.fit_sequence_points(sim, markers, tgt, mode=mode, smooth=smooth, config=cfg, **objs)
    seen = (~torch.isnan(tgt).any(-1)).float()
    rep = fit.points_report(names, markers.names, out["pt_err"].cpu().numpy(), seen.cpu().numpy(), out["info"].cpu().numpy(), iters)
    qpos = out["qpos"].double().cpu().numpy()
    takes = {}
    for b, k in enumerate(names):
        T = lens[b]
        takes[k] = {"qpos": qpos[b, :T], "pose_aa": np.zeros((T, 72)), "trans": np.zeros((T, 3))}
        if tracks[k].get("obj_pose") is not None:
            takes[k]["obj_pose"] = np.asarray(tracks[k]["obj_pose"])
    return takes, rep


def load_keypoint_tracks(path, cams_path, markers):
    """({take: {"uv": [T, C, K, 2], "conf": [T, C, K] or None, ...}}, {take: cameras [C, 16] or [T, C, 16]}) for the K points of `markers`"""
    import joblib
    tracks, cams = joblib.load(path), joblib.load(cams_path)
    K = len(markers)
    if not isinstance(tracks, dict) or not tracks:
        raise ValueError(f"{path}: expected a non-empty dict take -> {{'uv': [T, C, {K}, 2], ...}}")
    per_take = {}
    for k, v in tracks.items():
        uv = np.asarray(v["uv"]) if "uv" in v else None
        if uv is None or uv.ndim != 4 or uv.shape[2:] != (K, 2) or uv.shape[0] < 1 or not 1 <= uv.shape[1] <= 8:
            raise ValueError(f"take '{k}': uv must be [T, C, {K}, 2] with 1 .. 8 cameras for the {K} points of the marker set, got {None if uv is None else uv.shape}")
        if v.get("conf") is not None and np.asarray(v["conf"]).shape != uv.shape[:3]:
            raise ValueError(f"take '{k}': conf must be {list(uv.shape[:3])}, got {np.asarray(v['conf']).shape}")
        if isinstance(cams, dict) and k not in cams:
            raise ValueError(f"take '{k}': no cameras in {cams_path}")
        c = np.asarray(cams[k] if isinstance(cams, dict) else cams, np.float32)
        if c.shape not in ((uv.shape[1], 16), (uv.shape[0], uv.shape[1], 16)):
            raise ValueError(f"take '{k}': cameras must be [{uv.shape[1]}, 16] or [{uv.shape[0]}, {uv.shape[1]}, 16], got {c.shape}")
        per_take[k] = c
    if len({np.asarray(v["uv"]).shape[1] for v in tracks.values()}) != 1:
        raise ValueError(f"{path}: every take must have the same number of cameras")
    return tracks, per_take


def fit_keypoint_tracks(sim, tracks: dict, cams: dict, markers, marker_tracks=None, mode="chained", iters=30, smooth=1e-2, limits=False, w_floor=0.0, floor_z=0.0, w_obj=0.0):
    """fit_marker_tracks for 2D key points (tracks[take]["uv"] [T, C, K, 2], "conf" [T, C, K]; cams[take]) through fit_sequence_keypoints;
    marker_tracks: the same takes' 3D markers [T, K, 3] or None; the floor term with w_floor > 0, the takes' objects as obstacles with w_obj > 0"""
    from kinpoly_amd import fit
    names = list(tracks)
    K = len(markers)
    lens = [np.asarray(tracks[k]["uv"]).shape[0] for k in names]
    Tm = max(lens)
    pad = lambda a: np.concatenate([a, np.repeat(a[-1:], Tm - a.shape[0], 0)], 0)      # noqa: E731
    dev = lambda rows: torch.as_tensor(np.stack(rows), device=sim.device)      # noqa: E731
    uv = dev([pad(np.asarray(tracks[k]["uv"], np.float32)) for k in names])
    conf = dev([pad(np.ones((T,) + tuple(uv.shape[2:4]), np.float32) if tracks[k].get("conf") is None else np.asarray(tracks[k]["conf"], np.float32)) for k, T in zip(names, lens)])
    cam = dev([pad(np.broadcast_to(cams[k], (T,) + cams[k].shape[-2:]).astype(np.float32)) for k, T in zip(names, lens)])
    tgt = None
    if marker_tracks is not None:
        for k, T in zip(names, lens):
            if k not in marker_tracks or np.asarray(marker_tracks[k]["markers"]).shape[0] != T:
                raise ValueError(f"take '{k}': --tracks must carry markers [{T}, {K}, 3] for it")
        tgt = dev([pad(np.asarray(marker_tracks[k]["markers"], np.float32).reshape(-1, K, 3)) for k in names])
    cfg = fit.FitConfig(n_iters=iters, clamp_limits=limits, w_floor=w_floor, floor_z=floor_z, w_obj=w_obj)
    objs = dict(obj_qpos=object_rows(sim, tracks, names, lens, Tm)) if w_obj > 0.0 else {}
    out = fit.fit_sequence_keypoints(sim, markers, uv, cam, conf, tgt, mode=mode, smooth=smooth, config=cfg, **objs)
    seen = ((conf > 0) & ~torch.isnan(uv).any(-1)).float()
    rep = fit.keypoints_report(names, markers.names, out["uv_err"].cpu().numpy(), seen.cpu().numpy(), out["info"].cpu().numpy(), iters)
    qpos = out["qpos"].double().cpu().numpy()
    takes = {}
    for b, k in enumerate(names):
        T = lens[b]
        takes[k] = {"qpos": qpos[b, :T], "pose_aa": np.zeros((T, 72)), "trans": np.zeros((T, 3))}
        if tracks[k].get("obj_pose") is not None:
            takes[k]["obj_pose"] = np.asarray(tracks[k]["obj_pose"])
    return takes, rep


def load_tracks(path):
    import joblib
    tracks = joblib.load(path)
    if not isinstance(tracks, dict) or not tracks:
        raise ValueError(f"{path}: expected a non-empty dict take -> {{'wbpos': [T, 24, 3], ...}}")
    for k, v in tracks.items():
        wb = np.asarray(v["wbpos"])
        if wb.ndim == 2 and wb.shape[1] == 72:
            wb = wb.reshape(-1, 24, 3)
        if wb.ndim != 3 or wb.shape[1:] != (24, 3) or wb.shape[0] < 1:
            raise ValueError(f"take '{k}': wbpos must be [T, 24, 3], got {np.shape(v['wbpos'])}")
        if v.get("wbquat") is not None and np.asarray(v["wbquat"]).reshape(-1, 24, 4).shape[0] != wb.shape[0]:
            raise ValueError(f"take '{k}': wbquat must be [T, 24, 4] with wbpos' T")
    return tracks


def fit_tracks(sim, tracks: dict, mode="chained", iters=30, smooth=1e-2, limits=False, w_floor=0.0, floor_z=0.0, w_obj=0.0):
    """(takes in AmassSingleDataset's schema, report).  All takes go through ONE fit_sequence: shorter tracks are padded with their last frame and cut
    again (a padded frame costs a fit and changes nothing before it).  Orientations are used only when every take carries them.  w_floor > 0: the same
    targets with the floor term (fit.fit_pose routes the call through kp_sim_fit_points); the report then gains the penetration columns.  w_obj > 0:
    the takes' objects as static obstacles (kp_sim_fit_scene), and the object-penetration columns."""
    from kinpoly_amd import fit
    names = list(tracks)
    lens = [np.asarray(tracks[k]["wbpos"]).reshape(-1, 24, 3).shape[0] for k in names]
    Tm = max(lens)

    def padded(key, w):
        rows = []
        for k in names:
            a = np.asarray(tracks[k][key], np.float32).reshape(-1, 24, w)
            rows.append(np.concatenate([a, np.repeat(a[-1:], Tm - a.shape[0], 0)], 0))
        return torch.as_tensor(np.stack(rows), device=sim.device)

    tp = padded("wbpos", 3)
    tq = padded("wbquat", 4) if all(tracks[k].get("wbquat") is not None for k in names) else None
    cfg = fit.FitConfig(n_iters=iters, clamp_limits=limits, w_floor=w_floor, floor_z=floor_z, w_obj=w_obj)
    objs = dict(obj_qpos=object_rows(sim, tracks, names, lens, Tm)) if w_obj > 0.0 else {}
    out = fit.fit_sequence(sim, tp, tq, mode=mode, smooth=smooth, config=cfg, **objs)
    rep = fit.fit_report(sim, names, out["qpos"], tp, out["info"], iters)
    qpos = out["qpos"].double().cpu().numpy()
    takes = {}
    for b, k in enumerate(names):
        T = lens[b]
        takes[k] = {"qpos": qpos[b, :T], "pose_aa": np.zeros((T, 72)), "trans": np.zeros((T, 3))}
        if tracks[k].get("obj_pose") is not None:
            takes[k]["obj_pose"] = np.asarray(tracks[k]["obj_pose"])
    return takes, rep


def main(argv=None, sim=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tracks", default=None)
    ap.add_argument("--keypoints", default=None, help="2D key-point tracks {take: uv [T, C, K, 2], conf [T, C, K]} for the points of --markers")
    ap.add_argument("--cameras", default=None, help="the cameras of --keypoints: [C, 16] or {take: [C, 16] or [T, C, 16]}")
    ap.add_argument("--out", required=True)
    ap.add_argument("--mode", choices=("chained", "independent"), default="chained")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--smooth", type=float, default=1e-2)
    ap.add_argument("--limits", action="store_true")
    ap.add_argument("--markers", default=None, help="a MarkerSet json: the tracks carry 'markers' [T, K, 3] in place of wbpos")
    ap.add_argument("--floor", type=float, default=None, help="weight of the floor term (hull vertices below --floor_z)")
    ap.add_argument("--floor_z", type=float, default=0.0)
    ap.add_argument("--objects", type=float, default=None, help="weight of the object term (hull vertices inside the objects of each take's obj_pose)")
    a = ap.parse_args(argv)
    if a.floor is not None and not (a.floor >= 0.0 and np.isfinite(a.floor)):
        ap.error("--floor must be >= 0 and finite")
    if a.objects is not None and not (a.objects > 0.0 and np.isfinite(a.objects)):
        ap.error("--objects must be > 0 and finite")
    if a.floor is None and a.floor_z != 0.0:
        ap.error("--floor_z needs --floor")
    if (a.keypoints is None) != (a.cameras is None):
        ap.error("--keypoints and --cameras go together")
    if a.keypoints is not None and a.markers is None:
        ap.error("--keypoints needs --markers (the points the key points are)")
    if a.keypoints is None and a.tracks is None:
        ap.error("--tracks is required")
    markers = None
    if a.keypoints is not None:
        from kinpoly_amd import fit
        markers = fit.MarkerSet.load(a.markers)
        tracks, cams = load_keypoint_tracks(a.keypoints, a.cameras, markers)
        marker_tracks = load_marker_tracks(a.tracks, markers) if a.tracks is not None else None
    elif a.markers is not None:
        from kinpoly_amd import fit
        markers = fit.MarkerSet.load(a.markers)
        tracks = load_marker_tracks(a.tracks, markers)
    else:
        tracks = load_tracks(a.tracks)
    if sim is None:
        from kinpoly_amd import sim as kpsim
        if a.objects:
            from kinpoly_amd.model_compiler import STEP_KPM
            sim = kpsim.KpSim(kpsim.KpModel(STEP_KPM), 1)
        else:
            sim = kpsim.KpSim(kpsim.KpModel(), 1)
    if a.keypoints is not None:
        takes, rep = fit_keypoint_tracks(sim, tracks, cams, markers, marker_tracks, a.mode, a.iters, a.smooth, a.limits, a.floor or 0.0, a.floor_z, a.objects or 0.0)
    elif a.objects:
        fn, extra = (fit_marker_tracks, (markers,)) if markers is not None else (fit_tracks, ())
        takes, rep = fn(sim, tracks, *extra, a.mode, a.iters, a.smooth, a.limits, a.floor or 0.0, a.floor_z, a.objects)
    elif markers is not None:
        takes, rep = fit_marker_tracks(sim, tracks, markers, a.mode, a.iters, a.smooth, a.limits, a.floor or 0.0, a.floor_z)
    elif a.floor:                  # positions (and orientations, where every take carries them) with the floor term; --floor 0 is the term switched off
        takes, rep = fit_tracks(sim, tracks, a.mode, a.iters, a.smooth, a.limits, a.floor, a.floor_z)
    else:
        takes, rep = fit_tracks(sim, tracks, a.mode, a.iters, a.smooth, a.limits)
    import joblib
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    joblib.dump(takes, a.out)
    rp = os.path.join(os.path.dirname(os.path.abspath(a.out)), "fit_report.json")
    with open(rp, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({"takes": len(takes), "frames": int(sum(len(v["qpos"]) for v in takes.values())), "out": a.out, "report": rp,
                      **({"max_px_err": max(r["max_px_err"] or 0.0 for r in rep.values())} if a.keypoints is not None else
                         {"max_pos_err": max(r["max_pos_err" if "max_pos_err" in r else "max_pt_err"] or 0.0 for r in rep.values())})}))
    return takes, rep


if __name__ == "__main__":
    main()
