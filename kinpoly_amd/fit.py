"""Pose fitting: from body positions (marker or key-point tracks, another skeleton's joints, a head pose) to qpos.

The way INTO the engine for a user who holds body poses and not qpos: dataset.build_take_features, KpTakes, the UHC take library and every metric
start from qpos.  No reference counterpart (the reference converts SMPL axis-angles offline).  All the arithmetic is KpSim.fit_pose
(kp_sim_fit_pose: batched Levenberg-Marquardt on the device, one wavefront per row); this module holds the host logic around it: the configuration
and its checks, the default init, whole sequences (independent frames or chained with a smoothness prior) and the report.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

NQ, NV, NB, NU = 76, 75, 24, 69
_STANDING = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "standing_neutral.npz")


def standing_qpos() -> np.ndarray:
    """the standing pose of the reference's sample clip [76] (the repository's fixture)"""
    return np.load(_STANDING)["qpos"].astype(np.float64)


@dataclass
class FitConfig:
    """kp_fit_cfg with its defaults (kp_fit_cfg_default).  damp: one positive number for every dof, or 75 of them."""
    n_iters: int = 30
    mu0: float = 1e-2
    mu_min: float = 1e-7
    mu_max: float = 1e6
    mu_up: float = 8.0
    mu_down: float = 0.3
    damp: float | tuple = 1.0
    clamp_limits: bool = False
    w_floor: float = 0.0          # fit_points only (kp_fit_points_cfg): weight of the hull vertices below floor_z; 0 switches the term off
    floor_z: float = 0.0
    w_obj: float = 0.0            # fit_scene only (kp_fit_scene_cfg): weight of the hull vertices inside the scene's static objects; needs obj_qpos; 0: off
    z_near: float = 0.05          # fit_image only (kp_fit_image_cfg): the nearest camera depth (m) a weighted observation may have
    _names = ("mu0", "mu_min", "mu_max", "mu_up", "mu_down")

    def damp_vector(self) -> np.ndarray:
        d = np.asarray(self.damp, np.float64)
        if d.ndim == 0:
            d = np.full(NV, float(d))
        if d.shape != (NV,):
            raise ValueError(f"FitConfig: damp must be a number or {NV} numbers, got shape {d.shape}")
        return d

    def validate(self):
        """the refusals of kp_sim_fit_pose, before anything reaches the device"""
        if int(self.n_iters) != self.n_iters or self.n_iters < 0:
            raise ValueError(f"FitConfig: n_iters must be an integer >= 0, got {self.n_iters}")
        for k in self._names:
            if not float(getattr(self, k)) > 0.0:
                raise ValueError(f"FitConfig: {k} must be > 0, got {getattr(self, k)}")
        if not np.all(self.damp_vector() > 0.0):
            raise ValueError("FitConfig: every damp entry must be > 0")
        if not (float(self.w_floor) >= 0.0 and np.isfinite(float(self.w_floor))):
            raise ValueError(f"FitConfig: w_floor must be >= 0 and finite, got {self.w_floor}")
        if not np.isfinite(float(self.floor_z)):
            raise ValueError(f"FitConfig: floor_z must be finite, got {self.floor_z}")
        if not (float(self.w_obj) >= 0.0 and np.isfinite(float(self.w_obj))):
            raise ValueError(f"FitConfig: w_obj must be >= 0 and finite, got {self.w_obj}")
        if not (float(self.z_near) > 0.0 and np.isfinite(float(self.z_near))):
            raise ValueError(f"FitConfig: z_near must be > 0 and finite, got {self.z_near}")
        return self

    def native(self):
        """the KpFitCfg kp_sim_fit_pose takes"""
        from .sim import KpFitCfg
        self.validate()
        c = KpFitCfg()
        c.n_iters = int(self.n_iters)
        for k in self._names:
            setattr(c, k, float(getattr(self, k)))
        for d, v in enumerate(self.damp_vector()):
            c.damp[d] = float(v)
        c.clamp_limits = int(bool(self.clamp_limits))
        return c

    def native_points(self):
        """the KpFitPointsCfg kp_sim_fit_points takes"""
        from .sim import KpFitPointsCfg
        c = KpFitPointsCfg()
        c.fit = self.native()
        c.w_floor, c.floor_z = float(self.w_floor), float(self.floor_z)
        return c

    def native_scene(self):
        """the KpFitSceneCfg kp_sim_fit_scene takes"""
        from .sim import KpFitSceneCfg
        c = KpFitSceneCfg()
        c.pts = self.native_points()
        c.w_obj = float(self.w_obj)
        return c

    def native_image(self):
        """the KpFitImageCfg kp_sim_fit_image takes"""
        from .sim import KpFitImageCfg
        c = KpFitImageCfg()
        c.scene = self.native_scene()
        c.z_near = float(self.z_near)
        return c


def default_init(tgt_pos: torch.Tensor, std_qpos=None) -> torch.Tensor:
    """the standing pose, translated so that its pelvis (the root body, whose origin is qpos[0:3]) sits at the pelvis target: [..., 76]"""
    std = torch.as_tensor(standing_qpos() if std_qpos is None else np.asarray(std_qpos, np.float64), dtype=torch.float32, device=tgt_pos.device)
    q = std.expand(tuple(tgt_pos.shape[:-2]) + (NQ,)).clone()
    q[..., :3] = tgt_pos[..., 0, :]
    return q


def _check_objects(who, obj_qpos, lead):
    """obj_qpos [..., 35] of a fit with the scene's objects: the rows' leading shape, float32, contiguous"""
    if tuple(obj_qpos.shape) != tuple(lead) + (35,):
        raise ValueError(f"{who}: obj_qpos must be {tuple(lead) + (35,)}, got {tuple(obj_qpos.shape)}")
    return obj_qpos.float().contiguous()


def _check_targets(tgt_pos, tgt_quat):
    if tgt_pos.dim() < 2 or tuple(tgt_pos.shape[-2:]) != (NB, 3):
        raise ValueError(f"fit: tgt_pos must be [..., {NB}, 3], got {tuple(tgt_pos.shape)}")
    if tgt_quat is not None and tuple(tgt_quat.shape) != tuple(tgt_pos.shape[:-1]) + (4,):
        raise ValueError(f"fit: tgt_quat must be {tuple(tgt_pos.shape[:-1]) + (4,)}, got {tuple(tgt_quat.shape)}")


def fit_pose(sim, tgt_pos, tgt_quat=None, init=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None, config: FitConfig | None = None, std_qpos=None,
             obj_qpos=None) -> dict:
    """One fit per row: device tensors tgt_pos [..., 24, 3], tgt_quat [..., 24, 4] or None, init [..., 76] or None (default_init).  With tgt_quat and
    no w_rot the orientations count with weight 1.  Returns KpSim.fit_pose's dict (qpos, info).  With config.w_floor > 0 the same problem runs with the
    floor term through KpSim.fit_points (no points, tgt_pos given): info then has 12 columns (FIT_POINTS_INFO).  With obj_qpos [..., 35] (the rows'
    object poses) it runs through KpSim.fit_scene with the scene's static objects as obstacles at weight config.w_obj: info has 16 columns
    (FIT_SCENE_INFO).  Without obj_qpos the call takes the path it took before the argument existed."""
    _check_targets(tgt_pos, tgt_quat)
    floor = float((config or FitConfig()).w_floor) > 0.0
    if obj_qpos is not None:
        obj_qpos = _check_objects("fit_pose", obj_qpos, tgt_pos.shape[:-2])
        cfg = (config or FitConfig()).native_scene()
    else:
        cfg = (config or FitConfig()).native_points() if floor else (config or FitConfig()).native()
    tgt_pos = tgt_pos.float().contiguous()
    if init is None:
        init = default_init(tgt_pos, std_qpos)
    if tgt_quat is not None:
        tgt_quat = tgt_quat.float().contiguous()
        if w_rot is None:
            w_rot = torch.ones(tuple(tgt_pos.shape[:-1]), dtype=torch.float32, device=tgt_pos.device)
    if obj_qpos is not None:
        return sim.fit_scene(init.float().contiguous(), np.zeros(0, np.int32), np.zeros((0, 3), np.float32), None, None, tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior,
                             obj_qpos=obj_qpos, cfg=cfg)
    if floor:
        return sim.fit_points(init.float().contiguous(), np.zeros(0, np.int32), np.zeros((0, 3), np.float32), None, None, tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior, cfg=cfg)
    return sim.fit_pose(init.float().contiguous(), tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior, cfg=cfg)


def fit_sequence(sim, tgt_pos, tgt_quat=None, mode: str = "chained", smooth: float = 1e-2, init=None, config: FitConfig | None = None, std_qpos=None,
                 obj_qpos=None) -> dict:
    """Tracks tgt_pos [B, T, 24, 3] (tgt_quat [B, T, 24, 4] or None) -> qpos [B, T, 76], info [B, T, 8] (12 with config.w_floor > 0: fit_pose).
    independent: all B T rows in ONE call from one init (init [B, T, 76] or [76]-broadcastable, default default_init per frame).
    chained: frame t of all B tracks in one call, warm-started from the solution at t - 1, with that solution as the hinge prior at weight `smooth`
    (frame 0: from init [B, 76] or default_init, no prior).  obj_qpos [B, T, 35] or None: the frames' object poses (fit_pose; info then [B, T, 16])."""
    if mode not in ("chained", "independent"):
        raise ValueError(f"fit_sequence: mode must be 'chained' or 'independent', got {mode!r}")
    if tgt_pos.dim() != 4:
        raise ValueError(f"fit_sequence: tgt_pos must be [B, T, {NB}, 3], got {tuple(tgt_pos.shape)}")
    _check_targets(tgt_pos, tgt_quat)
    if not float(smooth) >= 0.0:
        raise ValueError(f"fit_sequence: smooth must be >= 0, got {smooth}")
    B, T = tgt_pos.shape[:2]
    if mode == "independent":
        if init is not None:
            init = init.float().expand(B, T, NQ)
        return fit_pose(sim, tgt_pos, tgt_quat, init=init, config=config, std_qpos=std_qpos, **({} if obj_qpos is None else dict(obj_qpos=obj_qpos)))
    if obj_qpos is not None:
        obj_qpos = _check_objects("fit_sequence", obj_qpos, (B, T))
    qs, infos = [], []
    q = init
    for t in range(T):
        prior = {} if t == 0 or smooth == 0.0 else dict(q_prior=q[:, 7:].contiguous(), w_prior=torch.full((B, NU), float(smooth), dtype=torch.float32, device=tgt_pos.device))
        if obj_qpos is not None:
            prior = dict(prior, obj_qpos=obj_qpos[:, t].contiguous())
        out = fit_pose(sim, tgt_pos[:, t], None if tgt_quat is None else tgt_quat[:, t], init=q, config=config, std_qpos=std_qpos, **prior)
        q = out["qpos"]
        qs.append(q); infos.append(out["info"])
    return {"qpos": torch.stack(qs, 1), "info": torch.stack(infos, 1)}


@dataclass(eq=False)
class MarkerSet:
    """K points rigidly attached to bodies: names [K], body [K] (0..23), offset [K, 3] in the body frames (m).  Shared by all rows of a fit."""
    names: tuple
    body: np.ndarray
    offset: np.ndarray

    def __post_init__(self):
        from .sim import marker_arrays
        self.names = tuple(str(n) for n in self.names)
        self.body, self.offset = marker_arrays("MarkerSet", self.body, self.offset)
        if len(self.names) != len(self.body):
            raise ValueError(f"MarkerSet: {len(self.names)} names for {len(self.body)} points")
        if len(set(self.names)) != len(self.names):
            raise ValueError("MarkerSet: names must be unique")

    def __len__(self):
        return len(self.body)

    def __eq__(self, other):
        return isinstance(other, MarkerSet) and self.names == other.names and np.array_equal(self.body, other.body) and np.array_equal(self.offset, other.offset)

    __hash__ = None

    @classmethod
    def body_origins(cls):
        """the 24 body origins as points: fit_points on these is fit_pose on tgt_pos"""
        return cls(tuple(f"body{b}" for b in range(NB)), np.arange(NB), np.zeros((NB, 3)))

    @classmethod
    def from_pose(cls, sim, qpos, world_points, body, names=None):
        """offsets calibrated from ONE pose: o = R_b^T (p - x_b) with the engine's forward kinematics (kp_sim_fk) at qpos [76]; world_points [K, 3],
        body [K]"""
        p = np.asarray(world_points, np.float64).reshape(-1, 3)
        body = np.asarray(body)
        if body.shape != (len(p),):
            raise ValueError(f"MarkerSet.from_pose: {len(p)} points and body {body.shape}")
        if len(p) and (body.min() < 0 or body.max() >= NB):
            raise ValueError("MarkerSet.from_pose: body must lie in 0..23")
        q = torch.as_tensor(np.asarray(qpos, np.float32).reshape(1, NQ), device=sim.device)
        out = sim.fk(q)
        x = out["wbpos"].view(NB, 3).double().cpu().numpy()[body]
        qt = out["wbquat"].view(NB, 4).double().cpu().numpy()[body]
        d = p - x
        # R^T d for the unit quaternion (w, u): the rotation by its conjugate
        w, u = qt[:, :1], -qt[:, 1:]
        t = 2.0 * np.cross(u, d)
        off = d + w * t + np.cross(u, t)
        return cls(tuple(names) if names is not None else tuple(f"m{k}" for k in range(len(p))), body, off)

    def save(self, path):
        import json
        with open(path, "w") as f:
            json.dump({"names": list(self.names), "body": [int(b) for b in self.body], "offset": [[float(v) for v in o] for o in self.offset]}, f, indent=1)

    @classmethod
    def load(cls, path):
        import json
        with open(path) as f:
            d = json.load(f)
        for k in ("names", "body", "offset"):
            if k not in d:
                raise ValueError(f"MarkerSet.load: {path} has no {k!r}")
        return cls(tuple(d["names"]), np.asarray(d["body"], np.int64).reshape(-1), np.asarray(d["offset"], np.float64).reshape(-1, 3))


def occlusion_weights(tgt, w=None):
    """(targets, weights) as fit_points hands them on: a point whose target holds a NaN gets weight 0 (an occluded marker); w None: ones"""
    seen = ~torch.isnan(tgt).any(dim=-1)
    w = torch.ones(tuple(tgt.shape[:-1]), dtype=torch.float32, device=tgt.device) if w is None else w.float()
    return tgt, torch.where(seen, w, torch.zeros_like(w)).contiguous()


def fit_points(sim, markers: MarkerSet, tgt, w=None, init=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None,
               config: FitConfig | None = None, std_qpos=None, want=("qpos", "info"), obj_qpos=None) -> dict:
    """One fit per row to the world targets tgt [..., K, 3] of the marker set (device tensors); w [..., K] or None (ones).  A target with a NaN is an
    occluded marker: its weight becomes 0 here.  init [..., 76] or None: the standing pose, translated so that its pelvis sits at the mean of the
    row's visible targets minus the same mean of the standing pose's markers.  config.w_floor / floor_z switch the floor term on.  Returns
    KpSim.fit_points' dict.  With obj_qpos [..., 35] the call goes through KpSim.fit_scene (static objects as obstacles at config.w_obj; info
    [..., 16]); without it, through KpSim.fit_points as before."""
    K = len(markers)
    if tgt.dim() < 2 or tuple(tgt.shape[-2:]) != (K, 3):
        raise ValueError(f"fit_points: tgt must be [..., {K}, 3] for this marker set, got {tuple(tgt.shape)}")
    if w is not None and tuple(w.shape) != tuple(tgt.shape[:-1]):
        raise ValueError(f"fit_points: w must be {tuple(tgt.shape[:-1])}, got {tuple(w.shape)}")
    if obj_qpos is not None:
        obj_qpos = _check_objects("fit_points", obj_qpos, tgt.shape[:-2])
    cfg = (config or FitConfig()).native_points() if obj_qpos is None else (config or FitConfig()).native_scene()
    tgt, w = occlusion_weights(tgt.float().contiguous(), w)
    if init is None:
        init = default_init_points(sim, markers, tgt, w, std_qpos)
    if tgt_quat is not None and w_rot is None:
        w_rot = torch.ones(tuple(tgt.shape[:-2]) + (NB,), dtype=torch.float32, device=tgt.device)
    if obj_qpos is not None:
        return sim.fit_scene(init.float().contiguous(), markers.body, markers.offset, tgt, w, tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior, obj_qpos=obj_qpos, cfg=cfg,
                             want=want)
    return sim.fit_points(init.float().contiguous(), markers.body, markers.offset, tgt, w, tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior, cfg=cfg, want=want)


def default_init_points(sim, markers: MarkerSet, tgt, w, std_qpos=None) -> torch.Tensor:
    """the standing pose, translated by (weighted mean of the row's targets) - (the same mean of the standing pose's own markers): [..., 76]"""
    std = np.asarray(standing_qpos() if std_qpos is None else std_qpos, np.float64)
    fk = sim.fk(torch.as_tensor(std.astype(np.float32).reshape(1, NQ), device=sim.device))
    x = fk["wbpos"].view(NB, 3)[torch.as_tensor(markers.body, dtype=torch.long, device=sim.device)]
    qt = fk["wbquat"].view(NB, 4)[torch.as_tensor(markers.body, dtype=torch.long, device=sim.device)]
    o = torch.as_tensor(markers.offset, device=sim.device)
    u = qt[:, 1:]
    t = 2.0 * torch.cross(u, o, dim=-1)
    p_std = x + o + qt[:, :1] * t + torch.cross(u, t, dim=-1)                      # [K, 3] the standing pose's markers
    ww = (w > 0).float().unsqueeze(-1)
    n = ww.sum(-2).clamp(min=1.0)
    shift = (torch.where(ww > 0, tgt, torch.zeros_like(tgt)) * ww).sum(-2) / n - (p_std * ww).sum(-2) / n
    q = torch.as_tensor(std, dtype=torch.float32, device=sim.device).expand(tuple(tgt.shape[:-2]) + (NQ,)).clone()
    q[..., :3] += shift
    return q


def fit_sequence_points(sim, markers: MarkerSet, tgt, w=None, mode: str = "chained", smooth: float = 1e-2, init=None, config: FitConfig | None = None, std_qpos=None,
                        obj_qpos=None) -> dict:
    """Marker tracks tgt [B, T, K, 3] (w [B, T, K] or None; NaN targets are occluded) -> qpos [B, T, 76], info [B, T, 12], pt_err [B, T, K].
    independent / chained as fit_sequence: chained warm-starts frame t from the solution at t - 1 with that solution as the hinge prior at weight
    `smooth` (frame 0: from init [B, 76] or the default, no prior).  obj_qpos [B, T, 35] or None: the frames' object poses (fit_points; info [B, T, 16])."""
    if mode not in ("chained", "independent"):
        raise ValueError(f"fit_sequence_points: mode must be 'chained' or 'independent', got {mode!r}")
    K = len(markers)
    if tgt.dim() != 4 or tuple(tgt.shape[-2:]) != (K, 3):
        raise ValueError(f"fit_sequence_points: tgt must be [B, T, {K}, 3], got {tuple(tgt.shape)}")
    if not float(smooth) >= 0.0:
        raise ValueError(f"fit_sequence_points: smooth must be >= 0, got {smooth}")
    B, T = tgt.shape[:2]
    want = ("qpos", "info", "pt_err")
    if mode == "independent":
        if init is not None:
            init = init.float().expand(B, T, NQ)
        return fit_points(sim, markers, tgt, w, init=init, config=config, std_qpos=std_qpos, want=want, **({} if obj_qpos is None else dict(obj_qpos=obj_qpos)))
    if obj_qpos is not None:
        obj_qpos = _check_objects("fit_sequence_points", obj_qpos, (B, T))
    outs = {k: [] for k in want}
    q = init
    for t in range(T):
        prior = {} if t == 0 or smooth == 0.0 else dict(q_prior=q[:, 7:].contiguous(), w_prior=torch.full((B, NU), float(smooth), dtype=torch.float32, device=tgt.device))
        if obj_qpos is not None:
            prior = dict(prior, obj_qpos=obj_qpos[:, t].contiguous())
        out = fit_points(sim, markers, tgt[:, t], None if w is None else w[:, t], init=q, config=config, std_qpos=std_qpos, want=want, **prior)
        q = out["qpos"]
        for k in want:
            outs[k].append(out[k])
    return {k: torch.stack(v, 1) for k, v in outs.items()}


def points_report(names, marker_names, pt_err, pt_w, info, n_iters: int) -> dict:
    """take -> the columns of a marker fit (host arrays): pt_err [B, T, K] (0 where skipped), pt_w [B, T, K] (> 0: the point counted), info [B, T, 12].
    Percentiles of the error over the counted points, per take and per marker; accepted share and failed rows as report_from_errors; the
    penetration columns from info 10 / 11."""
    err, w, info = np.asarray(pt_err, np.float64), np.asarray(pt_w, np.float64) > 0, np.asarray(info, np.float64)
    if len(names) != err.shape[0] or info.shape[:2] != err.shape[:2] or w.shape != err.shape or len(marker_names) != err.shape[2]:
        raise ValueError(f"points_report: {len(names)} names, {len(marker_names)} markers, errors {err.shape}, weights {w.shape}, info {info.shape}")
    pct = lambda v: {f"p{p}": (float(np.percentile(v, p)) if v.size else None) for p in (50, 90, 99)}      # noqa: E731
    out = {}
    for b, k in enumerate(names):
        e = err[b][w[b]]
        out[k] = dict(mean_pt_err=float(e.mean()) if e.size else None, max_pt_err=float(e.max()) if e.size else None, **{f"pt_err_{n}": v for n, v in pct(e).items()},
                      visible_share=float(w[b].mean()) if w[b].size else None,
                      per_marker={m: pct(err[b, :, j][w[b, :, j]]) for j, m in enumerate(marker_names)},
                      accepted_share=float(info[b, :, 2].sum() / max(1, n_iters * err.shape[1])), failed_rows=int((info[b, :, 7] != 0).sum()),
                      **penetration_columns(info[b]))
    return out


def penetration_columns(info) -> dict:
    """the floor figures of info rows [T, 12]: deepest hull vertex below the floor over the take (m), mean of the per-frame depth, frames with any; with
    fit_scene's rows [T, 16] the same three for the vertices counted inside static objects (info 12 / 13)"""
    info = np.asarray(info, np.float64)
    out = dict(max_penetration=float(info[:, 10].max()), mean_penetration=float(info[:, 10].mean()), frames_penetrating=int((info[:, 11] > 0).sum()))
    if info.shape[-1] >= 16:                      # fit_scene's rows: the object figures are present
        out.update(max_obj_penetration=float(info[:, 12].max()), mean_obj_penetration=float(info[:, 12].mean()), frames_in_objects=int((info[:, 13] > 0).sum()))
    return out


def fit_report(sim, names, qpos, tgt_pos, info, n_iters: int) -> dict:
    """take -> dict(mean_pos_err, max_pos_err in metres over frames and bodies, accepted_share: accepted steps / iterations run, failed_rows: rows with
    status 1).  qpos [B, T, 76], tgt_pos [B, T, 24, 3], info [B, T, 8] of fit_sequence; the errors are measured with the engine's own forward kinematics."""
    B, T = qpos.shape[:2]
    wb = sim.fk(qpos.reshape(B * T, NQ).contiguous())["wbpos"].view(B, T, NB, 3)
    err = (wb - tgt_pos.float()).norm(dim=-1)
    rep = report_from_errors(names, err.cpu().numpy(), info.cpu().numpy(), n_iters)
    if info.shape[-1] >= 12:                      # fit_points' rows: the penetration columns are present
        for b, k in enumerate(names):
            rep[k].update(penetration_columns(info[b].cpu().numpy()))
    return rep


def report_from_errors(names, err, info, n_iters: int) -> dict:
    """fit_report's host half: err [B, T, 24] position errors, info [B, T, 8] (or 12)"""
    err, info = np.asarray(err, np.float64), np.asarray(info, np.float64)
    if len(names) != err.shape[0] or info.shape[:2] != err.shape[:2]:
        raise ValueError(f"fit_report: {len(names)} names for errors {err.shape} and info {info.shape}")
    out = {}
    for b, k in enumerate(names):
        out[k] = dict(mean_pos_err=float(err[b].mean()), max_pos_err=float(err[b].max()),
                      accepted_share=float(info[b, :, 2].sum() / max(1, n_iters * err.shape[1])), failed_rows=int((info[b, :, 7] != 0).sum()))
    return out


# ---------------------------------------------------------------- 2D key points seen by calibrated cameras

def _quat_matrix(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


@dataclass(eq=False)
class Pinhole:
    """A calibrated camera as kp_sim_fit_image reads it: cam = R p + t (R [3, 3] world -> camera, t [3]), looking along +z,
    pixel = (cx + fx cam_x / cam_z, cy + fy cam_y / cam_z); x to the right, y down, row 0 at the top."""
    R: np.ndarray
    t: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float

    def __post_init__(self):
        self.R, self.t = np.asarray(self.R, np.float64).reshape(3, 3), np.asarray(self.t, np.float64).reshape(3)
        self.fx, self.fy, self.cx, self.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)

    def camera_points(self, points):
        return np.asarray(points, np.float64) @ self.R.T + self.t

    def project(self, points):
        """pixels [..., 2] of world points [..., 3] (host arrays, fp64); no test for points behind the camera"""
        c = self.camera_points(points)
        return np.stack([self.cx + self.fx * c[..., 0] / c[..., 2], self.cy + self.fy * c[..., 1] / c[..., 2]], -1)

    def pack(self) -> np.ndarray:
        """the 16 floats of a camera record: R (row-major), t, fx, fy, cx, cy"""
        return np.concatenate([self.R.ravel(), self.t, [self.fx, self.fy, self.cx, self.cy]]).astype(np.float32)

    @classmethod
    def from_axes(cls, eye, right, down, forward, fovy_deg, width, height):
        """square pixels from a vertical field of view: fx = fy = H / (2 tan(fovy / 2)), the principal point at the image centre"""
        R = np.stack([np.asarray(a, np.float64) for a in (right, down, forward)])
        f = float(height) / (2.0 * np.tan(0.5 * np.radians(float(fovy_deg))))
        return cls(R, -R @ np.asarray(eye, np.float64), f, f, 0.5 * float(width), 0.5 * float(height))

    @classmethod
    def from_camera(cls, camera7, width, height):
        """kp_sim_render's viewer camera: lookat[3], distance, azimuth, elevation, fovy (degrees)"""
        c = np.asarray(camera7, np.float64).reshape(7)
        az, el = np.radians(c[4]), np.radians(c[5])
        f = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        r = np.cross(f, [0.0, 0.0, 1.0]); r /= np.linalg.norm(r)
        u = np.cross(r, f)
        return cls.from_axes(c[:3] - c[3] * f, r, -u, f, c[6], width, height)

    @classmethod
    def from_head_camera(cls, camera8, width, height):
        """kp_sim_render_ego's pose camera: eye[3], quaternion (w, x, y, z; world from camera), fovy (degrees).  Its axes are the head body's
        (forward = R e_z, up = R e_y, right = -R e_x), so the pinhole's x is -c_x and its y is -c_y of c = R^T (p - eye)."""
        c = np.asarray(camera8, np.float64).reshape(8)
        Rc = _quat_matrix(c[3:7])
        return cls.from_axes(c[:3], -Rc[:, 0], -Rc[:, 1], Rc[:, 2], c[7], width, height)


def pack_cameras(cams, device) -> torch.Tensor:
    """cams as the device tensor fit_image takes: a sequence of Pinhole -> [C, 16]; a tensor [C, 16] or [..., C, 16] passes through"""
    if isinstance(cams, torch.Tensor):
        return cams.float().contiguous().to(device)
    if isinstance(cams, Pinhole):
        cams = [cams]
    return torch.as_tensor(np.stack([c.pack() for c in cams]).reshape(-1, 16), dtype=torch.float32, device=device)


def detection_weights(uv, uv_w=None):
    """(uv, weights) as fit_keypoints hands them on: an observation whose uv holds a NaN (an undetected key point) gets weight 0; uv_w None: ones"""
    seen = ~torch.isnan(uv).any(dim=-1)
    w = torch.ones(tuple(uv.shape[:-1]), dtype=torch.float32, device=uv.device) if uv_w is None else uv_w.float()
    return uv, torch.where(seen, w, torch.zeros_like(w)).contiguous()


def fit_keypoints(sim, markers: MarkerSet, uv, cams, uv_w=None, tgt=None, w=None, init=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None,
                  w_prior=None, obj_qpos=None, config: FitConfig | None = None, std_qpos=None, want=("qpos", "info")) -> dict:
    """One fit per row to the pixels uv [..., C, K, 2] at which C calibrated cameras see the marker set's points (device tensors); uv_w [..., C, K] or
    None (ones; a detector's confidence).  A uv with a NaN, or a weight <= 0, is an undetected key point.  cams: Pinholes, or a tensor [C, 16] (all
    rows) / [..., C, 16] (per row).  tgt [..., K, 3] / w: optional world targets of the same points (fit_points' term; NaN: occluded); tgt_pos and
    the others as fit_points.  init [..., 76] or None: fit_points' default when tgt is given, fit_pose's when tgt_pos is, otherwise the standing pose
    where the fixture has it.  config.w_floor / floor_z, w_obj with obj_qpos [..., 35] and z_near as in FitConfig.  Returns KpSim.fit_image's dict."""
    K = len(markers)
    if uv.dim() < 3 or tuple(uv.shape[-2:]) != (K, 2):
        raise ValueError(f"fit_keypoints: uv must be [..., C, {K}, 2] for this marker set, got {tuple(uv.shape)}")
    lead, Cn = tuple(uv.shape[:-3]), int(uv.shape[-3])
    if uv_w is not None and tuple(uv_w.shape) != lead + (Cn, K):
        raise ValueError(f"fit_keypoints: uv_w must be {lead + (Cn, K)}, got {tuple(uv_w.shape)}")
    cam = pack_cameras(cams, uv.device)
    if tuple(cam.shape) not in ((Cn, 16), lead + (Cn, 16)):
        raise ValueError(f"fit_keypoints: {Cn} cameras in uv, cams {tuple(cam.shape)}")
    if tgt is not None and tuple(tgt.shape) != lead + (K, 3):
        raise ValueError(f"fit_keypoints: tgt must be {lead + (K, 3)}, got {tuple(tgt.shape)}")
    if w is not None and (tgt is None or tuple(w.shape) != lead + (K,)):
        raise ValueError(f"fit_keypoints: w goes with tgt and must be {lead + (K,)}")
    if obj_qpos is not None:
        obj_qpos = _check_objects("fit_keypoints", obj_qpos, lead)
    cfg = (config or FitConfig()).native_image()
    uv, uv_w = detection_weights(uv.float().contiguous(), uv_w)
    if tgt is not None:
        tgt, w = occlusion_weights(tgt.float().contiguous(), w)
    if init is None:
        if tgt is not None:
            init = default_init_points(sim, markers, tgt, w, std_qpos)
        elif tgt_pos is not None:
            init = default_init(tgt_pos.float(), std_qpos)
        else:
            std = np.asarray(standing_qpos() if std_qpos is None else std_qpos, np.float64)
            init = torch.as_tensor(std, dtype=torch.float32, device=uv.device).expand(lead + (NQ,)).clone()
    if tgt_quat is not None and w_rot is None:
        w_rot = torch.ones(lead + (NB,), dtype=torch.float32, device=uv.device)
    return sim.fit_image(init.float().contiguous(), markers.body, markers.offset, cam, uv, uv_w, tgt, w, tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior,
                         obj_qpos=obj_qpos, cfg=cfg, want=want)


def fit_sequence_keypoints(sim, markers: MarkerSet, uv, cams, uv_w=None, tgt=None, w=None, mode: str = "chained", smooth: float = 1e-2, init=None,
                           config: FitConfig | None = None, std_qpos=None, obj_qpos=None) -> dict:
    """Key-point tracks uv [B, T, C, K, 2] (uv_w [B, T, C, K] or None; NaN: undetected) -> qpos [B, T, 76], info [B, T, 20], uv_err [B, T, C, K],
    pt_err [B, T, K].  cams: Pinholes or [C, 16] (fixed cameras), or [B, T, C, 16] (moving ones).  tgt [B, T, K, 3] / w: optional 3D tracks of the
    same points.  independent / chained as fit_sequence_points: chained warm-starts frame t from the solution at t - 1 with that solution as the
    hinge prior at weight `smooth` (frame 0: from init [B, 76] or fit_keypoints' default, no prior).  obj_qpos [B, T, 35] or None."""
    if mode not in ("chained", "independent"):
        raise ValueError(f"fit_sequence_keypoints: mode must be 'chained' or 'independent', got {mode!r}")
    K = len(markers)
    if uv.dim() != 5 or tuple(uv.shape[-2:]) != (K, 2):
        raise ValueError(f"fit_sequence_keypoints: uv must be [B, T, C, {K}, 2], got {tuple(uv.shape)}")
    if not float(smooth) >= 0.0:
        raise ValueError(f"fit_sequence_keypoints: smooth must be >= 0, got {smooth}")
    B, T = uv.shape[:2]
    want = ("qpos", "info", "pt_err", "uv_err")
    cam = pack_cameras(cams, uv.device)
    if mode == "independent":
        if init is not None:
            init = init.float().expand(B, T, NQ)
        return fit_keypoints(sim, markers, uv, cam, uv_w, tgt, w, init=init, config=config, std_qpos=std_qpos, want=want, obj_qpos=obj_qpos)
    if obj_qpos is not None:
        obj_qpos = _check_objects("fit_sequence_keypoints", obj_qpos, (B, T))
    outs = {k: [] for k in want}
    q = init
    at = lambda a, t: None if a is None else a[:, t].contiguous()      # noqa: E731
    for t in range(T):
        prior = {} if t == 0 or smooth == 0.0 else dict(q_prior=q[:, 7:].contiguous(), w_prior=torch.full((B, NU), float(smooth), dtype=torch.float32, device=uv.device))
        out = fit_keypoints(sim, markers, uv[:, t].contiguous(), cam if cam.dim() == 2 else cam[:, t].contiguous(), at(uv_w, t), at(tgt, t), at(w, t), init=q, config=config,
                            std_qpos=std_qpos, want=want, obj_qpos=at(obj_qpos, t), **prior)
        q = out["qpos"]
        for k in want:
            outs[k].append(out[k])
    return {k: torch.stack(v, 1) for k, v in outs.items()}


def keypoints_report(names, marker_names, uv_err, uv_w, info, n_iters: int) -> dict:
    """take -> the columns of a key-point fit (host arrays): uv_err [B, T, C, K] in pixels (0 where skipped), uv_w [B, T, C, K] (> 0: the observation
    counted), info [B, T, 20].  Percentiles of the reprojection error over the counted observations, per take, per camera and per marker; the detected
    share; rows behind a camera (status 2); accepted share, failed rows and the penetration columns as points_report."""
    err, w, info = np.asarray(uv_err, np.float64), np.asarray(uv_w, np.float64) > 0, np.asarray(info, np.float64)
    if len(names) != err.shape[0] or info.shape[:2] != err.shape[:2] or w.shape != err.shape or len(marker_names) != err.shape[3]:
        raise ValueError(f"keypoints_report: {len(names)} names, {len(marker_names)} markers, errors {err.shape}, weights {w.shape}, info {info.shape}")
    pct = lambda v: {f"p{p}": (float(np.percentile(v, p)) if v.size else None) for p in (50, 90, 99)}      # noqa: E731
    out = {}
    for b, k in enumerate(names):
        e = err[b][w[b]]
        out[k] = dict(mean_px_err=float(e.mean()) if e.size else None, max_px_err=float(e.max()) if e.size else None, **{f"px_err_{n}": v for n, v in pct(e).items()},
                      detected_share=float(w[b].mean()) if w[b].size else None,
                      per_camera=[pct(err[b, :, c][w[b, :, c]]) for c in range(err.shape[2])],
                      per_marker={m: pct(err[b, :, :, j][w[b, :, :, j]]) for j, m in enumerate(marker_names)},
                      min_depth=float(info[b, :, 19][info[b, :, 18] > 0].min()) if (info[b, :, 18] > 0).any() else None,
                      accepted_share=float(info[b, :, 2].sum() / max(1, n_iters * err.shape[1])), failed_rows=int((info[b, :, 7] == 1).sum()),
                      rows_behind_camera=int((info[b, :, 7] == 2).sum()), **penetration_columns(info[b]))
    return out
