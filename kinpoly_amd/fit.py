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


def default_init(tgt_pos: torch.Tensor, std_qpos=None) -> torch.Tensor:
    """the standing pose, translated so that its pelvis (the root body, whose origin is qpos[0:3]) sits at the pelvis target: [..., 76]"""
    std = torch.as_tensor(standing_qpos() if std_qpos is None else np.asarray(std_qpos, np.float64), dtype=torch.float32, device=tgt_pos.device)
    q = std.expand(tuple(tgt_pos.shape[:-2]) + (NQ,)).clone()
    q[..., :3] = tgt_pos[..., 0, :]
    return q


def _check_targets(tgt_pos, tgt_quat):
    if tgt_pos.dim() < 2 or tuple(tgt_pos.shape[-2:]) != (NB, 3):
        raise ValueError(f"fit: tgt_pos must be [..., {NB}, 3], got {tuple(tgt_pos.shape)}")
    if tgt_quat is not None and tuple(tgt_quat.shape) != tuple(tgt_pos.shape[:-1]) + (4,):
        raise ValueError(f"fit: tgt_quat must be {tuple(tgt_pos.shape[:-1]) + (4,)}, got {tuple(tgt_quat.shape)}")


def fit_pose(sim, tgt_pos, tgt_quat=None, init=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None, config: FitConfig | None = None, std_qpos=None) -> dict:
    """One fit per row: device tensors tgt_pos [..., 24, 3], tgt_quat [..., 24, 4] or None, init [..., 76] or None (default_init).  With tgt_quat and
    no w_rot the orientations count with weight 1.  Returns KpSim.fit_pose's dict (qpos, info)."""
    _check_targets(tgt_pos, tgt_quat)
    cfg = (config or FitConfig()).native()
    tgt_pos = tgt_pos.float().contiguous()
    if init is None:
        init = default_init(tgt_pos, std_qpos)
    if tgt_quat is not None:
        tgt_quat = tgt_quat.float().contiguous()
        if w_rot is None:
            w_rot = torch.ones(tuple(tgt_pos.shape[:-1]), dtype=torch.float32, device=tgt_pos.device)
    return sim.fit_pose(init.float().contiguous(), tgt_pos, tgt_quat, w_pos, w_rot, q_prior, w_prior, cfg=cfg)


def fit_sequence(sim, tgt_pos, tgt_quat=None, mode: str = "chained", smooth: float = 1e-2, init=None, config: FitConfig | None = None, std_qpos=None) -> dict:
    """Tracks tgt_pos [B, T, 24, 3] (tgt_quat [B, T, 24, 4] or None) -> qpos [B, T, 76], info [B, T, 8].
    independent: all B T rows in ONE call from one init (init [B, T, 76] or [76]-broadcastable, default default_init per frame).
    chained: frame t of all B tracks in one call, warm-started from the solution at t - 1, with that solution as the hinge prior at weight `smooth`
    (frame 0: from init [B, 76] or default_init, no prior)."""
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
        return fit_pose(sim, tgt_pos, tgt_quat, init=init, config=config, std_qpos=std_qpos)
    qs, infos = [], []
    q = init
    for t in range(T):
        prior = {} if t == 0 or smooth == 0.0 else dict(q_prior=q[:, 7:].contiguous(), w_prior=torch.full((B, NU), float(smooth), dtype=torch.float32, device=tgt_pos.device))
        out = fit_pose(sim, tgt_pos[:, t], None if tgt_quat is None else tgt_quat[:, t], init=q, config=config, std_qpos=std_qpos, **prior)
        q = out["qpos"]
        qs.append(q); infos.append(out["info"])
    return {"qpos": torch.stack(qs, 1), "info": torch.stack(infos, 1)}


def fit_report(sim, names, qpos, tgt_pos, info, n_iters: int) -> dict:
    """take -> dict(mean_pos_err, max_pos_err in metres over frames and bodies, accepted_share: accepted steps / iterations run, failed_rows: rows with
    status 1).  qpos [B, T, 76], tgt_pos [B, T, 24, 3], info [B, T, 8] of fit_sequence; the errors are measured with the engine's own forward kinematics."""
    B, T = qpos.shape[:2]
    wb = sim.fk(qpos.reshape(B * T, NQ).contiguous())["wbpos"].view(B, T, NB, 3)
    err = (wb - tgt_pos.float()).norm(dim=-1)
    return report_from_errors(names, err.cpu().numpy(), info.cpu().numpy(), n_iters)


def report_from_errors(names, err, info, n_iters: int) -> dict:
    """fit_report's host half: err [B, T, 24] position errors, info [B, T, 8]"""
    err, info = np.asarray(err, np.float64), np.asarray(info, np.float64)
    if len(names) != err.shape[0] or info.shape[:2] != err.shape[:2]:
        raise ValueError(f"fit_report: {len(names)} names for errors {err.shape} and info {info.shape}")
    out = {}
    for b, k in enumerate(names):
        out[k] = dict(mean_pos_err=float(err[b].mean()), max_pos_err=float(err[b].max()),
                      accepted_share=float(info[b, :, 2].sum() / max(1, n_iters * err.shape[1])), failed_rows=int((info[b, :, 7] != 0).sum()))
    return out
