"""Inverse dynamics of pose sequences (KpSim.inverse_dynamics): finite-difference velocities and accelerations of a motion, the
root residual wrench, and the plausibility scores built on them; the same scores with contact forces ESTIMATED from kinematics
(KpSim.estimate_contacts; DESIGN.md section 18: EstimateConfig, estimate_contacts_sequence, plausibility_estimated).  Torch only; everything but the
two *_sequence functions works on CPU tensors too.

Coordinates.  qfrc_inverse [., 75] is a generalized force in the model's dof coordinates: entries 0..2 pair with the root's linear velocity (world
axes), entries 3..5 with its angular velocity, which the free joint expresses in the ROOT's own axes (the motion axes of dofs 3..5 are the columns of
the root's rotation matrix, taken about the root position; forward_kin_bias in kp_step_kin.hpp), entries 6..74 are the 69 hinge torques in ctrl order.
"""
from __future__ import annotations

import dataclasses
import math

import torch

from .uhc_env import get_qvel_fd_new_t

NQ, NV, NU = 76, 75, 69


def _take_bounds(T: int, take_off, device):
    """per row the first row and the row past the last of its take; take_off: [n_takes + 1] row offsets (0 first, T last) or None = one take"""
    if take_off is None:
        return torch.zeros(T, dtype=torch.long, device=device), torch.full((T,), T, dtype=torch.long, device=device)
    off = torch.as_tensor(take_off, dtype=torch.long, device=device).reshape(-1)
    if off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != T or bool((off[1:] <= off[:-1]).any()):
        raise ValueError(f"motion_derivatives: take_off must rise from 0 to {T}, got {off.tolist()}")
    take = torch.searchsorted(off, torch.arange(T, device=device), right=True) - 1
    return off[take], off[take + 1]


def motion_derivatives(qpos: torch.Tensor, dt: float, take_off=None):
    """qpos [T, 76] -> (qvel [T, 75], qacc [T, 75]) by the take library's convention: qvel[t] = get_qvel_fd_new(qpos[t], qpos[t + 1], dt), the last row
    of a take repeating its predecessor's; qacc[t] = (qvel[t + 1] - qvel[t]) / dt, the last two rows repeating the one before them.  No clamp (the
    observation clamps at +-10; a dynamics score must not).  take_off: row offsets [n_takes + 1] of takes stored back to back -- no difference crosses
    a boundary.  A take of one row has zero velocity, one of fewer than three rows zero acceleration."""
    if qpos.dim() != 2 or qpos.shape[1] != NQ:
        raise ValueError(f"motion_derivatives: qpos must be [T, {NQ}], got {tuple(qpos.shape)}")
    T = qpos.shape[0]
    if T == 0:
        return qpos.new_zeros((0, NV)), qpos.new_zeros((0, NV))
    start, end = _take_bounds(T, take_off, qpos.device)
    t = torch.arange(T, device=qpos.device)
    iv = torch.maximum(torch.minimum(t, end - 2), start)               # the row whose forward difference this row takes
    qvel = get_qvel_fd_new_t(qpos[iv], qpos[torch.minimum(iv + 1, end - 1)], dt)
    ia = torch.maximum(torch.minimum(t, end - 3), start)
    qacc = (qvel[torch.minimum(ia + 1, end - 1)] - qvel[ia]) / dt
    return qvel, qacc


def _quat_rotate(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """R(q) v for q [., 4] = (w, x, y, z), normalised here"""
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    u, w = q[..., 1:], q[..., :1]
    c = torch.cross(u, v, dim=-1)
    return v + 2.0 * (w * c + torch.cross(u, c, dim=-1))


def root_residual(qfrc_inverse: torch.Tensor, qpos: torch.Tensor):
    """The residual wrench on the root: (force [., 3], torque [., 3]) in WORLD axes, the torque about the root position qpos[., 0:3].  It is what no
    contact and no joint supplies: zero for a physically possible motion."""
    return qfrc_inverse[..., :3], _quat_rotate(qpos[..., 3:7], qfrc_inverse[..., 3:6])


def inverse_dynamics_sequence(sim, qpos: torch.Tensor, dt: float, obj_qpos: torch.Tensor | None = None, chunk_rows: int = 65536, take_off=None,
                              want=("qfrc_inverse", "qfrc_constraint", "qfrc_bias", "contact", "net_wrench", "ncon")) -> dict:
    """KpSim.inverse_dynamics over a whole sequence qpos [T, 76] (+ obj_qpos [T, 35]) with motion_derivatives' qvel / qacc, chunk_rows rows per launch.
    Returns the kernel's outputs named in `want` for all T rows, plus 'qvel' and 'qacc'."""
    q = qpos.to(sim.device, torch.float32).contiguous()
    o = None if obj_qpos is None else obj_qpos.to(sim.device, torch.float32).contiguous()
    qvel, qacc = motion_derivatives(q, dt, take_off)
    parts = []
    for a in range(0, q.shape[0], max(int(chunk_rows), 1)):
        b = a + max(int(chunk_rows), 1)
        parts.append(sim.inverse_dynamics(q[a:b], qvel[a:b].contiguous(), qacc[a:b].contiguous(), None if o is None else o[a:b], want=want))
    out = {k: torch.cat([p[k] for p in parts]) for k in want} if parts else sim.inverse_dynamics(q, qvel, qacc, o, want=want)
    out["qvel"], out["qacc"] = qvel, qacc
    return out


def plausibility(qfrc_inverse: torch.Tensor, qpos: torch.Tensor, qvel: torch.Tensor, torque_lim, weight: float) -> dict:
    """Per-frame dynamics scores of a motion from its inverse dynamics (rows [T, .]) and their means under 'mean':
        resid_force       |root residual force| / weight (weight = m g in N: 1.0 = the whole body held up by nothing)
        resid_torque      |root residual torque| in N m (about the root position)
        joint_torque_rms  rms of the 69 joint torques, N m
        over_limit        share of the joints with |tau| > torque_lim [69]
        power             sum_j |tau_j qvel_j| over the joints, W"""
    f, tq = root_residual(qfrc_inverse, qpos)
    tau = qfrc_inverse[..., 6:]
    lim = torch.as_tensor(torque_lim, dtype=tau.dtype, device=tau.device)
    out = {"resid_force": f.norm(dim=-1) / weight, "resid_torque": tq.norm(dim=-1), "joint_torque_rms": tau.pow(2).mean(-1).sqrt(),
           "over_limit": (tau.abs() > lim).to(tau.dtype).mean(-1), "power": (tau * qvel[..., 6:]).abs().sum(-1)}
    out["mean"] = {k: v.mean() for k, v in out.items()}
    return out


ESTIMATE_WANT = ("qfrc_inverse", "qfrc_contact", "contact", "lambda", "resid", "net_wrench", "ncon", "info")


@dataclasses.dataclass
class EstimateConfig:
    """kp_estimate_cfg without a device.  None = the convention of kp_estimate_cfg_default for the model the call runs on:
    w_f = 1 / (m g)^2, w_m = 1 / (m g x 1 m)^2, rho = 1e-3 w_f.  mu = 0: the model's friction coefficient."""
    reach: float = 0.03
    w_f: float | None = None
    w_m: float | None = None
    rho: float | None = None
    mu: float = 0.0
    n_iters: int = 20

    def __post_init__(self):
        if not (math.isfinite(self.reach) and self.reach > 0):
            raise ValueError(f"EstimateConfig: reach must be > 0 and finite, got {self.reach}")
        for k in ("w_f", "w_m", "rho"):
            v = getattr(self, k)
            if v is not None and not (math.isfinite(v) and v > 0):
                raise ValueError(f"EstimateConfig: {k} must be > 0 and finite, got {v}")
        if not (math.isfinite(self.mu) and self.mu >= 0):
            raise ValueError(f"EstimateConfig: mu must be >= 0 and finite, got {self.mu}")
        if int(self.n_iters) < 0:
            raise ValueError(f"EstimateConfig: n_iters must be >= 0, got {self.n_iters}")

    def resolved(self, weight: float) -> dict:
        """every field as a number; weight = m g in N fills the conventions"""
        if not (math.isfinite(weight) and weight > 0):
            raise ValueError(f"EstimateConfig: the body weight must be > 0 and finite, got {weight}")
        w_f = 1.0 / weight ** 2 if self.w_f is None else self.w_f
        return dict(reach=self.reach, w_f=w_f, w_m=1.0 / weight ** 2 if self.w_m is None else self.w_m, rho=1e-3 * w_f if self.rho is None else self.rho,
                    mu=self.mu, n_iters=int(self.n_iters))

    def native(self, sim):
        """the KpEstimateCfg of a KpSim's model: kp_estimate_cfg_default, then the fields given here"""
        from .sim import KpEstimateCfg
        c = KpEstimateCfg.default(sim.model)
        c.reach, c.mu, c.n_iters = self.reach, self.mu, int(self.n_iters)
        if self.w_f is not None:
            c.w_f = self.w_f
            c.rho = 1e-3 * self.w_f                 # the convention follows the weight it is stated in
        if self.w_m is not None:
            c.w_m = self.w_m
        if self.rho is not None:
            c.rho = self.rho
        return c


def estimate_contacts_sequence(sim, qpos: torch.Tensor, dt: float, obj_qpos: torch.Tensor | None = None, chunk_rows: int = 65536, take_off=None,
                               cfg: EstimateConfig | None = None, want=ESTIMATE_WANT) -> dict:
    """KpSim.estimate_contacts over a whole sequence qpos [T, 76] (+ obj_qpos [T, 35]) with motion_derivatives' qvel / qacc (take_off respected: no
    difference crosses a take boundary), chunk_rows rows per launch.  Returns the kernel's outputs named in `want` for all T rows, plus 'qvel', 'qacc'."""
    q = qpos.to(sim.device, torch.float32).contiguous()
    o = None if obj_qpos is None else obj_qpos.to(sim.device, torch.float32).contiguous()
    qvel, qacc = motion_derivatives(q, dt, take_off)
    c = (cfg or EstimateConfig()).native(sim)
    parts = []
    for a in range(0, q.shape[0], max(int(chunk_rows), 1)):
        b = a + max(int(chunk_rows), 1)
        parts.append(sim.estimate_contacts(q[a:b], qvel[a:b].contiguous(), qacc[a:b].contiguous(), None if o is None else o[a:b], cfg=c, want=want))
    out = {k: torch.cat([p[k] for p in parts]) for k in want} if parts else sim.estimate_contacts(q, qvel, qacc, o, cfg=c, want=want)
    out["qvel"], out["qacc"] = qvel, qacc
    return out


def plausibility_estimated(est: dict, qpos: torch.Tensor, torque_lim, weight: float) -> dict:
    """plausibility's scores from the ESTIMATED contact forces: est = estimate_contacts_sequence's dict (qfrc_inverse, qvel, net_wrench, ncon).  The same
    keys, with the root residual now what no force inside the friction pyramids of the nearby points can supply, plus per row
        grf           the estimated ground reaction: net contact force [., 3] / weight
    and under 'mean' also support_share, the fraction of rows with at least one candidate."""
    out = plausibility(est["qfrc_inverse"], qpos, est["qvel"], torque_lim, weight)
    out["grf"] = est["net_wrench"][..., :3] / weight
    out["mean"]["grf"] = out["grf"].reshape(-1, 3).mean(0)
    out["mean"]["support_share"] = (est["ncon"] > 0).to(est["qfrc_inverse"].dtype).mean()
    return out


def body_imu(motion: dict, xquat: torch.Tensor, body: int, offset=None, g=(0.0, 0.0, -9.81)):
    """Gyro and accelerometer of a point fixed on a body, in the body's own frame: what an IMU mounted there reads.  motion: KpSim.body_motion's dict
    with body_vel and body_acc [..., 24, 6]; xquat [..., 24, 4] or [..., 96]: the bodies' world orientations (fk()'s wbquat, the stored field xquat);
    offset [3]: the point in the body's frame (None: the frame origin); g: the gravity vector.  With R the body's rotation, r = R offset:
        gyro = R^T w,     accel = R^T (a + alpha x r + w x (w x r) - g)            (proper acceleration: +9.81 up at rest)
    Returns (gyro [..., 3], accel [..., 3])."""
    vel, acc = motion["body_vel"][..., body, :], motion["body_acc"][..., body, :]
    q = xquat.reshape(*xquat.shape[:-2], 24, 4)[..., body, :] if xquat.shape[-1] == 4 else xquat.reshape(*xquat.shape[:-1], 24, 4)[..., body, :]
    w, al, a = vel[..., :3], acc[..., :3], acc[..., 3:]
    gv = torch.as_tensor(g, dtype=a.dtype, device=a.device)
    if offset is not None:
        r = _quat_rotate(q, torch.as_tensor(offset, dtype=a.dtype, device=a.device).expand_as(a))
        a = a + torch.cross(al, r, dim=-1) + torch.cross(w, torch.cross(w, r, dim=-1), dim=-1)
    conj = q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=q.dtype, device=q.device)
    return _quat_rotate(conj, w), _quat_rotate(conj, a - gv)
