"""Ground reaction forces from the contact-force read-out (KpSim.contact_forces).  Torch only; works on CPU tensors too.

The read-out's `wrench` is [N, 26, 6] per entity (24 bodies of SMPL_BODY_NAMES, then the two object slots): net contact force[3] and torque[3] about the
WORLD ORIGIN, world axes, z up, floor at z = 0.  Everything here is linear algebra on those rows.
"""
from __future__ import annotations

import torch

# ankle and toe of each side (indices into SMPL_BODY_NAMES): the hulls a standing humanoid loads
FOOT_BODIES = {"L": (3, 4), "R": (7, 8)}
GRAVITY = 9.81          # |mjOption.gravity| of the compiled model (model_compiler.MJ_DEFAULTS)


def shift_wrench(wrench: torch.Tensor, point) -> torch.Tensor:
    """The same wrenches with the torque taken about `point` ([3] or broadcastable to [..., 3]) instead of the point it is about now:
    tau' = tau - point x F.  shift_wrench(shift_wrench(w, a), b) == shift_wrench(w, a + b)."""
    p = torch.as_tensor(point, dtype=wrench.dtype, device=wrench.device).expand(wrench.shape[:-1] + (3,))
    f, t = wrench[..., :3], wrench[..., 3:]
    return torch.cat([f, t - torch.cross(p, f, dim=-1)], dim=-1)


def ground_reaction(wrench: torch.Tensor, groups=FOOT_BODIES, min_fz: float = 1.0) -> dict:
    """Per group of entities (default: the two feet) from wrench [N, 26, 6]:
        force        [N, G, 3]  sum of the group's contact forces
        torque       [N, G, 3]  sum of their torques about the world origin
        cop          [N, G, 2]  centre of pressure on z = 0: cop_x = -tau_y / F_z, cop_y = tau_x / F_z; NaN where F_z <= min_fz
        free_moment  [N, G]     moment about the vertical through the CoP: tau_z - (cop_x F_y - cop_y F_x); NaN where F_z <= min_fz
        support      [N, G]     bool, F_z > min_fz
    min_fz (N): below it a foot counts as unloaded (the solver's margin contacts carry 0 N; 1 N is 0.15 % of body weight).
    groups: dict name -> entity indices; the G axis follows its order."""
    idx = [torch.as_tensor(list(v), dtype=torch.long, device=wrench.device) for v in groups.values()]
    w = torch.stack([wrench.index_select(-2, i).sum(-2) for i in idx], dim=-2)
    f, t = w[..., :3], w[..., 3:]
    support = f[..., 2] > min_fz
    fz = torch.where(support, f[..., 2], torch.full_like(f[..., 2], float("nan")))
    cop = torch.stack([-t[..., 1] / fz, t[..., 0] / fz], dim=-1)
    free = t[..., 2] - (cop[..., 0] * f[..., 1] - cop[..., 1] * f[..., 0])
    return {"force": f, "torque": t, "cop": cop, "free_moment": free, "support": support}


def wrench_from_contacts(contact: torch.Tensor) -> torch.Tensor:
    """Adapter from contact rows to ground_reaction's input: contact [..., 64, 12] (A, B, dist, pos[3], normal[3], force[3], zero rows past ncon; the
    rows of KpSim.contact_forces, inverse_dynamics and estimate_contacts) -> wrench [..., 26, 6], per entity the sum of the forces on it and of their
    torques about the world origin.  A row acts on A; where B is an object slot (24 + k) the opposite force acts on it, as contact_forces' wrench
    counts it.  Rows with a zero force add nothing, so the padding needs no count."""
    a, b = contact[..., 0].long(), contact[..., 1].long()
    w = torch.cat([contact[..., 9:12], torch.cross(contact[..., 3:6], contact[..., 9:12], dim=-1)], dim=-1)
    out = contact.new_zeros(contact.shape[:-2] + (26, 6))
    out.scatter_add_(-2, a.clamp(0, 25).unsqueeze(-1).expand_as(w), w)
    on_b = (b >= 24).unsqueeze(-1)
    out.scatter_add_(-2, b.clamp(0, 25).unsqueeze(-1).expand_as(w), torch.where(on_b, -w, torch.zeros_like(w)))
    return out


def total_mass(model) -> float:
    """mass (kg) of the humanoid: model = a compiled blob's path, the dict read_kpm returns, or anything with a body_mass array"""
    if isinstance(model, str):
        from .model_compiler import read_kpm
        model = read_kpm(model)
    bm = model["body_mass"] if isinstance(model, dict) else model.body_mass
    return float(torch.as_tensor(bm, dtype=torch.float64).sum())


def body_weight(model) -> float:
    """m g in newtons"""
    return total_mass(model) * GRAVITY
