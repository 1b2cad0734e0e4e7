"""Balance of a motion: the centre of mass, the capture point and the zero-moment point against the support polygon.

The centroidal quantities come from KpSim.body_motion (kp_sim_body_motion), the support polygon from the contact rows of KpSim.inverse_dynamics on the
same rows.  Everything but centroidal() and balance_sequence() is plain torch / numpy on whatever device its inputs live; the hull runs on the host
(a monotone chain over at most 64 points per row).  The floor is the plane z = 0, gravity points along -z with magnitude g.
"""
from __future__ import annotations

import numpy as np
import torch

from . import dynamics
from .sim import CENTROID_FIELDS

MAXPTS = 64                       # contact rows per frame (kp_sim_inverse_dynamics' contact output)
FLOOR_Z = 0.05                    # a contact on the world (B = -1) counts as a FLOOR contact when its normal is +z and it lies below this height


def centroidal(sim, qpos, qvel=None, qacc=None) -> dict:
    """KpSim.body_motion's centroid rows by name: com, com_vel, L_com, com_acc, Ldot_com [..., 3]; ke, pe, mass [...] (device tensors)"""
    c = sim.body_motion(qpos, qvel, qacc, outputs=("centroid",))["centroid"]
    return {k: c[..., s] for k, s in CENTROID_FIELDS.items()}


def _hull(pts: np.ndarray) -> np.ndarray:
    """convex hull of pts [n, 2], counter-clockwise, no repeated and no collinear vertex (Andrew's monotone chain); n = 0, 1, 2 and degenerate sets
    return the 0, 1 or 2 extreme points"""
    pts = np.unique(np.asarray(pts, np.float64).reshape(-1, 2), axis=0)            # sorted by x, then y; duplicates dropped
    if len(pts) <= 2:
        return pts

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0.0:
                out.pop()
            out.append(p)
        return out

    lo, up = half(pts), half(pts[::-1])
    return np.array(lo[:-1] + up[:-1])


def support_polygon(contact, ncon):
    """The support polygon of every row: contact [T, 64, 12], ncon [T] as inverse_dynamics(..., want=("contact", "ncon")) returns them -> (poly [T, 64, 2],
    npoly [T]) on the host, float64 / int64: the convex hull (counter-clockwise) of the floor-contact points, rows past npoly zero.  npoly = 0: no
    floor contact; 1 and 2: a point and a segment."""
    c = torch.as_tensor(contact).detach().cpu().numpy().astype(np.float64).reshape(-1, MAXPTS, 12)
    n = torch.as_tensor(ncon).detach().cpu().numpy().astype(np.int64).reshape(-1)
    poly, npoly = np.zeros((len(c), MAXPTS, 2)), np.zeros(len(c), np.int64)
    for t in range(len(c)):
        r = c[t, :min(max(int(n[t]), 0), MAXPTS)]
        r = r[(r[:, 1] == -1.0) & (r[:, 8] > 0.99) & (r[:, 5] < FLOOR_Z)]
        h = _hull(r[:, 3:5])
        poly[t, :len(h)] = h; npoly[t] = len(h)
    return poly, npoly


def capture_point(com, com_vel, g: float = 9.81):
    """com_xy + v_xy sqrt(z_com / g) of the linear inverted pendulum [..., 2]; z_com <= 0 gives the ground projection itself"""
    com, com_vel = torch.as_tensor(com), torch.as_tensor(com_vel)
    return com[..., :2] + com_vel[..., :2] * (com[..., 2:3].clamp_min(0.0) / g).sqrt()


def zmp(com, com_acc, Ldot_com, mass, g: float = 9.81):
    """The zero-moment point on the floor z = 0 [..., 2]: where the contact force F = m (com_acc + g e_z) has to act so that its moment about the
    centre of mass has the horizontal components of Ldot_com.  NaN where F_z <= 0 (free fall or faster: no such point)."""
    com, acc, Ld = torch.as_tensor(com), torch.as_tensor(com_acc), torch.as_tensor(Ldot_com)
    m = torch.as_tensor(mass, dtype=com.dtype, device=com.device)
    F = m[..., None] * acc if m.dim() else m * acc
    Fz = F[..., 2] + m * g
    Fz = torch.where(Fz > 0.0, Fz, torch.full_like(Fz, float("nan")))
    px = com[..., 0] + (-com[..., 2] * F[..., 0] - Ld[..., 1]) / Fz
    py = com[..., 1] + (Ld[..., 0] - com[..., 2] * F[..., 1]) / Fz
    return torch.stack([px, py], -1)


def margin(point, polygon):
    """Signed distance of point [T, 2] to the polygon of its row (support_polygon's pair): positive inside, -distance outside (a point or a segment
    has no inside: <= 0), NaN for a row without a polygon.  Host, float64 [T]."""
    poly, npoly = polygon
    p = torch.as_tensor(point).detach().cpu().numpy().astype(np.float64).reshape(-1, 2)
    T = len(p)
    out = np.full(T, np.nan)
    k = np.arange(MAXPTS)[None]
    nn = np.maximum(npoly, 1)[:, None]
    a = poly[np.arange(T)[:, None], k % nn]; b = poly[np.arange(T)[:, None], (k + 1) % nn]          # edges; past npoly they repeat earlier ones
    ab, ap = b - a, p[:, None] - a
    den = (ab * ab).sum(-1)
    t = np.clip(np.where(den > 0.0, (ap * ab).sum(-1) / np.where(den > 0.0, den, 1.0), 0.0), 0.0, 1.0)
    dist = np.linalg.norm(ap - t[..., None] * ab, axis=-1).min(1)
    cross = ab[..., 0] * ap[..., 1] - ab[..., 1] * ap[..., 0]
    inside = (npoly >= 3) & (cross >= 0.0).all(1)
    has = npoly > 0
    out[has] = np.where(inside, dist, -dist)[has]
    return out


def balance(centroid, contact, ncon, g: float = 9.81) -> dict:
    """Balance scores of rows: centroid [T, 18], contact [T, 64, 12], ncon [T].  Per frame (host, float64 [T]) com_margin, xcom_margin, zmp_margin: signed
    distance of the centre of mass' ground projection, of the capture point and of the zero-moment point to the support polygon (NaN without floor
    contact; zmp_margin also where the contact force would have to pull).  Summary: stable_frac = frames with floor contact whose capture point lies
    inside the polygon / frames with floor contact (NaN if none); airborne_frac = frames without floor contact / T; zmp_out_mean = mean distance of the
    zero-moment point outside the polygon over the frames that have one (inside counts 0)."""
    c = torch.as_tensor(centroid).detach().double().cpu().reshape(-1, 18)
    f = {k: c[:, s] for k, s in CENTROID_FIELDS.items()}
    poly = support_polygon(contact, ncon)
    out = {"com_margin": margin(f["com"][:, :2], poly), "xcom_margin": margin(capture_point(f["com"], f["com_vel"], g), poly),
           "zmp_margin": margin(zmp(f["com"], f["com_acc"], f["Ldot_com"], f["mass"], g), poly), "npoly": poly[1]}
    out.update(summary(out))
    return out


def summary(frames: dict, rows=slice(None)) -> dict:
    """stable_frac, airborne_frac, zmp_out_mean (balance()'s docstring) over the frames `rows` of balance()'s per-frame arrays"""
    npoly, xcom, zm = frames["npoly"][rows], frames["xcom_margin"][rows], frames["zmp_margin"][rows]
    grounded = npoly > 0
    z = zm[grounded]
    z = z[np.isfinite(z)]
    return {"stable_frac": float((xcom[grounded] > 0.0).mean()) if grounded.any() else float("nan"),
            "airborne_frac": float((~grounded).mean()) if len(grounded) else float("nan"),
            "zmp_out_mean": float(np.maximum(-z, 0.0).mean()) if len(z) else float("nan")}


def balance_sequence(sim, qpos_seq, dt: float, take_off=None, g: float = 9.81) -> dict:
    """balance() of a pose sequence qpos_seq [T, 76] that was never simulated: dynamics.motion_derivatives for qvel / qacc (take_off: row offsets of takes
    stored back to back, no difference crosses a boundary), ONE body_motion call and ONE inverse_dynamics call for all rows."""
    q = torch.as_tensor(qpos_seq).to(sim.device, torch.float32).contiguous()
    qvel, qacc = dynamics.motion_derivatives(q, dt, take_off)
    qvel, qacc = qvel.contiguous(), qacc.contiguous()
    cen = sim.body_motion(q, qvel, qacc, outputs=("centroid",))["centroid"]
    inv = sim.inverse_dynamics(q, qvel, qacc, want=("contact", "ncon"))
    out = balance(cen, inv["contact"], inv["ncon"], g)
    out["centroid"], out["qvel"], out["qacc"] = cen, qvel, qacc
    return out
