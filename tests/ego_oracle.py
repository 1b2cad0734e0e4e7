"""fp64 numpy restatement of the egocentric renderer (kinpoly_amd/csrc/kp_render_ego.hpp: "one pixel, exactly"), for tests/test_ego_cpu.py and
tests/test_gpu_ego.py: the pose camera's rays, the hit loop for a given (origin, directions), the hit point carried to frame B by the rigid motion
of what was hit, its projection through camera B, `ok`, and the cell means.  The clipping of a ray against a hull, a box and a cylinder is
tests/render_oracle.py's (whose `render` builds its own rays from the free camera, so the loop over the entities is restated here).

Everything works on one image (or one pair) at a time, vectorised over its pixels."""
from __future__ import annotations

import math

import numpy as np

from tests.render_oracle import MAXALT, clip_planes, edge_pixels, qmat

MIN_Z = 0.01          # ok = c_z > MIN_Z


def camera_axes(cam8):
    """(eye, forward, right, up, tan(fovy / 2)) of a pose-camera row: R = R(q / |q|), forward = R e_z, up = R e_y, right = -R e_x"""
    c = np.asarray(cam8, np.float64)
    R = qmat(c[3:7] / np.linalg.norm(c[3:7]))
    return c[:3], R[:, 2], -R[:, 0], R[:, 1], math.tan(0.5 * math.radians(c[7]))


def pose_rays(cam8, W, H):
    """origin [3] and unit directions [H * W, 3] of a pose camera, through the pixel centres, row 0 at the top"""
    o, f, r, u, th = camera_axes(cam8)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    sx = (2.0 * (x.ravel() + 0.5) / W - 1.0) * th * (W / H)
    sy = (1.0 - 2.0 * (y.ravel() + 0.5) / H) * th
    d = f[None] + sx[:, None] * r[None] + sy[:, None] * u[None]
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def free_camera_row(cam7):
    """the pose row [8] that sees what the free camera (lookat[3], distance, azimuth, elevation, fovy) sees: zero roll"""
    c = np.asarray(cam7, np.float64)
    az, el = math.radians(c[4]), math.radians(c[5])
    f = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    r = np.cross(f, [0.0, 0.0, 1.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return np.concatenate([c[:3] - c[3] * f, mat_quat(np.stack([-r, u, f], 1)), [c[6]]])


def mat_quat(R):
    """unit quaternion (w, x, y, z) of a rotation matrix"""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * math.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def trace(planes, xpos, xquat, geoms, geom_ids, o, d, zfar=100.0, hide_body=-1):
    """The nearest hit of every ray (o, d [N, 3]): floor up to zfar, the hulls of the K figures (xpos [K, 24, 3], xquat [K, 24, 4]) except body
    hide_body of figure 0, the world-frame object geoms [n, 17] with model indices geom_ids; first wins on a tie.  Flat [N] arrays geom, depth,
    shade and alt [N, MAXALT] with the meaning of tests/render_oracle.render."""
    N = len(d)
    best, geom, shade = np.full(N, np.inf), np.full(N, -1), np.zeros(N)
    alt = np.full((N, MAXALT), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[2] / d[:, 2]
    hit = (d[:, 2] < 0) & (t > 0) & (t <= zfar)
    best[hit], geom[hit], shade[hit] = t[hit], 0, -d[hit, 2]
    xpos, xquat = np.asarray(xpos, np.float64), np.asarray(xquat, np.float64)
    for k in range(xpos.shape[0]):
        for b in range(24):
            if k == 0 and b == hide_body:
                continue
            R = qmat(xquat[k, b])
            pl = planes[b]
            t_in, t_out, den, t = clip_planes(pl[:, :3], pl[:, 3], R.T @ (o - xpos[k, b]), d @ R)
            hit = (t_in <= t_out) & (t_in > 0) & (t_in < best)
            if not hit.any():
                continue
            first = np.where(den < 0, t, -np.inf).argmax(1)
            idx = np.nonzero(hit)[0]
            best[idx], geom[idx], shade[idx] = t_in[idx], 100 * k + 1 + b, -den[idx, first[idx]]
            cand = (den[idx] < 0) & (t[idx] >= t_in[idx, None] - 1e-4)
            assert cand.sum(1).max() <= MAXALT
            alt[idx] = np.nan
            for row, i in enumerate(idx):
                c = -den[i, cand[row]]
                alt[i, :len(c)] = c
    for g, gid in zip(np.asarray(geoms, np.float64).reshape(-1, 17), geom_ids):
        R = g[7:16].reshape(3, 3)
        ol, dl = R.T @ (o - g[4:7]), d @ R
        if g[0] == 0:
            n = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1.0]])
            t_in, t_out, den, t = clip_planes(n, np.repeat(g[1:4], 2), ol, dl)
            den_in = den[np.arange(N), np.where(den < 0, t, -np.inf).argmax(1)]
        else:
            n = np.array([[0, 0, 1], [0, 0, -1.0]])
            t_in, t_out, den, t = clip_planes(n, np.array([g[2], g[2]]), ol, dl)
            den_in = den[np.arange(N), np.where(den < 0, t, -np.inf).argmax(1)]
            a = dl[:, 0] ** 2 + dl[:, 1] ** 2
            hb = ol[0] * dl[:, 0] + ol[1] * dl[:, 1]
            c = ol[0] ** 2 + ol[1] ** 2 - g[1] ** 2
            disc = hb * hb - a * c
            with np.errstate(divide="ignore", invalid="ignore"):
                sq = np.sqrt(np.maximum(disc, 0.0))
                t0, t1 = (-hb - sq) / a, (-hb + sq) / a
            side = a > 0
            t_out = np.where(side & (disc < 0), -np.inf, np.where(side, np.minimum(t_out, t1), np.where(c > 0, -np.inf, t_out)))
            enter = side & (disc >= 0) & (t0 > t_in)
            p = ol[None] + t0[:, None] * dl
            den_in = np.where(enter, (p[:, 0] * dl[:, 0] + p[:, 1] * dl[:, 1]) / g[1], den_in)
            t_in = np.where(enter, t0, t_in)
        hit = (t_in <= t_out) & (t_in > 0) & (t_in < best)
        best[hit], geom[hit], shade[hit] = t_in[hit], 25 + gid, -den_in[hit]
        alt[hit] = np.nan
    return dict(geom=geom, depth=best, shade=shade, alt=alt)


def carry(geom, point, direction, A, B):
    """Every pixel's point in frame B and whether what it shows is there in B: floor pixels stay, a body's move with R_B R_A^T (of the body's
    normalised quaternions) about the body origins, an object geom's with the geom's world poses (absent from B: not there), sky pixels are their
    direction (a point at infinity).
    A / B: dict(xpos [K, 24, 3], xquat [K, 24, 4], geoms [n, 17], geom_ids).  Returns (p_B [N, 3], there [N] bool, infinite [N] bool)."""
    p = point.copy()
    there = np.ones(len(geom), bool)
    sky = geom < 0
    p[sky] = direction[sky]
    xa, qa, xb, qb = (np.asarray(S[k], np.float64) for S in (A, B) for k in ("xpos", "xquat"))
    for gid in np.unique(geom):
        m = geom == gid
        if gid <= 0:
            continue
        if 25 <= gid < 100:
            ga = np.asarray(A["geoms"], np.float64).reshape(-1, 17)[list(A["geom_ids"]).index(gid - 25)]
            if (gid - 25) not in list(B["geom_ids"]):
                there[m] = False
                continue
            gb = np.asarray(B["geoms"], np.float64).reshape(-1, 17)[list(B["geom_ids"]).index(gid - 25)]
            Ra, pa, Rb, pb = ga[7:16].reshape(3, 3), ga[4:7], gb[7:16].reshape(3, 3), gb[4:7]
        else:
            k, b = gid // 100, gid % 100 - 1
            Ra, pa, Rb, pb = qmat(qa[k, b] / np.linalg.norm(qa[k, b])), xa[k, b], qmat(qb[k, b] / np.linalg.norm(qb[k, b])), xb[k, b]
        p[m] = pb[None] + (point[m] - pa[None]) @ (Rb @ Ra.T).T
    return p, there, sky


def project(p_b, there, infinite, cam8_b, W, H):
    """flow [N, 2] in pixels, ok [N] and c_z [N] of the carried points through camera B"""
    eye, f, r, u, th = camera_axes(cam8_b)
    R = np.stack([-r, u, f], 1)                                    # world from camera: columns e_x, e_y, e_z
    c = np.where(infinite[:, None], p_b, p_b - eye[None]) @ R     # R^T v per pixel
    ok = there & (c[:, 2] > MIN_Z)
    with np.errstate(divide="ignore", invalid="ignore"):
        un = (W / 2.0) * (1.0 + (-c[:, 0] / c[:, 2]) / (th * W / H))
        vn = (H / 2.0) * (1.0 - (c[:, 1] / c[:, 2]) / th)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    flow = np.stack([un - (x.ravel() + 0.5), vn - (y.ravel() + 0.5)], 1)
    flow[~ok] = 0.0
    return flow, ok, c[:, 2]


def render(planes, A, cam8_a, W, H, B=None, cam8_b=None, zfar=100.0, hide_body=-1):
    """One image of frame A = dict(xpos, xquat, geoms, geom_ids) through the pose camera cam8_a, and with frame B and its camera the flow of every
    pixel.  Returns dict of [H, W(, ...)] arrays: geom, depth, shade, point, alt, edge -- and flow [H, W, 2], ok [H, W], cz [H, W] with a B side."""
    o, d = pose_rays(cam8_a, W, H)
    out = trace(planes, A["xpos"], A["xquat"], A["geoms"], A["geom_ids"], o, d, zfar, hide_body)
    point = o[None] + np.where(np.isfinite(out["depth"]), out["depth"], 0.0)[:, None] * d
    if B is not None:
        p_b, there, infinite = carry(out["geom"], point, d, A, B)
        out["flow"], out["ok"], out["cz"] = project(p_b, there, infinite, cam8_b, W, H)
    out["point"] = point
    out = {k: v.reshape((H, W) + v.shape[1:]) for k, v in out.items()}
    out["edge"] = edge_pixels(out["geom"])
    return out


def cell_means(flow, ok, gy, gx):
    """[gy, gx, 2]: the mean of flow [H, W, 2] over the ok pixels of every cell of the grid, 0 for a cell without one"""
    H, W = ok.shape
    f = np.where(ok[..., None], np.asarray(flow, np.float64), 0.0).reshape(gy, H // gy, gx, W // gx, 2).sum((1, 3))
    n = np.asarray(ok, np.float64).reshape(gy, H // gy, gx, W // gx).sum((1, 3))
    return np.where(n[..., None] > 0, f / np.maximum(n, 1.0)[..., None], 0.0)
