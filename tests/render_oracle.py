"""fp64 numpy restatement of the offscreen renderer (kinpoly_amd/csrc/kp_render.hpp: "one pixel, exactly"), for tests/test_render_cpu.py and
tests/test_gpu_render.py: the camera, the clipping of a ray against a hull's face planes, boxes, cylinders, the floor and the shading, plus a
brute-force builder of the face planes that shares no code with the library's.

Everything works on one image at a time, vectorised over its pixels."""
from __future__ import annotations

import itertools
import math

import numpy as np

# the library's default style (kp_render_style_default): figures 0..3, objects, the two floor cells, sky
STYLE = dict(figure=[(0.8, 0.8, 0.8), (0.7, 0.0, 0.0), (0.1, 0.5, 0.1), (0.1, 0.2, 0.7)], object=(0.75, 0.6, 0.35),
             floor=[(0.45, 0.45, 0.45), (0.6, 0.6, 0.6)], sky=(0.75, 0.85, 1.0))
MAXALT = 24


def hull_planes(verts):
    """Face planes [n, 4] = (unit outward normal, d) of the convex hull of verts [m, 3]: every vertex triple whose plane has all vertices on one side
    (within 1e-9), oriented so that n.x <= d inside, duplicates (all four components within 1e-7) merged, in order of the triples."""
    V = np.asarray(verts, np.float64)
    tri = np.array(list(itertools.combinations(range(len(V)), 3)))
    a = V[tri[:, 0]]
    n = np.cross(V[tri[:, 1]] - a, V[tri[:, 2]] - a)
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 1e-14
    n, a = n[ok] / ln[ok, None], a[ok]
    d = np.einsum("ij,ij->i", n, a)
    S = n @ V.T - d[:, None]
    hi, lo = np.maximum(S.max(1), 0.0), np.minimum(S.min(1), 0.0)
    out = []
    for i in np.nonzero((hi <= 1e-9) | (lo >= -1e-9))[0]:
        p = np.append(n[i], d[i]) if hi[i] <= 1e-9 else -np.append(n[i], d[i])
        if not any(np.all(np.abs(q - p) <= 1e-7) for q in out):
            out.append(p)
    return np.array(out)


def model_planes(kpm):
    """per body: hull_planes of the blob's hull vertices"""
    verts, vadr = kpm["verts"].reshape(-1, 3), kpm["vert_adr"]
    return [hull_planes(verts[vadr[b]:vadr[b + 1]]) for b in range(24)]


def camera_rays(cam7, W, H):
    """origin [3] and unit directions [H * W, 3] of the free camera (lookat[3], distance, azimuth, elevation, fovy; degrees)"""
    c = np.asarray(cam7, np.float64)
    az, el = math.radians(c[4]), math.radians(c[5])
    f = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    r = np.cross(f, [0.0, 0.0, 1.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    th = math.tan(0.5 * math.radians(c[6]))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    sx = (2.0 * (x.ravel() + 0.5) / W - 1.0) * th * (W / H)
    sy = (1.0 - 2.0 * (y.ravel() + 0.5) / H) * th
    d = f[None] + sx[:, None] * r[None] + sy[:, None] * u[None]
    return c[:3] - c[3] * f, d / np.linalg.norm(d, axis=1, keepdims=True)


def qmat(q):
    w, x, y, z = np.asarray(q, np.float64)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def clip_planes(n, dd, ol, dl):
    """ray (ol, dl [N, 3]) against the half-spaces n.x <= dd: t_in [N], t_out [N], den [N, P], t [N, P]"""
    den = dl @ n.T
    dist = dd - n @ ol
    with np.errstate(divide="ignore", invalid="ignore"):
        t = dist[None] / den
    t_in = np.where(den < 0, t, -np.inf).max(1)
    t_out = np.where(den > 0, t, np.inf).min(1)
    t_out = np.where(((den == 0) & (dist[None] < 0)).any(1), -np.inf, t_out)
    return t_in, t_out, den, t


def render(planes, xpos, xquat, geoms, geom_ids, cam7, W, H, zfar=100.0):
    """One image.  planes: model_planes(); xpos [K, 24, 3] / xquat [K, 24, 4] body poses of the K figures; geoms [n, 17] world-frame object geoms
    (oracle.kpo.object_geoms) with their model geom indices geom_ids.  Returns dict of [H, W] arrays: geom, depth, shade (-n.dir of the hit face),
    point [H, W, 3] (the hit point) and alt [H, W, MAXALT] (figure pixels: -n.dir of every face of the hit body whose entering t lies within 1e-4
    of the largest; NaN elsewhere)."""
    o, d = camera_rays(cam7, W, H)
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
    point = o[None] + np.where(np.isfinite(best), best, 0.0)[:, None] * d
    return dict(geom=geom.reshape(H, W), depth=best.reshape(H, W), shade=shade.reshape(H, W), point=point.reshape(H, W, 3), alt=alt.reshape(H, W, MAXALT))


def edge_pixels(geom):
    """pixels whose 3 x 3 neighbourhood (clipped to the image) in the oracle's geom image is not uniform"""
    g = np.pad(geom, 1, mode="edge")
    H, W = geom.shape
    edge = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            edge |= g[dy:dy + H, dx:dx + W] != geom
    return edge


def level(base, shade):
    """the stored colour of a hit: 255 x base x (0.35 + 0.65 max(0, shade)), before rounding; base [..., 3] or [3], shade [...]"""
    return 255.0 * np.asarray(base, np.float64) * (0.35 + 0.65 * np.maximum(0.0, np.asarray(shade, np.float64)))[..., None]


def rgba_mismatch(o, rgba, style=STYLE):
    """bool [H, W]: pixels of the kernel's rgba [H, W, 4] that are outside what the oracle image o (render()) accepts: within 1 level of the hit
    face's shade -- on figure pixels of any face in the accept-set `alt`, on floor pixels whose hit point lies within 1e-3 of a cell line of either
    grey; the sky colour where nothing is hit; alpha 255 everywhere."""
    got = rgba[..., :3].astype(np.float64)
    geom, shade = o["geom"], o["shade"]
    bad = rgba[..., 3] != 255

    def off(want):
        return (np.abs(got - np.rint(want)) > 1.0).any(-1)

    sky = geom < 0
    bad |= sky & off(255.0 * np.asarray(style["sky"]))
    fl = geom == 0
    par = (np.floor(o["point"][..., 0]) + np.floor(o["point"][..., 1])).astype(np.int64) & 1
    grey = [off(level(style["floor"][i], shade)) for i in (0, 1)]
    mine = np.where(par == 1, grey[1], grey[0])
    near = (np.abs(o["point"][..., :2] - np.round(o["point"][..., :2])) < 1e-3).any(-1)
    bad |= fl & np.where(near, grey[0] & grey[1], mine)
    ob = (geom >= 25) & (geom < 100)
    bad |= ob & off(level(style["object"], shade))
    fig = ((geom >= 1) & (geom < 25)) | (geom > 100)
    for k in range(4):
        m = fig & (geom // 100 == k)
        if not m.any():
            continue
        ok = np.zeros(geom.shape, bool)
        for j in range(MAXALT):
            a = o["alt"][..., j]
            ok |= ~np.isnan(a) & ~off(level(style["figure"][k], np.nan_to_num(a)))
        bad |= m & ~ok
    return bad
