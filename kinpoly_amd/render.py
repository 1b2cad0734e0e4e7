"""Offscreen frames of what the engine simulates: the camera, sequences of frames and a PNG writer around KpSim.render (kp_sim_render).

The reference looks at a roll-out through MuJoCo's GL viewer (Visualizer.render / save_screen_shots; scripts/eval_uhc.py:85-131,
scripts/eval_pose_all.py:468-531).  This engine has no viewer: a HIP ray-caster draws the collision geometry (the 24 convex hulls of every figure, the
scene's boxes and cylinders, a checkered floor) into device tensors, and this module turns them into PNG files with the standard library alone.
"""
from __future__ import annotations

import math
import os
import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

FRAME_BYTE_BUDGET = 64 << 20      # render_sequence keeps the output of one launch under this many bytes


@dataclass
class Camera:
    """The viewer's free camera; the defaults are the reference visualiser's (lookat z 1.0, azimuth 45, elevation -8, distance 5, fovy 45; degrees)."""
    lookat: tuple = field(default_factory=lambda: (0.0, 0.0, 1.0))
    distance: float = 5.0
    azimuth: float = 45.0
    elevation: float = -8.0
    fovy: float = 45.0

    def row(self) -> list:
        return [float(self.lookat[0]), float(self.lookat[1]), float(self.lookat[2]), float(self.distance), float(self.azimuth), float(self.elevation), float(self.fovy)]

    def tensor(self, device, rows: int = 1):
        """[rows, 7] float32 on `device`: the layout kp_sim_render reads"""
        import torch
        return torch.tensor([self.row()], dtype=torch.float32, device=device).repeat(rows, 1).contiguous()

    def basis(self):
        """(position, forward, right, up) in fp64: forward = (cos el cos az, cos el sin az, sin el), right = normalize(forward x z), up = right x forward"""
        az, el = math.radians(self.azimuth), math.radians(self.elevation)
        f = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        r = np.cross(f, [0.0, 0.0, 1.0])
        r /= np.linalg.norm(r)
        return np.asarray(self.lookat, np.float64) - self.distance * f, f, r, np.cross(r, f)

    def rays(self, width: int, height: int):
        """(origin [3], directions [H, W, 3]) in fp64: unit rays through the pixel centres ((x + .5) / W, (y + .5) / H), row 0 at the top"""
        o, f, r, u = self.basis()
        th = math.tan(0.5 * math.radians(self.fovy))
        sx = (2.0 * (np.arange(width) + 0.5) / width - 1.0) * th * (width / height)
        sy = (1.0 - 2.0 * (np.arange(height) + 0.5) / height) * th
        d = f[None, None] + sx[None, :, None] * r[None, None] + sy[:, None, None] * u[None, None]
        return o, d / np.linalg.norm(d, axis=2, keepdims=True)


def follow(qpos, camera: Camera | None = None):
    """The visualiser's --focus: a camera per row whose lookat.xy is the row's root xy (qpos [R, >= 2] device tensor -> [R, 7] on its device)."""
    cam = (camera or Camera()).tensor(qpos.device, qpos.shape[0])
    cam[:, :2] = qpos[:, :2].to(cam.dtype)
    return cam


def render_sequence(sim, figures, obj_pose=None, camera=None, width: int = 320, height: int = 240, focus: bool = True, style=None,
                    byte_budget: int = FRAME_BYTE_BUDGET):
    """Frames of a take: figures = one [T,76] array or a list of them (figure 0 simulated, figure 1 expert, ...; cut to the shortest), obj_pose [T,35]
    or None -> uint8 [T, H, W, 4] on the host.  focus: the camera follows figure 0's root.  The frames are rendered in chunks whose device output
    (4 bytes per pixel) stays under byte_budget."""
    import torch
    figs = [figures] if getattr(figures, "ndim", 0) == 2 else list(figures)
    T = min(len(f) for f in figs)
    if obj_pose is not None:
        T = min(T, len(obj_pose))
    dev = sim.device
    q = torch.stack([torch.as_tensor(np.asarray(f[:T], np.float32)[:, :76]) for f in figs], 1).to(dev).contiguous()
    op = None if obj_pose is None else torch.as_tensor(np.asarray(obj_pose[:T], np.float32)).to(dev).contiguous()
    chunk = max(1, int(byte_budget) // (4 * int(width) * int(height)))
    out = np.empty((T, height, width, 4), np.uint8)
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        cam = follow(q[a:b, 0], camera) if focus else (camera if camera is not None else Camera())
        out[a:b] = sim.render(q[a:b].contiguous(), None if op is None else op[a:b].contiguous(), cam, width, height, ("rgba",), style)["rgba"].cpu().numpy()
    return out


def render_env(sim, obj_qpos, envs=None, camera=None, width: int = 320, height: int = 240):
    """render_rgb of the batched envs: figure 0 = the simulated pose, figure 1 = the simulator's target pose (the kinematic target / the expert frame),
    the env's objects when it has any -> uint8 [n, H, W, 4] on the device.  camera None: the default camera following every env's root."""
    import torch
    q = torch.stack([sim.get("qpos"), sim.get("target_qpos")], 1)
    if envs is not None:
        idx = torch.as_tensor(envs, device=sim.device).long()
        q = q[idx]
        obj_qpos = None if obj_qpos is None else obj_qpos[idx]
    cam = follow(q[:, 0]) if camera is None else camera
    return sim.render(q.contiguous(), None if obj_qpos is None else obj_qpos.contiguous(), cam, width, height, ("rgba",))["rgba"]


def write_png(path: str, array) -> None:
    """uint8 [H, W], [H, W, 3] or [H, W, 4] -> an 8-bit grey / RGB / RGBA PNG (zlib and struct only: no imaging library is needed)."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3, 4)) or a.size == 0:
        raise ValueError(f"write_png: expected a non-empty uint8 [H,W], [H,W,3] or [H,W,4] array, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    raw = np.zeros((h, 1 + w * ch), np.uint8)          # every scanline starts with filter type 0
    raw[:, 1:] = a.reshape(h, w * ch)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b"")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(png)
