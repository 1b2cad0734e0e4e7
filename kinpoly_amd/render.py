"""Offscreen frames of what the engine simulates: the camera, sequences of frames and a PNG writer around KpSim.render (kp_sim_render); and the
wearer's own view around KpSim.render_ego (kp_sim_render_ego): a camera on the head, first-person frames and per-frame optical-flow features.

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


HEAD_BODY = 13                    # body "Head" of the SMPL tree; its frame on the shipped blobs: +z forward, +y up, +x to the figure's left


def _qmat64(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def _qmul64(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


_HEAD_CENTROID = {}


def head_hull_centroid(kpm_path: str | None = None):
    """The vertex centroid of the head hull in the head's frame, read from a model blob (default: the shipped one): (-0.0065, 0.1096, -0.0272), which
    lies 7.8 cm inside every face of the hull -- an eye there never sees the head (a camera inside a hull does not see it)."""
    from .model_compiler import DEFAULT_KPM, read_kpm
    path = kpm_path or DEFAULT_KPM
    if path not in _HEAD_CENTROID:
        m = read_kpm(path)
        adr = np.asarray(m["vert_adr"]).astype(np.int64)
        _HEAD_CENTROID[path] = np.asarray(m["verts"], np.float64).reshape(-1, 3)[adr[HEAD_BODY]:adr[HEAD_BODY + 1]].mean(0)
    return _HEAD_CENTROID[path].copy()


@dataclass
class HeadCamera:
    """A camera that rides on the head body: the eye at `offset` in the head's frame (None: the head hull's vertex centroid), looking along the head's
    +z with the head's +y up, pitched by `pitch` degrees about the camera's right axis (positive looks down); fovy in degrees.  hide_head: do not
    draw the head hull (for an offset outside it)."""
    offset: tuple | None = None
    fovy: float = 90.0
    pitch: float = 0.0
    hide_head: bool = False

    def eye_offset(self):
        return head_hull_centroid() if self.offset is None else np.asarray(self.offset, np.float64)

    def pitch_quat(self):
        """the pitch in the camera's own frame: looking down is a positive turn about +x (the right axis is -x)"""
        a = 0.5 * math.radians(self.pitch)
        return np.array([math.cos(a), math.sin(a), 0.0, 0.0])

    @property
    def hide_body(self) -> int:
        return HEAD_BODY if self.hide_head else -1

    def row(self, head_pos, head_quat):
        """the pose-camera row [8] in fp64: eye[3], quaternion[4] (w, x, y, z; world from camera), fovy"""
        hq = np.asarray(head_quat, np.float64)
        eye = np.asarray(head_pos, np.float64) + _qmat64(hq) @ self.eye_offset()
        return np.concatenate([eye, _qmul64(hq / np.linalg.norm(hq), self.pitch_quat()), [float(self.fovy)]])

    def rows(self, wbpos, wbquat):
        """[R, 8] float32 on the device of wbpos [R, 72] / wbquat [R, 96] (fk()'s body poses): the layout kp_sim_render_ego reads"""
        import torch
        hp, hq = wbpos[:, 3 * HEAD_BODY: 3 * HEAD_BODY + 3], wbquat[:, 4 * HEAD_BODY: 4 * HEAD_BODY + 4]
        off = torch.tensor(self.eye_offset(), dtype=hp.dtype, device=hp.device)
        w, v = hq[:, :1], hq[:, 1:]
        t = 2.0 * torch.linalg.cross(v, off.expand_as(v))
        eye = hp + off + w * t + torch.linalg.cross(v, t)
        pw, px = float(self.pitch_quat()[0]), float(self.pitch_quat()[1])            # hq x (pw, px, 0, 0)
        q = torch.stack([hq[:, 0] * pw - hq[:, 1] * px, hq[:, 0] * px + hq[:, 1] * pw, hq[:, 2] * pw + hq[:, 3] * px, hq[:, 3] * pw - hq[:, 2] * px], 1)
        return torch.cat([eye, q, torch.full_like(hp[:, :1], float(self.fovy))], 1).contiguous()

    def imu(self, sim, qpos, dt: float, take_off=None):
        """(gyro [T, 3], accel [T, 3]) of an IMU at the camera's eye, in the HEAD's frame, for the frames ego_sequence renders of qpos [T, 76]:
        dynamics.motion_derivatives' qvel / qacc, one KpSim.body_motion call, dynamics.body_imu on the head body (device tensors)"""
        import torch
        from . import dynamics
        q = torch.as_tensor(np.asarray(qpos, np.float32)[:, :76]).to(sim.device).contiguous()
        qvel, qacc = dynamics.motion_derivatives(q, dt, take_off)
        motion = sim.body_motion(q, qvel.contiguous(), qacc.contiguous(), outputs=("body_vel", "body_acc"))
        return dynamics.body_imu(motion, sim.fk(q)["wbquat"], HEAD_BODY, self.eye_offset())

    def basis(self, head_pos, head_quat):
        """(eye, forward, right, up) in fp64: forward = R e_z, up = R e_y, right = -R e_x of the camera's quaternion"""
        r = self.row(head_pos, head_quat)
        R = _qmat64(r[3:7])
        return r[:3], R[:, 2], -R[:, 0], R[:, 1]

    def rays(self, head_pos, head_quat, width: int, height: int):
        """(origin [3], directions [H, W, 3]) in fp64: unit rays through the pixel centres, row 0 at the top"""
        o, f, r, u = self.basis(head_pos, head_quat)
        th = math.tan(0.5 * math.radians(self.fovy))
        sx = (2.0 * (np.arange(width) + 0.5) / width - 1.0) * th * (width / height)
        sy = (1.0 - 2.0 * (np.arange(height) + 0.5) / height) * th
        d = f[None, None] + sx[None, :, None] * r[None, None] + sy[:, None, None] * u[None, None]
        return o, d / np.linalg.norm(d, axis=2, keepdims=True)


def flow_grid(dim: int) -> int:
    """g of a feature width dim = 2 g^2 (512 -> 16, 128 -> 8); anything else is refused"""
    g = int(round(math.sqrt(max(int(dim), 0) / 2.0)))
    if g < 1 or 2 * g * g != int(dim):
        raise ValueError(f"ego_flow_features: dim must be 2 g^2 for a whole g (512 = a 16 x 16 grid, 128 = 8 x 8), got dim = {dim}")
    return g


def ego_sequence(sim, qpos, obj_pose=None, camera: HeadCamera | None = None, width: int = 128, height: int = 128, style=None, byte_budget: int = FRAME_BYTE_BUDGET):
    """What the wearer sees over a take: qpos [T,76], obj_pose [T,35] or None -> uint8 [T, H, W, 4] on the host, rendered in chunks whose device
    output stays under byte_budget."""
    import torch
    camera = camera or HeadCamera()
    T = len(qpos) if obj_pose is None else min(len(qpos), len(obj_pose))
    dev = sim.device
    q = torch.as_tensor(np.asarray(qpos[:T], np.float32)[:, :76]).to(dev).contiguous()
    op = None if obj_pose is None else torch.as_tensor(np.asarray(obj_pose[:T], np.float32)).to(dev).contiguous()
    chunk = max(1, int(byte_budget) // (4 * int(width) * int(height)))
    out = np.empty((T, height, width, 4), np.uint8)
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        out[a:b] = sim.render_ego(q[a:b].contiguous(), None if op is None else op[a:b].contiguous(), camera, width=width, height=height, want=("rgba",),
                                  hide_body=camera.hide_body, style=style)["rgba"].cpu().numpy()
    return out


def ego_flow_features(sim, qpos, obj_pose=None, dim: int = 512, size: int = 128, camera: HeadCamera | None = None, scale: float = 30.0, rows_per_call: int = 2048):
    """Per-frame optical-flow features of a take, from the head camera: qpos [T,76], obj_pose [T,35] or None -> float32 [T, dim] on the host.
    dim = 2 g^2; row t is the mean flow (kp_sim_render_ego's cells) of the frame pair (t - 1 -> t) over a g x g grid of a size x size image, divided
    by the focal length in pixels ((size / 2) / tan(fovy / 2)) and multiplied by scale: image-plane velocity in focal lengths per second for
    scale = the frame rate (30 Hz).  Row 0 is zeros.  The layout of a row is [g (top to bottom), g (left to right), (u, v)]."""
    import torch
    g = flow_grid(dim)
    if int(size) < 8 * g or int(size) % (8 * g) != 0:
        raise ValueError(f"ego_flow_features: size must be a multiple of 8 g = {8 * g} for dim = {dim}, got size = {size}")
    camera = camera or HeadCamera()
    T = len(qpos) if obj_pose is None else min(len(qpos), len(obj_pose))
    out = np.zeros((T, int(dim)), np.float32)
    if T < 2:
        return out
    dev = sim.device
    q = torch.as_tensor(np.asarray(qpos[:T], np.float32)[:, :76]).to(dev).contiguous()
    op = None if obj_pose is None else torch.as_tensor(np.asarray(obj_pose[:T], np.float32)).to(dev).contiguous()
    k = float(scale) / ((0.5 * int(size)) / math.tan(0.5 * math.radians(camera.fovy)))
    for a in range(0, T - 1, int(rows_per_call)):
        b = min(T - 1, a + int(rows_per_call))
        cells = sim.render_ego(q[a:b].contiguous(), None if op is None else op[a:b].contiguous(), camera, q[a + 1:b + 1].contiguous(),
                               None if op is None else op[a + 1:b + 1].contiguous(), camera, width=int(size), height=int(size), want=("cells",), grid=g,
                               hide_body=camera.hide_body)["cells"]
        out[a + 1:b + 1] = (cells.reshape(b - a, int(dim)) * k).cpu().numpy()
    return out


def render_env_ego(sim, obj_qpos, envs=None, camera: HeadCamera | None = None, width: int = 64, height: int = 64):
    """render_ego of the batched envs: what every env's simulated figure sees from its head, with the env's objects -> uint8 [n, H, W, 4] on the device."""
    import torch
    camera = camera or HeadCamera()
    q = sim.get("qpos")
    if envs is not None:
        idx = torch.as_tensor(envs, device=sim.device).long()
        q = q[idx]
        obj_qpos = None if obj_qpos is None else obj_qpos[idx]
    return sim.render_ego(q.contiguous(), None if obj_qpos is None else obj_qpos.contiguous(), camera, width=width, height=height, want=("rgba",),
                          hide_body=camera.hide_body)["rgba"]


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
