"""The scenes, cameras and fp64 oracle images that tests/test_ego_cpu.py and tests/test_gpu_ego.py share: the CPU file holds every oracle image to
the edge-share cap before the GPU file compares a kernel against it.

Frame A is the pose of tests/golden/standing_neutral.npz (the figure faces +y), bare or with chair, box, table, can and step 0.6 to 1.0 m around
it; frame B a seeded perturbation of A (joints +-0.05 rad, root moved 3 cm and yawed 3 degrees, the box pushed 2 cm).  Every number is rounded to
fp32 before the oracle or the kernel sees it.  A scene is dict(xpos [K, 24, 3], xquat [K, 24, 4], blk [35] or None, geoms [n, 17], geom_ids)."""
import functools
import os

import numpy as np

from kinpoly_amd.model_compiler import STEP_KPM, read_kpm
from kinpoly_amd.render import HeadCamera
from oracle.kpo import OracleSim, object_geoms
from tests import ego_oracle as EO
from tests import render_oracle as RO
from tests.pose_oracle import live_geoms

KPM = read_kpm(STEP_KPM)
STANDING = np.load(os.path.join(os.path.dirname(__file__), "golden", "standing_neutral.npz"))["qpos"].astype(np.float64)
HEAD = 13
EDGE_CAP = 0.30
OK_BAND = 1e-5                    # pixels whose oracle c_z lies this close to the ok threshold are exempt from the flow / ok comparison
SIZES = ((64, 64), (37, 50))      # (W, H)
PITCHES = (0.0, 30.0)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def planes():
    return RO.model_planes(KPM)


def yaw(a):
    return np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)])


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def parked():
    blk = np.zeros(35)
    for i in range(5):
        blk[7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    return blk


def objects_block():
    """chair, box, table, can and step around the standing figure (which faces +y): 0.6 to 1.0 m from its root"""
    x, y = STANDING[0], STANDING[1]
    blk = parked()
    for oi, pose in {0: [x + 0.60, y + 0.50, 0.38] + list(yaw(0.7)), 1: [x - 0.40, y + 0.70, 0.3] + list(yaw(-0.4)), 2: [x + 0.10, y + 0.95, 0.6] + list(yaw(0.2)),
                     3: [x - 0.60, y + 0.30, 0.15, 1.0, 0.0, 0.0, 0.0], 4: [x + 0.30, y - 0.70, 0.3705] + list(yaw(1.1))}.items():
        blk[7 * oi: 7 * oi + 7] = pose
    return f32(blk)


@functools.lru_cache(maxsize=None)
def _oracle_sim():
    return OracleSim(kpm=STEP_KPM)


def scene(qpos_list, blk=None):
    """body poses of the figures (OracleSim's forward kinematics) and the world-frame object geoms, rounded to fp32"""
    o = _oracle_sim()
    xp, xq = [], []
    for q in qpos_list:
        o.reset(np.asarray(q, np.float64), np.zeros(75))
        xp.append(f32(o.get("xpos")).reshape(24, 3)); xq.append(f32(o.get("xquat")).reshape(24, 4))
    geoms, ids = (np.zeros((0, 17)), []) if blk is None else (object_geoms(KPM, blk), live_geoms(KPM, blk))
    return dict(xpos=np.stack(xp), xquat=np.stack(xq), blk=blk, geoms=geoms, geom_ids=ids)


def second_figure(q):
    """the wearer's pose again, 1.3 m ahead and 0.5 m to the side: beyond the objects, where a 37 x 50 image keeps enough pixels off an edge"""
    q2 = np.array(q, np.float64)
    q2[0] += 0.5; q2[1] += 1.3
    return q2


def perturbed(q, seed):
    rng = np.random.default_rng(seed)
    p = np.array(q, np.float64)
    p[7:] += rng.uniform(-0.05, 0.05, 69)
    a = rng.uniform(0, 2 * np.pi)
    p[:3] += 0.03 * np.array([np.cos(a) * 0.8, np.sin(a) * 0.8, 0.6])
    p[3:7] = qmul(yaw(np.radians(3.0)), p[3:7])
    return p


@functools.lru_cache(maxsize=None)
def frame_a(objects: bool, figures: int = 1):
    qs = [STANDING] + ([second_figure(STANDING)] if figures == 2 else [])
    return scene(qs, objects_block() if objects else None)


@functools.lru_cache(maxsize=None)
def frame_b(seed: int, figures: int = 1):
    """the seeded perturbation of frame A with objects: the box (object 1) pushed 2 cm"""
    qs = [perturbed(STANDING, seed)] + ([perturbed(second_figure(STANDING), seed + 100)] if figures == 2 else [])
    blk = objects_block().copy()
    a = np.random.default_rng(seed + 1000).uniform(0, 2 * np.pi)
    blk[7:9] += 0.02 * np.array([np.cos(a), np.sin(a)])
    return scene(qs, f32(blk))


def head_row(sc, pitch=0.0, fovy=90.0):
    """the fp32-rounded pose-camera row of a HeadCamera on figure 0's head"""
    return f32(HeadCamera(fovy=fovy, pitch=pitch).row(sc["xpos"][0, HEAD], sc["xquat"][0, HEAD]))


# ------------------------------------------------------------------ still images
STILL = [(W, H, p, ob) for W, H in SIZES for p in PITCHES for ob in (False, True)]
STILL_IDS = [f"{W}x{H}-{'down30' if p else 'level'}-{'objects' if ob else 'floor'}" for W, H, p, ob in STILL]


@functools.lru_cache(maxsize=None)
def still_case(W, H, pitch, objects):
    sc = frame_a(objects)
    cam = head_row(sc, pitch)
    return sc, cam, EO.render(planes(), sc, cam, W, H)


# ------------------------------------------------------------------ flow: three rows (seeds 1..3; level, 20 down, 10 down), one or two figures.
# 30 down with the objects AND a second figure leaves 34 % of a 37 x 50 image on an edge, above the cap; the stills cover 30 down
FLOW = [(W, H, k) for W, H in SIZES for k in (1, 2)]
FLOW_IDS = [f"{W}x{H}-{k}fig" for W, H, k in FLOW]
FLOW_PITCH = (0.0, 20.0, 10.0)


@functools.lru_cache(maxsize=None)
def flow_row(W, H, figures, r, shared_camera):
    """row r of a flow case -> (A, B, cam_a, cam_b, oracle image).  shared_camera: every row is seen through row 0's pair of cameras (camera_rows = 1)"""
    A, B = frame_a(True, figures), frame_b(1 + r, figures)
    c = 0 if shared_camera else r
    cam_a, cam_b = head_row(frame_a(True, figures), FLOW_PITCH[c]), head_row(frame_b(1 + c, figures), FLOW_PITCH[c])
    return A, B, cam_a, cam_b, EO.render(planes(), A, cam_a, W, H, B, cam_b)


def exempt(o):
    """edge pixels plus the ok band"""
    return o["edge"] | (np.abs(o["cz"] - EO.MIN_Z) <= OK_BAND)


# ------------------------------------------------------------------ closed forms
def rotated_row(cam8, axis, degrees):
    """the camera turned by `degrees` about one of its own axes ('forward', 'up'), the eye unchanged"""
    a = 0.5 * np.radians(degrees)
    local = {"forward": [0.0, 0.0, 1.0], "up": [0.0, 1.0, 0.0]}[axis]
    out = np.array(cam8, np.float64)
    out[3:7] = qmul(out[3:7] / np.linalg.norm(out[3:7]), np.concatenate([[np.cos(a)], np.sin(a) * np.asarray(local)]))
    return out


def homography_flow(cam_a, cam_b, W, H):
    """the flow of every pixel under a pure camera rotation (same eye, same fovy): x' ~ K R_B^T R_A K^-1 x, independent of what the pixel shows"""
    _, fa, ra, ua, th = EO.camera_axes(cam_a)
    _, fb, rb, ub, thb = EO.camera_axes(cam_b)
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    sx, sy = (2.0 * x / W - 1.0) * th * (W / H), (1.0 - 2.0 * y / H) * th
    d = fa[None, None] + sx[..., None] * ra[None, None] + sy[..., None] * ua[None, None]
    cx, cy, cz = d @ rb, d @ ub, d @ fb
    return np.stack([(W / 2.0) * (1.0 + (cx / cz) / (thb * W / H)) - x, (H / 2.0) * (1.0 - (cy / cz) / thb) - y], -1), cz


def down_row(eye, fovy=90.0):
    """a camera at `eye` looking straight down (forward = -z), up = +y"""
    return np.concatenate([np.asarray(eye, np.float64), EO.mat_quat(np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])), [fovy]])


def empty_scene():
    """one figure parked far below the horizon's reach of a downward camera: 60 m to the side (the kernel always draws figure 0)"""
    q = STANDING.copy()
    q[0] += 60.0
    return scene([q], None)
