"""The offscreen renderer (kp_sim_render / KpSim.render / render_rgb) on a real MI355X against the fp64 restatement tests/render_oracle.py.

Scenes: A = the standing pose (qpos = 0, root z 0.92, unit quaternion); B = a seeded random pose (joints uniform +-0.6 rad, root quaternion
(0.7, 0.1, 0.2, 0.68)) with chair, box, table, can and step placed within 1.5 m.  Both are close-ups (lookat = the root): at the viewer's default 5 m a
body has almost no interior pixels at these sizes.  Body poses come from OracleSim.reset, object geoms from oracle.kpo.object_geoms.

An edge pixel -- one whose 3 x 3 neighbourhood in the ORACLE's geom image is not uniform -- is exempt from every comparison; the oracle images are
held to conditions of their own (edge share, interior figure pixels) before the kernel is looked at.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from kinpoly_amd.model_compiler import STEP_KPM, read_kpm  # noqa: E402
from oracle.kpo import OracleSim, object_geoms  # noqa: E402
from tests import render_oracle as RO  # noqa: E402
from tests.pose_oracle import live_geoms  # noqa: E402

KPM = read_kpm(STEP_KPM)

# depth along the ray against the fp64 oracle, relative, on non-edge pixels: the largest error seen on the MI355X over the scenes and cameras of this
# file (printed by every comparison below), and the bound = four times that (the kernel multiplies by v_rcp_f32 where the oracle divides).  The largest
# is a floor pixel of the 65-row test seen at a grazing angle (t = -o.z / d.z: the fp32 rounding of a small d.z, 6e-8 absolute, is that share of it);
# the hull and object pixels stay below 9e-7 (B 64x96: 8.6e-7, A 37x50: 6.4e-7, A 64x64: 4.6e-7, two figures: 3.0e-7)
DEPTH_REL_MEASURED = 2.094e-6
DEPTH_REL_BOUND = 4 * DEPTH_REL_MEASURED

CLOSE = (1.5, 45.0, -8.0)          # distance, azimuth, elevation
HIGH = (2.5, 135.0, -30.0)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def planes():
    return RO.model_planes(KPM)


def parked():
    blk = np.zeros(35)
    for i in range(5):
        blk[7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    return blk


def yaw(a):
    return [np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)]


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(xpos [24, 3], xquat [24, 4], blk [35] or None, root [3]), every number rounded to fp32 (what the kernel is given)"""
    q = np.zeros(76)
    blk = None
    if name == "A":
        q[2], q[3] = 0.92, 1.0
    else:
        rng = np.random.default_rng(11)
        q[:3] = [0.3, -0.2, 0.95]
        q[3:7] = np.array([0.7, 0.1, 0.2, 0.68]) / np.linalg.norm([0.7, 0.1, 0.2, 0.68])
        q[7:] = rng.uniform(-0.6, 0.6, 69)
        blk = parked()
        x, y = q[0], q[1]
        for oi, pose in {0: [x + 0.9, y + 0.5, 0.38] + yaw(0.7), 1: [x - 0.5, y + 0.9, 0.3] + yaw(-0.4), 2: [x + 0.3, y - 1.1, 0.6] + yaw(0.2),
                         3: [x - 0.7, y - 0.5, 0.15, 1.0, 0.0, 0.0, 0.0], 4: [x + 0.2, y + 1.2, 0.3705] + yaw(1.1)}.items():
            blk[7 * oi: 7 * oi + 7] = pose
        blk = f32(blk)
    o = OracleSim(kpm=STEP_KPM)
    o.reset(q, np.zeros(75))
    return dict(xpos=f32(o.get("xpos")).reshape(24, 3), xquat=f32(o.get("xquat")).reshape(24, 4), blk=blk, root=f32(q[:3]))


def camera(sc, dist, az, el):
    return f32(list(sc["root"]) + [dist, az, el, 45.0])


def oracle_image(xpos, xquat, blk, cam, W, H, zfar=100.0):
    geoms, ids = (np.zeros((0, 17)), []) if blk is None else (object_geoms(KPM, blk), live_geoms(KPM, blk))
    o = RO.render(planes(), np.asarray(xpos).reshape(-1, 24, 3), np.asarray(xquat).reshape(-1, 24, 4), geoms, ids, cam, W, H, zfar)
    o["edge"] = RO.edge_pixels(o["geom"])
    return o


@functools.lru_cache(maxsize=None)
def oracle_case(name, W, H, view):
    sc = scene(name)
    return oracle_image(sc["xpos"], sc["xquat"], sc["blk"], camera(sc, *view), W, H)


@pytest.fixture(scope="module")
def sim():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim.KpSim(kpsim.KpModel(STEP_KPM), 4)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def run(sim, xpos, xquat, blk, cam, W, H, style=None):
    """xpos [R, K, 24, 3] ... -> dict of numpy arrays [R, H, W(, 4)]"""
    xpos, xquat = np.asarray(xpos), np.asarray(xquat)
    R, K = xpos.shape[:2]
    out = sim.render_poses(dev(xpos.reshape(R, K, 72)), dev(xquat.reshape(R, K, 96)), None if blk is None else dev(np.asarray(blk).reshape(R, 35)),
                           dev(np.asarray(cam).reshape(-1, 7)), W, H, ("rgba", "geom", "depth"), style)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(got, o, what):
    """geom equal, depth within DEPTH_REL_BOUND, rgba within the oracle's accept-set, all on the oracle's non-edge pixels; returns the depth error"""
    inner = ~o["edge"]
    hit = inner & np.isfinite(o["depth"])
    ngeom = int((got["geom"] != o["geom"])[inner].sum())
    inf_ok = bool(np.all(np.isposinf(got["depth"][inner & ~hit])))
    with np.errstate(invalid="ignore"):
        rel = float((np.abs(got["depth"][hit] - o["depth"][hit]) / o["depth"][hit]).max()) if hit.any() else 0.0
    nrgba = int((RO.rgba_mismatch(o, got["rgba"]) & inner).sum())
    print(f"{what}: {int(inner.sum())} non-edge pixels, geom mismatches {ngeom}, depth rel err {rel:.3e} (bound {DEPTH_REL_BOUND:.1e}), rgba outside the accept-set {nrgba}")
    assert ngeom == 0
    assert inf_ok
    assert rel <= DEPTH_REL_BOUND
    assert nrgba == 0
    return rel


# scene B at 37 x 50 is seen from azimuth 135: from azimuth 45 its bent pose and the objects leave 36 % edge pixels, above what an oracle image may
# have (30 %); from 135 it is 28.6 %, with figure and objects in view
SIDE = (1.5, 135.0, -8.0)
CASES = [(n, W, H, v) for n in "AB" for W, H, v in ((64, 64, CLOSE), (64, 96, HIGH), (37, 50, SIDE if n == "B" else CLOSE))]


@pytest.mark.parametrize("name,W,H,view", CASES, ids=[f"{n}-{W}x{H}" for n, W, H, _ in CASES])
def test_image_matches_oracle(sim, name, W, H, view):
    o = oracle_case(name, W, H, view)
    # the oracle image alone: enough of it is interior, and the close-ups show the figure
    share = o["edge"].mean()
    fig = ~o["edge"] & (o["geom"] >= 1) & (o["geom"] <= 24)
    print(f"{name} {W}x{H}: edge share {100 * share:.1f} %, non-edge figure pixels {int(fig.sum())} from {len(np.unique(o['geom'][fig]))} bodies")
    assert share <= 0.30
    if (W, H) == (64, 64):
        assert fig.sum() >= 300 and len(np.unique(o["geom"][fig])) >= 8
    if name == "B":
        assert ((o["geom"] >= 25) & (o["geom"] < 100) & ~o["edge"]).sum() >= 50      # objects are in view
    sc = scene(name)
    got = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], None if sc["blk"] is None else sc["blk"][None], camera(sc, *view), W, H)
    compare({k: v[0] for k, v in got.items()}, o, f"{name} {W}x{H}")


def test_camera_per_row_65_rows(sim):
    """65 rows x 32 x 32, a camera of its own per row (the grid's row / tile indexing): every row against its own oracle image.  Scene A from 2.2 m and
    more: closer, or with scene B's objects, a 32 x 32 image has more than 30 % edge pixels."""
    sc = scene("A")
    R, W, H = 65, 32, 32
    cams = np.stack([f32(list(sc["root"]) + [2.2 + 0.01 * r, 5.5 * r, -8.0 - 0.3 * r, 45.0]) for r in range(R)])
    got = run(sim, np.tile(sc["xpos"], (R, 1, 1, 1)), np.tile(sc["xquat"], (R, 1, 1, 1)), None, cams, W, H)
    worst = 0.0
    for r in range(R):
        o = oracle_image(sc["xpos"], sc["xquat"], None, cams[r], W, H)
        assert o["edge"].mean() <= 0.30
        inner = ~o["edge"]
        hit = inner & np.isfinite(o["depth"])
        assert np.array_equal(got["geom"][r][inner], o["geom"][inner]), r
        worst = max(worst, float((np.abs(got["depth"][r][hit] - o["depth"][hit]) / o["depth"][hit]).max()))
        assert not (RO.rgba_mismatch(o, got["rgba"][r]) & inner).any(), r
    print(f"65 rows: depth rel err {worst:.3e} (bound {DEPTH_REL_BOUND:.1e})")
    assert worst <= DEPTH_REL_BOUND


def test_two_figures(sim):
    """the second figure 0.4 m beside the first, seen from azimuth 0 with the lookat between them: its bodies carry geom ids 101.. and the second
    base colour"""
    sc = scene("A")
    xpos = np.stack([sc["xpos"], f32(sc["xpos"] + np.array([0.0, 0.4, 0.0]))])
    xquat = np.stack([sc["xquat"], sc["xquat"]])
    cam = f32(list(sc["root"] + np.array([0.0, 0.2, 0.0])) + [1.5, 0.0, -8.0, 45.0])
    o = oracle_image(xpos, xquat, None, cam, 64, 64)
    assert o["edge"].mean() <= 0.30
    assert ((o["geom"] > 100) & ~o["edge"]).sum() >= 100 and ((o["geom"] >= 1) & (o["geom"] <= 24) & ~o["edge"]).sum() >= 100
    got = run(sim, xpos[None], xquat[None], None, cam, 64, 64)
    compare({k: v[0] for k, v in got.items()}, o, "two figures 64x64")


def test_rows_are_independent(sim):
    a, b = scene("A"), scene("B")
    xpos = np.stack([a["xpos"], b["xpos"], f32(a["xpos"] + np.array([0.3, 0.0, 0.1]))])[:, None]
    xquat = np.stack([a["xquat"], b["xquat"], a["xquat"]])[:, None]
    blk = np.stack([parked(), b["blk"], b["blk"]])
    cams = np.stack([camera(a, *CLOSE), camera(b, *HIGH), camera(b, 2.0, 80.0, -15.0)])
    whole = run(sim, xpos, xquat, blk, cams, 37, 50)
    for r in range(3):
        one = run(sim, xpos[r:r + 1], xquat[r:r + 1], blk[r:r + 1], cams[r:r + 1], 37, 50)
        for k in ("rgba", "geom", "depth"):
            assert np.array_equal(one[k][0], whole[k][r]), (r, k)


def test_no_objects_equals_all_parked(sim):
    sc = scene("B")
    cam = camera(sc, *CLOSE)
    none = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], None, cam, 64, 64)
    allp = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], parked()[None], cam, 64, 64)
    for k in ("rgba", "geom", "depth"):
        assert np.array_equal(none[k], allp[k]), k
    assert not ((none["geom"] >= 25) & (none["geom"] < 100)).any()


def test_object_behind_camera_is_absent(sim):
    """the can 1 m behind the camera, on its axis: t < 0 on every ray"""
    sc = scene("A")
    cam = camera(sc, *CLOSE)
    pos, f = RO.camera_rays(cam, 8, 8)[0], None
    az, el = np.radians(45.0), np.radians(-8.0)
    f = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    blk = parked()
    blk[21:28] = list(pos - 1.0 * f) + [1.0, 0.0, 0.0, 0.0]
    got = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], blk[None], cam, 64, 64)
    ref = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], None, cam, 64, 64)
    assert not (got["geom"] >= 25).any()
    for k in ("rgba", "geom", "depth"):
        assert np.array_equal(got[k], ref[k]), k
    blk[21:24] = pos + 1.0 * f                                  # and 1 m in front of it: there it is
    assert (run(sim, sc["xpos"][None, None], sc["xquat"][None, None], blk[None], cam, 64, 64)["geom"] == 25 + 8).sum() > 50


def test_camera_inside_a_hull_does_not_see_it(sim):
    """the camera at the pelvis' centre of mass (distance 0), looking at body 2: no pixel shows the pelvis, other bodies and the floor are still there"""
    sc = scene("A")
    ipos = KPM["body_ipos"].reshape(24, 3)[0]
    at = sc["xpos"][0] + RO.qmat(sc["xquat"][0]) @ ipos
    v = sc["xpos"][2] - at
    cam = f32(list(at) + [0.0, np.degrees(np.arctan2(v[1], v[0])), np.degrees(np.arcsin(v[2] / np.linalg.norm(v))), 45.0])
    pl = planes()[0]
    assert np.all(pl[:, :3] @ ipos < pl[:, 3] - 1e-3)             # strictly inside the hull
    got = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], None, cam, 64, 64)
    assert not (got["geom"] == 1).any()
    assert (got["geom"] == 0).any() and ((got["geom"] > 1) & (got["geom"] <= 24)).any()
    o = oracle_image(sc["xpos"], sc["xquat"], None, cam, 64, 64)
    assert np.array_equal(got["geom"][0][~o["edge"]], o["geom"][~o["edge"]])


def test_zfar_turns_far_floor_into_sky(sim):
    from kinpoly_amd.sim import KpRenderStyle
    sc = scene("A")
    cam = camera(sc, *CLOSE)
    far = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], None, cam, 64, 64)
    st = KpRenderStyle.default()
    st.zfar = 4.0
    near = run(sim, sc["xpos"][None, None], sc["xquat"][None, None], None, cam, 64, 64, st)
    floor = far["geom"] == 0
    cut = floor & (far["depth"] > 4.0)
    assert cut.sum() > 100 and (floor & ~cut).sum() > 100
    assert np.all(near["geom"][cut] == -1) and np.all(np.isposinf(near["depth"][cut]))
    sky = np.rint(255 * np.array(RO.STYLE["sky"] + (1.0,))).astype(np.uint8)
    assert np.all(near["rgba"][cut] == sky)
    for k in ("rgba", "geom", "depth"):
        assert np.array_equal(near[k][~cut], far[k][~cut]), k


def test_refusals_launch_nothing(sim):
    """every refusal returns -1 with a message and leaves the outputs untouched"""
    from kinpoly_amd import sim as kpsim
    L = sim.L
    xp, xq = torch.zeros((2, 5, 72), device="cuda"), torch.zeros((2, 5, 96), device="cuda")
    cam = dev(np.tile([0, 0, 1, 5, 45, -8, 45.0], (2, 1)))
    blk = dev(np.tile(parked(), (2, 1)))
    geom = torch.full((2, 16, 16), 7, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(h=None, R=2, K=1, xpos=xp, xquat=xq, obj=None, camera=cam, cam_rows=2, W=16, H=16, outs=(geom, None, None)):
        return L.kp_sim_render(sim.h if h is None else h, R, K, p(xpos), p(xquat), p(obj), p(camera), cam_rows, W, H, None, *[p(t) for t in outs])

    for kw, word in ((dict(K=0), b"n_fig"), (dict(K=5), b"n_fig"), (dict(W=0), b"width"), (dict(W=4097), b"width"), (dict(H=0), b"height"), (dict(H=4097), b"height"),
                     (dict(xpos=None), b"xpos"), (dict(xquat=None), b"xquat"), (dict(camera=None), b"camera"), (dict(cam_rows=3), b"camera_rows"),
                     (dict(outs=(None, None, None)), b"null output"), (dict(R=-1), b"n_rows")):
        assert call(**kw) == -1 and word in L.kp_last_error(), kw
    torch.cuda.synchronize()
    assert bool((geom == 7).all())
    # obj_qpos on a blob without object geoms; a blob with more than 16 object geoms; a blob with an object geom of another type
    import os
    import tempfile
    from kinpoly_amd.model_compiler import write_kpm
    for n_geoms, word in ((0, b"no object geoms"), (17, b"more object geoms"), (-1, b"neither a box")):
        m = dict(KPM)
        if n_geoms == -1:                                           # a geom type the kernel does not draw (a sphere, say)
            og = m["obj_geoms"].reshape(-1, 18).copy(); og[3, 1] = 2.0
            m["obj_geoms"] = og.ravel()
        elif n_geoms == 0:
            for k in ("obj_geoms", "obj_geom_adr", "obj_mass", "obj_inertial"):
                m.pop(k, None)
        else:
            og = m["obj_geoms"].reshape(-1, 18)
            m["obj_geoms"] = np.concatenate([og, np.tile(og[-1:], (n_geoms - len(og), 1))]).ravel()
            adr = np.array(m["obj_geom_adr"]).copy(); adr[-1] = n_geoms
            m["obj_geom_adr"] = adr
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.kpm")
            write_kpm(m, path)
            other = kpsim.KpSim(kpsim.KpModel(path), 1)
        assert call(h=other.h, obj=blk) == -1 and word in L.kp_last_error(), n_geoms
    torch.cuda.synchronize()
    assert bool((geom == 7).all())
    assert call() == 0                                              # and the same call, legal, draws
    torch.cuda.synchronize()
    assert not bool((geom == 7).any())
    with pytest.raises(ValueError):
        sim.render(torch.zeros((2, 75), device="cuda"))
    with pytest.raises(ValueError):
        sim.render(torch.zeros((2, 76), device="cuda"), want=("colour",))


def _env(kind):
    """a 4-env batched env after one step: 'ar' / 'uhc' without objects, 'ar_step' with the step box of the clip (1 m ahead of envs 0 and 1),
    'uhc_takes' on the fixture's take library with objects"""
    import os
    golden = os.path.join(os.path.dirname(__file__), "golden")
    std = np.load(os.path.join(golden, "standing_neutral.npz"))
    n = 4
    torch.manual_seed(0)
    if kind in ("ar", "ar_step"):
        from kinpoly_amd.env import BatchedHumanoidAREnv, standing_context
        env = BatchedHumanoidAREnv(n, 0, mode="test", seed=0)
        ctx = standing_context(n, 8, std["qpos"], std["qvel"], env.sim)
        if kind == "ar_step":
            one_hot = torch.zeros((n, 4), device=env.device); one_hot[:2, 3] = 1.0
            pose = torch.tensor([std["qpos"][0] + 1.0, std["qpos"][1], 0.3705, 1.0, 0, 0, 0], device=env.device).repeat(n, 1)
            ctx["action_one_hot"] = one_hot
            ctx["obj_pose"] = pose.unsqueeze(1).repeat(1, 8, 1).contiguous()
        env.load_context(ctx)
        env.reset()
        a = torch.zeros((n, 80), device=env.device)
        a[:, :74] = env.sim.get("qpos")[:, 2:]
        env.step(a)
    elif kind == "uhc":
        from kinpoly_amd.uhc_env import BatchedHumanoidEnv
        clips = np.tile(std["qpos"], (n, 6, 1))
        clips[:, :, 7:] += 0.05 * np.sin(0.4 * np.arange(6)[None, :, None] + np.arange(69)[None, None] + np.arange(n)[:, None, None])
        env = BatchedHumanoidEnv(n, 0)
        env.load_expert(torch.tensor(clips, dtype=torch.float32))
        env.reset()
        env.step(torch.zeros((n, 75), device=env.device))
    else:
        from kinpoly_amd.dataset import SmplObjDataset
        from kinpoly_amd.uhc_env import BatchedHumanoidEnv
        pkl = os.path.join(golden, "uhc_obj_takes_small.pkl")
        env = BatchedHumanoidEnv(n, 0)
        env.load_takes(SmplObjDataset({"file_path": pkl, "test_file_path": pkl, "t_min": 90}, "train").to_library(env.sim))      # envs 0..3: sit, push, avoid, step
        env.reset()
        env.step(torch.zeros((n, 75), device=env.device))
    return env


@pytest.mark.parametrize("kind", ["ar", "uhc", "ar_step", "uhc_takes"])
def test_env_render_rgb_equals_sim_render(kind):
    """render_rgb = figure 0 the simulated pose, figure 1 the simulator's target, the env's objects.  The expected frames are put together here from
    fk() and render_poses, with the object block read from the simulator."""
    from kinpoly_amd.render import Camera, follow
    env = _env(kind)
    n, objects = 4, kind in ("ar_step", "uhc_takes")
    assert bool(env.has_objects) == objects
    q = torch.stack([env.sim.get("qpos"), env.sim.get("target_qpos")], 1).contiguous()
    cam = follow(q[:, 0], Camera(distance=3.0))
    img = env.render_rgb(camera=cam, width=48, height=40)
    assert img.shape == (n, 40, 48, 4) and img.dtype == torch.uint8 and img.is_cuda
    f = env.sim.fk(q.view(2 * n, 76))
    blk = env.sim.get("obj_qpos") if objects else None
    out = env.sim.render_poses(f["wbpos"].view(n, 2, 72), f["wbquat"].view(n, 2, 96), blk, cam, 48, 40, ("rgba", "geom"))
    assert torch.equal(img, out["rgba"])
    g = out["geom"]
    assert bool(((g >= 1) & (g <= 24)).any()) and bool((g == 0).any())       # the simulated figure and the floor are in the frame
    seen = [bool(((g[e] >= 25) & (g[e] < 100)).any()) for e in range(n)]
    if kind == "ar_step":
        assert seen == [True, True, False, False] and bool((g[:2] == 25 + 9).any())      # the step box of envs 0 and 1, parked for the others
    elif kind == "uhc_takes":
        assert seen[0] and seen[1]                                           # the chair behind the sitting take, the table and box of the push take
    else:
        assert not any(seen)
    sub = env.render_rgb(envs=[2, 0], width=48, height=40)                   # a subset, the default camera following each root
    whole = env.render_rgb(width=48, height=40)
    assert torch.equal(sub, whole[[2, 0]])
    if objects:
        assert not torch.equal(whole, env.sim.render(q, None, follow(q[:, 0]), 48, 40)["rgba"])      # and the objects are in those frames too


def test_render_sequence_chunks(sim):
    """render_sequence with a byte budget of three frames (so 11 frames take four launches) equals one KpSim.render call: the figures cut to the
    shortest, the camera following figure 0's root in every chunk, or fixed"""
    from kinpoly_amd.render import Camera, follow, render_sequence
    rng = np.random.default_rng(4)
    std = np.zeros(76); std[2], std[3] = 0.92, 1.0
    pred = np.tile(std, (13, 1)); pred[:, 7:] += rng.uniform(-0.3, 0.3, (13, 69)); pred[:, 0] += 0.2 * np.arange(13)
    expert = np.tile(std, (11, 1)); expert[:, 1] += 0.4
    obj = np.tile(parked(), (12, 1)); obj[:, 21:28] = [0.5, -0.6, 0.15, 1.0, 0.0, 0.0, 0.0]; obj[:, 21] += 0.2 * np.arange(12)
    W, H, cam = 40, 24, Camera(distance=3.0, azimuth=80.0)
    q = torch.stack([dev(pred[:11]), dev(expert)], 1).contiguous()
    for focus in (True, False):
        got = render_sequence(sim, [pred, expert], obj, cam, W, H, focus=focus, byte_budget=3 * 4 * W * H)
        assert got.shape == (11, H, W, 4) and got.dtype == np.uint8
        want = sim.render(q, dev(obj[:11]), follow(q[:, 0], cam) if focus else cam, W, H)["rgba"].cpu().numpy()
        assert np.array_equal(got, want)
    assert not np.array_equal(got[0], got[10])                               # the fixed camera sees the figure walk away
    one = render_sequence(sim, pred, None, cam, W, H, byte_budget=1)         # a budget below one frame still renders, a frame per launch
    assert np.array_equal(one, sim.render(dev(pred), None, follow(dev(pred), cam), W, H)["rgba"].cpu().numpy())
