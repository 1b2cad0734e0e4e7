"""The egocentric renderer (kp_sim_render_ego / KpSim.render_ego / HeadCamera / ego_flow_features) on a real MI355X against the fp64 restatement
tests/ego_oracle.py.  The scenes, cameras and oracle images are tests/ego_cases.py's; tests/test_ego_cpu.py holds every one of them to the 30 % cap
on exempt pixels.  As in tests/test_gpu_render.py, a pixel whose 3 x 3 neighbourhood in the ORACLE's geom image is not uniform is exempt from every
comparison, and so is a pixel whose oracle c_z lies within 1e-5 of the ok threshold."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from kinpoly_amd.model_compiler import STEP_KPM  # noqa: E402
from kinpoly_amd.render import HeadCamera  # noqa: E402
from tests import ego_cases as EC  # noqa: E402
from tests import ego_oracle as EO  # noqa: E402
from tests import render_oracle as RO  # noqa: E402
from tests.test_gpu_render import compare  # noqa: E402  (geom equal, depth within DEPTH_REL_BOUND, rgba in the accept-set, on non-edge pixels)

# flow against the fp64 oracle, in pixels, on the oracle's non-exempt ok pixels: the largest error seen on the MI355X over the flow cases of this
# file (test_flow_matches_oracle prints every case's), and the bound = four times that -- the project's rule for the depth bound: the kernel
# multiplies by v_rcp_f32 where the oracle divides, and carries the point in fp32.  The worst is the 64 x 64 row pitched 20 degrees down (flows up to
# 9.45 px); the 37 x 50 cases stay below 1.0e-5.  The closed forms are held to the same bound (measured: roll 6.5e-6, yaw 8.9e-6, descent 3.6e-6).
FLOW_PX_MEASURED = 1.236e-5
FLOW_PX_BOUND = 4 * FLOW_PX_MEASURED

OUTS = ("rgba", "geom", "depth", "flow", "ok")


@pytest.fixture(scope="module")
def sim():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim.KpSim(kpsim.KpModel(STEP_KPM), 4)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def blocks(scenes):
    return None if scenes[0]["blk"] is None else dev(np.stack([s["blk"] for s in scenes]))


def run(sim, A, cams_a, W, H, B=None, cams_b=None, want=("rgba", "geom", "depth"), grid=None, hide_body=-1):
    """A / B: one scene per row; cams: [1 or R, 8] -> dict of numpy arrays with a leading row axis"""
    R, K = len(A), A[0]["xpos"].shape[0]
    pose = lambda S, k, w: dev(np.stack([s[k] for s in S]).reshape(R, K, w))  # noqa: E731
    b = {} if B is None else dict(xpos_b=pose(B, "xpos", 72), xquat_b=pose(B, "xquat", 96), obj_qpos_b=blocks(B), camera_b=dev(np.asarray(cams_b).reshape(-1, 8)))
    out = sim.render_ego_poses(pose(A, "xpos", 72), pose(A, "xquat", 96), blocks(A), dev(np.asarray(cams_a).reshape(-1, 8)), width=W, height=H, want=want, grid=grid,
                               hide_body=hide_body, **b)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ still images
@pytest.mark.parametrize("W,H,pitch,objects", EC.STILL, ids=EC.STILL_IDS)
def test_still_matches_oracle(sim, W, H, pitch, objects):
    sc, cam, o = EC.still_case(W, H, pitch, objects)
    assert o["edge"].mean() <= EC.EDGE_CAP
    got = run(sim, [sc], cam, W, H)
    compare({k: v[0] for k, v in got.items()}, o, f"ego {W}x{H} pitch {pitch} objects {objects}")
    assert not (got["geom"] == 1 + EC.HEAD).any()           # the eye is inside the head hull: the head is never seen


@pytest.mark.parametrize("view", [(1.5, 45.0, -8.0), (2.5, 135.0, -30.0)], ids=["close", "high"])
def test_free_camera_row_equals_kp_sim_render(sim, view):
    """the viewer's free camera as its equivalent pose row (zero roll): k_render_ego's geom image is kp_sim_render's"""
    sc = EC.frame_a(True)
    W, H = 64, 48
    cam7 = EC.f32(list(EC.f32(EC.STANDING[:3])) + list(view) + [45.0])
    cam8 = EC.f32(EO.free_camera_row(cam7))
    o = RO.render(EC.planes(), sc["xpos"], sc["xquat"], sc["geoms"], sc["geom_ids"], cam7, W, H)
    inner = ~RO.edge_pixels(o["geom"])
    assert inner.mean() >= 1.0 - EC.EDGE_CAP
    ego = run(sim, [sc], cam8, W, H, want=("geom",))["geom"][0]
    free = sim.render_poses(dev(sc["xpos"].reshape(1, 1, 72)), dev(sc["xquat"].reshape(1, 1, 96)), dev(sc["blk"][None]), dev(cam7[None]), W, H, ("geom",))["geom"][0].cpu().numpy()
    assert ((free >= 1) & (free <= 24) & inner).sum() >= 20 and ((free >= 25) & inner).sum() >= 20       # figure and objects are in view, off the edges
    assert np.array_equal(ego[inner], free[inner]) and np.array_equal(ego[inner], o["geom"][inner])


# ------------------------------------------------------------------ flow
def flow_error(got, o, what):
    """ok equal and the flow error in pixels, on the oracle's non-exempt pixels; returns the worst error"""
    keep = ~EC.exempt(o)
    assert 1.0 - keep.mean() <= EC.EDGE_CAP
    assert np.array_equal(got["geom"][keep], o["geom"][keep]), what
    nok = int((got["ok"].astype(bool) != o["ok"])[keep].sum())
    both = keep & o["ok"]
    err = float(np.abs(got["flow"][both] - o["flow"][both]).max())
    zero = bool(np.all(got["flow"][got["ok"] == 0] == 0.0))
    print(f"{what}: {int(keep.sum())} compared pixels, ok mismatches {nok}, flow err {err:.3e} px (bound {FLOW_PX_BOUND:.1e}), max |flow| {np.abs(o['flow'][both]).max():.2f} px")
    assert nok == 0 and zero
    return err


@pytest.mark.parametrize("shared", [False, True], ids=["camera-per-row", "one-camera"])
@pytest.mark.parametrize("W,H,figures", EC.FLOW, ids=EC.FLOW_IDS)
def test_flow_matches_oracle(sim, W, H, figures, shared):
    rows = [EC.flow_row(W, H, figures, r, shared) for r in range(3)]
    cams_a, cams_b = (rows[0][2], rows[0][3]) if shared else (np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]))
    got = run(sim, [r[0] for r in rows], cams_a, W, H, [r[1] for r in rows], cams_b, want=OUTS)
    worst = max(flow_error({k: v[r] for k, v in got.items()}, rows[r][4], f"flow {W}x{H} {figures} fig row {r} {'one camera' if shared else 'own camera'}") for r in range(3))
    print(f"flow {W}x{H} {figures} fig: worst {worst:.3e} px")
    assert worst <= FLOW_PX_BOUND


@pytest.mark.parametrize("axis,degrees", [("forward", 5.0), ("up", 3.0)])
def test_pure_rotation_is_the_homography(sim, axis, degrees):
    """the same eye, the camera turned: floor, figures, objects and sky all move by the homography, at every pixel of the image"""
    W, H = 48, 40
    A = EC.frame_a(True, 2)
    cam_a = EC.f32(EC.head_row(A, 30.0))
    cam_b = EC.f32(EC.rotated_row(cam_a, axis, degrees))
    got = run(sim, [A], cam_a, W, H, [A], cam_b, want=OUTS)
    g = got["geom"][0]
    assert (g == -1).any() and (g == 0).any() and ((g >= 1) & (g <= 24)).any() and (g > 100).any() and ((g >= 25) & (g < 100)).any()
    want, cz = EC.homography_flow(cam_a, cam_b, W, H)
    assert (cz > 0.1).all() and got["ok"].all()
    err = float(np.abs(got["flow"][0] - want).max())
    print(f"pure rotation about {axis} by {degrees}: flow err {err:.3e} px against the homography (bound {FLOW_PX_BOUND:.1e})")
    assert err <= FLOW_PX_BOUND


def test_descending_camera_scales_about_the_centre(sim):
    W, H = 48, 40
    sc = EC.empty_scene()
    h, delta = 2.0, 0.25
    cam_a, cam_b = EC.f32(EC.down_row([0.3, -0.2, h])), EC.f32(EC.down_row([0.3, -0.2, h - delta]))
    got = run(sim, [sc], cam_a, W, H, [sc], cam_b, want=OUTS)
    assert (got["geom"] == 0).all() and got["ok"].all()
    x, y = np.meshgrid(np.arange(W) + 0.5 - W / 2.0, np.arange(H) + 0.5 - H / 2.0)
    err = float(np.abs(got["flow"][0] - np.stack([x, y], -1) * (h / (h - delta) - 1.0)).max())
    print(f"descending camera: flow err {err:.3e} px against h / (h - delta) (bound {FLOW_PX_BOUND:.1e})")
    assert err <= FLOW_PX_BOUND


def test_identical_frames_and_a_geom_parked_in_b(sim):
    A = EC.frame_a(True)
    cam = EC.head_row(A, 30.0)
    got = run(sim, [A], cam, 64, 64, [A], cam, want=OUTS)
    print(f"identical frames: max |flow| {float(np.abs(got['flow']).max()):.3e} px (bound {FLOW_PX_BOUND:.1e})")
    assert got["ok"].all() and float(np.abs(got["flow"]).max()) <= FLOW_PX_BOUND
    B = EC.scene([EC.STANDING], EC.parked())
    got = run(sim, [A], cam, 64, 64, [B], cam, want=OUTS)
    obj = (got["geom"] >= 25) & (got["geom"] < 100)
    assert obj.sum() > 100 and not got["ok"][obj].any() and got["ok"][~obj].all() and np.all(got["flow"][obj] == 0.0)


# ------------------------------------------------------------------ cells
@pytest.mark.parametrize("W,H,gy,gx", [(32, 32, 4, 4), (48, 32, 2, 3)], ids=["32x32-4x4", "48x32-2x3"])
def test_cells(sim, W, H, gy, gx):
    """row 0: the perturbed pair; row 1: camera B turned 80 degrees, so that one side of the image falls behind it and whole cells have no ok pixel"""
    A, B = EC.frame_a(False), EC.scene([EC.perturbed(EC.STANDING, 1)], None)
    cam_b = EC.head_row(B)
    cam_a, cams_b = np.stack([EC.head_row(A)] * 2), EC.f32(np.stack([cam_b, EC.rotated_row(cam_b, "up", 80.0)]))
    every = run(sim, [A, A], cam_a, W, H, [B, B], cams_b, want=OUTS + ("cells",), grid=(gy, gx))
    assert every["cells"].shape == (2, gy, gx, 2)
    empty = 0
    for r in range(2):
        ok = every["ok"][r].astype(bool)
        want = EO.cell_means(every["flow"][r], ok, gy, gx)
        tol = 1e-5 * max(1.0, float(np.abs(every["flow"][r]).max()))
        err = float(np.abs(every["cells"][r] - want).max())
        print(f"cells {W}x{H} {gy}x{gx} row {r}: err {err:.3e} (bound {tol:.1e}), ok share {100 * ok.mean():.0f} %")
        assert err <= tol
        none = ~ok.reshape(gy, H // gy, gx, W // gx).any((1, 3))
        assert np.all(every["cells"][r][none] == 0.0)
        empty += int(none.sum())
    assert every["ok"][0].all() and empty >= 1 and every["ok"][1].any()
    alone = run(sim, [A, A], cam_a, W, H, [B, B], cams_b, want=("cells",), grid=(gy, gx))
    assert list(alone) == ["cells"] and np.array_equal(alone["cells"].view(np.uint32), every["cells"].view(np.uint32))
    again = run(sim, [A, A], cam_a, W, H, [B, B], cams_b, want=OUTS + ("cells",), grid=(gy, gx))
    for k in every:
        assert np.array_equal(again[k].view(np.uint8), every[k].view(np.uint8)), k


# ------------------------------------------------------------------ rows, hide_body, refusals
def test_rows_are_independent(sim):
    W, H = 37, 50
    rows = [EC.flow_row(W, H, 1, r, False) for r in range(3)]
    cams_a, cams_b = np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows])
    whole = run(sim, [r[0] for r in rows], cams_a, W, H, [r[1] for r in rows], cams_b, want=OUTS)
    for r in range(3):
        one = run(sim, [rows[r][0]], cams_a[r], W, H, [rows[r][1]], cams_b[r], want=OUTS)
        for k in OUTS:
            assert np.array_equal(one[k][0].view(np.uint8), whole[k][r].view(np.uint8)), (r, k)


def test_hide_body(sim):
    """an eye 20 cm in front of the face looking back at the head: hide_body = 13 removes geom 14, and on the other non-edge pixels nothing changes"""
    sc = EC.frame_a(True)
    hp, hq = sc["xpos"][0, EC.HEAD], sc["xquat"][0, EC.HEAD]
    adr = np.asarray(EC.KPM["vert_adr"]).astype(int)
    face = float(np.asarray(EC.KPM["verts"], np.float64).reshape(-1, 3)[adr[EC.HEAD]:adr[EC.HEAD + 1], 2].max())      # how far the hull reaches along the head's +z
    eye = hp + EO.qmat(hq) @ (HeadCamera().eye_offset() * [1, 1, 0] + [0, 0, face + 0.20])
    cam = EC.f32(np.concatenate([eye, EC.qmul(hq / np.linalg.norm(hq), [0.0, 0.0, 1.0, 0.0]), [60.0]]))      # turned about the up axis: looking back
    W, H = 64, 64
    seen = EO.render(EC.planes(), sc, cam, W, H)
    hidden = EO.render(EC.planes(), sc, cam, W, H, hide_body=EC.HEAD)
    assert ((seen["geom"] == 14) & ~seen["edge"]).sum() > 200 and not (hidden["geom"] == 14).any()
    assert seen["edge"].mean() <= EC.EDGE_CAP and hidden["edge"].mean() <= EC.EDGE_CAP
    a, b = run(sim, [sc], cam, W, H), run(sim, [sc], cam, W, H, hide_body=EC.HEAD)
    compare({k: v[0] for k, v in a.items()}, seen, "looking back at the head")
    compare({k: v[0] for k, v in b.items()}, hidden, "looking back, head hidden")
    assert not (b["geom"] == 14).any()
    other = (a["geom"][0] != 14) & ~seen["edge"] & ~hidden["edge"]
    for k in a:
        assert np.array_equal(a[k][0][other], b[k][0][other]), k


def test_refusals_launch_nothing(sim):
    """every refusal returns -1 with a message that names the argument and leaves the outputs untouched"""
    L = sim.L
    R, W, H = 2, 16, 16
    xp, xq = torch.zeros((R, 1, 72), device="cuda"), torch.zeros((R, 1, 96), device="cuda")
    xq[..., 0::4] = 1.0
    cam = dev(np.tile([0, 0, 1, 1, 0, 0, 0, 90.0], (R, 1)))
    blk = dev(np.tile(EC.parked(), (R, 1)))
    geom = torch.full((R, H, W), 7, dtype=torch.int32, device="cuda")
    flow = torch.full((R, H, W, 2), 7.0, device="cuda")
    ok = torch.full((R, H, W), 7, dtype=torch.uint8, device="cuda")
    cells = torch.full((R, 2, 2, 2), 7.0, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    bside = dict(xpos_b=xp, xquat_b=xq, camera_b=cam)

    def call(K=1, xpos=xp, xquat=xq, obj=None, camera=cam, xpos_b=None, xquat_b=None, obj_b=None, camera_b=None, cam_rows=R, W=W, H=H, hide=-1, gx=2, gy=2,
             outs=(geom, None, None, None, None, None), rows=R):
        return L.kp_sim_render_ego(sim.h, rows, K, p(xpos), p(xquat), p(obj), p(camera), p(xpos_b), p(xquat_b), p(obj_b), p(camera_b), cam_rows, W, H, hide, None, gx, gy,
                                   *[p(t) for t in outs])

    full = (geom, None, None, flow, ok, cells)
    for kw, word in ((dict(K=0), b"n_fig"), (dict(K=5), b"n_fig"), (dict(W=0), b"width"), (dict(H=4097), b"height"), (dict(xpos=None), b"xpos"), (dict(xquat=None), b"xquat"),
                     (dict(camera=None), b"camera"), (dict(cam_rows=3), b"camera_rows"), (dict(outs=(None,) * 6), b"null output"), (dict(rows=-1), b"n_rows"),
                     (dict(hide=-2), b"hide_body"), (dict(hide=24), b"hide_body"),
                     (dict(xpos_b=xp), b"B side"), (dict(xpos_b=xp, xquat_b=xq), b"B side"), (dict(camera_b=cam), b"B side"), (dict(obj_b=blk), b"B side"),
                     (dict(obj=blk, **bside), b"obj_qpos_b"), (dict(obj_b=blk, **bside), b"obj_qpos_b"),
                     (dict(outs=(geom, None, None, flow, None, None)), b"need a B side"), (dict(outs=(geom, None, None, None, ok, None)), b"need a B side"),
                     (dict(outs=(geom, None, None, None, None, cells)), b"need a B side"),
                     (dict(outs=full, gx=3, **bside), b"grid"), (dict(outs=full, gy=0, **bside), b"grid"), (dict(outs=full, W=24, H=24, **bside), b"grid")):
        assert call(**kw) == -1 and word in L.kp_last_error(), (kw.keys(), L.kp_last_error())
    torch.cuda.synchronize()
    assert bool((geom == 7).all()) and bool((flow == 7).all()) and bool((ok == 7).all()) and bool((cells == 7).all())
    assert call(outs=full, **bside) == 0                       # and the same call, legal, draws
    torch.cuda.synchronize()
    assert not bool((geom == 7).any()) and not bool((flow == 7).any()) and not bool((ok == 7).any()) and not bool((cells == 7).any())
    with pytest.raises(ValueError):
        sim.render_ego(torch.zeros((2, 75), device="cuda"), None, cam)
    with pytest.raises(ValueError):
        sim.render_ego(torch.zeros((2, 76), device="cuda"), None, cam, want=("colour",))
    with pytest.raises(ValueError):
        sim.render_ego(torch.zeros((2, 76), device="cuda"), None, cam[:, :7].contiguous())


# ------------------------------------------------------------------ envs and features
@pytest.mark.parametrize("kind", ["ar_step", "uhc_takes"])
def test_env_render_ego_equals_sim_render_ego(kind):
    """render_ego of both batched envs: what each env's simulated figure sees from its head, with the env's objects"""
    from tests.test_gpu_render import _env
    env = _env(kind)
    n = 4
    cam = HeadCamera(pitch=25.0, fovy=150.0)                 # wide: the step box of the AR clip stands 1 m to the wearer's right
    img = env.render_ego(width=40, height=32, camera=cam)
    assert img.shape == (n, 32, 40, 4) and img.dtype == torch.uint8 and img.is_cuda
    q = env.sim.get("qpos").contiguous()
    blk = env.sim.get("obj_qpos").contiguous()
    out = env.sim.render_ego(q, blk, cam, width=40, height=32, want=("rgba", "geom"))
    assert torch.equal(img, out["rgba"])
    f = env.sim.fk(q)
    rows = cam.rows(f["wbpos"], f["wbquat"])
    assert torch.equal(env.sim.render_ego_poses(f["wbpos"].view(n, 1, 72), f["wbquat"].view(n, 1, 96), blk, rows, width=40, height=32)["rgba"], img)
    g = out["geom"]
    assert bool((g == 0).any()) and bool(((g >= 1) & (g <= 24)).any()) and not bool((g == 1 + EC.HEAD).any())      # floor and the wearer's own body, never the head
    assert bool(((g >= 25) & (g < 100)).any())                                                                       # and an object of the scene
    assert torch.equal(env.render_ego(envs=[2, 0], width=40, height=32, camera=cam), img[[2, 0]])
    assert env.render_ego().shape == (n, 64, 64, 4)


def _take(T=12):
    rng = np.random.default_rng(5)
    q = np.tile(EC.STANDING, (T, 1))
    q[:, 7:] += np.cumsum(rng.uniform(-0.02, 0.02, (T, 69)), 0)
    q[:, 1] += 0.02 * np.arange(T)
    obj = np.tile(EC.objects_block(), (T, 1))
    obj[:, 7] += 0.01 * np.arange(T)
    return q, obj


def test_ego_flow_features(sim):
    from kinpoly_amd.render import ego_flow_features, ego_sequence
    q, obj = _take()
    cam = HeadCamera(pitch=20.0)
    feat = ego_flow_features(sim, q, obj, dim=32, size=32, camera=cam)
    assert feat.shape == (12, 32) and feat.dtype == np.float32 and np.all(feat[0] == 0.0) and np.isfinite(feat).all() and np.abs(feat[1:]).max() > 1e-3
    import math
    focal = (0.5 * 32) / math.tan(0.5 * math.radians(cam.fovy))
    for t in (1, 7, 11):
        cells = sim.render_ego(dev(q[t - 1:t]), dev(obj[t - 1:t]), cam, dev(q[t:t + 1]), dev(obj[t:t + 1]), cam, width=32, height=32, want=("cells",), grid=4)["cells"]
        assert np.array_equal(feat[t], (cells.reshape(32) * (30.0 / focal)).cpu().numpy())
    assert np.array_equal(ego_flow_features(sim, q, obj, dim=32, size=32, camera=cam, rows_per_call=4), feat)      # chunks of 4 pairs
    frames = ego_sequence(sim, q, obj, cam, 40, 24, byte_budget=3 * 4 * 40 * 24)
    assert frames.shape == (12, 24, 40, 4) and frames.dtype == np.uint8
    assert np.array_equal(frames, sim.render_ego(dev(q), dev(obj), cam, width=40, height=24)["rgba"].cpu().numpy())


def test_rendered_of_features_feed_the_kinematic_model():
    """rendered_of_features has synthetic_of_features' schema: StateARDataset takes it, and one supervised forward of a net with an `of` block runs"""
    import test_context_obs_cpu as CC
    from kinpoly_amd import dataset as D
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd import pretrain as P
    from kinpoly_amd import sim as kp
    from kinpoly_amd.model_compiler import read_kpm
    std = np.load(os.path.join(os.path.dirname(__file__), "golden", "standing_neutral.npz"))
    torch.manual_seed(0)
    F = 32
    net = E.build_net(use_context=True, of_dim=F, rnn_hdim=32, mlp_hsize=(64, 32, 32)).cuda()
    sim = kp.KpSim(kp.KpModel(kp.STEP_KPM, **E.model_options(net)), 8)
    takes = D.synthetic_takes(sim, std["qpos"], n_per_action=2, T_range=(12, 13), body_mass=read_kpm(kp.STEP_KPM)["body_mass"], seed=2)
    of = D.rendered_of_features(takes, sim, dim=F, size=32)
    syn = D.synthetic_of_features(takes, F, seed=1)
    assert set(of) == set(syn) and all(of[k].shape == syn[k].shape and of[k].dtype == syn[k].dtype for k in of)
    assert all(np.all(v[0] == 0.0) and np.isfinite(v).all() for v in of.values()) and max(np.abs(v).max() for v in of.values()) > 1e-3
    ds = D.StateARDataset(takes, fr_num=12, seed=3, device="cuda", of_features=of)
    assert ds.get_len() == 8 and ds.of_dim == F
    data = next(P.sampling_batches(ds, 8, 8, "cuda"))
    assert tuple(data["of"].shape) == (8, 12, F)
    loss = P.compute_loss(P.forward_supervised(net, CC.torch_fk(torch.float32, "cuda", sim), data), data)[0]
    assert bool(torch.isfinite(loss))
