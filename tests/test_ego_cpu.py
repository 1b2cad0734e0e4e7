"""The egocentric renderer without a GPU: the fp64 oracle tests/ego_oracle.py and the host code (HeadCamera, the feature and script refusals) held
to closed forms, and every oracle image that tests/test_gpu_ego.py compares the kernel against held to the edge-share cap first."""
import os

import numpy as np
import pytest

from kinpoly_amd.render import HeadCamera, ego_flow_features, flow_grid, head_hull_centroid, write_png
from tests import ego_cases as EC
from tests import ego_oracle as EO

W, H = 48, 40


def pair(A, cam_a, B, cam_b, w=W, h=H):
    return EO.render(EC.planes(), A, cam_a, w, h, B, cam_b)


@pytest.mark.parametrize("axis,degrees", [("forward", 5.0), ("up", 3.0)])
def test_pure_rotation_is_the_homography(axis, degrees):
    """the same eye, the camera turned: every pixel -- floor, two figures, objects and sky alike -- moves by the homography, whatever its depth"""
    A = EC.frame_a(True, 2)
    cam_a = EC.head_row(A, 30.0)
    cam_b = EC.rotated_row(cam_a, axis, degrees)
    o = pair(A, cam_a, A, cam_b)
    kinds = o["geom"]
    assert (kinds == -1).any() and (kinds == 0).any() and ((kinds >= 1) & (kinds <= 24)).any() and (kinds > 100).any() and ((kinds >= 25) & (kinds < 100)).any()
    want, cz = EC.homography_flow(cam_a, cam_b, W, H)
    assert np.array_equal(o["ok"], cz > EO.MIN_Z) and o["ok"].all()
    assert np.abs(o["flow"] - want).max() <= 1e-9
    if axis == "forward":                                   # a roll: the offsets from the image centre turn by the angle, one way or the other
        x, y = np.meshgrid(np.arange(W) + 0.5 - W / 2.0, np.arange(H) + 0.5 - H / 2.0)
        off, new = np.stack([x, y], -1), np.stack([x, y], -1) + o["flow"]
        a = np.radians(degrees)
        errs = []
        for s in (1.0, -1.0):
            Rz = np.array([[np.cos(a), -s * np.sin(a)], [s * np.sin(a), np.cos(a)]])
            errs.append(np.abs(new - off @ Rz.T).max())
        assert min(errs) <= 1e-9 and max(errs) > 1.0


def test_descending_camera_scales_about_the_centre():
    """straight down from h = 2 m over a bare floor, descending by 0.25 m: every pixel's offset from the centre grows by h / (h - delta)"""
    sc = EC.empty_scene()
    h, delta = 2.0, 0.25
    cam_a, cam_b = EC.down_row([0.3, -0.2, h]), EC.down_row([0.3, -0.2, h - delta])
    o = pair(sc, cam_a, sc, cam_b)
    assert (o["geom"] == 0).all() and o["ok"].all()
    x, y = np.meshgrid(np.arange(W) + 0.5 - W / 2.0, np.arange(H) + 0.5 - H / 2.0)
    want = np.stack([x, y], -1) * (h / (h - delta) - 1.0)
    assert np.abs(o["flow"] - want).max() <= 1e-9


def test_identical_frames_have_no_flow():
    A = EC.frame_a(True, 2)
    cam = EC.head_row(A, 15.0)
    o = pair(A, cam, A, cam)
    assert o["ok"].all() and (o["geom"] == -1).any()
    assert np.abs(o["flow"]).max() <= 1e-9


def test_parked_in_b_is_not_ok_and_cells_skip_it():
    """the objects of A parked in B: their pixels have ok = 0 and flow 0, and the cell means leave them out"""
    A = EC.frame_a(True)
    B = EC.scene([EC.STANDING], EC.parked())
    cam = EC.head_row(A, 30.0)
    o = pair(A, cam, B, cam, 32, 32)
    obj = (o["geom"] >= 25) & (o["geom"] < 100)
    assert obj.any() and not o["ok"][obj].any() and o["ok"][~obj].all()
    assert np.abs(o["flow"][obj]).max() == 0.0
    o["flow"][..., 0] = 1.0                                 # a known field: u = 1 everywhere, so a cell's mean is 1 when it has an ok pixel, else 0
    cells = EO.cell_means(o["flow"], o["ok"], 4, 4)
    has = o["ok"].reshape(4, 8, 4, 8).any((1, 3))
    assert np.array_equal(cells[..., 0], has.astype(np.float64))
    assert np.allclose(EO.cell_means(o["flow"], np.zeros_like(o["ok"]), 2, 2), 0.0)


def test_free_camera_row_sees_what_the_free_camera_sees():
    from tests import render_oracle as RO
    cam7 = [0.1, -0.2, 0.9, 2.0, 50.0, -12.0, 45.0]
    o7, d7 = RO.camera_rays(cam7, 20, 14)
    o8, d8 = EO.pose_rays(EO.free_camera_row(cam7), 20, 14)
    assert np.abs(o7 - o8).max() <= 1e-12 and np.abs(d7 - d8).max() <= 1e-12


def test_head_camera_on_the_standing_pose():
    sc = EC.frame_a(False)
    hp, hq = sc["xpos"][0, EC.HEAD], sc["xquat"][0, EC.HEAD]
    cam = HeadCamera()
    eye, f, r, u = cam.basis(hp, hq)
    assert abs(np.degrees(np.arcsin(f[2]))) < 10.0           # forward within 10 degrees of horizontal
    assert u[2] > 0.95
    assert np.allclose(np.cross(f, u), r) and abs(np.linalg.norm(f) - 1) < 1e-12       # right = forward x up
    for toe in (4, 8):                                       # L_Toe, R_Toe: ahead of the eye
        assert f @ (sc["xpos"][0, toe] - eye) > 0.0
    # the wearer's left hand appears on the left: its right-axis coordinate is negative
    assert r @ (sc["xpos"][0, 18] - eye) < 0.0 < r @ (sc["xpos"][0, 23] - eye)      # L_Hand, R_Hand
    # pitch: positive looks down, about the right axis, which stays
    _, fd, rd, _ = HeadCamera(pitch=30.0).basis(hp, hq)
    assert np.allclose(rd, r) and np.isclose(np.degrees(np.arccos(fd @ f)), 30.0) and fd[2] < f[2]
    # the default eye: the head hull's vertex centroid, strictly inside the hull by more than 1 mm (the library's host-side plane builder)
    from kinpoly_amd import sim as kpsim
    pl, adr = kpsim.KpModel(kpsim.STEP_KPM).hull_planes()
    head = pl[adr[EC.HEAD]:adr[EC.HEAD + 1]].astype(np.float64)
    c = head_hull_centroid()
    assert np.allclose(c, [-0.0065, 0.1096, -0.0272], atol=1e-4)
    assert np.all(head[:, :3] @ c < head[:, 3] - 1e-3)
    assert np.allclose(eye, hp + EO.qmat(hq) @ c)
    # rays: the centre of an odd image looks along forward
    o, d = cam.rays(hp, hq, 5, 3)
    assert np.allclose(o, eye) and np.allclose(d[1, 2], f) and d.shape == (3, 5, 3)
    o2, d2 = EO.pose_rays(cam.row(hp, hq), 5, 3)
    assert np.allclose(d.reshape(-1, 3), d2)


def test_head_camera_rows_match_row():
    torch = pytest.importorskip("torch")
    sc = EC.frame_a(False)
    cam = HeadCamera(pitch=20.0, fovy=75.0)
    got = cam.rows(torch.tensor(sc["xpos"].reshape(1, 72), dtype=torch.float64), torch.tensor(sc["xquat"].reshape(1, 96), dtype=torch.float64)).numpy()[0]
    # row() normalises the head quaternion, rows() takes fk()'s as it is: a unit quaternion rounded to fp32 is off by 6e-8 at most
    assert np.abs(got - cam.row(sc["xpos"][0, EC.HEAD], sc["xquat"][0, EC.HEAD])).max() <= 2e-7


@pytest.mark.parametrize("W,H,pitch,objects", EC.STILL, ids=EC.STILL_IDS)
def test_still_oracle_images_meet_the_edge_cap(W, H, pitch, objects):
    """what test_gpu_ego.py compares stills against: at most 30 % edge pixels, no pixel of the head, and the view the issue describes"""
    _, _, o = EC.still_case(W, H, pitch, objects)
    share = o["edge"].mean()
    print(f"{W}x{H} pitch {pitch} objects {objects}: edge share {100 * share:.1f} %")
    assert share <= EC.EDGE_CAP
    assert not (o["geom"] == 1 + EC.HEAD).any()
    assert (o["geom"] == 0).any()
    if pitch:
        assert ((o["geom"] >= 1) & (o["geom"] <= 24)).any()                # pitched down, the torso enters the frame
    if objects:
        assert ((o["geom"] >= 25) & (o["geom"] < 100) & ~o["edge"]).sum() >= 20


@pytest.mark.parametrize("W,H,figures", EC.FLOW, ids=EC.FLOW_IDS)
def test_flow_oracle_images_meet_the_exempt_cap(W, H, figures):
    """edge pixels plus the ok band: at most 30 % of every image of the flow cases, per-row cameras and the shared one"""
    for shared in (False, True):
        for r in range(3):
            o = EC.flow_row(W, H, figures, r, shared)[4]
            share = EC.exempt(o).mean()
            print(f"{W}x{H} {figures} fig row {r} shared {shared}: exempt share {100 * share:.1f} %, ok {100 * o['ok'].mean():.1f} %, max |flow| {np.abs(o['flow']).max():.2f} px")
            assert share <= EC.EDGE_CAP
            assert o["ok"][~EC.exempt(o)].mean() > 0.9
            if figures == 2:
                assert ((o["geom"] > 100) & ~o["edge"]).sum() >= 10


def test_refusals():
    with pytest.raises(ValueError, match="dim"):
        ego_flow_features(None, np.zeros((4, 76)), None, dim=500)
    with pytest.raises(ValueError, match="dim"):
        flow_grid(0)
    assert flow_grid(512) == 16 and flow_grid(128) == 8 and flow_grid(32) == 4
    with pytest.raises(ValueError, match="size"):
        ego_flow_features(None, np.zeros((4, 76)), None, dim=512, size=64)
    from kinpoly_amd import dataset as D
    with pytest.raises(ValueError, match="dim"):
        D.rendered_of_features({"a": dict(qpos=np.zeros((4, 76)))}, None, dim=500)
    assert "wild" in D.of_source_refusal("rendered", True) and D.of_source_refusal("rendered", False) is None and D.of_source_refusal("auto", True) is None
    with pytest.raises(ValueError, match="wild"):
        D.select_of_features("rendered", {}, "/nonexistent", 512, 0, None, wild=True)


def _script(name):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", name + ".py")
    spec = importlib.util.spec_from_file_location("ego_cpu_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["train_ar_policy", "eval_ar_policy", "exp_arnet_all"])
def test_of_source_argument(name, capsys):
    pytest.importorskip("torch")
    mod = _script(name)
    first = lambda r: r[1] if isinstance(r, tuple) else r  # noqa: E731
    assert first(mod.parse_args([])).of_source == "auto"
    assert first(mod.parse_args(["--wild"])).of_source == "auto"
    assert first(mod.parse_args(["--of_source", "rendered"])).of_source == "rendered"
    with pytest.raises(SystemExit):
        mod.parse_args(["--of_source", "rendered", "--wild"])
    assert "wild" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.parse_args(["--of_source", "pwc"])


def test_of_source_auto_is_the_old_rule(tmp_path):
    """auto: the file when it exists, else the stand-in, bit for bit what synthetic_of_features gives; standin ignores the file; file insists on it"""
    from kinpoly_amd import dataset as D
    takes = {"t": dict(head_vels=np.ones((5, 6)), qpos=np.ones((5, 76)))}
    missing = str(tmp_path / "of.p")
    of, said = D.select_of_features("auto", takes, missing, 16, 3)
    assert np.array_equal(of["t"], D.synthetic_of_features(takes, 16, seed=3)["t"]) and said == f"synthetic stand-in (no {missing})"
    with pytest.raises(FileNotFoundError):
        D.select_of_features("file", takes, missing, 16, 3)
    open(missing, "wb").close()
    assert D.select_of_features("auto", takes, missing, 16, 3) == (missing, missing)
    assert D.select_of_features("file", takes, missing, 16, 3)[0] == missing
    assert isinstance(D.select_of_features("standin", takes, missing, 16, 3)[0], dict)


def test_take_object_block():
    from kinpoly_amd import dataset as D
    obj = np.tile([0.5, 0.6, 0.3, 1.0, 0, 0, 0], (3, 1))
    one_hot = np.zeros((3, 4)); one_hot[:, 3] = 1.0
    blk = D.take_object_block(dict(obj_pose=obj, action_one_hot=one_hot))
    assert blk.shape == (3, 35) and np.array_equal(blk[:, 28:35], obj) and np.array_equal(blk[0, :3], [100.0, 100.0, 0.0])
    assert D.take_object_block(dict(obj_pose=obj, action_one_hot=np.zeros((3, 4)))) is None
    assert D.take_object_block(dict(obj_pose=blk)) is blk or np.array_equal(D.take_object_block(dict(obj_pose=blk)), blk)


def test_write_png_of_an_ego_frame(tmp_path):
    import struct
    import zlib
    fr = np.zeros((64, 64, 4), np.uint8); fr[..., 3] = 255; fr[10:20, 5:9, 0] = 200
    path = str(tmp_path / "take" / "ego_0000.png")
    write_png(path, fr)
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (64, 64) and raw[24:26] == b"\x08\x06"
    n = struct.unpack(">I", raw[33:37])[0]
    data = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(64, 1 + 64 * 4)
    assert np.array_equal(data[:, 1:].reshape(64, 64, 4), fr)
