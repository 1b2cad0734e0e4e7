"""Host side of the offscreen renderer, no GPU: the hulls' face planes (kp_model_hull_planes) against the brute-force builder of tests/render_oracle.py,
the PNG writer, the camera, and scripts/render_results.py's reading of the two evaluation pickles."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm
from tests import render_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOBS = {"default": DEFAULT_KPM, "step": STEP_KPM}
_cache = {}


def both(which):
    """(library planes [n, 4], adr [25], oracle planes per body, blob dict) of a shipped blob, computed once"""
    if which not in _cache:
        from kinpoly_amd.sim import KpModel
        planes, adr = KpModel(BLOBS[which]).hull_planes()
        kpm = read_kpm(BLOBS[which])
        _cache[which] = (planes, adr, RO.model_planes(kpm), kpm)
    return _cache[which]


@pytest.mark.parametrize("which", list(BLOBS))
def test_hull_plane_counts(which):
    planes, adr, want, _ = both(which)
    assert planes.shape == (2302, 4) and planes.dtype == np.float32
    assert adr[0] == 0 and adr[-1] == 2302 and len(adr) == 25
    cnt = np.diff(adr)
    assert cnt.tolist() == [len(w) for w in want]
    assert cnt.min() >= 86 and cnt.max() <= 98


@pytest.mark.parametrize("which", list(BLOBS))
def test_hull_plane_values(which):
    planes, adr, want, kpm = both(which)
    verts, vadr = kpm["verts"].reshape(-1, 3), kpm["vert_adr"]
    for b in range(24):
        got = planes[adr[b]:adr[b + 1]].astype(np.float64)
        diff = np.abs(got[:, None] - want[b][None]).max(2)
        assert diff.min(1).max() <= 1e-6, b                      # every plane matches an oracle plane
        assert diff.min(0).max() <= 1e-6, b                      # and vice versa
        assert np.abs(np.linalg.norm(got[:, :3], axis=1) - 1.0).max() <= 1e-6
        sd = got[:, :3] @ verts[vadr[b]:vadr[b + 1]].T - got[:, 3:4]
        assert sd.max() <= 1e-6, b                               # every vertex inside every half-space
        assert ((np.abs(sd) <= 1e-6).sum(1) >= 3).all(), b       # at least three vertices on each plane


def test_hull_planes_null_arguments():
    import ctypes as C
    from kinpoly_amd.sim import KpModel, load_library
    L = load_library()
    assert L.kp_model_hull_planes(None, None, None) == -1 and b"null model" in L.kp_last_error()
    m = KpModel()
    assert L.kp_model_hull_planes(m.h, None, None) == 2302
    adr = np.zeros(25, np.int32)
    assert L.kp_model_hull_planes(m.h, None, adr.ctypes.data_as(C.c_void_p)) == 2302 and adr[-1] == 2302


def decode_png(buf):
    """a hand decoder for what write_png writes: 8-bit, filter 0 on every scanline, one IDAT"""
    assert buf[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(buf):
        n, tag = struct.unpack(">I4s", buf[at:at + 8])
        data = buf[at + 8:at + 8 + n]
        assert struct.unpack(">I", buf[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data)); at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, lace) == (8, 0, 0, 0)
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, ch)


@pytest.mark.parametrize("shape", [(5, 7, 4), (3, 2, 3), (4, 6)])
def test_write_png_round_trip(tmp_path, shape):
    from kinpoly_amd.render import write_png
    img = np.random.default_rng(1).integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "sub" / "a.png")
    write_png(path, img)
    back = decode_png(open(path, "rb").read())
    assert np.array_equal(back.reshape(shape), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(path)), img)
    with pytest.raises(ValueError):
        write_png(path, img.astype(np.float32))


def test_camera_rays_equal_the_oracle():
    from kinpoly_amd.render import Camera
    c = Camera()
    assert c.row() == [0.0, 0.0, 1.0, 5.0, 45.0, -8.0, 45.0]                     # the reference visualiser's defaults
    for cam, W, H in ((c, 64, 48), (Camera((0.3, -1.2, 0.9), 1.5, 135.0, -30.0, 60.0), 37, 50)):
        o, d = cam.rays(W, H)
        wo, wd = RO.camera_rays(cam.row(), W, H)
        assert np.abs(o - wo).max() <= 1e-12 and np.abs(d.reshape(-1, 3) - wd).max() <= 1e-12
        assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() <= 1e-12
    # row 0 is the top of the image, column 0 its left: up has positive z, right = forward x z
    o, d = c.rays(4, 4)
    assert d[0, 0, 2] > d[3, 0, 2]
    pos, f, r, u = c.basis()
    assert np.dot(d[0, 3] - d[0, 0], r) > 0 and u[2] > 0 and abs(np.dot(f, r)) < 1e-15


def load_script():
    spec = importlib.util.spec_from_file_location("render_results", os.path.join(ROOT, "scripts", "render_results.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_render_results_reads_both_pickle_layouts(tmp_path):
    import joblib
    rr = load_script()
    rng = np.random.default_rng(0)
    ar = {"sit-1": {"pred": [rng.normal(size=76) for _ in range(7)], "target": [rng.normal(size=76) for _ in range(7)],
                    "obj_pose": [rng.normal(size=35) for _ in range(7)], "percent": 1.0, "fail_safe": False}}
    uhc = {"t0": {"pred": [rng.normal(size=111) for _ in range(9)], "gt": [rng.normal(size=76) for _ in range(6)], "percent": 0.5, "fail_safe": False},
           "t1": {"pred": [rng.normal(size=76) for _ in range(4)], "gt": [rng.normal(size=76) for _ in range(5)], "percent": 1.0, "fail_safe": False}}
    joblib.dump(ar, str(tmp_path / "ar.pkl")); joblib.dump(uhc, str(tmp_path / "uhc.pkl"))
    a = rr.load_results(str(tmp_path / "ar.pkl"))["sit-1"]
    assert a["pred"].shape == (7, 76) and a["expert"].shape == (7, 76) and a["obj_pose"].shape == (7, 35)
    assert np.array_equal(a["expert"], np.asarray(ar["sit-1"]["target"])) and np.array_equal(a["obj_pose"], np.asarray(ar["sit-1"]["obj_pose"]))
    u = rr.load_results(str(tmp_path / "uhc.pkl"))
    assert u["t0"]["pred"].shape == (6, 76) and u["t0"]["expert"].shape == (6, 76) and u["t0"]["obj_pose"].shape == (6, 35)      # cut to the shorter
    assert np.array_equal(u["t0"]["obj_pose"], np.asarray(uhc["t0"]["pred"])[:6, 76:])
    assert u["t1"]["pred"].shape == (4, 76) and u["t1"]["expert"].shape == (4, 76) and u["t1"]["obj_pose"] is None
    joblib.dump({"x": 1}, str(tmp_path / "bad.pkl"))
    with pytest.raises(SystemExit, match="coverage_full"):
        rr.load_results(str(tmp_path / "bad.pkl"))
    args = rr.build_parser().parse_args(["--results", "r.pkl", "--takes", "a,b", "--width", "64", "--height", "48", "--azimuth", "10", "--distance", "3",
                                         "--hide_expert", "--no_focus", "--every", "2", "--kpm", "m.kpm", "--video", "--video_dir", "v"])
    assert (args.takes, args.every, args.hide_expert, args.no_focus, args.video, args.video_dir) == ("a,b", 2, True, True, True, "v")


def test_render_results_missing_file_exits_with_a_message(tmp_path):
    rr = load_script()
    with pytest.raises(SystemExit, match="no such results file"):
        rr.main(["--results", str(tmp_path / "nothing.pkl")])


def test_eval_uhc_names_the_new_script():
    text = open(os.path.join(ROOT, "scripts", "eval_uhc.py")).read()
    assert "render_results.py" in text.split('"""')[1]
