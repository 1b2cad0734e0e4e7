"""The host half of the physics metrics (kinpoly_amd.metrics: pen_metric, foot_sliding, interaction_success) against the reference's own
compute_physcis_metris / compute_foot_sliding / compute_obj_interact, run on the fp64 oracle's frames (tests/golden/physics_metrics.npz,
tools/make_golden_physics.py).  The oracle's per-frame pen, hit masks and body positions are the inputs here; the device query that produces
them on the GPU is tested in test_gpu_pose_contacts.py."""
import os

import numpy as np
import pytest

from kinpoly_amd import metrics as M

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "physics_metrics.npz"))
T = int(G["T"])
NAMES = [str(n) for n in G["names"]]


def _side(i, side):
    sl = slice(i * T, (i + 1) * T)
    q = G["qpos_" + side][sl].astype(np.float64)
    return dict(pen=G["frame_pen_" + side][sl], hits=G["frame_hits_" + side][sl], toes=G["frame_toes_" + side][sl], head=G["frame_head_" + side][sl],
                z=q[:, 2], obj=G["obj_pose"][sl].astype(np.float64), head_gt=G["head_pose_gt"][sl, :3])


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_pen_and_slide_match_reference(i):
    for side in ("pred", "gt"):
        d = _side(i, side)
        assert abs(M.pen_metric(d["pen"]) - G["pen_" + side][i]) < 1e-12 * max(1.0, abs(G["pen_" + side][i]))
        slide = (M.foot_sliding(d["toes"][:, 0], d["z"]) + M.foot_sliding(d["toes"][:, 1], d["z"])) / 2
        assert abs(slide - G["slide_" + side][i]) < 1e-12 * max(1.0, abs(G["slide_" + side][i]))


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_interaction_success_matches_reference(i):
    name = NAMES[i]
    action = name.split("-")[0]
    for side in ("pred", "gt"):
        d = _side(i, side)
        fs = bool(G["fail_safe"][i]) if side == "pred" else None
        got = M.interaction_success(action, d["hits"], d["z"], d["obj"], d["head"], d["head_gt"], fs)
        want = bool(G["succ_" + side][i])
        if action in ("sit", "avoid", "push", "step", "None"):
            assert got == want
        else:                                   # an action prefix the reference does not know: its compute_obj_interact leaves succ False
            assert got is True and want is False  # (and its compute_metrics raises KeyError first); here it counts as a success


def test_fixture_covers_every_branch():
    acts = {n.split("-")[0] for n in NAMES}
    assert {"sit", "avoid", "push", "step", "None"} <= acts and acts - {"sit", "avoid", "push", "step", "None"}
    for a in ("sit", "avoid", "push", "step"):
        got = {bool(G["succ_pred"][i]) for i, n in enumerate(NAMES) if n.startswith(a + "-") and not G["fail_safe"][i]}
        assert got == {True, False}, a
    fs = [i for i in range(len(NAMES)) if G["fail_safe"][i]]
    assert fs and all(not G["succ_pred"][i] and G["succ_gt"][i] for i in fs)
    assert G["pen_pred"].max() > 100 and G["slide_pred"].max() > 1.0


def test_hit_masks_name_the_reference_geoms():
    """the chair take touches the pelvis / hips (geoms 1, 2, 6), the Can take a leg, the step take a foot: bit b = geom b + 1"""
    h = {n: np.bitwise_or.reduce(_side(i, "pred")["hits"], axis=0) for i, n in enumerate(NAMES)}
    assert h["sit-seat"][0] | h["sit-seat"][1]
    assert not ((h["sit-brush"][0] | h["sit-brush"][1]) & sum(1 << b for b in (0, 1, 5, 9, 10)))
    assert h["avoid-legs"][8] & 0xFFF and not h["avoid-clear"].any()
    assert h["step-up"][9] & sum(1 << b for b in (3, 4, 7, 8))
