"""The conditions on the inputs of tests/test_gpu_collide_sweep.py, on the fp64 oracle alone (no kernel involved): every family of tests/collide_cases.py
reaches the contact counts and pair kinds it is there for, the cull-edge scenes sit where they claim to, the share of scenes the oracle itself cannot
answer reproducibly stays within 3 % per family, and no scene reaches the 64-contact ceiling."""
import collections

import numpy as np
import pytest

import collide_cases as CC


@pytest.fixture(scope="module")
def scenes():
    return CC.all_scenes()


def by_family(scenes, fam):
    return [s for s in scenes if s["family"] == fam]


def kinds_of(scenes):
    """Counter of (pair kind, number of contacts) over the object pairs of the scenes"""
    c = collections.Counter()
    for s in scenes:
        for kind, rows in CC.object_pairs(s):
            if len(rows):
                c[(kind, len(rows))] += 1
    return c


def test_scene_table(scenes):
    fams = collections.Counter(s["family"] for s in scenes)
    print("scenes per family:", dict(fams))
    assert set(fams) == {"F1", "F2", "F3", "F4", "F5", "F6"} and all(32 <= fams[f] <= 56 for f in ("F1", "F2", "F3", "F4", "F5")) and len(scenes) <= 256
    for s in scenes:
        assert np.array_equal(s["q"], CC.f32(s["q"])) and np.array_equal(s["blk"], CC.f32(s["blk"])), "every input is an fp32 value"
        assert s["q"].shape == (76,) and s["blk"].shape == (35,) and len(s["slots"]) <= CC.MAXOBJ and set(s["routes"]) <= {"dyn", "static", "pose"}
        for oi in CC.active(s["blk"]):
            assert abs(np.linalg.norm(s["blk"][7 * oi + 3: 7 * oi + 7]) - 1.0) < 1e-6 or "scaled" in s["tags"]
    again = [CC.family_f1(), CC.family_f3()]
    for fam in again:                  # seeded: the same scenes every time
        for a in fam:
            b = next(s for s in scenes if s["name"] == a["name"])
            assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["blk"], b["blk"])


def test_floor_families_reach_every_count(scenes):
    f1, f2 = kinds_of(by_family(scenes, "F1")), kinds_of(by_family(scenes, "F2"))
    print("F1:", dict(f1), "\nF2:", dict(f2))
    assert {n for (k, n) in f1 if k == "floor-box"} >= {1, 2, 4}
    assert {n for (k, n) in f2 if k == "floor-cyl"} == {1, 2, 3, 4}
    tags1 = collections.Counter(t for s in by_family(scenes, "F1") for t in s["tags"])
    assert tags1["random"] >= 20 and tags1["face"] >= 8 and tags1["edge"] >= 4 and tags1["corner"] >= 3
    # the axis flip of plane_cylinder is taken both ways: cylinders whose axis points up and down, and lying ones
    az = [g["mat"][2, 2] for s in by_family(scenes, "F2") for oi in s["slots"] for g in CC.placed(oi, s["blk"][7 * oi: 7 * oi + 7]) if g["type"] == 1]
    assert sum(a > 0.01 for a in az) >= 10 and sum(a < -0.01 for a in az) >= 10 and sum(abs(a) < 1e-6 for a in az) >= 3
    assert sum(a == 1.0 for a in az) >= 2, "exactly upright (identity quaternion)"
    tilts = sorted({t for s in by_family(scenes, "F2") for t in s["tags"] if t.startswith("tilt")})
    assert tilts == ["tilt0.02", "tilt0.1", "tilt0.5", "tilt1.2"]
    for s in by_family(scenes, "F2"):          # tilts in (0, 0.02) rad are test_gpu_round3's subject: none here
        for oi in s["slots"]:
            for g in CC.placed(oi, s["blk"][7 * oi: 7 * oi + 7]):
                if g["type"] == 1:
                    tilt = np.arccos(min(1.0, abs(g["mat"][2, 2])))
                    assert tilt < 1e-6 or tilt > 0.0199, (s["name"], tilt)


def test_object_object_families_reach_every_kind(scenes):
    f3, f4 = kinds_of(by_family(scenes, "F3")), kinds_of(by_family(scenes, "F4"))
    print("F3:", dict(f3), "\nF4:", dict(f4))
    assert f3[("box-box", 1)] >= 10 and sum(v for (k, n), v in f3.items() if k == "box-box" and n >= 4) >= 8
    assert sum(v for (k, n), v in f4.items() if k == "cyl-box") >= 20 and sum(v for (k, n), v in f4.items() if k == "cyl-cyl") >= 6
    pairs = collections.Counter(s["slots"] for s in by_family(scenes, "F3") + by_family(scenes, "F4"))
    assert set(pairs) >= {(CC.BOX, CC.TABLE), (CC.BOX, CC.STEP), (CC.CHAIR, CC.BOX), (CC.CHAIR, CC.STEP), (CC.CAN, CC.STEP), (CC.BOX, CC.CAN), (CC.TABLE, CC.CAN)}
    # both roles: the upper box of a face-on-face pair sits in the lower slot in some scenes and in the higher slot in others
    faces = [s["name"] for s in by_family(scenes, "F3") if "face" in s["tags"]]
    assert any(n.startswith("F3/1-on-4") for n in faces) and any(n.startswith("F3/4-on-1") for n in faces) and any("yaw1.571" in n for n in faces) and any("yaw0.000" in n for n in faces)
    # the bisection met its targets: every random pair's closest contact lies in [-0.01, 0.0009] up to the fp32 rounding of the poses
    for s in by_family(scenes, "F3") + by_family(scenes, "F4"):
        if "random" in s["tags"]:
            d = min(r[:, 0].min() for k, r in CC.object_pairs(s) if len(r) and not k.startswith("floor"))
            assert -0.02 < d < CC.MARGIN, (s["name"], d)


def test_hull_family_and_its_cull_edges(scenes):
    f5 = by_family(scenes, "F5")
    kinds = collections.Counter()
    o = CC.OracleSim(kpm=CC.STEP_KPM)
    for s in f5:
        b, gi = s["target"]
        oi = int(CC.OG[gi, 0])
        g = next(g for g in CC.placed(oi, s["blk"][7 * oi: 7 * oi + 7]) if g["gi"] == gi)
        kind, rows = CC.hull_rows(s["q"], b, g)
        kinds[(kind, len(rows))] += 1
        c = CC.oracle_contacts(o, s, "dyn")
        hull_obj = (c["body"] < 24) & (c["b2"] >= 24)
        assert hull_obj.any(), (s["name"], "every F5 scene has a hull - object contact")
        if "a" in s["tags"]:
            assert len(rows) == 1 and CC.MARGIN - 1e-4 < rows[0, 0] < CC.MARGIN, (s["name"], rows)
            assert any(CC.MARGIN - 1e-4 < d < CC.MARGIN for d in c["dist"][hull_obj & (c["body"] == b)]), s["name"]
        if "b" in s["tags"]:
            assert len(rows) == 1 and s["un"] < 5e-7, (s["name"], s["un"])
        if "c" in s["tags"]:
            # no face plane of the box separates the hull: on every face axis some vertex lies on the box's side of the plane
            V = (CC.hull_parts(s["q"], b)[3] - g["pos"]) @ g["mat"]
            assert len(rows) == 1 and all((V[:, k] < g["size"][k] + CC.MARGIN).any() and (V[:, k] > -g["size"][k] - CC.MARGIN).any() for k in range(3)), s["name"]
    print("F5 target pairs:", dict(kinds))
    assert kinds[("hull-box", 1)] >= 15 and kinds[("hull-cyl", 1)] >= 10
    tags = collections.Counter(t for s in f5 for t in s["tags"])
    assert tags["a"] >= 8 and tags["b"] == 4 and tags["c"] >= 3 and tags["random"] >= 32


def test_placement_edges(scenes):
    f6 = by_family(scenes, "F6")
    by = {s["name"]: s for s in scenes}
    norms = collections.Counter()
    for s in f6:
        if "scaled" in s["tags"]:
            base = by[s["base"]]
            for oi in CC.active(s["blk"]):
                qa, qb = s["blk"][7 * oi + 3: 7 * oi + 7], base["blk"][7 * oi + 3: 7 * oi + 7]
                fac = qa[np.argmax(np.abs(qb))] / qb[np.argmax(np.abs(qb))]
                assert np.array_equal(qa, fac * qb) and np.array_equal(s["blk"][7 * oi: 7 * oi + 3], base["blk"][7 * oi: 7 * oi + 3])
                norms[float(fac)] += 1
    assert set(norms) == {0.5, 2.0, -1.0}
    o = CC.OracleSim(kpm=CC.STEP_KPM)
    # three active objects: the oracle's set_object refuses a slot past MAXOBJ (kpo_set_object returns), so the pinned rule is the device's own stated one,
    # ascending model order truncated at the cap: the box and the table get the slots, the step (resting 3 mm inside the box's top) does not exist
    s = by["F6/three-dynamic-objects"]
    assert CC.active(s["blk"]) == [CC.BOX, CC.TABLE, CC.STEP] and s["slots"] == (CC.BOX, CC.TABLE)
    box, step = CC.placed(CC.BOX, s["blk"][7:14])[0], CC.placed(CC.STEP, s["blk"][28:35])[0]
    assert len(CC.pair_rows(box, step)[1]) >= 4, "the step would touch the box if it had a slot"
    o.clear_objects(); o.set_object(2, CC.KPM, CC.STEP, s["blk"][28:35])
    o.reset(s["q"], np.zeros(75))
    assert len(o.contacts_full()["body"]) == 0, "slot 2 is refused by the oracle"
    # five active objects as static obstacles: the oracle's set_geoms keeps the first MAXGEOM of object_geoms' ascending list (chair 2, box 1, table 5), so
    # the device is pinned to the oracle here; the Can, touched by the right hand's hull, and the step fall off the end
    s = by["F6/five-static-objects"]
    allg = CC.object_geoms(CC.KPM, s["blk"])
    assert len(allg) == 10 > CC.MAXGEOM
    b, gi = s["target"]
    can = CC.placed(CC.CAN, s["blk"][21:28])[0]
    assert len(CC.hull_rows(s["q"], b, can)[1]) == 1, "the Can would touch the hull if its geom had a row"
    full = CC.oracle_contacts(o, s, "static")
    o.clear_objects(); o.set_geoms(allg[:CC.MAXGEOM]); o.reset(s["q"], np.zeros(75))
    first8 = o.contacts_full()
    assert np.array_equal(full["body"], first8["body"]) and np.array_equal(full["dist"], first8["dist"]) and len(full["body"]) >= 1
    o.clear_objects(); o.set_geoms(allg[8:9]); o.reset(s["q"], np.zeros(75))
    assert b in o.contacts_full()["body"] and b not in full["body"], "the ninth geom alone (the Can) does touch that hull; in the truncated scene nothing does"


@pytest.mark.parametrize("route", ["dyn", "static"])
def test_conditioning_and_contact_ceiling(scenes, route):
    ref = CC.references(route)
    worst = np.zeros(3)
    for fam in ("F1", "F2", "F3", "F4", "F5", "F6"):
        ss = [s for s in by_family(scenes, fam) if route in s["routes"]]
        if not ss:
            continue
        ill = [s["name"] for s in ss if ref[s["name"]]["ill"]]
        flips = sum(ref[s["name"]]["changed"] for s in ss)
        ws = [ref[s["name"]]["spread"].max(0) for s in ss if not ref[s["name"]]["ill"] and len(ref[s["name"]]["spread"])]
        w = np.max(ws, 0) if ws else np.zeros(3)
        worst = np.maximum(worst, w)
        print(f"{route} {fam}: {len(ss)} scenes, {len(ill)} ill-conditioned {ill} ({flips} set changes); largest spread of the rest: dist {w[0]:.2e} pos {w[1]:.2e} normal {w[2]:.2e}")
        assert len(ill) <= 0.03 * len(ss), (fam, ill)
        for s in ss:
            assert len(ref[s["name"]]["ref"]["body"]) < 64, s["name"]
    assert worst[0] <= 1e-5 and worst[1] <= 1e-5
