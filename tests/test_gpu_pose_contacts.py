"""The batched pose-contact query (kp_sim_pose_contacts / KpSim.pose_contacts) and the physics metrics built on it, on a real MI355X,
against the fp64 oracle (OracleSim forward + its contact list, tests/pose_oracle.py) and the reference's numbers (tests/golden/physics_metrics.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from kinpoly_amd.model_compiler import STEP_KPM, read_kpm  # noqa: E402
from oracle import np_oracle as O  # noqa: E402
from oracle.kpo import OracleSim, narrowphase, shape_record  # noqa: E402
from tests.pose_oracle import oracle_frame  # noqa: E402

KPM = read_kpm(STEP_KPM)
STD = np.load(os.path.join(os.path.dirname(__file__), "golden", "standing_neutral.npz"))["qpos"]


@pytest.fixture(scope="module")
def sim():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim.KpSim(kpsim.KpModel(STEP_KPM), 1)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def parked(n):
    blk = np.zeros((n, 35))
    for i in range(5):
        blk[:, 7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    return blk


def lying(rng, n, depth):
    """the humanoid on its back (root rolled by 90 degrees about y), its lowest hull vertex `depth` below the floor"""
    q = np.tile(STD, (n, 1))
    q[:, 3:7] = [np.cos(np.pi / 4), 0, np.sin(np.pi / 4), 0]
    q[:, 7:] += rng.normal(size=(n, 69)) * 0.05
    for e in range(n):
        q[e, 2] = 0.0
        fk = O.qpos_fk(q[e], KPM["body_pos"].reshape(24, 3), KPM["body_ipos"].reshape(24, 3), KPM["body_parent"])
        verts, vadr = KPM["verts"].reshape(-1, 3), KPM["vert_adr"]
        zmin = min((fk["wbpos"][b] + verts[vadr[b]:vadr[b + 1]] @ O.quaternion_matrix3(fk["wbquat"][b]).T)[:, 2].min() for b in range(24))
        q[e, 2] = -zmin - depth
    return q


def seeded_rows():
    """~200 rows: standing, perturbed, lifted, sunk and lying poses x {no objects, chair, Can, step, table + box, all parked}"""
    rng = np.random.default_rng(77)
    x0, y0 = STD[0], STD[1]
    scenes = [None, {0: [x0 + 0.35, y0, 0.38, 1, 0, 0, 0]}, {3: [x0 + 0.36, y0 + 0.05, 0.69, 1, 0, 0, 0]}, {4: [x0, y0, 0.3705, 1, 0, 0, 0]},
              {2: [x0 + 0.55, y0, 0.95, 1, 0, 0, 0], 1: [x0 + 0.4, y0, 1.2, 1, 0, 0, 0]}, {}]
    qs, blks = [], []
    for si, scene in enumerate(scenes):
        for kind in ("standing", "perturbed", "lifted", "sunk", "lying"):
            k = 7 if kind != "standing" else 5
            if kind == "lying":
                q = lying(rng, k, rng.uniform(0.0, 0.01))
            else:
                q = np.tile(STD, (k, 1))
                q[:, :2] += rng.normal(size=(k, 2)) * 0.05
                if kind != "standing":
                    q[:, 7:] += rng.normal(size=(k, 69)) * 0.15
                q[:, 2] += {"standing": 0.0, "perturbed": 0.0, "lifted": 0.341 if si == 3 else 0.1, "sunk": -0.03}[kind] + rng.normal(size=k) * 0.005
            b = parked(k)
            if scene:
                for oi, pose in scene.items():
                    b[:, 7 * oi: 7 * oi + 7] = pose
                    b[:, 7 * oi: 7 * oi + 2] += rng.normal(size=(k, 2)) * 0.03
            qs.append(q); blks.append(b if scene is not None else None)
    return qs, blks


def run(sim, q, blk):
    out = sim.pose_contacts(dev(q), None if blk is None else dev(blk))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def near_tie(o, q, blk):
    """the oracle frame has a contact within 1e-5 of the margin, or a hull whose two deepest vertices lie within 1e-6 of each other"""
    f = oracle_frame(o, KPM, q, blk)
    if any(abs(d - 0.001) < 1e-5 for _, _, d in f["contacts"]):
        return True
    verts, vadr = KPM["verts"].reshape(-1, 3), KPM["vert_adr"]
    for b in range(24):
        z = np.sort((f["xpos"][b] + verts[vadr[b]:vadr[b + 1]] @ O.quaternion_matrix3(f["xquat"][b]).T)[:, 2])
        if z[0] < 0.001 and z[1] - z[0] < 1e-6:
            return True
    return False


def test_pose_contacts_match_oracle(sim):
    qs, blks = seeded_rows()
    o = OracleSim(kpm=STEP_KPM)
    n, bad, ties = 0, [], 0
    for q, blk in zip(qs, blks):
        got = run(sim, q, blk)
        for e in range(len(q)):
            f = oracle_frame(o, KPM, q[e].astype(np.float32).astype(np.float64), None if blk is None else blk[e].astype(np.float32).astype(np.float64))
            n += 1
            ok = np.array_equal(got["hits"][e], f["hits"]) and got["ncon"][e] == f["ncon"] and abs(got["pen"][e] - f["pen"]) < 2e-5
            if not ok:
                if near_tie(o, q[e].astype(np.float32).astype(np.float64), None if blk is None else blk[e].astype(np.float32).astype(np.float64)):
                    ties += 1
                else:
                    bad.append((e, got["ncon"][e], f["ncon"], got["pen"][e], f["pen"], got["hits"][e].tolist(), f["hits"].tolist()))
    print(f"pose contacts vs oracle: {n} rows, {ties} near-tie rows differ")
    assert n >= 190
    assert not bad, bad[:5]
    assert ties < 0.02 * n
    allhits = np.concatenate([run(sim, q, b)["hits"] for q, b in zip(qs, blks)])
    assert {8, 9, 0}.issubset({g for g in range(10) if allhits[:, g].any()})          # the Can, the step and the chair were touched


def test_more_than_64_contacts(sim):
    """a lying pose lowered into the floor: the device counts every contact (the step path keeps 64); the oracle's narrow phase per hull is the truth"""
    q = lying(np.random.default_rng(5), 1, 0.5)
    got = run(sim, q, None)
    f = O.qpos_fk(q[0].astype(np.float32).astype(np.float64), KPM["body_pos"].reshape(24, 3), KPM["body_ipos"].reshape(24, 3), KPM["body_parent"])
    verts, vadr, nadr, nbr = KPM["verts"].reshape(-1, 3), KPM["vert_adr"], KPM["vert_nbr_adr"], KPM["vert_nbr"]
    pm_max, pm_tol = KPM["planemesh"]
    ncon, pen = 0, 0.0
    for b in range(24):
        vb = verts[vadr[b]:vadr[b + 1]]
        graph = [list(nbr[nadr[v]:nadr[v + 1]]) for v in range(vadr[b], vadr[b + 1])]
        R = O.quaternion_matrix3(f["wbquat"][b])
        hull = shape_record("hull", pos=f["wbpos"][b], mat=R, center=f["wbpos"][b] + R @ KPM["body_ipos"].reshape(24, 3)[b])
        c = narrowphase("plane_mesh", b=hull, verts_b=vb, graph=graph,
                        margin=0.001, tol_rbound=pm_tol * KPM["mesh_rbound"][b], maxcon=int(pm_max))
        ncon += len(c); pen += np.maximum(0.0, -c[:, 0] - 0.005).sum()
    print("lying pose in the floor:", got["ncon"][0], "contacts (oracle", ncon, ")")
    assert ncon >= 65
    assert got["ncon"][0] == ncon
    assert abs(got["pen"][0] - pen) < 2e-5


def test_rows_are_independent(sim):
    qs, blks = seeded_rows()
    q = np.concatenate(qs)
    b = np.concatenate([x if x is not None else parked(len(y)) for x, y in zip(blks, qs)])
    whole = run(sim, q, b)
    perm = np.random.default_rng(3).permutation(len(q))
    sh = run(sim, q[perm], b[perm])
    for k in ("pen", "ncon", "hits"):
        assert np.array_equal(sh[k], whole[k][perm])
    parts = [run(sim, q[a:a + 37], b[a:a + 37]) for a in range(0, len(q), 37)]
    for k in ("pen", "ncon", "hits"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])
    none = run(sim, q, None)
    allp = run(sim, q, parked(len(q)))
    for k in ("pen", "ncon", "hits"):
        assert np.array_equal(none[k], allp[k])
    assert not none["hits"].any()


def test_physics_metrics_match_reference_fixture(sim):
    from kinpoly_amd import metrics as M
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "physics_metrics.npz"))
    T = int(g["T"])
    names = [str(n) for n in g["names"]]
    results, gt = {}, {}
    for i, k in enumerate(names):
        sl = slice(i * T, (i + 1) * T)
        results[k] = {"pred": list(g["qpos_pred"][sl].astype(np.float64)), "obj_pose": list(g["obj_pose"][sl].astype(np.float64)),
                      "percent": 1.0, "fail_safe": bool(g["fail_safe"][i])}
        gt[k] = {"qpos": g["qpos_gt"][sl].astype(np.float64), "head_pose": g["head_pose_gt"][sl]}
    m = M.coverage_physics_metrics(results, gt, sim, chunk_rows=100)        # several chunks
    for i, k in enumerate(names):
        p = m["per_take"][k]
        known = k.split("-")[0] in ("sit", "avoid", "push", "step", "None")
        assert bool(p["succ"]) == (bool(g["succ_pred"][i]) if known else True), k
        assert bool(p["succ_gt"]) == (bool(g["succ_gt"][i]) if known else True), k
        for side in ("pred", "gt"):
            assert abs(p["pen_" + side] - g["pen_" + side][i]) < 0.01, (k, side)
            assert abs(p["slide_" + side] - g["slide_" + side][i]) <= 1e-3 * abs(g["slide_" + side][i]) + 1e-6, (k, side)
    assert set(m["succ_by_action"]) == {n.split("-")[0] for n in names}
    assert abs(m["pen_pred"] - np.mean([m["per_take"][k]["pen_pred"] for k in names])) < 1e-12


def test_abi_errors(sim):
    L = sim.L
    z = torch.zeros((2, 96), dtype=torch.float32, device="cuda")
    pen = torch.zeros(2, dtype=torch.float32, device="cuda")
    nc = torch.zeros(2, dtype=torch.int32, device="cuda")
    hits = torch.zeros((2, 10), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = (p(z), p(z), None, C.c_float(0.005), p(pen), p(nc), p(hits))
    assert L.kp_sim_pose_contacts(None, 2, *good) == -1 and b"null sim" in L.kp_last_error()
    assert L.kp_sim_pose_contacts(sim.h, -1, *good) == -1 and b"n_rows" in L.kp_last_error()
    assert L.kp_sim_pose_contacts(sim.h, 2, None, p(z), *good[2:]) == -1 and b"xpos" in L.kp_last_error()
    assert L.kp_sim_pose_contacts(sim.h, 2, p(z), None, *good[2:]) == -1 and b"xquat" in L.kp_last_error()
    for k in (4, 5, 6):
        args = list(good); args[k] = None
        assert L.kp_sim_pose_contacts(sim.h, 2, *args) == -1 and b"null output" in L.kp_last_error()
    assert L.kp_sim_pose_contacts(sim.h, 0, *good) == 0
    assert L.kp_sim_pose_contacts(sim.h, 0, None, None, None, C.c_float(0.005), None, None, None) == -1      # null pointers are checked first
    with pytest.raises(ValueError):
        sim.pose_contacts(torch.zeros((2, 75), device="cuda"))
    with pytest.raises(ValueError):
        sim.pose_contacts(torch.zeros((2, 76), device="cuda"), torch.zeros((3, 35), device="cuda"))
    out = sim.pose_contacts(torch.zeros((0, 76), device="cuda"))
    assert out["pen"].shape == (0,) and out["hits"].shape == (0, 10)
