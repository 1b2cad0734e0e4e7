"""Pose fitting to points at body offsets with a floor term, without a GPU: the identity the design rests on (weighted points
are point masses: J^T W J is the joint-space inertia of the ten floats per body the kernel writes), the fp64 reference tests/fit_points_oracle.py on
EVERY case the GPU tests use (this is where the inputs are chosen), the floor bound, the binding's checks on CPU tensors, the host logic of
kinpoly_amd/fit.py and scripts/fit_takes.py, and the library's surface."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fit_points_oracle as FT  # noqa: E402
import fit_pose_oracle as FP  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
from kinpoly_amd import build as kpbuild  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)
F32 = torch.float32


@pytest.fixture(scope="module")
def o():
    return FT.oracle(DEFAULT_KPM)


@pytest.fixture(scope="module")
def states():
    return ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"]), ID.sweep_states(KPM, STD["qpos"])


# ---------------------------------------------------------------- the identity the design rests on

def test_weighted_points_are_point_masses(o, states):
    """sum_k w_k J_k^T J_k from the oracle's own point Jacobians = the joint-space inertia assembled (composite-rigid-body algorithm) from the ten floats
    per body the kernel writes: several points per body, bodies that carry none, weights with zeros, with and without w_rot on the diagonal"""
    db, bp = np.asarray(KPM["dof_body"]).astype(int), np.asarray(KPM["body_parent"]).astype(int)
    rng = np.random.default_rng(11)
    for i, (name, q) in enumerate(FP.jacobian_poses(STD["qpos"], states[0]).items()):
        counts = rng.integers(0, 6, 24); counts[rng.integers(24)] = 0; counts[0] = 0 if i % 2 else 7
        body, off = FT.marker_set(list(counts), 40 + i)
        w = rng.uniform(0.0, 3.0, len(body)); w[::5] = 0.0
        wr = rng.uniform(0.0, 1.0, 24) if i % 2 else np.zeros(24)
        xpos, xquat = FP.fk(o, q)
        tq = xquat if i % 2 else None
        pb = FT.problem(KPM, body, off, rng.normal(size=(len(body), 3)), w, tgt_quat=tq, w_rot=wr if i % 2 else None)
        _, _, H, res = FT.normal_system(o, pb, q, 0.0, FT.DEFAULT_CFG)
        ci = FT.body_floats(xpos, res["p"], body, pb["w"], wr)
        assert np.all(ci[counts == 0, 9] == 0.0)
        M = FT.inertia_from_floats(o, q, ci, db, bp)
        d = float(np.abs(H - M).max())
        print(f"{name}: {len(body)} points, |sum w J^T J - M(ten floats)| max {d:.2e} on entries up to {np.abs(M).max():.1f}")
        assert d < 1e-10
    # the floor's blocks are the same thing: every vertex below the floor a point mass w_floor at its place
    q = FT.grounded(o, KPM, states[0][0]["q"], -0.05)
    cfg = dict(FT.DEFAULT_CFG, w_floor=7.0)
    pb = FT.problem(KPM, tgt_pos=np.zeros((24, 3)), w_pos=np.zeros(24))
    _, g, H, res = FT.normal_system(o, pb, q, 0.0, cfg)
    act = res["depth"] > 0
    assert 4 < act.sum() < 1199
    xpos, _ = FP.fk(o, q)
    M = FT.inertia_from_floats(o, q, FT.body_floats(xpos, res["hp"][act], pb["hb"][act], np.full(act.sum(), 7.0)), db, bp)
    assert float(np.abs(H - M).max()) < 1e-10
    # and the gradient is exact: central differences of the true cost
    eps, worst = 1e-6, 0.0
    body, off = FT.marker_set(FT.counts_53(), 1)
    pb = FT.problem(KPM, body, off, FT.marker_positions(o, states[0][2]["q"], body, off) + 0.01, q_prior=STD["qpos"][7:], w_prior=np.full(69, 0.1))
    _, g, _, _ = FT.normal_system(o, pb, q, 0.0, cfg)
    for k in range(0, 75, 3):
        e = np.zeros(75); e[k] = eps
        fd = (FT.evaluate(o, pb, FP.oplus(q, e), cfg)[0] - FT.evaluate(o, pb, FP.oplus(q, -e), cfg)[0]) / (2 * eps)
        worst = max(worst, abs(fd + g[k]) / max(1.0, abs(g[k])))
    print(f"gradient (points + prior + floor) against central differences of the cost: {worst:.2e}")
    assert worst < 1e-6


# ---------------------------------------------------------------- the cases of the GPU tests

def test_marker_sets_of_the_gpu_tests():
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    assert len(body) == 53 and np.linalg.norm(off, axis=1).max() <= FT.OFFSET_RADIUS + 1e-7 and np.array_equal(off, FT.f32(off))
    counts = np.bincount(body, minlength=24)
    assert counts.min() >= 2 and counts[0] >= 3 and not np.all(np.diff(body) >= 0), "every body carries markers; the caller's order is not the sorted one"
    # three points off one line per body: its own markers, and for a body with two the joint that ties it to its parent (its own origin)
    for b in range(24):
        pts = list(off[body == b]) + ([np.zeros(3)] if counts[b] < 3 else [])
        d = pts[1] - pts[0]
        assert max(np.linalg.norm(np.cross(p - pts[0], d)) / np.linalg.norm(d) for p in pts[2:]) > 0.01, b
    body, off = FT.marker_set(FT.counts_67(), FT.SEED_67)
    counts = np.bincount(body, minlength=24)
    assert len(body) == 67 and counts.max() == 40 and (counts == 0).sum() == 9


def test_reference_converges_on_every_reachable_case(o, states):
    """every one of the 67 reachable cases (53 markers, no orientations): max |e_k| <= 1e-5 m within the case's n_iters, and the pose IS determined
    by the markers: the hinges come back at the truth"""
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    worst_e, worst_h, need = 0.0, 0.0, 0
    for i, q in enumerate(FP.truth_poses(*states)):
        c = FT.reachable_case(o, q, 100 + i, body, off, exact=True)
        r = FT.lm(o, c["q0"], FT.problem(KPM, body, off, c["pt_tgt"]), dict(n_iters=FT.reach_iters(i)))
        dh = float(np.abs((r["qpos"][7:] - c["q_true"][7:] + np.pi) % (2 * np.pi) - np.pi).max())
        worst_e, worst_h = max(worst_e, r["info"][8]), max(worst_h, dh)
        first = next(n + 1 for n in range(len(r["costs"])) if r["costs"][n] <= 0.5 * 1e-10)      # cost <= 1/2 (1e-5)^2 bounds every |e_k| by 1e-5
        need = max(need, first)
        assert r["info"][8] <= 1e-5, f"case {i}: max |e_k| {r['info'][8]:.2e} m after {FT.reach_iters(i)} iterations"
        assert dh < 1e-3 and np.abs(r["qpos"][:3] - c["q_true"][:3]).max() < 1e-4, f"case {i}: hinges {dh:.2e} rad off the truth: another pose fits the markers"
    print(f"reachable cases: max |e_k| {worst_e:.2e} m, hinges within {worst_h:.2e} rad of the truth, cost under 5e-11 after at most {need} iterations")


def test_floor_cases_keep_their_active_sets_clear_of_the_plane(o, states):
    """In the fp64 loop no hull vertex comes within 1e-5 m of floor_z at any pose at which the GPU test compares with the reference: the pose the gradient is
    formed at and the trial pose of the one-step cases, every pose the loop evaluates in the FLOOR_COMPARE_ITERS iterations of the floor cases, at both of
    their weights.  That makes the active sets equal on the device only where the device follows the reference to better than that margin: the one-step
    cases at FLOOR_PARITY_W and the floor cases at FLOOR_COMPARE_W, not at w_floor = 2400 (fit_points_oracle.FLOOR_COMPARE_ITERS says what is held there)."""
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    worst, conds = np.inf, {}
    for i, q in enumerate(FP.truth_poses(*states)):
        c = FT.sunk_marker_case(o, KPM, q, i, body, off)
        for wf in (FT.FLOOR_PARITY_W, FT.FLOOR_W):
            r = FT.lm(o, c["q0"], FT.problem(KPM, body, off, c["pt_tgt"]), dict(n_iters=1, w_floor=wf))
            worst = min(worst, r["margin"])
            assert r["margin"] >= 1e-5, f"one-step floor case {i}, w_floor {wf}: a vertex {r['margin']:.2e} m from the plane"
            assert r["info"][11] == 0 or r["info"][10] > 0
            conds[wf] = max(conds.get(wf, 0.0), float(np.linalg.cond(r["A"])) * 2.0 ** -23)
    for name, (q, fz) in FT.floor_poses(states[0]).items():
        c = FT.floor_case(o, KPM, q, fz)
        for wf in (FT.FLOOR_COMPARE_W, FT.FLOOR_W):
            r = FT.lm(o, c["q0"], FT.problem(KPM, tgt_pos=c["tgt_pos"]), dict(n_iters=FT.FLOOR_COMPARE_ITERS, w_floor=wf, floor_z=fz))
            worst = min(worst, r["margin"])
            assert r["margin"] >= 1e-5, f"floor case {name}, w_floor {wf}: a vertex {r['margin']:.2e} m from the plane at an iterate"
            assert r["info"][2] >= FT.FLOOR_COMPARE_ITERS - 1 and r["info"][11] > 0, "the compared iterations move the pose, and vertices are below the floor at their end"
            conds[(name, wf)] = float(np.linalg.cond(r["A"])) * 2.0 ** -23
        assert conds[(name, FT.FLOOR_COMPARE_W)] < 0.1 < conds[(name, FT.FLOOR_W)]
    print(f"floor cases: the nearest vertex stays {worst:.2e} m from the plane; one-step cond(A) 2^-23 up to {conds}")
    assert conds[FT.FLOOR_PARITY_W] < 1e-2 and conds[FT.FLOOR_W] > 1.0, "why the parity variant under the dq cap does not run at w_floor = 2400 (fit_points_oracle.FLOOR_PARITY_W)"


def test_equivalence_reference_fixture(o, states):
    """tests/golden/fit_points_equiv_ref.npz is the fp64 loop on the body origins after EQUIV_ITERS iterations, and that loop has come to rest: the last
    step is below 1e-12, the targets (fp32 roundings of reachable positions) are met to their rounding"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "fit_points_equiv_ref.npz"))
    qpos, info = FT.equiv_reference(o, FP.truth_poses(*states))
    assert np.allclose(gold["qpos"], qpos, atol=1e-9) and np.allclose(gold["info"], info, rtol=1e-9, atol=1e-15), "the fixture is stale"
    print(f"equivalence reference: final max |e_pos| up to {info[:, 4].max():.2e} m, last |dq| up to {info[:, 6].max():.2e}")
    assert info[:, 6].max() < 1e-12 and info[:, 4].max() < 5e-7 and np.all(info[:, 7] == 0)


def test_floor_bound(o, states):
    """Targets: 24 origins moved delta = 0.03 m down, w_pos 1, w_floor 2400.  'Translate up by delta' is feasible and costs 1/2 24 delta^2, so a pose
    whose cost lies below that has 1/2 w_floor d_max^2 <= 1/2 24 delta^2: d_max <= delta sqrt(24 / 2400) = 3 mm.  The fp64 loop gets there."""
    assert FT.FLOOR_BOUND == pytest.approx(0.003, rel=1e-12)
    for name, (q, fz) in FT.floor_poses(states[0]).items():
        c = FT.floor_case(o, KPM, q, fz)
        assert abs(FT.lowest_vertex(o, KPM, c["q_on"]) - fz) < 1e-6
        pb = FT.problem(KPM, tgt_pos=c["tgt_pos"])
        cfg = dict(n_iters=FT.FLOOR_ITERS, w_floor=FT.FLOOR_W, floor_z=fz)
        cand, _ = FT.evaluate(o, pb, c["q_on"], {**FT.DEFAULT_CFG, **cfg})
        assert cand == pytest.approx(c["cand_cost"], rel=1e-4), "the candidate touches the floor and misses every target by delta"
        r = FT.lm(o, c["q0"], pb, cfg)
        free = FT.lm(o, c["q0"], pb, dict(cfg, w_floor=0.0))
        print(f"{name}: cost {r['info'][0]:.4e} -> {r['info'][1]:.4e} (candidate {cand:.4e}), deepest vertex {r['info'][10] * 1e3:.3f} mm ({r['info'][11]:.0f} below), "
              f"without the floor {free['info'][10] * 1e3:.2f} mm")
        assert r["info"][1] < cand and r["info"][10] <= FT.FLOOR_BOUND
        assert free["info"][10] >= 0.029 and free["info"][1] < 1e-12


# ---------------------------------------------------------------- the binding on CPU tensors

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def cpu_sim(monkeypatch):
    from kinpoly_amd import sim as S
    monkeypatch.setattr(S, "_dev", lambda name, t, shape, dtype=F32: None)
    sim = object.__new__(S.KpSim)
    sim.L, sim.h, sim.device, sim.model = _Recorder(), None, "cpu", None
    return sim


def test_binding_shapes_and_want(cpu_sim):
    from kinpoly_amd import sim as S
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    cfg = S.KpFitPointsCfg()
    for lead in ((), (5,), (2, 3)):
        out = cpu_sim.fit_points(torch.zeros(lead + (76,)), body, off, torch.zeros(lead + (53, 3)), cfg=cfg, want=("qpos", "info", "dq", "pt_err"))
        assert {k: tuple(v.shape) for k, v in out.items()} == {"qpos": lead + (76,), "info": lead + (12,), "dq": lead + (75,), "pt_err": lead + (53,)}
    assert [c[0] for c in cpu_sim.L.calls] == ["kp_sim_fit_points"] * 3 and cpu_sim.L.calls[1][1][1] == 5
    cpu_sim.L.calls.clear()
    out = cpu_sim.fit_points(torch.zeros(2, 0, 76), body, off, torch.zeros(2, 0, 53, 3), cfg=cfg, want=("pt_err",))
    assert tuple(out["pt_err"].shape) == (2, 0, 53) and cpu_sim.L.calls == [], "no rows, no native call"
    out = cpu_sim.fit_points(torch.zeros(4, 76), [], np.zeros((0, 3)), tgt_pos=torch.zeros(4, 24, 3), cfg=cfg, want=("info", "pt_err"))
    assert tuple(out["pt_err"].shape) == (4, 0) and tuple(out["info"].shape) == (4, 12), "K = 0 with tgt_pos"
    q, t = torch.zeros(5, 76), torch.zeros(5, 53, 3)
    for call, msg in ((lambda: cpu_sim.fit_points(q, body, off, t, want=("nope",), cfg=cfg), "want must name"),
                      (lambda: cpu_sim.fit_points(q, body, off, t, want=(), cfg=cfg), "want must name"),
                      (lambda: cpu_sim.fit_points(q, body, off, cfg=cfg), "pt_tgt is required"),
                      (lambda: cpu_sim.fit_points(q, body, off, t[:, :52], cfg=cfg), "pt_tgt must be"),
                      (lambda: cpu_sim.fit_points(q, body, off, t[:4], cfg=cfg), "pt_tgt must be"),
                      (lambda: cpu_sim.fit_points(q, body, off, t, torch.zeros(5, 52), cfg=cfg), "pt_w must be"),
                      (lambda: cpu_sim.fit_points(q[:, :75], body, off, t, cfg=cfg), "qpos0 must be"),
                      (lambda: cpu_sim.fit_points(q, body, off, t, tgt_pos=torch.zeros(5, 23, 3), cfg=cfg), "tgt_pos must be"),
                      (lambda: cpu_sim.fit_points(q, body, off, t, q_prior=torch.zeros(5, 69), cfg=cfg), "go together"),
                      (lambda: cpu_sim.fit_points(q, [], np.zeros((0, 3)), cfg=cfg), "nothing to fit"),
                      (lambda: cpu_sim.fit_points(q, body[:52], off, t, cfg=cfg), "pt_offset must be"),
                      (lambda: cpu_sim.fit_points(q, body.astype(np.float32), off, t, cfg=cfg), "integer"),
                      (lambda: cpu_sim.fit_points(q, np.where(body == 3, 24, body), off, t, cfg=cfg), "0..23"),
                      (lambda: cpu_sim.fit_points(q, np.where(body == 3, -1, body), off, t, cfg=cfg), "0..23"),
                      (lambda: cpu_sim.fit_points(q, body, np.where(off > 0.1, np.inf, off), t, cfg=cfg), "finite"),
                      (lambda: cpu_sim.fit_points(torch.zeros(5, 76), np.zeros(1025, int), np.zeros((1025, 3)), torch.zeros(5, 1025, 3), cfg=cfg), "at most 1024")):
        with pytest.raises(ValueError, match=msg):
            call()


def test_marker_set_and_config_validation(tmp_path):
    from kinpoly_amd.fit import FitConfig, MarkerSet
    m = MarkerSet.body_origins()
    assert len(m) == 24 and list(m.body) == list(range(24)) and not m.offset.any() and m.body.dtype == np.int32 and m.offset.dtype == np.float32
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    m = MarkerSet([f"m{k}" for k in range(53)], body, off)
    m.save(tmp_path / "set.json")
    back = MarkerSet.load(tmp_path / "set.json")
    assert back.names == m.names and np.array_equal(back.body, m.body) and np.array_equal(back.offset, m.offset), "fp32 offsets survive json exactly"
    for bad in (lambda: MarkerSet(["a"], [0, 1], np.zeros((2, 3))), lambda: MarkerSet(["a", "a"], [0, 1], np.zeros((2, 3))), lambda: MarkerSet(["a"], [24], np.zeros((1, 3))),
                lambda: MarkerSet(["a"], [0], np.full((1, 3), np.nan)), lambda: MarkerSet(["a"], [0], np.zeros((1, 2))), lambda: MarkerSet(["a"], [0.5], np.zeros((1, 3)))):
        with pytest.raises(ValueError):
            bad()
    json.dump({"names": ["a"], "body": [0]}, open(tmp_path / "short.json", "w"))
    with pytest.raises(ValueError, match="offset"):
        MarkerSet.load(tmp_path / "short.json")
    assert FitConfig().w_floor == 0.0 and FitConfig().floor_z == 0.0, "the defaults leave every existing call as it is"
    c = FitConfig(n_iters=7, w_floor=2400.0, floor_z=0.05).native_points()
    assert c.fit.n_iters == 7 and c.w_floor == 2400.0 and c.floor_z == pytest.approx(0.05) and list(c.fit.damp) == [1.0] * 75
    for bad in (dict(w_floor=-1.0), dict(w_floor=float("nan")), dict(w_floor=float("inf")), dict(floor_z=float("nan")), dict(floor_z=float("inf")), dict(mu0=0.0)):
        with pytest.raises(ValueError, match="FitConfig"):
            FitConfig(**bad).native_points()


class OracleFkSim:
    """a sim whose fk is the oracle's and whose fit_points records its arguments and answers with its init"""
    device = torch.device("cpu")

    def __init__(self, o):
        self.o, self.calls = o, []

    def fk(self, rows):
        xp, xq = zip(*[FP.fk(self.o, r.double().numpy()) for r in rows])
        return {"wbpos": torch.tensor(np.stack(xp).reshape(len(rows), 72), dtype=F32), "wbquat": torch.tensor(np.stack(xq).reshape(len(rows), 96), dtype=F32)}

    def fit_points(self, qpos0, pt_body, pt_offset, pt_tgt=None, pt_w=None, tgt_pos=None, tgt_quat=None, w_pos=None, w_rot=None, q_prior=None, w_prior=None, cfg=None,
                   want=("qpos", "info")):
        lead = tuple(qpos0.shape[:-1])
        pt_w = torch.ones(lead + (len(pt_body),)) if pt_w is None else pt_w
        self.calls.append(dict(qpos0=qpos0.clone(), pt_tgt=None if pt_tgt is None else pt_tgt.clone(), pt_w=pt_w.clone(), tgt_pos=tgt_pos, tgt_quat=tgt_quat, w_rot=w_rot,
                               q_prior=q_prior, w_prior=w_prior, cfg=cfg, want=want, K=len(pt_body)))
        q = qpos0.clone(); q[..., 7] += 1.0
        info = torch.zeros(lead + (12,)); info[..., 2] = 3.0; info[..., 10] = 0.002; info[..., 11] = 4.0
        out = {"qpos": q, "info": info, "pt_err": torch.where(pt_w > 0, torch.full_like(pt_w, 0.01), torch.zeros_like(pt_w))}
        return {k: out[k] for k in want}


def test_from_pose_round_trip_and_occlusion(o, states):
    from kinpoly_amd import fit
    sim = OracleFkSim(o)
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    q = states[0][2]["q"]                                              # lying: every body frame turned
    world = FT.marker_positions(o, q, body, off)
    m = fit.MarkerSet.from_pose(sim, q, world, body)
    print(f"MarkerSet.from_pose: offsets back within {np.abs(m.offset - off).max():.2e} m")
    assert np.abs(m.offset - off).max() < 5e-7 and np.array_equal(m.body, body), "o = R_b^T (p - x_b), through an fp32 forward pass"
    # a NaN target is an occluded marker: weight 0, whatever weight was given; the init sits on the visible markers
    tgt = torch.tensor(world, dtype=F32).expand(3, 53, 3).clone()
    tgt[1, 4, 2] = float("nan"); tgt[2, 7] = float("nan")
    w = torch.full((3, 53), 2.0)
    fit.fit_points(sim, m, tgt, w)
    got = sim.calls[-1]["pt_w"]
    assert got[1, 4] == 0 and got[2, 7] == 0 and int((got == 2.0).sum()) == 3 * 53 - 2
    assert torch.isfinite(sim.calls[-1]["qpos0"]).all() and sim.calls[-1]["qpos0"].shape == (3, 76)
    fit.fit_points(sim, m, tgt)
    assert int((sim.calls[-1]["pt_w"] == 1.0).sum()) == 3 * 53 - 2 and int((sim.calls[-1]["pt_w"] == 0.0).sum()) == 2
    with pytest.raises(ValueError, match="tgt must be"):
        fit.fit_points(sim, m, tgt[:, :52])
    with pytest.raises(ValueError, match="w must be"):
        fit.fit_points(sim, m, tgt, w[:, :52])
    # sequences: one call for independent frames, one per frame when chained, the solution at t - 1 as init and prior
    tr = tgt[None].expand(2, 3, 53, 3).contiguous()
    n0 = len(sim.calls)
    out = fit.fit_sequence_points(sim, m, tr, mode="independent")
    assert len(sim.calls) == n0 + 1 and out["qpos"].shape == (2, 3, 76) and out["pt_err"].shape == (2, 3, 53) and out["info"].shape == (2, 3, 12)
    out = fit.fit_sequence_points(sim, m, tr, mode="chained", smooth=0.25, config=fit.FitConfig(w_floor=5.0))
    assert len(sim.calls) == n0 + 4 and sim.calls[n0 + 1]["q_prior"] is None and sim.calls[-1]["cfg"].w_floor == 5.0
    assert torch.equal(sim.calls[-1]["qpos0"], out["qpos"][:, 1]) and torch.equal(sim.calls[-1]["q_prior"], out["qpos"][:, 1, 7:]) and bool((sim.calls[-1]["w_prior"] == 0.25).all())
    for bad in (dict(mode="other"), dict(smooth=-1.0)):
        with pytest.raises(ValueError, match="fit_sequence_points"):
            fit.fit_sequence_points(sim, m, tr, **bad)
    seen = (~torch.isnan(tr).any(-1)).float().numpy()
    rep = fit.points_report(["a", "b"], m.names, out["pt_err"].numpy(), seen, out["info"].numpy(), n_iters=6)
    assert rep["a"]["max_pt_err"] == pytest.approx(0.01) and rep["a"]["pt_err_p90"] == pytest.approx(0.01) and rep["a"]["visible_share"] == pytest.approx(1 - 2 / 159)
    assert rep["a"]["max_penetration"] == pytest.approx(0.002) and rep["a"]["frames_penetrating"] == 3 and rep["a"]["accepted_share"] == pytest.approx(0.5)
    assert set(rep["b"]["per_marker"]) == set(m.names) and rep["b"]["per_marker"]["m4"]["p50"] == pytest.approx(0.01)


def test_fit_takes_markers_arguments(o, tmp_path):
    """scripts/fit_takes.py --markers / --floor with a stub solver: the pickle loads with AmassSingleDataset; K mismatches and wbpos-only tracks are refused"""
    import joblib
    from kinpoly_amd import fit
    from kinpoly_amd.dataset import AmassSingleDataset
    spec = importlib.util.spec_from_file_location("fit_takes", os.path.join(ROOT, "scripts", "fit_takes.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    fit.MarkerSet([f"m{k}" for k in range(53)], body, off).save(tmp_path / "set.json")
    rng = np.random.default_rng(0)
    tracks = {"walk": {"markers": rng.normal(size=(100, 53, 3))}, "sit": {"markers": rng.normal(size=(95, 53, 3)), "obj_pose": np.zeros((95, 35))}}
    tracks["walk"]["markers"][3, 5] = np.nan
    joblib.dump(tracks, tmp_path / "in.pkl")
    sim = OracleFkSim(o)
    args = ["--tracks", str(tmp_path / "in.pkl"), "--out", str(tmp_path / "o" / "takes.pkl"), "--iters", "4", "--markers", str(tmp_path / "set.json"), "--floor", "2400", "--floor_z", "0.05"]
    takes, rep = mod.main(args, sim=sim)
    assert len(sim.calls) == 100 and sim.calls[0]["cfg"].fit.n_iters == 4 and sim.calls[0]["cfg"].w_floor == 2400.0 and sim.calls[0]["cfg"].floor_z == pytest.approx(0.05)
    assert sim.calls[3]["pt_w"][0, 5] == 0 and sim.calls[3]["pt_w"].sum() == 2 * 53 - 1
    on_disk = json.load(open(tmp_path / "o" / "fit_report.json"))
    assert set(on_disk) == set(tracks) and {"max_pt_err", "pt_err_p99", "per_marker", "max_penetration", "frames_penetrating"} <= set(on_disk["walk"])
    ds = AmassSingleDataset({"file_path": str(tmp_path / "o" / "takes.pkl"), "t_min": 90}, "train")
    assert ds.data_keys == ["walk", "sit"] and list(ds.lens) == [100, 95] and takes["sit"]["obj_pose"].shape == (95, 35)
    joblib.dump({"x": {"markers": np.zeros((5, 52, 3))}}, tmp_path / "k52.pkl")
    with pytest.raises(ValueError, match=r"markers must be \[T, 53, 3\]"):
        mod.main(["--tracks", str(tmp_path / "k52.pkl"), "--out", str(tmp_path / "x.pkl"), "--markers", str(tmp_path / "set.json")], sim=sim)
    joblib.dump({"x": {"wbpos": np.zeros((5, 24, 3))}}, tmp_path / "wb.pkl")
    with pytest.raises(ValueError, match="no 'markers'"):
        mod.main(["--tracks", str(tmp_path / "wb.pkl"), "--out", str(tmp_path / "x.pkl"), "--markers", str(tmp_path / "set.json")], sim=sim)
    for bad in (["--floor", "-1"], ["--floor_z", "0.1"]):
        with pytest.raises(SystemExit):
            mod.main(["--tracks", str(tmp_path / "wb.pkl"), "--out", str(tmp_path / "x.pkl")] + bad, sim=sim)
    # --floor on body-position tracks: the same targets (orientations included) with the floor term, fit_report's columns plus the penetration ones
    tq = np.zeros((5, 24, 4)); tq[..., 0] = 1.0
    joblib.dump({"x": {"wbpos": rng.normal(size=(5, 24, 3)), "wbquat": tq}}, tmp_path / "wbq.pkl")
    n0 = len(sim.calls)
    _, rep = mod.main(["--tracks", str(tmp_path / "wbq.pkl"), "--out", str(tmp_path / "y.pkl"), "--floor", "10", "--floor_z", "0.02"], sim=sim)
    last = sim.calls[-1]
    assert len(sim.calls) == n0 + 5 and last["K"] == 0 and last["pt_tgt"] is None and last["tgt_pos"].shape == (1, 24, 3) and last["tgt_quat"].shape == (1, 24, 4)
    assert last["cfg"].w_floor == 10.0 and last["cfg"].floor_z == pytest.approx(0.02) and bool((last["w_rot"] == 1).all()), "the take's orientations are used"
    assert {"mean_pos_err", "max_pos_err", "accepted_share", "failed_rows", "max_penetration", "mean_penetration", "frames_penetrating"} == set(rep["x"])
    assert rep["x"]["max_penetration"] == pytest.approx(0.002) and rep["x"]["frames_penetrating"] == 5
    # --floor 0 is the term switched off: the path and the output of a run without the flag (this stub has no fit_pose: the old path would call it)
    with pytest.raises(AttributeError, match="fit_pose"):
        mod.main(["--tracks", str(tmp_path / "wbq.pkl"), "--out", str(tmp_path / "z.pkl"), "--floor", "0"], sim=sim)
    m2 = fit.MarkerSet.load(tmp_path / "set.json")
    assert m2 == fit.MarkerSet([f"m{k}" for k in range(53)], body, off) and m2 != fit.MarkerSet.body_origins()


# ---------------------------------------------------------------- surface

def test_header_binding_and_symbols():
    """fails on the parent commit: the symbols are new"""
    from kinpoly_amd import sim as kpsim
    hdr = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    assert ("int kp_sim_fit_points(kp_sim*, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const kp_fit_points_cfg* cfg, "
            "const kp_fit_points_out* out);") in hdr
    assert "void kp_fit_points_cfg_default(kp_fit_points_cfg* cfg);" in hdr
    for word in ("majoriser", "ISOTROPIC", "No reference counterpart", "before the first HIP call"):
        assert word in hdr, word
    assert len(kpsim._SIGNATURES["kp_sim_fit_points"][1]) == 6 and "kp_fit_points_cfg_default" in kpsim._SIGNATURES
    assert [f[0] for f in kpsim.KpFitPointsIn._fields_] == ["qpos0", "pt_tgt", "pt_w", "tgt_pos", "tgt_quat", "w_pos", "w_rot", "q_prior", "w_prior"]
    assert [f[0] for f in kpsim.KpFitPointsOut._fields_] == ["qpos", "info", "dq", "pt_err"] == list(kpsim.fit_points_outputs(3))
    assert ctypes.sizeof(kpsim.KpFitPointsCfg) == ctypes.sizeof(kpsim.KpFitCfg) + 8 and ctypes.sizeof(kpsim.KpMarkerSet) == 24
    assert list(kpsim.FIT_POINTS_INFO)[:8] == list(kpsim.FIT_INFO) and list(kpsim.FIT_POINTS_INFO)[8:] == ["max_ept", "rms_ept", "max_depth", "n_below"]
    if not os.path.exists(kpbuild.LIB):
        pytest.fail(f"{kpbuild.LIB} is missing: build() first")
    L = ctypes.CDLL(kpbuild.LIB)
    for sym in ("kp_sim_fit_points", "kp_fit_points_cfg_default"):
        assert hasattr(L, sym), sym
    cfg = kpsim.KpFitPointsCfg()
    cfg.w_floor = 3.0; cfg.floor_z = 1.0
    L.kp_fit_points_cfg_default(ctypes.byref(cfg))
    ref = kpsim.KpFitCfg(); L.kp_fit_cfg_default(ctypes.byref(ref))
    assert bytes(cfg.fit) == bytes(ref) and cfg.w_floor == 0.0 and cfg.floor_z == 0.0
    L.kp_last_error.restype = ctypes.c_char_p
    L.kp_sim_fit_points.restype = ctypes.c_int; L.kp_sim_fit_points.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert L.kp_sim_fit_points(None, 1, None, None, None, None) == -1 and b"kp_sim_fit_points: null handle" in L.kp_last_error()
