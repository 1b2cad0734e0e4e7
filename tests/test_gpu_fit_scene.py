"""Pose fitting that keeps the hulls out of the scene's static objects (kp_sim_fit_scene) on a real MI355X: the kernel against
the fp64 reference tests/fit_scene_oracle.py on identical fp32 inputs, on the cases tests/test_fit_scene_cpu.py has chosen; bit-for-bit equality with
kp_sim_fit_points where the term is absent, row independence, one step against the dense solve, three iterations with equal discrete choices, thirty
iterations against the derived bound, the pose-contact walk, non-interference with the control step, and the refusals.

Tolerances not capped by the feature's specification = 4 x the device's separation from the fp64 reference measured on the MI355X (discrete accept and
plane flips at the rounding floor move figures by small factors: the margin of sections 17 and 20); every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fit_points_oracle as FT  # noqa: E402
import fit_pose_oracle as FP  # noqa: E402
import fit_scene_oracle as FS  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

STD = H.STD
KPM = read_kpm(STEP_KPM)
ROWS = FS.ROWS
ALL = ("qpos", "info", "dq", "pt_err")
SAME = slice(0, 12)                  # the info columns kp_sim_fit_points has too

# caps the specification sets: one step at w_obj 1 (section 20's cap), the normwise backward error of the step at w_obj 2400 (n u, n = 75, u = 2^-24), the
# derived bound on the deepest counted vertex
CAP = {"dq": 2.8e-4, "backward2400": 75 * 2.0 ** -24, "depth": FS.OBJ_BOUND}
# 4 x the largest separation from the fp64 reference measured on the MI355X (measured value in the comment)
TOL = {
    "dq": 4 * 2.152e-04,            # one step at w_obj = w_floor = 1 against the dense fp64 solve, relative inf-norm, worst of the 16 perturbed rows (can@0.66+p; the others 4.8e-06 .. 1.9e-04); measured 2.152e-04: the cap holds
    "cost": 4 * 1.766e-05,          # first cost and cost after the step, relative to the row's first cost; measured 1.766e-05
    "backward2400": 4 * 1.185e-07,  # the step at w_obj = w_floor = 2400 in the reference's system, normwise backward error; measured 1.185e-07 (its dq is 1.3e-01 off at cond(A) 2^-23 up to 18)
    "cost02400": 4 * 7.923e-06,     # the same, first cost, relative; measured 7.923e-06
    "it3_cost": 4 * 3.435e-05,      # three iterations at w 4: final cost against the reference's, relative to the first cost; measured 3.435e-05
    "it3_depth": 4 * 1.597e-06,     # the same: deepest counted vertex against the reference's [m]; measured 1.597e-06
    "it3_qpos": 4 * 7.998e-05,      # the same: qpos against the reference's; measured 7.998e-05
    "it30_depth": 4 * 1.513e-03,    # thirty iterations at 2400 on the cases held to the reference's own figure: deepest counted vertex against the reference's [m]; measured 1.513e-03 (sit: 21.9 mm against 20.4, the hands pinched between the seat and the back; sit_moved 1.8e-04)
}
for _k, _c in CAP.items():
    if _k in TOL:
        TOL[_k] = min(TOL[_k], _c)
M = H.Measured()


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def oracle():
    return memo("oracle", lambda: FS.oracle(STEP_KPM))


def cases():
    return memo("cases", lambda: FS.scene_cases(oracle(), KPM, ID.named_states(read_kpm(DEFAULT_KPM), KPM, STD["qpos"], STD["qvel"])))


def rows(R):
    """the first R rows of the comparisons: the 16 distinct ones in turn"""
    base = memo("rows", lambda: FS.compare_rows(cases()))
    return [base[e % len(base)] for e in range(R)]


def step_rows(R):
    """the first R rows of the one-step comparison: the same scenes from section 20's perturbed inits"""
    base = memo("step_rows", lambda: FS.step_rows(cases()))
    return [base[e % len(base)] for e in range(R)]


def reference(key, cfg, of=rows):
    """the fp64 loop on the 16 distinct rows for a configuration: computed once, shared by the row counts"""
    def make():
        return [FS.lm(oracle(), r["q0"], FS.problem(KPM, FS.scene_geoms(KPM, r["blk"]), tgt_pos=r["tgt_pos"]), cfg) for r in of(16)]
    return memo(("ref", key), make)


def cfg(kp, w_obj=0.0, w_floor=0.0, floor_z=0.0, **kw):
    c = kp.KpFitSceneCfg.default()
    c.w_obj, c.pts.w_floor, c.pts.floor_z = w_obj, w_floor, floor_z
    for k, v in kw.items():
        setattr(c.pts.fit, k, v)
    return c


def pcfg(kp, w_floor=0.0, **kw):
    c = kp.KpFitPointsCfg.default()
    c.w_floor = w_floor
    for k, v in kw.items():
        setattr(c.fit, k, v)
    return c


def stack(rs, key):
    return dev(np.stack([r[key] for r in rs]))


def bits(t):
    return t.contiguous().view(torch.int32)


NONE = (np.zeros(0, np.int32), np.zeros((0, 3), np.float32))      # no points: the 24 origins through tgt_pos


def scene(sim, rs, c, obj=True, want=ALL, blk=None):
    return sim.fit_scene(stack(rs, "q0"), *NONE, tgt_pos=stack(rs, "tgt_pos"), obj_qpos=(stack(rs, "blk") if blk is None else blk) if obj else None, cfg=c, want=want)


def same_as_points(a, b, what):
    for k in ("qpos", "dq", "pt_err"):
        assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k}"
    assert torch.equal(bits(a["info"][:, SAME]), bits(b["info"])), f"{what}: info 0..11"
    assert not a["info"][:, 15].any()


# ---------------------------------------------------------------- 1. where the term is absent: kp_sim_fit_points, bit for bit

@pytest.mark.parametrize("R", ROWS)
def test_equals_fit_points_where_the_term_is_absent(kp, R):
    sim, lean, rs = handle(kp, STEP_KPM), handle(kp), rows(R)
    q0, tp = stack(rs, "q0"), stack(rs, "tgt_pos")
    body, off = FT.marker_set(FT.counts_53(), FT.SEED_53)
    tgt = dev(np.stack([FT.marker_positions(oracle(), r["q0"], body, off) for r in rows(16)]) + 0.01)[torch.arange(R, device="cuda") % 16].contiguous()
    for name, pts in (("origins", dict(pt=NONE, kw=dict(tgt_pos=tp))), ("k53", dict(pt=(body, off), kw=dict(pt_tgt=tgt)))):
        ref = sim.fit_points(q0, *pts["pt"], cfg=pcfg(kp, FS.FLOOR_W, n_iters=5), want=ALL, **pts["kw"])
        assert bool((ref["info"][:, 2] > 0).all())
        full = cfg(kp, FS.OBJ_W, FS.FLOOR_W, n_iters=5)
        parked = dev(np.tile(FS.parked_block(), (R, 1)))
        far = dev(np.tile(FS.block(chair=[5.0, 5.0, 0.39, 1, 0, 0, 0], table=[-6.0, 2.0, 0.8, 0.9, 0.1, 0.2, 0.3]), (R, 1)))      # placed (within 50 m), separated from every hull
        for what, s, objs, c in (("null obj_qpos", sim, None, full), ("null obj_qpos, floor blob", lean, None, full), ("every object parked", sim, parked, full),
                                 ("objects separated from every hull", sim, far, full), ("w_obj = 0", sim, stack(rs, "blk"), cfg(kp, 0.0, FS.FLOOR_W, n_iters=5))):
            out = s.fit_scene(q0, *pts["pt"], obj_qpos=objs, cfg=c, want=ALL, **pts["kw"])
            same_as_points(out, ref, f"{name}, {what}")
            if what == "w_obj = 0":
                assert bool((out["info"][:, 13] > 0).any()), "12..14 are computed whether or not w_obj > 0"
            else:
                assert not out["info"][:, 12:15].any(), what


# ---------------------------------------------------------------- 2. rows are independent; calls repeat

def test_bitwise_consistency(kp, monkeypatch):
    sim, rs = handle(kp, STEP_KPM), rows(67)
    c = cfg(kp, FS.OBJ_W, FS.FLOOR_W, n_iters=6)
    monkeypatch.delenv("KP_ROWS_CHUNK", raising=False)
    full = scene(sim, rs, c)
    again = scene(sim, rs, c)
    for k in ALL:
        assert torch.equal(bits(full[k]), bits(again[k])), f"a second call: {k}"
    for e in (0, 41, 66):
        alone = scene(sim, rs[e:e + 1], c)
        for k in ALL:
            assert torch.equal(bits(full[k][e]), bits(alone[k][0])), f"row {e} of 67 against the row alone: {k}"
    monkeypatch.setenv("KP_ROWS_CHUNK", "64")
    chunked = scene(sim, rs, c)
    monkeypatch.delenv("KP_ROWS_CHUNK")
    for k in ALL:
        assert torch.equal(bits(full[k]), bits(chunked[k])), f"KP_ROWS_CHUNK = 64: {k}"
    assert bool((full["info"][:, 2] > 0).all()) and bool(torch.isfinite(full["qpos"]).all()) and bool((full["info"][:, 14] > 0).any())
    lead = sim.fit_scene(stack(rs[:6], "q0").view(2, 3, 76), *NONE, tgt_pos=stack(rs[:6], "tgt_pos").view(2, 3, 24, 3), obj_qpos=stack(rs[:6], "blk").view(2, 3, 35), cfg=c, want=ALL)
    assert lead["info"].shape == (2, 3, 16) and torch.equal(bits(lead["qpos"].view(6, 76)), bits(full["qpos"][:6]))


def test_geoms_stay_in_their_row_and_a_nan_row_is_refused(kp):
    sim, rs = handle(kp, STEP_KPM), rows(5)
    c = cfg(kp, FS.OBJ_W, FS.FLOOR_W, n_iters=6)
    clean = scene(sim, rs, c)
    # row 2 without objects between rows that carry some: it is fit_points' row, and its neighbours do not move
    blk = stack(rs, "blk")
    blk[2] = dev(FS.parked_block())
    mixed = scene(sim, rs, c, blk=blk)
    pts = sim.fit_points(stack(rs, "q0"), *NONE, tgt_pos=stack(rs, "tgt_pos"), cfg=pcfg(kp, FS.FLOOR_W, n_iters=6), want=ALL)
    for k in ("qpos", "dq"):
        assert torch.equal(bits(mixed[k][2]), bits(pts[k][2])), f"the row without objects: {k}"
        assert not torch.equal(bits(clean[k][2]), bits(pts[k][2])), "the objects of row 2 matter when they are there"
    assert torch.equal(bits(mixed["info"][2, SAME]), bits(pts["info"][2])) and not mixed["info"][2, 12:].any()
    # a NaN object pose: status 1, the input back, zeros in 8..14; the neighbours keep their bits
    for col in (1, 4):
        bad = stack(rs, "blk")
        bad[2, 7 * int(np.flatnonzero(np.abs(rs[2]["blk"][0::7]) < 50)[0]) + col] = float("nan")
        out = scene(sim, rs, c, blk=bad)
        for e in (0, 1, 3, 4):
            for k in ALL:
                assert torch.equal(bits(out[k][e]), bits(clean[k][e])), f"NaN in column {col}: row {e}, {k}"
        assert out["info"][2, 7] == 1 and out["info"][2, 2] == 0 and not out["info"][2, 8:].any() and not out["dq"][2].any()
        assert torch.equal(bits(out["qpos"][2]), bits(stack(rs, "q0")[2])), "the input comes back as given"


@pytest.mark.parametrize("scene_name", ["floor", "h_push"])
def test_the_control_step_is_bit_identical(kp, scene_name):
    rs = rows(67)

    def between(sim):
        objs = scene_name == "h_push"
        out = scene(sim, rs[:5], cfg(kp, FS.OBJ_W, FS.FLOOR_W, n_iters=4), obj=objs)
        assert torch.isfinite(out["qpos"]).all()
        stored = sim.fit_scene(sim.view("qpos"), *NONE, tgt_pos=sim.fk(sim.view("qpos"))["wbpos"].view(67, 24, 3), obj_qpos=stack(rs, "blk") if objs else None,
                               cfg=cfg(kp, 10.0, 10.0, n_iters=2))      # on the stored rows too
        assert not stored["info"][:, 7].any()
    H.control_step_untouched(kp, scene_name, between)


# ---------------------------------------------------------------- 3. one step against the dense solve

@pytest.mark.parametrize("w", [FS.PARITY_W, FS.OBJ_W])
@pytest.mark.parametrize("R", ROWS)
def test_one_step_against_the_dense_solve(kp, R, w):
    """On section 20's perturbed inits (fit_scene_oracle.step_rows says why): at w 1 under section 20's cap with the reference's discrete choices, at w 2400
    the normwise backward error in the reference's system.  The unperturbed rows -- a translation of 0.02 .. 0.03 m -- are printed beside them."""
    ref = reference(("step", w), dict(n_iters=1, mu0=1e-2, w_obj=w, w_floor=w), step_rows)
    out = scene(handle(kp, STEP_KPM), step_rows(R), cfg(kp, w, w, n_iters=1, mu0=1e-2))
    if w == FS.PARITY_W and R == 67:
        plain, pref = scene(handle(kp, STEP_KPM), rows(16), cfg(kp, w, w, n_iters=1, mu0=1e-2)), reference(("plain", w), dict(n_iters=1, mu0=1e-2, w_obj=w, w_floor=w))
        for e in range(16):
            d = plain["dq"][e].double().cpu().numpy()
            M.note("dq on the translation rows (reported)", np.abs(d - pref[e]["dq"]).max() / np.abs(pref[e]["dq"]).max())
            M.note("backward error on the translation rows (reported)", np.abs(pref[e]["A"] @ d - pref[e]["g"]).max() / (np.abs(pref[e]["A"]).sum(1).max() * np.abs(d).max() + np.abs(pref[e]["g"]).max()))
    dq, info = out["dq"].double().cpu().numpy(), out["info"].double().cpu().numpy()
    worst = {}
    for e in range(R):
        r = ref[e % 16]
        err = float(np.abs(dq[e] - r["dq"]).max() / np.abs(r["dq"]).max())
        eta = float(np.abs(r["A"] @ dq[e] - r["g"]).max() / (np.abs(r["A"]).sum(1).max() * np.abs(dq[e]).max() + np.abs(r["g"]).max()))
        c0, c1 = abs(info[e, 0] - r["info"][0]) / r["info"][0], abs(info[e, 1] - r["info"][1]) / r["info"][0]
        if e < 16:
            print(f"one step (w {w:g}), R = {R}, row {e} {step_rows(R)[e]['name']}: |dq - ref|/|ref| {err:.3e}, backward error {eta:.3e}, cond(A) 2^-23 {np.linalg.cond(r['A']) * 2.0 ** -23:.2e}, "
                  f"first cost {c0:.3e}, cost after {c1:.3e}, accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}, counted {info[e, 13]:.0f} / {r['info'][13]:.0f} in {info[e, 14]:.0f} / {r['info'][14]:.0f} pairs")
        assert info[e, 7] == 0
        if w == FS.OBJ_W:
            M.note("backward2400", eta, worst); M.note("cost02400", c0, worst); M.note("dq2400 (reported)", err)
        else:
            M.note("dq", err, worst); M.note("cost", max(c0, c1), worst)
            assert info[e, 2] == r["info"][2] and info[e, 13] == r["info"][13] and info[e, 14] == r["info"][14], f"row {e}: the discrete choices of the reference"
    if w == FS.OBJ_W:
        print(f"one step (w 2400), R = {R}: normwise backward error {worst['backward2400']:.3e} (tolerance {TOL['backward2400']:.3e}, cap {CAP['backward2400']:.3e}), first cost {worst['cost02400']:.3e}")
        assert worst["backward2400"] <= TOL["backward2400"] <= CAP["backward2400"] and worst["cost02400"] <= TOL["cost02400"]
    else:
        print(f"one step (w 1), R = {R}: worst dq {worst['dq']:.3e} (tolerance {TOL['dq']:.3e}, cap {CAP['dq']:.3e}), worst cost {worst['cost']:.3e} (tolerance {TOL['cost']:.3e})")
        assert worst["dq"] <= TOL["dq"] <= CAP["dq"] and worst["cost"] <= TOL["cost"]


# ---------------------------------------------------------------- 4. three iterations with the reference's discrete choices

@pytest.mark.parametrize("R", ROWS)
def test_three_iterations(kp, R):
    w = FS.COMPARE_W
    ref = reference("it3", dict(n_iters=FS.COMPARE_ITERS, w_obj=w, w_floor=w))
    out = scene(handle(kp, STEP_KPM), rows(R), cfg(kp, w, w, n_iters=FS.COMPARE_ITERS))
    q, info = out["qpos"].double().cpu().numpy(), out["info"].double().cpu().numpy()
    worst = {}
    for e in range(R):
        r = ref[e % 16]
        dc, dd, dqp = abs(info[e, 1] - r["info"][1]) / r["info"][0], abs(info[e, 12] - r["info"][12]), float(np.abs(q[e] - r["qpos"]).max())
        if e < 16:
            print(f"three iterations (w {w:g}), R = {R}, row {e} {rows(R)[e]['name']}: cost {dc:.3e}, depth {dd:.3e} m, qpos {dqp:.3e}, accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}, "
                  f"counted {info[e, 13]:.0f} / {r['info'][13]:.0f}, pairs {info[e, 14]:.0f} / {r['info'][14]:.0f}")
        M.note("it3_cost", dc, worst); M.note("it3_depth", dd, worst); M.note("it3_qpos", dqp, worst)
        assert info[e, 2] == r["info"][2] and info[e, 13] == r["info"][13] and info[e, 14] == r["info"][14] and info[e, 11] == r["info"][11] and info[e, 7] == 0, f"row {e}"
    print(f"three iterations, R = {R}: cost {worst['it3_cost']:.3e} (tolerance {TOL['it3_cost']:.3e}), depth {worst['it3_depth']:.3e} m ({TOL['it3_depth']:.3e}), qpos {worst['it3_qpos']:.3e} ({TOL['it3_qpos']:.3e})")
    assert worst["it3_cost"] <= TOL["it3_cost"] and worst["it3_depth"] <= TOL["it3_depth"] and worst["it3_qpos"] <= TOL["it3_qpos"]


# ---------------------------------------------------------------- 5. thirty iterations: the bound, and the contact walk

def test_thirty_iterations_on_the_bound_cases(kp):
    sim, cs = handle(kp, STEP_KPM), cases()
    names = list(cs)
    rs = [cs[n] for n in names]
    full = dict(n_iters=FS.OBJ_ITERS, w_obj=FS.OBJ_W, w_floor=FS.FLOOR_W)
    ref = memo("ref30", lambda: [FS.lm(oracle(), c["q0"], FS.problem(KPM, FS.scene_geoms(KPM, c["blk"]), tgt_pos=c["tgt_pos"]), full) for c in rs])
    on = scene(sim, rs, cfg(kp, FS.OBJ_W, FS.FLOOR_W, n_iters=FS.OBJ_ITERS))
    off = scene(sim, rs, cfg(kp, 0.0, FS.FLOOR_W, n_iters=FS.OBJ_ITERS))
    start = scene(sim, rs, cfg(kp, FS.OBJ_W, FS.FLOOR_W, n_iters=0))
    blk = stack(rs, "blk")
    pen_fit = sim.pose_contacts(on["qpos"].contiguous(), blk, pen_margin=FS.PEN_MARGIN)["pen"].cpu().numpy()
    pen_raw = sim.pose_contacts(stack(rs, "q0"), blk, pen_margin=FS.PEN_MARGIN)["pen"].cpu().numpy()
    info, io, i0 = on["info"].double().cpu().numpy(), off["info"].double().cpu().numpy(), start["info"].double().cpu().numpy()
    for e, name in enumerate(names):
        r, c = ref[e], rs[e]
        derived = r["info"][1] <= c["cand_cost"]
        print(f"{name}: cost {info[e, 0]:.4e} -> {info[e, 1]:.4e} (reference {r['info'][1]:.4e}, candidate {c['cand_cost']:.4e}), deepest counted vertex {i0[e, 12] * 1e3:.2f} -> {info[e, 12] * 1e3:.3f} mm "
              f"(reference {r['info'][12] * 1e3:.3f}), {info[e, 13]:.0f} counted in {info[e, 14]:.0f} pairs, accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}, without the term {io[e, 12] * 1e3:.2f} mm, "
              f"pose-contact walk pen {pen_raw[e]:.4f} -> {pen_fit[e]:.4f} m, {'bound derived' if derived else 'held to the reference'}")
        assert info[e, 7] == 0 and info[e, 1] < info[e, 0]
        assert io[e, 12] >= 0.029 and i0[e, 12] >= 0.029, f"{name}: without the term the push stays"
        if derived:
            M.note("it30_depth_derived", info[e, 12])
            assert info[e, 12] <= CAP["depth"], name
        else:
            M.note("it30_depth", abs(info[e, 12] - r["info"][12]))
            assert info[e, 12] <= r["info"][12] + TOL["it30_depth"], name
        if c["walk"]:
            assert pen_raw[e] > 0.0 and pen_fit[e] == 0.0, f"{name}: kp_sim_pose_contacts at pen_margin 3 mm"


# ---------------------------------------------------------------- 6. refusals

def test_refusals(kp, tmp_path):
    from kinpoly_amd.model_compiler import write_kpm
    m = read_kpm(DEFAULT_KPM)
    m["obj_geoms"] = np.zeros((0, 18), m["obj_geoms"].dtype)
    write_kpm(m, str(tmp_path / "no_objects.kpm"))
    sim, lean, rs = handle(kp, STEP_KPM), kp.KpSim(kp.KpModel(str(tmp_path / "no_objects.kpm")), 1), rows(5)
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    q0, tp, blk = stack(rs, "q0"), stack(rs, "tgt_pos"), stack(rs, "blk")
    bufs, fout = H.sentinel(kp.fit_scene_outputs(0), kp.KpFitPointsOut)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ms = kp.KpMarkerSet(0, None, None)
    fin = kp.KpFitPointsIn(P(q0), None, None, P(tp))
    ok, f, B = cfg(kp, 1.0), L.kp_sim_fit_scene, ctypes.byref
    assert f(None, 5, B(ms), B(fin), P(blk), B(ok), B(fout)) != 0 and "null handle" in err()
    assert f(sim.h, -1, B(ms), B(fin), P(blk), B(ok), B(fout)) != 0 and "n_rows" in err()
    assert f(sim.h, 5, None, B(fin), P(blk), B(ok), B(fout)) != 0 and "null markers" in err()
    assert f(sim.h, 5, B(ms), None, P(blk), B(ok), B(fout)) != 0 and "null in" in err()
    assert f(sim.h, 5, B(ms), B(fin), P(blk), None, B(fout)) != 0 and "null cfg" in err()
    assert f(sim.h, 5, B(ms), B(fin), P(blk), B(ok), None) != 0 and "null out" in err()
    assert f(sim.h, 5, B(ms), B(kp.KpFitPointsIn(P(q0))), P(blk), B(ok), B(fout)) != 0 and "nothing to fit" in err()
    for v in (-1.0, float("nan"), float("inf")):
        assert f(sim.h, 5, B(ms), B(fin), P(blk), B(cfg(kp, v)), B(fout)) != 0 and "w_obj" in err(), v
        assert f(sim.h, 5, B(ms), B(fin), P(blk), B(cfg(kp, 1.0, v)), B(fout)) != 0 and "w_floor" in err(), v
    assert f(sim.h, 5, B(ms), B(fin), P(blk), B(cfg(kp, 1.0, n_iters=-1)), B(fout)) != 0 and "n_iters" in err()
    assert f(lean.h, 5, B(ms), B(fin), P(blk), B(ok), B(fout)) != 0 and "no object geoms" in err()
    wide = kp.KpSim(kp.KpModel(STEP_KPM, threads_per_env=128), 5)
    assert f(wide.h, 5, B(ms), B(fin), P(blk), B(ok), B(fout)) != 0 and "threads_per_env" in err()
    assert f(sim.h, 0, B(ms), B(fin), P(blk), B(ok), B(fout)) == 0, "n_rows == 0 does nothing"
    H.refused_calls_wrote_nothing(bufs)
    for call in (lambda: sim.fit_scene(q0, *NONE, tgt_pos=tp, obj_qpos=blk[:4]), lambda: sim.fit_scene(q0, *NONE, tgt_pos=tp, obj_qpos=blk.cpu()),
                 lambda: sim.fit_scene(q0, *NONE, tgt_pos=tp, obj_qpos=blk.double()), lambda: sim.fit_scene(q0, *NONE, obj_qpos=blk),
                 lambda: sim.fit_scene(q0, *NONE, tgt_pos=tp, obj_qpos=blk, cfg=cfg(kp, -1.0))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(kp.KinPolyNativeError, match="no object geoms"):
        lean.fit_scene(q0, *NONE, tgt_pos=tp, obj_qpos=blk)
    torch.cuda.synchronize()                                             # no sticky HIP error: the next launch works
    assert torch.isfinite(scene(sim, rs, cfg(kp, 1.0, n_iters=1))["qpos"]).all()


def test_zz_measured_figures():
    """the figures this run measured, beside the tolerances (runs last in the file)"""
    for k in sorted(M):
        print(f"measured {k}: {M[k]:.3e}" + (f"  (tolerance {TOL[k]:.3e})" if k in TOL else ""))
