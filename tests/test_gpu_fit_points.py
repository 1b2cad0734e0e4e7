"""Pose fitting to points at body offsets with a floor term (kp_sim_fit_points) on a real MI355X: the kernel against the fp64
reference tests/fit_points_oracle.py on identical fp32 inputs, on the cases tests/test_fit_points_cpu.py has chosen; equivalence with kp_sim_fit_pose,
convergence, occlusion, the floor and its bound, edge rows, bitwise consistency, non-interference with the control step, markers to takes end to end and
the refusals.

Tolerances = 4 x the largest figure measured on the MI355X (the project's convention), each under the cap the feature's specification sets where it
sets one; every figure is printed before it is asserted."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fit_points_oracle as FT  # noqa: E402
import fit_pose_oracle as FP  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
KPM = read_kpm(DEFAULT_KPM)
ROWS = FT.ROWS
HAND = 18                 # the left hand: the end of the longest chain

# caps: a figure above these is a finding, whatever was measured.  dq: section 17's one-step figure (2.823e-05) x 10; conv_pos: the project's cap;
# floor_depth: the derived bound; e2e_rms: 2.5 x the injected noise
# backward2400: n u for the n = 75 unknowns of the solve in fp32 (u = 2^-24), the order of a backward-stable solve's normwise backward error
CAP = {"dq": 10 * 2.823e-05, "conv_pos": 1e-4, "floor_depth": FT.FLOOR_BOUND, "e2e_rms": 5e-3, "backward2400": 75 * 2.0 ** -24}
# 4 x the largest deviation measured on the MI355X (measured value in the comment)
TOL = {
    "dq": 4 * 2.091e-04,            # one LM step against the dense fp64 solve, relative inf-norm, worst of the six variants under the cap (k53_floor; the others 8.3e-06 .. 5.3e-05); measured 2.091e-04: the cap holds
    "cost": 4 * 1.776e-05,          # first cost and cost after the step against the reference's, relative to the row's first cost; measured 1.776e-05 (k53_floor; the others <= 3.7e-06)
    "backward2400": 4 * 1.284e-07,  # the w_floor = 2400 variant: |A dq - g|_inf / (|A|_inf |dq|_inf + |g|_inf) in the reference's system; measured 1.284e-07 (its dq is 3.4e-01 off at cond(A) 8e7)
    "equiv_qpos": 4 * 3.238e-05,    # fit_points on the body origins / fit_pose against the fp64 reference after 30 iterations, qpos; measured 3.238e-05 (the twist directions positions barely see)
    "equiv_cost0": 4 * 4.716e-07,   # the same, first cost, relative; measured 4.716e-07
    "equiv_cost1": 4 * 1.399e-13,         # the same, final cost, absolute (both sit at their rounding floor); measured 1.399e-13
    "equiv_epos": 4 * 2.376e-07,          # the same, final max position error against the reference's [m] (fit_points: info[8], fit_pose: info[4]); measured 2.376e-07
    "conv_pos": 4 * 3.282e-07,      # reachable cases: final max |e_k| [m]; measured 3.282e-07
    "conv_hinge": 4 * 5.960e-06,    # recovered hinge angles against the truth (mod 2 pi) [rad]; measured 5.960e-06
    "conv_root": 4 * 5.960e-08,     # recovered root position [m]; measured 5.960e-08
    "floor_cost": 4 * 7.272e-02,    # floor cases (w_floor 2400) after FLOOR_COMPARE_ITERS iterations: cost against the reference's, relative; measured 7.272e-02 (lying; 5e-03 on the other two): cond(A) 1e7 .. 1e8, see FLOOR_PARITY_W
    "floor4_cost": 4 * 6.180e-06,         # floor cases at FLOOR_COMPARE_W after FLOOR_COMPARE_ITERS iterations: cost against the reference's, relative; measured 6.180e-06
    "floor4_depth": 4 * 1.396e-07,        # the same, info[10] against the reference's [m]; measured 1.396e-07
    "floor4_qpos": 4 * 4.844e-05,         # the same, qpos against the reference's; measured 4.844e-05
    "floor_depth": 4 * 2.791e-04,   # the same, info[10] against the reference's [m]; measured 2.791e-04 (lying; 4e-06 and 2e-05 on the other two)
}
for _k, _c in CAP.items():
    if _k in TOL:
        TOL[_k] = min(TOL[_k], _c)


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def states():
    return memo("states", lambda: (ID.named_states(KPM, read_kpm(STEP_KPM), STD["qpos"], STD["qvel"]), ID.sweep_states(KPM, STD["qpos"])))


def oracle():
    return memo("oracle", lambda: FT.oracle(DEFAULT_KPM))


def truths():
    return memo("truths", lambda: FP.truth_poses(*states()))


def markers(which):
    """(body, offset) of a marker set of the tests"""
    def make():
        if which == "k1":
            return np.array([HAND], np.int32), FT.f32(np.array([[0.05, 0.02, -0.03]]))
        if which == "k24":
            return np.arange(24, dtype=np.int32), np.zeros((24, 3))
        return FT.marker_set(FT.counts_67(), FT.SEED_67) if which == "k67" else FT.marker_set(FT.counts_53(), FT.SEED_53)
    return memo(("markers", which), make)


def reachable(which="k53"):
    """the 67 reachable cases of a marker set, computed once and left unchanged"""
    return memo(("reachable", which), lambda: [FT.reachable_case(oracle(), q, 100 + i, *markers(which)) for i, q in enumerate(truths())])


def sunk():
    return memo("sunk", lambda: [FT.sunk_marker_case(oracle(), KPM, q, i, *markers("k53")) for i, q in enumerate(truths())])


def cfg(kp, w_floor=0.0, floor_z=0.0, **kw):
    c = kp.KpFitPointsCfg.default()
    c.w_floor, c.floor_z = w_floor, floor_z
    for k, v in kw.items():
        setattr(c.fit, k, v)
    return c


def stack(cases, key, R):
    return dev(np.stack([c[key] for c in cases[:R]]))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b, what, keys=None):
    for k in (a if keys is None else keys):
        assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k}"


ALL = ("qpos", "info", "dq", "pt_err")
M = H.Measured()


# ---------------------------------------------------------------- 1. one-step parity

# k53_floor: the floor at FLOOR_PARITY_W under the same cap as the others; k53_floor2400: the floor bound's weight, where cond(A) reaches 8e7 and the dq
# figure is held to the conditioning bound cond(A) 2^-23 of its row instead (fit_points_oracle.FLOOR_PARITY_W says why)
VARIANTS = ("k1", "k24", "k53", "k67", "k53_full", "k53_floor", "k53_floor2400")
FLOOR_W_OF = {"k53_floor": FT.FLOOR_PARITY_W, "k53_floor2400": FT.FLOOR_W}


def one_step_inputs(variant):
    """per row: dict(q0, pt_tgt, optional tgt_pos, tgt_quat, w_rot, q_prior, w_prior), the marker set and the floor weight"""
    which = variant.split("_")[0]
    cs = sunk() if variant in FLOOR_W_OF else reachable(which)
    rows = [dict(q0=c["q0"], pt_tgt=c["pt_tgt"]) for c in cs]
    if variant == "k53_full":
        fp = memo("fp_reach", lambda: [FP.reachable_case(oracle(), q, 100 + i) for i, q in enumerate(truths())])
        rng = np.random.default_rng(7)
        for r, c in zip(rows, fp):
            r.update(tgt_pos=c["tgt_pos"], tgt_quat=c["tgt_quat"], w_rot=c["w_rot"], q_prior=ID.f32(STD["qpos"][7:]), w_prior=ID.f32(rng.uniform(0.0, 0.1, 69)))
    return rows, markers(which), FLOOR_W_OF.get(variant, 0.0)


def one_step_reference(variant):
    """the fp64 loop's single iteration on all 67 rows of a variant: computed once, shared by the row counts"""
    def make():
        rows, (body, off), wf = one_step_inputs(variant)
        out = []
        for r in rows:
            pb = FT.problem(KPM, body, off, r["pt_tgt"], None, r.get("tgt_pos"), r.get("tgt_quat"), None, r.get("w_rot"), r.get("q_prior"), r.get("w_prior"))
            out.append(FT.lm(oracle(), r["q0"], pb, dict(n_iters=1, mu0=1e-2, w_floor=wf)))
        return out
    return memo(("one_step_ref", variant), make)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("R", ROWS)
def test_one_step_parity(kp, R, variant):
    rows, (body, off), wf = one_step_inputs(variant)
    ref = one_step_reference(variant)
    opt = {k: stack(rows, k, R) for k in ("tgt_pos", "tgt_quat", "w_rot", "q_prior", "w_prior") if k in rows[0]}
    out = handle(kp).fit_points(stack(rows, "q0", R), body, off, stack(rows, "pt_tgt", R), cfg=cfg(kp, wf, n_iters=1, mu0=1e-2), want=ALL, **opt)
    dq, info = out["dq"].double().cpu().numpy(), out["info"].double().cpu().numpy()
    worst = {}
    for e in range(R):
        r = ref[e]
        err = float(np.abs(dq[e] - r["dq"]).max() / np.abs(r["dq"]).max())
        bound = float(np.linalg.cond(r["A"])) * 2.0 ** -23
        c0, c1 = abs(info[e, 0] - r["info"][0]) / r["info"][0], abs(info[e, 1] - r["info"][1]) / r["info"][0]      # both on the row's own scale, its first cost
        print(f"one step ({variant}), R = {R}, row {e}: |dq - ref|/|ref| {err:.3e}, cond(A) 2^-23 {bound:.3e}, first cost {c0:.3e}, cost after {c1:.3e}, "
              f"accepted {info[e, 2]:.0f} / {r['info'][2]:.0f}, below the floor {info[e, 11]:.0f} / {r['info'][11]:.0f}")
        M.note(f"dq_{variant}", err, worst); M.note(f"cost_{variant}", max(c0, c1), worst)
        if variant == "k53_floor2400":      # held to the normwise backward error of the step in the reference's system, and to the first cost
            eta = float(np.abs(r["A"] @ dq[e] - r["g"]).max() / (np.abs(r["A"]).sum(1).max() * np.abs(dq[e]).max() + np.abs(r["g"]).max()))
            M.note("backward2400", eta, worst); M.note("cost02400", c0, worst)
        else:
            M.note("dq", err, worst); M.note("cost", max(c0, c1), worst)
        assert info[e, 2] == r["info"][2] and info[e, 7] == 0 and (variant != "k53_floor" or info[e, 11] == r["info"][11])
    if variant == "k53_floor2400":
        print(f"one step ({variant}), R = {R}: worst dq {worst['dq_' + variant]:.3e} and cost {worst['cost_' + variant]:.3e} (reported: cond(A) reaches 8e7), normwise backward error "
              f"{worst['backward2400']:.3e} (tolerance {TOL['backward2400']:.3e}, cap {CAP['backward2400']:.3e}), first cost {worst['cost02400']:.3e} (tolerance {TOL['cost']:.3e})")
        assert worst["backward2400"] <= TOL["backward2400"] and worst["cost02400"] <= TOL["cost"]
        return
    print(f"one step ({variant}), R = {R}: worst dq {worst['dq']:.3e} (tolerance {TOL['dq']:.3e}, cap {CAP['dq']:.3e}), worst cost {worst['cost']:.3e} (tolerance {TOL['cost']:.3e})")
    assert worst["dq"] <= TOL["dq"] and worst["cost"] <= TOL["cost"]
    assert np.allclose(info[:, 6], np.abs(dq).max(1), rtol=1e-6)


# ---------------------------------------------------------------- 2. equivalence with kp_sim_fit_pose

EQUIV_ITERS = FT.EQUIV_ITERS
EQUIV_GOLD = np.load(os.path.join(ROOT, "tests", "golden", "fit_points_equiv_ref.npz"))      # the fp64 loop's results; tests/test_fit_points_cpu.py recomputes them


@pytest.mark.parametrize("R", ROWS)
def test_body_origins_as_points_equal_fit_pose(kp, R):
    from kinpoly_amd.fit import MarkerSet
    cs, sim = reachable("k24"), handle(kp)
    ms = MarkerSet.body_origins()
    q0, tgt = stack(cs, "q0", R), stack(cs, "pt_tgt", R)
    a = sim.fit_points(q0, ms.body, ms.offset, tgt, cfg=cfg(kp, n_iters=EQUIV_ITERS))
    pc = kp.KpFitCfg.default(); pc.n_iters = EQUIV_ITERS
    b = sim.fit_pose(q0, tgt, cfg=pc)
    qa, qb, ia, ib = (t.double().cpu().numpy() for t in (a["qpos"], b["qpos"], a["info"], b["info"]))
    qr, ir = EQUIV_GOLD["qpos"][:R], EQUIV_GOLD["info"][:R]
    # what separates each of the two from the fp64 reference: qpos, first cost (relative), final cost and final max position error (absolute: both are at
    # their rounding floor).  fit_points measures the position error on its points (info[8]); without tgt_pos its info[4] is 0 by contract.
    ea, eb = ia[:, 8], ib[:, 4]
    sep = {"qpos": max(np.abs(qa - qr).max(), np.abs(qb - qr).max()), "cost0": max(np.abs(ia[:, 0] / ir[:, 0] - 1).max(), np.abs(ib[:, 0] / ir[:, 0] - 1).max()),
           "cost1": max(np.abs(ia[:, 1] - ir[:, 1]).max(), np.abs(ib[:, 1] - ir[:, 1]).max()), "epos": max(np.abs(ea - ir[:, 4]).max(), np.abs(eb - ir[:, 4]).max())}
    for k, v in sep.items():
        M.note(f"equiv_{k}", v)
    apart = {"qpos": np.abs(qa - qb).max(), "cost0": np.abs(ia[:, 0] / ib[:, 0] - 1).max(), "cost1": np.abs(ia[:, 1] - ib[:, 1]).max(), "epos": np.abs(ea - eb).max()}
    same_bits = all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in ((qa, qb), (ia[:, :4], ib[:, :4]), (ea, eb), (ia[:, 5:8], ib[:, 5:8])))
    print(f"body origins as points against fit_pose, R = {R}, {EQUIV_ITERS} iterations: from the fp64 reference / from each other: " +
          ", ".join(f"{k} {sep[k]:.3e} / {apart[k]:.3e} (tolerance {TOL['equiv_' + k]:.3e})" for k in sep) + f"; bit for bit: {same_bits} (reported, not required)")
    # Reported, not asserted (a departure): accepted steps, final mu and the last |dq|.  At convergence the cost sits at its rounding floor
    # (1e-14), where whether a trial is 'strictly smaller' is rounding noise; every flip moves the count by one, mu by a factor 8 / 0.3 and the last step with it.
    print(f"    accepted steps {ia[:, 2].min():.0f} .. {ia[:, 2].max():.0f} / {ib[:, 2].min():.0f} .. {ib[:, 2].max():.0f} (reference {ir[:, 2].min():.0f} .. {ir[:, 2].max():.0f}), differing on "
          f"{int((ia[:, 2] != ib[:, 2]).sum())} rows; final mu differing on {int((ia[:, 3] != ib[:, 3]).sum())} rows (largest ratio {np.max(np.maximum(ia[:, 3] / ib[:, 3], ib[:, 3] / ia[:, 3])):.1e}); "
          f"last |dq| {ia[:, 6].max():.2e} / {ib[:, 6].max():.2e}")
    assert np.all(ia[:, 7] == 0) and np.all(ib[:, 7] == 0), "status"
    assert np.all(ia[:, 5] == 0) and np.all(ib[:, 5] == 0) and np.all(ia[:, 4] == 0), "no orientation term on either side; without tgt_pos no origin term"
    for k in sep:
        assert sep[k] <= TOL["equiv_" + k], f"{k}: from the reference"
        assert apart[k] <= TOL["equiv_" + k], f"{k}: from each other"


# ---------------------------------------------------------------- 3. convergence on the reachable cases

@pytest.mark.parametrize("R", ROWS)
def test_convergence_on_reachable_cases(kp, R):
    cs = reachable()
    body, off = markers("k53")
    n = max(FT.reach_iters(i) for i in range(R))
    out = handle(kp).fit_points(stack(cs, "q0", R), body, off, stack(cs, "pt_tgt", R), cfg=cfg(kp, n_iters=n), want=("qpos", "info", "pt_err"))
    info, q = out["info"].double().cpu().numpy(), out["qpos"].double().cpu().numpy()
    qt = np.stack([c["q_true"] for c in cs[:R]])
    hinge = np.abs((q[:, 7:] - qt[:, 7:] + np.pi) % (2 * np.pi) - np.pi).max(1)
    root = np.abs(q[:, :3] - qt[:, :3]).max(1)
    M.note("conv_pos", info[:, 8].max()); M.note("conv_hinge", hinge.max()); M.note("conv_root", root.max())
    print(f"reachable cases (53 markers, no orientations), R = {R}, {n} iterations: max |e_k| {info[:, 8].max():.3e} m (tolerance {TOL['conv_pos']:.3e}, cap {CAP['conv_pos']:.0e}), "
          f"rms {info[:, 9].max():.3e} m, hinge angles {hinge.max():.3e} rad ({TOL['conv_hinge']:.3e}), root position {root.max():.3e} m ({TOL['conv_root']:.3e}); "
          f"accepted steps {info[:, 2].min():.0f} .. {info[:, 2].max():.0f}")
    assert np.all(info[:, 7] == 0)
    assert info[:, 8].max() <= TOL["conv_pos"], "no case is excluded"
    assert hinge.max() <= TOL["conv_hinge"] and root.max() <= TOL["conv_root"]
    pe = out["pt_err"].double().cpu().numpy()
    assert np.allclose(pe.max(1), info[:, 8], rtol=1e-6) and np.allclose(np.sqrt((pe ** 2).mean(1)), info[:, 9], rtol=1e-5), "info 8 / 9 are the max and the rms of pt_err"
    assert np.all(info[:, 4] == 0) and np.all(info[:, 5] == 0), "no origin term, no orientation term"


# ---------------------------------------------------------------- 4. occlusion

@pytest.mark.parametrize("R", ROWS)
def test_occluded_markers_equal_removed_markers(kp, R):
    sim, cs = handle(kp), reachable()
    body, off = markers("k53")
    gone = np.zeros(53, bool); gone[np.random.default_rng(4).permutation(53)[:18]] = True          # a third
    assert len(set(body[gone])) > 5 and gone[0]
    tgt = stack(cs, "pt_tgt", R)
    occl = tgt.clone(); occl[:, dev(gone, torch.bool)] = float("nan")
    w = torch.ones(R, 53, device="cuda"); w[:, dev(gone, torch.bool)] = 0.0
    w[:, np.flatnonzero(gone)[1]] = -3.0                                                          # w <= 0: skipped alike
    c = cfg(kp, n_iters=6)
    a = sim.fit_points(stack(cs, "q0", R), body, off, occl, w, cfg=c, want=ALL)
    b = sim.fit_points(stack(cs, "q0", R), body[~gone], off[~gone], tgt[:, dev(~gone, torch.bool)].contiguous(), cfg=c, want=ALL)
    same(a, b, "occluded against removed", ("qpos", "info", "dq"))
    assert not a["pt_err"][:, dev(gone, torch.bool)].any() and torch.equal(bits(a["pt_err"][:, dev(~gone, torch.bool)]), bits(b["pt_err"]))
    assert not a["info"][:, 7].any() and bool((a["info"][:, 8] > 0).all())


# ---------------------------------------------------------------- 5. the floor

def floor_cases():
    return memo("floor", lambda: {k: FT.floor_case(oracle(), KPM, q, fz) for k, (q, fz) in FT.floor_poses(states()[0]).items()})


def floor_reference(wf=FT.FLOOR_W):
    def make():
        return {k: FT.lm(oracle(), c["q0"], FT.problem(KPM, tgt_pos=c["tgt_pos"]), dict(n_iters=FT.FLOOR_COMPARE_ITERS, w_floor=wf, floor_z=c["floor_z"]))
                for k, c in floor_cases().items()}
    return memo(("floor_ref", wf), make)


@pytest.mark.parametrize("name", ["standing", "lying", "sit_z05"])
@pytest.mark.parametrize("R", ROWS)
def test_floor_bound_and_parity(kp, R, name):
    """Targets 0.03 m under a pose that stands on floor_z, w_pos 1, w_floor 2400 (K = 0, tgt_pos given): the deepest vertex ends within the derived
    3 mm; without the floor term it sits 0.03 m deep.  After FLOOR_COMPARE_ITERS iterations cost and depth are compared with the reference's: loosely at
    w_floor 2400, where the fp32 trajectory parts from the fp64 one, and with equal vertex counts at FLOOR_COMPARE_W (fit_points_oracle.FLOOR_COMPARE_ITERS)."""
    sim, c, ref = handle(kp), floor_cases()[name], floor_reference()[name]
    q0, tp = dev(np.tile(c["q0"], (R, 1))), dev(np.tile(c["tgt_pos"], (R, 1, 1)))
    on = sim.fit_points(q0, [], np.zeros((0, 3)), tgt_pos=tp, cfg=cfg(kp, FT.FLOOR_W, c["floor_z"], n_iters=FT.FLOOR_ITERS))["info"].double().cpu().numpy()
    free = sim.fit_points(q0, [], np.zeros((0, 3)), tgt_pos=tp, cfg=cfg(kp, 0.0, c["floor_z"], n_iters=FT.FLOOR_ITERS))["info"].double().cpu().numpy()
    print(f"floor ({name}, floor_z {c['floor_z']}), R = {R}, {FT.FLOOR_ITERS} iterations: cost {on[0, 0]:.4e} -> {on[0, 1]:.4e} (translate-up candidate {c['cand_cost']:.4e}), deepest vertex "
          f"{on[:, 10].max() * 1e3:.4f} mm, {on[0, 11]:.0f} below (bound {FT.FLOOR_BOUND * 1e3:.1f} mm); without the floor term {free[:, 10].min() * 1e3:.3f} mm, {free[0, 11]:.0f} below")
    assert np.all(on[:, 7] == 0) and np.all(on[:, 10] <= CAP["floor_depth"]) and np.all(on[:, 1] < c["cand_cost"])
    assert np.all(free[:, 10] >= 0.029) and np.all(free[:, 11] > 0), "info 10 / 11 are computed whether or not w_floor > 0"
    assert np.all(on == on[0]), "equal rows, equal results"
    few = sim.fit_points(q0, [], np.zeros((0, 3)), tgt_pos=tp, cfg=cfg(kp, FT.FLOOR_W, c["floor_z"], n_iters=FT.FLOOR_COMPARE_ITERS))["info"].double().cpu().numpy()
    rel, dd = abs(few[0, 1] - ref["info"][1]) / ref["info"][1], abs(few[0, 10] - ref["info"][10])
    M.note("floor_cost", rel); M.note("floor_depth", dd)
    print(f"floor ({name}), {FT.FLOOR_COMPARE_ITERS} iterations against the reference: cost {few[0, 1]:.6e} / {ref['info'][1]:.6e}, relative {rel:.3e} (tolerance {TOL['floor_cost']:.3e}); "
          f"deepest vertex {few[0, 10]:.6e} / {ref['info'][10]:.6e} m, apart {dd:.3e} ({TOL['floor_depth']:.3e}); below {few[0, 11]:.0f} / {ref['info'][11]:.0f}, accepted {few[0, 2]:.0f} / {ref['info'][2]:.0f}")
    assert few[0, 2] == ref["info"][2]
    assert rel <= TOL["floor_cost"] and dd <= TOL["floor_depth"]
    # the same comparison where the device can follow the reference (FLOOR_COMPARE_W): equal active sets, so the counts are asserted too
    ref4 = floor_reference(FT.FLOOR_COMPARE_W)[name]
    f4 = sim.fit_points(q0, [], np.zeros((0, 3)), tgt_pos=tp, cfg=cfg(kp, FT.FLOOR_COMPARE_W, c["floor_z"], n_iters=FT.FLOOR_COMPARE_ITERS), want=("qpos", "info"))
    i4, q4 = f4["info"].double().cpu().numpy(), f4["qpos"].double().cpu().numpy()
    rel4, dd4, dq4 = abs(i4[0, 1] - ref4["info"][1]) / ref4["info"][1], abs(i4[0, 10] - ref4["info"][10]), np.abs(q4[0] - ref4["qpos"]).max()
    M.note("floor4_cost", rel4); M.note("floor4_depth", dd4); M.note("floor4_qpos", dq4)
    print(f"floor ({name}), w_floor {FT.FLOOR_COMPARE_W}, {FT.FLOOR_COMPARE_ITERS} iterations against the reference: cost {i4[0, 1]:.6e} / {ref4['info'][1]:.6e}, relative {rel4:.3e} "
          f"(tolerance {TOL['floor4_cost']:.3e}); deepest vertex {i4[0, 10]:.6e} / {ref4['info'][10]:.6e} m, apart {dd4:.3e} ({TOL['floor4_depth']:.3e}); qpos apart {dq4:.3e} "
          f"({TOL['floor4_qpos']:.3e}); below {i4[0, 11]:.0f} / {ref4['info'][11]:.0f}, accepted {i4[0, 2]:.0f} / {ref4['info'][2]:.0f}")
    assert i4[0, 2] == ref4["info"][2] and i4[0, 11] == ref4["info"][11] and ref4["info"][11] > 0, "accepted steps and the number of vertices below the floor"
    assert rel4 <= TOL["floor4_cost"] and dd4 <= TOL["floor4_depth"] and dq4 <= TOL["floor4_qpos"]


def test_floor_off_the_ground_changes_no_bit(kp):
    """every hull vertex above floor_z at every pose the loop sees: w_floor = 2400 and w_floor = 0 give the same bits"""
    sim, cs = handle(kp), reachable()
    body, off = markers("k53")
    q0, tgt = stack(cs, "q0", 67).clone(), stack(cs, "pt_tgt", 67).clone()
    q0[:, 2] += 1.5; tgt[..., 2] += 1.5
    a = sim.fit_points(q0, body, off, tgt, cfg=cfg(kp, FT.FLOOR_W, n_iters=6), want=ALL)
    b = sim.fit_points(q0, body, off, tgt, cfg=cfg(kp, 0.0, n_iters=6), want=ALL)
    same(a, b, "floor on against floor off, in the air")
    assert not a["info"][:, 10].any() and not a["info"][:, 11].any() and bool((a["info"][:, 2] > 0).all())
    low = sim.fit_points(q0, body, off, tgt, cfg=cfg(kp, 0.0, 5.0, n_iters=0))["info"]
    assert bool((low[:, 11] == 1199).all()) and bool((low[:, 10] > 1.0).all()), "under a floor at 5 m every vertex of the blob is below it"


# ---------------------------------------------------------------- 6. edge rows

def test_edge_rows(kp):
    sim, cs = handle(kp), reachable()
    body, off = markers("k53")
    q0, tgt, w = stack(cs, "q0", 5), stack(cs, "pt_tgt", 5), torch.ones(5, 53, device="cuda")
    c6 = cfg(kp, n_iters=6)
    ref = sim.fit_points(q0, body, off, tgt, w, cfg=c6, want=ALL)
    keep = [0, 1, 3, 4]
    for where in ("qpos0", "pt_w", "pt_tgt"):
        b = dict(qpos0=q0.clone(), pt_w=w.clone(), pt_tgt=tgt.clone())
        b[where][2].view(-1)[9] = float("inf") if where == "pt_tgt" else float("nan")
        out = sim.fit_points(b["qpos0"], body, off, b["pt_tgt"], b["pt_w"], cfg=c6, want=ALL)
        assert out["info"][2, 7] == 1 and torch.equal(bits(out["qpos"][2]), bits(b["qpos0"][2])), f"{where}: status 1, the input comes back"
        assert not out["info"][2, 8:].any() and not out["pt_err"][2].any() and out["info"][2, 2] == 0
        for k in ALL:
            assert torch.equal(bits(out[k][keep]), bits(ref[k][keep])), f"{where}: the neighbours' bits do not move ({k})"
    # an Inf target under weight zero is an occluded marker, not an error
    b = tgt.clone(); b[2, 3] = float("inf"); wz = w.clone(); wz[2, 3] = 0.0
    assert not sim.fit_points(q0, body, off, b, wz, cfg=c6)["info"][:, 7].any()
    # K = 0 with tgt_pos is fit_pose's problem
    fp = memo("fp_reach", lambda: [FP.reachable_case(oracle(), q, 100 + i) for i, q in enumerate(truths())])
    tp, tq = stack(fp, "tgt_pos", 5), stack(fp, "tgt_quat", 5)
    k0 = sim.fit_points(q0, [], np.zeros((0, 3)), tgt_pos=tp, tgt_quat=tq, w_rot=torch.ones(5, 24, device="cuda"), cfg=cfg(kp, n_iters=FP.GPU_CONVERGENCE_ITERS), want=ALL)
    assert k0["pt_err"].shape == (5, 0) and not k0["info"][:, 7].any() and not k0["info"][:, 8:10].any()
    assert float(k0["info"][:, 4].max()) <= 1e-5 and float(k0["info"][:, 5].max()) <= 1e-5
    # n_iters = 0: the input with its quaternion normalised, both costs filled, the figures of the input pose
    nq = q0.clone(); nq[:, 3:7] *= 1.7
    z = sim.fit_points(nq, body, off, tgt, cfg=cfg(kp, n_iters=0), want=ALL)
    assert torch.equal(bits(z["qpos"][:, :3]), bits(nq[:, :3])) and torch.equal(bits(z["qpos"][:, 7:]), bits(nq[:, 7:]))
    assert float((z["qpos"][:, 3:7].norm(dim=1) - 1.0).abs().max()) < 1e-6, "a quaternion of non-unit length is normalised"
    assert torch.equal(z["info"][:, 0], z["info"][:, 1]) and bool((z["info"][:, 0] > 0).all()) and not z["info"][:, 2].any() and not z["dq"].any()
    assert torch.allclose(z["info"][:, 0], ref["info"][:, 0], rtol=1e-5) and bool((z["info"][:, 8] > 1e-3).all())
    # the fit from the non-unit quaternion converges like the one from its normalised form
    u = sim.fit_points(nq, body, off, tgt, cfg=cfg(kp, n_iters=FT.REACH_ITERS))
    assert float(u["info"][:, 8].max()) <= TOL["conv_pos"] and not u["info"][:, 7].any()
    # all weights zero: the input comes back, status 0, nothing counted
    nw = sim.fit_points(q0, body, off, tgt, torch.zeros(5, 53, device="cuda"), cfg=cfg(kp, n_iters=3), want=ALL)
    base = sim.fit_points(q0, body, off, tgt, cfg=cfg(kp, n_iters=0))
    assert torch.equal(bits(nw["qpos"]), bits(base["qpos"])) and not nw["info"][:, 7].any() and not nw["info"][:, :3].any() and not nw["dq"].any()
    assert not nw["info"][:, 8:10].any() and not nw["pt_err"].any()


# ---------------------------------------------------------------- 7. bitwise checks

def test_bitwise_consistency(kp, monkeypatch):
    sim, cs = handle(kp), sunk()
    body, off = markers("k53")
    q0, tgt = stack(cs, "q0", 67), stack(cs, "pt_tgt", 67)
    c = cfg(kp, FT.FLOOR_W, n_iters=6)
    monkeypatch.delenv("KP_ROWS_CHUNK", raising=False)
    full = sim.fit_points(q0, body, off, tgt, cfg=c, want=ALL)
    same(full, sim.fit_points(q0, body, off, tgt, cfg=c, want=ALL), "a second call")
    for e in (0, 41, 66):
        alone = sim.fit_points(q0[e:e + 1], body, off, tgt[e:e + 1], cfg=c, want=ALL)
        for k in ALL:
            assert torch.equal(bits(full[k][e]), bits(alone[k][0])), f"row {e} of 67 against the row alone: {k}"
    for k in ALL:
        one = sim.fit_points(q0, body, off, tgt, cfg=c, want=(k,))
        assert tuple(one) == (k,) and torch.equal(bits(one[k]), bits(full[k])), f"outputs one at a time: {k}"
    lead = sim.fit_points(q0[:6].view(2, 3, 76), body, off, tgt[:6].view(2, 3, 53, 3), cfg=c, want=ALL)
    assert lead["pt_err"].shape == (2, 3, 53) and lead["info"].shape == (2, 3, 12) and torch.equal(bits(lead["qpos"].view(6, 76)), bits(full["qpos"][:6]))
    # the marker set in another order with pt_w = ones against NULL: a stable sort keeps every body's points in the caller's order, so permute whole bodies
    order = np.concatenate([np.flatnonzero(body == b) for b in np.random.default_rng(5).permutation(24)])
    assert not np.array_equal(order, np.arange(53))
    perm = sim.fit_points(q0, body[order], off[order], tgt[:, dev(order, torch.long)].contiguous(), torch.ones(67, 53, device="cuda"), cfg=c, want=ALL)
    same(full, perm, "bodies permuted, explicit unit weights", ("qpos", "info", "dq"))
    assert torch.equal(bits(perm["pt_err"]), bits(full["pt_err"][:, dev(order, torch.long)])), "pt_err comes back in the caller's order"
    # two launches (row0 = 64, a last chunk of three) against one
    monkeypatch.setenv("KP_ROWS_CHUNK", "64")
    same(full, sim.fit_points(q0, body, off, tgt, cfg=c, want=ALL), "KP_ROWS_CHUNK = 64")
    monkeypatch.delenv("KP_ROWS_CHUNK")
    assert bool((full["info"][:, 11] > 0).any()) and bool(torch.isfinite(full["qpos"]).all())


# ---------------------------------------------------------------- 8. nothing else moves

@pytest.mark.parametrize("scene", ["floor", "h_push"])
def test_the_control_step_is_bit_identical(kp, scene):
    cs = sunk()
    body, off = markers("k53")
    q0, tgt = stack(cs, "q0", 5), stack(cs, "pt_tgt", 5)

    def between(sim):
        out = sim.fit_points(q0, body, off, tgt, cfg=cfg(kp, FT.FLOOR_W, n_iters=4), want=ALL)
        assert torch.isfinite(out["qpos"]).all()
        stored = sim.fit_points(sim.view("qpos"), [], np.zeros((0, 3)), tgt_pos=sim.fk(sim.view("qpos"))["wbpos"].view(67, 24, 3), cfg=cfg(kp, 10.0, n_iters=2))      # on the stored rows too
        assert not stored["info"][:, 7].any()
    H.control_step_untouched(kp, scene, between, floor=states()[0])


# ---------------------------------------------------------------- 9. end to end

def test_markers_to_takes_end_to_end(kp, tmp_path):
    """A short seeded motion; marker tracks by the oracle's FK; 2 mm of noise, 5 % of the markers dropped; the chained fit; the markers of the fitted
    motion through kp_sim_fk against the CLEAN tracks: rms within 5 mm = 2.5 x the injected noise (53 markers average the noise down and the smoothing
    can only help).  The pickle scripts/fit_takes.py --markers writes loads through AmassSingleDataset."""
    import joblib
    from kinpoly_amd import dataset, fit
    sim = handle(kp)
    body, off = markers("k53")
    ms = fit.MarkerSet([f"m{k}" for k in range(53)], body, off)
    takes = dataset.synthetic_takes(sim, STD["qpos"], n_per_action=1, T_range=(40, 41), with_objects=False)
    names = sorted(takes)[:2]
    clean = np.stack([np.stack([FT.marker_positions(oracle(), q, body, off) for q in np.asarray(takes[k]["qpos"], np.float64)]) for k in names])      # [B, 40, 53, 3]
    rng = np.random.default_rng(9)
    noisy = clean + rng.normal(size=clean.shape) * 0.002
    drop = rng.uniform(size=clean.shape[:3]) < 0.05
    noisy[drop] = np.nan
    out = fit.fit_sequence_points(sim, ms, dev(noisy), mode="chained", smooth=1e-2, config=fit.FitConfig(n_iters=30))
    assert not out["info"][..., 7].any() and not out["pt_err"][dev(drop, torch.bool)].any()
    B, T = clean.shape[:2]
    fk = sim.fk(out["qpos"].reshape(B * T, 76).contiguous())
    xp, xq = fk["wbpos"].view(-1, 24, 3).double().cpu().numpy(), fk["wbquat"].view(-1, 24, 4).double().cpu().numpy()
    got = np.stack([FT.world_points(xp[i], xq[i], body.astype(int), off) for i in range(B * T)]).reshape(clean.shape)
    rms = float(np.sqrt(((got - clean) ** 2).sum(-1).mean()))
    print(f"chained marker fit of {B} takes x {T} frames, 2 mm noise, {drop.mean() * 100:.1f} % dropped: marker rms against the clean tracks {rms * 1e3:.3f} mm (cap {CAP['e2e_rms'] * 1e3:.0f} mm), "
          f"against the noisy ones (info 9) {float(out['info'][..., 9].mean()) * 1e3:.3f} mm")
    assert rms <= CAP["e2e_rms"]
    spec = importlib.util.spec_from_file_location("fit_takes", os.path.join(ROOT, "scripts", "fit_takes.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    ms.save(tmp_path / "set.json")
    joblib.dump({k: {"markers": noisy[b]} for b, k in enumerate(names)}, tmp_path / "in.pkl")
    _, rep = mod.main(["--tracks", str(tmp_path / "in.pkl"), "--out", str(tmp_path / "takes.pkl"), "--markers", str(tmp_path / "set.json"), "--floor", "100"], sim=sim)
    ds = dataset.AmassSingleDataset({"file_path": str(tmp_path / "takes.pkl"), "t_min": 30}, "train")
    assert ds.data_keys == names and list(ds.lens) == [40, 40]
    assert all(r["failed_rows"] == 0 and "max_penetration" in r and "per_marker" in r for r in rep.values())


# ---------------------------------------------------------------- 10. refusals

def test_refusals(kp):
    from kinpoly_amd import fit
    sim, cs = handle(kp), reachable()
    L, err = sim.L, lambda: sim.L.kp_last_error().decode()      # noqa: E731
    body, off = markers("k53")
    off = np.ascontiguousarray(off, np.float32)
    q0, tgt = stack(cs, "q0", 5), stack(cs, "pt_tgt", 5)
    table = kp.fit_points_outputs(53)
    bufs, fout = H.sentinel(table, kp.KpFitPointsOut)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    HP = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    ms = kp.KpMarkerSet(53, HP(body), HP(off))
    fin = kp.KpFitPointsIn(P(q0), P(tgt))
    ok, f, B = cfg(kp), L.kp_sim_fit_points, ctypes.byref
    assert f(None, 5, B(ms), B(fin), B(ok), B(fout)) != 0 and "null handle" in err()
    assert f(sim.h, -1, B(ms), B(fin), B(ok), B(fout)) != 0 and "n_rows" in err()
    assert f(sim.h, 5, None, B(fin), B(ok), B(fout)) != 0 and "null markers" in err()
    assert f(sim.h, 5, B(ms), None, B(ok), B(fout)) != 0 and "null in" in err()
    assert f(sim.h, 5, B(ms), B(fin), None, B(fout)) != 0 and "null cfg" in err()
    assert f(sim.h, 5, B(ms), B(fin), B(ok), None) != 0 and "null out" in err()
    for K in (-1, 1025):
        assert f(sim.h, 5, B(kp.KpMarkerSet(K, HP(body), HP(off))), B(fin), B(ok), B(fout)) != 0 and "n_points" in err()
    assert f(sim.h, 5, B(kp.KpMarkerSet(53, None, HP(off))), B(fin), B(ok), B(fout)) != 0 and "null pt_body" in err()
    assert f(sim.h, 5, B(kp.KpMarkerSet(53, HP(body), None)), B(fin), B(ok), B(fout)) != 0 and "null pt_offset" in err()
    for v in (24, -1):
        bad = body.copy(); bad[17] = v
        assert f(sim.h, 5, B(kp.KpMarkerSet(53, HP(bad), HP(off))), B(fin), B(ok), B(fout)) != 0 and "pt_body[17]" in err()
    for v in (np.nan, np.inf):
        bad = off.copy(); bad[30, 1] = v
        assert f(sim.h, 5, B(kp.KpMarkerSet(53, HP(body), HP(bad))), B(fin), B(ok), B(fout)) != 0 and "pt_offset[30]" in err()
    assert f(sim.h, 5, B(ms), B(kp.KpFitPointsIn(None, P(tgt))), B(ok), B(fout)) != 0 and "qpos0" in err()
    assert f(sim.h, 5, B(ms), B(kp.KpFitPointsIn(P(q0), None)), B(ok), B(fout)) != 0 and "pt_tgt" in err()
    assert f(sim.h, 5, B(kp.KpMarkerSet(0, None, None)), B(kp.KpFitPointsIn(P(q0), None)), B(ok), B(fout)) != 0 and "nothing to fit" in err()
    assert f(sim.h, 5, B(ms), B(kp.KpFitPointsIn(P(q0), P(tgt), None, None, None, None, None, P(q0), None)), B(ok), B(fout)) != 0 and "go together" in err()
    assert f(sim.h, 5, B(ms), B(fin), B(ok), B(kp.KpFitPointsOut(None, P(bufs["info"]), None, None))) != 0 and "out qpos" in err()
    assert f(sim.h, 5, B(ms), B(fin), B(ok), B(kp.KpFitPointsOut(P(bufs["qpos"]), None, None, None))) != 0 and "out info" in err()
    for k, v in (("n_iters", -1), ("mu0", 0.0), ("mu_min", -1.0), ("mu_max", float("nan")), ("mu_up", 0.0), ("mu_down", -0.5)):
        assert f(sim.h, 5, B(ms), B(fin), B(cfg(kp, **{k: v})), B(fout)) != 0 and k in err(), k
    bad = cfg(kp); bad.fit.damp[40] = 0.0
    assert f(sim.h, 5, B(ms), B(fin), B(bad), B(fout)) != 0 and "damp[40]" in err()
    for v in (-1.0, float("nan"), float("inf")):
        assert f(sim.h, 5, B(ms), B(fin), B(cfg(kp, w_floor=v)), B(fout)) != 0 and "w_floor" in err(), v
    for v in (float("nan"), float("-inf")):
        assert f(sim.h, 5, B(ms), B(fin), B(cfg(kp, floor_z=v)), B(fout)) != 0 and "floor_z" in err(), v
    wide = kp.KpSim(kp.KpModel(threads_per_env=128), 5)
    assert f(wide.h, 5, B(ms), B(fin), B(ok), B(fout)) != 0 and "threads_per_env" in err()
    assert f(sim.h, 0, B(ms), B(fin), B(ok), B(fout)) == 0, "n_rows == 0 does nothing"
    H.refused_calls_wrote_nothing(bufs)
    # the Python layer: wrong shapes, host tensors, the configuration
    for call in (lambda: sim.fit_points(q0[:, :75], body, off, tgt), lambda: sim.fit_points(q0, body, off, tgt[:4]), lambda: sim.fit_points(q0, body, off, tgt[:, :52]),
                 lambda: sim.fit_points(q0, body, off, tgt, torch.ones(5, 52, device="cuda")), lambda: sim.fit_points(q0.cpu(), body, off, tgt),
                 lambda: sim.fit_points(q0, body, off, tgt.cpu()), lambda: sim.fit_points(q0.double(), body, off, tgt), lambda: sim.fit_points(q0, body, off),
                 lambda: sim.fit_points(q0, [], np.zeros((0, 3))), lambda: sim.fit_points(q0, body, off, tgt, want=("nope",)),
                 lambda: fit.fit_points(sim, fit.MarkerSet.body_origins(), tgt), lambda: fit.fit_points(sim, fit.MarkerSet.body_origins(), tgt[:, :24], config=fit.FitConfig(w_floor=-1.0))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(kp.KinPolyNativeError, match="damp"):
        sim.fit_points(q0, body, off, tgt, cfg=bad)
    torch.cuda.synchronize()                                             # no sticky HIP error: the next launch works
    assert torch.isfinite(sim.fit_points(q0, body, off, tgt, cfg=cfg(kp, n_iters=1))["qpos"]).all()


def test_zz_measured_figures():
    """the figures this run measured, beside the tolerances (runs last in the file)"""
    for k in sorted(M):
        print(f"measured {k}: {M[k]:.3e}" + (f"  (tolerance {TOL[k]:.3e})" if k in TOL else ""))
