"""CPU: the edge takes of tests/take_edges.py.  The oracle's get_expert against what the reference itself computed on them (tests/golden/uhc_take_edges.npz,
tools/make_golden_take_edges.py), the builder's conditions, and the tolerance model the GPU test (tests/test_gpu_take_edges.py) holds both fp32 paths to."""
import math

import numpy as np
import pytest

import take_edges as E
from oracle import np_oracle as O


@pytest.fixture(scope="module")
def fx():
    g = E.load_fixture()
    rows, take_off = E.build()
    return g, rows, take_off, E.rows_for_reference(rows), E.take_slice(take_off), E.fixture_dts(g)


def _names(di):
    return E.NAMES if di == 0 else E.EDGE


def test_oracle_equals_the_reference_on_the_edge_takes(fx):
    """oracle.np_oracle.get_expert on rows_for_reference(rows) against the reference's get_expert, per take, per table and at both dt, at 1e-10 relative to
    max(1, |value|) (the bound of tests/test_oracle_golden.py): the unwrap loops, the clamp, the `angle > pi` branch, the w < 0 branch and the cut-off"""
    g, rows, take_off, ref, sl, dts = fx
    assert list(g["take_names"]) == list(E.NAMES) and np.array_equal(g["rows"], rows) and np.array_equal(g["take_off"], take_off)
    assert abs(dts[0] - 1 / 30) < 1e-9 and abs(dts[1] - 1.0) < 1e-8
    for di, dt in enumerate(dts):
        for name in _names(di):
            tab = E.oracle_tables(ref[sl[name]], dt)
            for t in E.DERIVED:
                want = g[E.fixture_key(di, name, t)]
                assert tab[t].shape == want.shape == (E.LENS[name], want.shape[1])
                err = float((np.abs(tab[t] - want) / np.maximum(1.0, np.abs(want))).max())
                assert err <= 1e-10, (dt, name, t, err)
            for t in ("height_lb", "head_height_lb"):
                assert abs(tab[t] - float(g[E.fixture_key(di, name, t)])) <= 1e-10, (dt, name, t)


def test_the_fixture_reaches_the_branches(fx):
    """what the takes are there for, read off the reference's own output"""
    g, rows, take_off, ref, sl, dts = fx
    jw = ref[sl["joint_wrap"]]
    raw = np.diff(jw[:, 7:], axis=0)
    assert (np.abs(raw) > 3 * math.pi).any() and ((np.abs(raw) > math.pi) & (np.abs(raw) < 3 * math.pi)).any()          # two turns of the unwrap, and one
    assert (raw > math.pi).any() and (raw < -math.pi).any()
    q30, q1 = g[E.fixture_key(0, "joint_wrap", "qvel")][:, 6:], g[E.fixture_key(1, "joint_wrap", "qvel")][:, 6:]
    assert np.abs(q1).max() <= math.pi and np.abs(q1).max() > math.pi - 0.06                                              # unwrapped into (-pi, pi], not clamped at 1 s
    assert (q30 == 10).any() and (q30 == -10).any() and ((np.abs(q30) > 7) & (np.abs(q30) < 10)).any()                   # clamp on (0.34 * 30) and off (0.25 * 30)
    for name in ("root_turns", "root_sign"):
        ang, w = E.pair_rotations(ref[sl[name]])
        full = np.where(w[:, 0] < 0, 2 * math.pi - ang[:, 0], ang[:, 0])
        turns = np.array(E.TURNS)
        want = turns if name == "root_turns" else 2 * math.pi - turns                                                     # every pair of root_sign has one flipped row
        np.testing.assert_allclose(full, want, rtol=0, atol=2e-6)
        rangv, broot = g[E.fixture_key(1, name, "qvel")][1:, 3:6], g[E.fixture_key(1, name, "bangvel")][1:, :3]
        np.testing.assert_allclose(np.linalg.norm(rangv, axis=1)[1:], np.where(turns > math.pi, 2 * math.pi - turns, turns)[1:], rtol=0, atol=2e-6)   # wrapped
        np.testing.assert_allclose(np.linalg.norm(broot, axis=1)[1:], full[1:], rtol=0, atol=2e-6)                        # bangvel keeps 2 acos(w)
        assert not rangv[0].any() and not broot[0].any()                                                                 # the 1e-4 rad pair: under the cut-off
        v30 = g[E.fixture_key(0, name, "qvel")][1:, :3]
        assert (np.abs(v30[0::2]) == 10).any() and np.abs(v30[1::2]).max() < 10 and np.abs(v30[1::2]).max() > 3          # 0.5 m a frame clamped, 0.2 m not
    st = E.fixture_key(0, "still", "")
    for t in E.FD:
        assert not g[st + t].any()
    ud = ref[sl["upside_down"]]
    assert abs(np.hypot(ud[0, 3], ud[0, 6]) - math.sin(0.1)) < 1e-6 and abs(np.hypot(ud[1, 3], ud[1, 6]) - math.sin(0.1)) < 1e-6
    assert abs(abs(O.get_heading(ud[2, 3:7]) - math.pi) - 5e-4) < 1e-6 and ud[2, 6] * ud[3, 6] < 0                        # pi - 5e-4, then -pi + 5e-4


def test_builder_conditions_and_placed_minima(fx):
    g, rows, take_off, ref, sl, dts = fx
    assert rows.dtype == np.float64 and rows.shape == (352, 76) and list(np.diff(take_off)) == [E.LENS[n] for n in E.NAMES]
    E.check_conditions(rows, take_off)
    E.check_minima(rows, take_off)
    r32 = rows.astype(np.float32)
    for name in ("len63", "len64", "len65", "len129"):
        T = E.LENS[name]
        z = r32[sl[name], 2]
        assert int(z.argmin()) == T - 1 == E.CATALOGUE[name]["min_root_row"] and E.CATALOGUE[name]["min_head_row"] == 0
        assert float(g[E.fixture_key(0, name, "height_lb")]) == float(z.min())         # the fp32 value, exactly
        hz = np.array([O.qpos_fk(x, *E.MODEL[:3])["wbpos"][13][2] for x in ref[sl[name]]])
        assert int(hz.argmin()) == 0 and abs(float(g[E.fixture_key(0, name, "head_height_lb")]) - hz[0]) < 1e-12
        assert np.diff(np.sort(z.astype(np.float64))).min() >= 1e-3 and np.diff(np.sort(hz)).min() >= 1e-3
        ang, _ = E.pair_rotations(ref[sl[name]])
        assert ang.min() >= 1e-3                                                       # every relative body rotation of the smooth takes
    assert {63, 64, 65, 129} == {E.LENS[n] for n in E.NAMES[5:]}
    # refused: a joint step of exactly pi; a turn inside the cut-off's band; a heading divisor under 0.05; a root turn of pi
    with pytest.raises(ValueError, match="odd multiple of pi"):
        E.assemble([E.broken_take()])
    std = rows[sl["still"]].copy()
    for angle, axis, msg in ((5e-4, [0.6, 0.0, 0.8], "cut-off"), (math.pi, [0.6, 0.0, 0.8], "within 0.01 rad of pi")):
        bad = std.copy()
        bad[1, 3:7] = O.quaternion_multiply(O.quaternion_about_axis(angle, axis), bad[0, 3:7])
        with pytest.raises(ValueError, match=msg):
            E.assemble([bad])
    bad = std.copy(); bad[:, 3:7] = O.quaternion_about_axis(math.pi - 0.05, [1.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="sqrt"):
        E.assemble([bad])


def test_tolerance_model(fx):
    """The bounds come from the oracle alone (take_edges' docstring).  Every bound is at most a tenth of the error of the nearest wrong branch; the oracle under a
    second seed of half-ulp perturbations stays inside the bounds around the fixture, so the reference itself satisfies the rule the fp32 paths are held to;
    a difference taken across a take boundary misses the first row's bounds by more than ten times."""
    g, rows, take_off, ref, sl, dts = fx
    for di, dt in enumerate(dts):
        names = _names(di)
        bnd, cap = E.bounds(dt, names), E.caps(dt, names)
        lo, hi = E.spreads(rows, take_off, names, dt, seed=2)
        for name in names:
            for t in E.DERIVED:
                want = g[E.fixture_key(di, name, t)]
                b, c = bnd[(name, t)], cap[(name, t)]
                exact = E.exact_zero(name, t, want)
                assert b.shape == c.shape == want.shape and (b[~exact] > 0).all() and np.isfinite(c[~exact]).all()
                ratio = float((b[~exact] / c[~exact]).max()) if (~exact).any() else 0.0
                print(f"dt {dt:.4f} {name} {t}: largest bound {float(np.where(exact, 0, b).max()):.3e}, largest bound / cap {ratio:.3f}, exact entries {int(exact.sum())} of {exact.size}")
                assert ratio <= 1.0, (dt, name, t, ratio)
                rot = exact if t == "bangvel" else exact & (np.arange(want.shape[1]) // 3 == 1) if t == "qvel" else np.zeros_like(exact)
                assert not lo[(name, t)][rot].any() and not hi[(name, t)][rot].any(), (dt, name, t)     # rows moved by half an ulp: the cut-off keeps the rotational zeros
                off = np.maximum(np.abs(lo[(name, t)] - want), np.abs(hi[(name, t)] - want))
                assert (off[~exact] <= b[~exact]).all(), (dt, name, t, float((off[~exact] / b[~exact]).max()))
    dt = dts[0]
    bnd = E.bounds(dt)
    for k in range(1, len(E.NAMES)):
        name, o0 = E.NAMES[k], int(take_off[k])
        across = O.get_qvel_fd_new(ref[o0 - 1].copy(), ref[o0].copy(), dt).clip(-10.0, 10.0)
        want = g[E.fixture_key(0, name, "qvel")][0]
        miss = np.abs(across - want)
        b = np.where(want == 0, 0.0, bnd[(name, "qvel")][0])
        assert ((miss > 10 * b) & (miss > 0)).sum() >= 3, (name, int(((miss > 10 * b) & (miss > 0)).sum()))
