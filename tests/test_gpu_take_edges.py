"""GPU: the take library's table kernels (kp_takes: k_take_tables, k_take_minima) and the torch path (uhc_env.get_expert_batch) on the edge takes of
tests/take_edges.py, each against what the reference itself computed (tests/golden/uhc_take_edges.npz) under absolute bounds that come from the reference
alone (take_edges.bounds; checked without a GPU by tests/test_take_edges_cpu.py), never against each other; the exact expectations; independence of
neighbours and order bit for bit; and k_uhc_assign / k_uhc_track at the ends of the short takes.  Every figure is printed before it is asserted
(`take_edges ...` lines; measured on an MI355X: profiles/take_edges/tolerances.log)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import take_edges as E  # noqa: E402

FK_TABLES = ("qpos", "wbpos", "wbquat", "bquat", "body_com", "head_pose", "ee_wpos")
FD_TABLES = ("qvel", "rlinv", "rangv", "rlinv_local", "bangvel")
PER_ROW = ("qpos", "qpos_fk", "wbpos", "wbquat", "bquat", "body_com", "com", "head_pose", "ee_wpos", "ee_pos", "rq_rmh", "qvel", "rlinv", "rangv", "rlinv_local", "bangvel")


def _np(t):
    return t.double().cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    from kinpoly_amd.sim import KpTakes
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv
    g = E.load_fixture()
    rows, take_off = E.build()
    assert np.array_equal(g["rows"], rows) and np.array_equal(g["take_off"], take_off)
    dts = E.fixture_dts(g)
    env = BatchedHumanoidEnv(2, 0)
    r32 = rows.astype(np.float32)
    n_edge = int(take_off[len(E.EDGE)])
    libs = [KpTakes(env.sim, r32, take_off, dts[0]), KpTakes(env.sim, r32[:n_edge], take_off[:len(E.EDGE) + 1], dts[1])]
    return dict(g=g, rows=rows, r32=r32, take_off=take_off, dts=dts, env=env, libs=libs, sl=E.take_slice(take_off))


def _want(g, di, name, table):
    q = g[E.fixture_key(di, name, "qvel")]
    return q[:, :3] if table == "rlinv" else q[:, 3:6] if table == "rangv" else g[E.fixture_key(di, name, table)]


def _sub(a, table):
    return a[:, :3] if table == "rlinv" else a[:, 3:6] if table == "rangv" else a


def test_tables_against_the_reference_fixture(ctx):
    """Per take, per table and at both dt (1 / 30 s: all nine takes; 1 s: the five edge takes): max |library - fixture| and max |get_expert_batch - fixture|,
    each against the per-entry bound of take_edges.bounds (8 x the reference's own spread under fp32 input rounding + an 8 ulp floor; every bound at most a
    tenth of the error of the nearest wrong branch, take_edges.caps).  Exact zeros of the fixture's finite differences are compared exactly.
    Measured on an MI355X: the worst error / bound over all entries is 0.43 (rq_rmh of len64, torch path; library 0.42 on len129), 0.37 on rangv
    (root_sign at 1 s, both paths); rangv is met to 6e-6 rad/s at 1 / 30 s; DESIGN.md section 9 has the table."""
    from kinpoly_amd.uhc_env import get_expert_batch
    g, env, dts = ctx["g"], ctx["env"], ctx["dts"]
    failures = []
    for di, dt in enumerate(dts):
        names = E.NAMES if di == 0 else E.EDGE
        bnd, cap = E.bounds(dt, names), E.caps(dt, names)
        lib = ctx["libs"][di]
        assert lib.K == len(names) and list(lib.lens) == [E.LENS[n] for n in names]
        for k, name in enumerate(names):
            tk = lib.take(k)
            ex = get_expert_batch(env.sim, torch.tensor(ctx["r32"][ctx["sl"][name]])[None], env.body_mass, dt)
            for t in FK_TABLES:
                assert torch.equal(tk[t], ex[t][0]), (dt, name, t)          # pure forward kinematics: copies of kp_sim_fk's outputs on both paths
            for t in ("rlinv", "rangv"):
                assert torch.equal(tk[t], _sub(tk["qvel"], t)) and torch.equal(ex[t][0], _sub(ex["qvel"][0], t)), (dt, name, t)
            for t in E.DERIVED + ("rlinv", "rangv"):
                want = _want(g, di, name, t)
                key = "qvel" if t in ("rlinv", "rangv") else t
                b, c = _sub(bnd[(name, key)], t), _sub(cap[(name, key)], t)
                exact = _sub(E.exact_zero(name, key, g[E.fixture_key(di, name, key)]), t)
                el, et = np.abs(_np(tk[t]) - want), np.abs(_np(ex[t][0]) - want)
                rl, rt = (float((e[~exact] / b[~exact]).max()) if (~exact).any() else 0.0 for e in (el, et))
                print(f"take_edges dt {dt:.4f} {name} {t}: library {el.max():.3e} torch {et.max():.3e} largest bound {float(np.where(exact, 0, b).max()):.3e} "
                      f"worst error / bound library {rl:.3f} torch {rt:.3f} smallest cap {float(np.where(exact, np.inf, c).min()):.3e} "
                      f"worst bound / cap {float(np.where(exact, 0, b / c).max()):.3f} exact zeros {int(exact.sum())} of {exact.size}")
                for path, e, r in (("library", el, rl), ("torch", et, rt)):
                    if r > 1.0 or e[exact].any():
                        failures.append((dt, name, t, path, f"{r:.3f}", float(e[exact].max()) if exact.any() else 0.0))
    assert not failures, failures


def test_exact_expectations(ctx):
    g, dts, sl = ctx["g"], ctx["dts"], ctx["sl"]
    for di, lib in enumerate(ctx["libs"]):
        names = E.NAMES if di == 0 else E.EDGE
        for k, name in enumerate(names):
            tk = lib.take(k)
            for t in FD_TABLES:                                              # frame 0 repeats frame 1's finite differences
                assert torch.equal(tk[t][0], tk[t][1]), (di, name, t)
            # the minima: of the fp32 input heights and of the library's own head heights, exactly
            z = torch.tensor(ctx["r32"][sl[name], 2], device=tk["qpos"].device)
            assert torch.equal(tk["qpos"][:, 2], z)
            assert torch.equal(tk["height_lb"], z.min()) and torch.equal(tk["head_height_lb"], tk["head_pose"][:, 2].min()), (di, name)
            assert float(tk["height_lb"]) == float(g[E.fixture_key(di, name, "height_lb")])                                   # the reference read the same fp32 value
            tol = 2 * float(E.bounds(dts[di], names)[(name, "ee_pos")][:, 12:15].max())          # the head's position error, bounded as ee_pos bounds it (|.| <= sqrt(3) max)
            assert abs(float(tk["head_height_lb"]) - float(g[E.fixture_key(di, name, "head_height_lb")])) <= tol, (di, name)
            if "min_root_row" in E.CATALOGUE[name]:
                assert int(tk["qpos"][:, 2].argmin()) == E.CATALOGUE[name]["min_root_row"] == E.LENS[name] - 1
                assert int(tk["head_pose"][:, 2].argmin()) == E.CATALOGUE[name]["min_head_row"] == 0
                top2 = torch.sort(tk["head_pose"][:, 2]).values[:2]
                assert float(top2[1] - top2[0]) > 5e-4                       # placed 1e-3 apart in fp64: fp32 FK cannot reorder them
        still = lib.take(E.NAMES.index("still"))
        for t in FD_TABLES:
            assert torch.equal(still[t], torch.zeros_like(still[t])), (di, t)
        for name in ("root_turns", "root_sign"):
            tk = lib.take(E.NAMES.index(name))
            p = E.CATALOGUE[name]["cutoff_pair"]                             # the 1e-4 rad pair: table row p + 1, and row 0 which repeats it
            for r in (0, p + 1):
                assert torch.equal(tk["rangv"][r], torch.zeros(3, device=tk["rangv"].device)), (di, name, r)
                assert torch.equal(tk["bangvel"][r, :3], torch.zeros(3, device=tk["rangv"].device)), (di, name, r)
            assert bool(tk["rangv"][p + 2].any()) and bool(tk["bangvel"][p + 2, :3].any())                                    # the 1e-3 rad pair is not cut off
        jw = lib.take(E.NAMES.index("joint_wrap"))["qvel"][:, 6:]
        want = torch.tensor(g[E.fixture_key(di, "joint_wrap", "qvel")][:, 6:], device=jw.device)
        clamped = want.abs() == 10
        assert bool(clamped.any()) == (di == 0)                               # at 1 s nothing reaches the clamp: the unwrap alone decides
        assert torch.equal(jw[clamped], want[clamped].float()), di            # exactly +-10 with the fixture's sign
        if di == 0:
            assert bool((want == 10).any()) and bool((want == -10).any()) and bool((~clamped & (want != 0)).any())


def test_no_dependence_on_neighbours_or_order(ctx):
    """the takes in reversed order, and each take alone (K = 1): every per-take table bit-identical to the first library's; the 2-, 3-, 6- and 10-row takes
    sit between each other and the 129-row take there"""
    from kinpoly_amd.sim import KpTakes
    env, r32, take_off, sl, dt = ctx["env"], ctx["r32"], ctx["take_off"], ctx["sl"], ctx["dts"][0]
    first = ctx["libs"][0]
    K = len(E.NAMES)
    rev_rows = np.concatenate([r32[sl[n]] for n in reversed(E.NAMES)], 0)
    rev_off = np.concatenate([[0], np.cumsum([E.LENS[n] for n in reversed(E.NAMES)])]).astype(np.int32)
    rev = KpTakes(env.sim, rev_rows, rev_off, dt)
    for k, name in enumerate(E.NAMES):
        a = first.take(k)
        alone = KpTakes(env.sim, np.ascontiguousarray(r32[sl[name]]), np.array([0, E.LENS[name]], np.int32), dt)
        for other, what in ((rev.take(K - 1 - k), "reversed"), (alone.take(0), "alone")):
            assert other["len"] == a["len"]
            for t in PER_ROW + ("height_lb", "head_height_lb"):
                assert torch.equal(a[t], other[t]), (name, what, t)


@pytest.mark.parametrize("obs_v", [0, 1])
def test_assign_and_track_at_the_ends_of_short_takes(ctx, obs_v):
    """reset onto `still` (2 rows) and `root_turns` (10 rows) at start = 0, len - 2 and len - 1: state and stored target are the library rows that
    min(start + t, len - 1) names (the target one row later for obs_v 1), after the reset and after one and two tracking steps; `end` follows
    start + t >= len + trail"""
    from kinpoly_amd.sim import KpTakes
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv
    trail = obs_v                                                            # 0 and 1: both sides of `len + trail`
    env = BatchedHumanoidEnv(6, 0, env_expert_trail_steps=trail)
    env.obs_v = obs_v                                                        # read by load_takes: which library row becomes the stored target
    env.term_body = "head"                                                   # never fails
    lib = KpTakes(env.sim, ctx["r32"], ctx["take_off"], ctx["dts"][0])
    env.load_takes(lib)
    ks = [E.NAMES.index("still"), E.NAMES.index("root_turns")]
    ids = np.array([ks[0], ks[0], ks[1], ks[1], ks[1], ks[0]], np.int32)
    lens = np.array([E.LENS[E.NAMES[k]] for k in ids])
    start = np.array([0, 1, 0, 8, 9, 0], np.int32)
    assert list(start[[1, 4]]) == list(lens[[1, 4]] - 1) and start[3] == lens[3] - 2
    env.reset(None, take_ids=ids, start=start)
    look = 0 if obs_v == 0 else 1

    def check(t):
        q, v = env.sim.get("qpos"), env.sim.get("qvel")
        for e in range(6):
            tk = lib.take(int(ids[e]))
            row, ro = min(start[e] + t, lens[e] - 1), min(start[e] + t + look, lens[e] - 1)
            if t == 0:
                assert torch.equal(q[e], tk["qpos"][row]) and torch.equal(v[e], tk["qvel"][row]), (t, e)
            assert torch.equal(env.sim.get("target_qpos")[e], tk["qpos_fk"][ro]), (t, e)
            assert torch.equal(env.sim.get("target_wbpos")[e], tk["wbpos"][ro]) and torch.equal(env.sim.get("target_wbquat")[e], tk["wbquat"][ro]), (t, e)
            assert torch.equal(env.sim.get("target_com")[e], tk["body_com"][ro]), (t, e)
            tb = env.sim.get("target_bquat")[e]
            assert torch.equal(tb[:4], tk["qpos_fk"][ro, 3:7]) and torch.equal(tb[4:], tk["bquat"][ro, 4:]), (t, e)
            assert torch.equal(env._base[e], tk["qpos_fk"][row]), (t, e)      # the next control step's base pose: the row itself

    check(0)
    a = torch.zeros((6, 75), device=env.device)
    for t in (1, 2):
        _, _, done, info = env.step(a)
        assert env.cur_t.tolist() == [t] * 6 and not bool(info["fail"].any())
        check(t)                                                              # t = 1 from start = len - 2 reads the last row; from there on it stays
        assert info["end"].tolist() == [bool(s + t >= n + trail) for s, n in zip(start, lens)], t
        np.testing.assert_array_equal(info["percent"].cpu().numpy(), (np.float32(t) / lens.astype(np.float32)).astype(np.float32))
