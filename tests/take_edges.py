"""The edge takes of the take-library tests (tests/test_take_edges_cpu.py, tests/test_gpu_take_edges.py, tools/make_golden_take_edges.py): nine takes
built in fp64 from a fixed seed, the conditions that keep them off the reference's discontinuities, and the tolerance model.

Both fp32 paths (kp_takes and uhc_env.get_expert_batch) read float32(rows); both fp64 references (the reference's get_expert behind
tests/golden/uhc_take_edges.npz and oracle.np_oracle.get_expert) read rows_for_reference(rows): the same fp32 values with the root quaternion renormalised
in fp64.  The reference takes the rotation angle from acos(w) and sqrt(1 - w^2), which amplify the 6e-8 by which an fp32 quaternion misses unit norm; the
fp32 paths take it from atan2(|xyz|, w), which does not care about the scale.

The takes (NAMES, in library order; CATALOGUE holds what the tests need to know about each):
  still        2 rows, identical: every finite-difference table is exactly 0.
  joint_wrap   3 rows: joints uniform in +-3.1, then plus STEPS (cycled over the 69 joints), then minus them again.  One and two turns of the unwrap in both
               directions, the clamp on (0.34 * 30 > 10) and off (0.25 * 30 < 10), joint quaternions of bangvel that change sign where an angle crosses pi.
  root_turns   10 rows: pair i turns the root by TURNS[i] about an axis of its own, none aligned with a coordinate axis, while the root translates by 0.5 m
               (clamped at 1 / 30 s) on even pairs and 0.2 m (6 m/s, not clamped) on odd ones; rlinv_local tells the frame of the row the difference ends on
               from the frame of the row it starts on.
  root_sign    the same turns (other axes), the stored root quaternion multiplied by -1 on every second row: w of the relative quaternion is negative, and
               bangvel keeps the reference's unwrapped angle 2 pi - turn.
  upside_down  6 rows: two with a roll of pi - 0.2 about x (sqrt(w^2 + z^2) = 0.1, the divisor of rq_rmh), then headings of pi - 5e-4 and -pi + 5e-4, then
               two plain rows.
  len63, len64, len65, len129   smooth motion around the 64-lane stride of k_take_minima; the lowest root height at the last row (index 62, 63 = last lane
               of the first stride, 64 = lane 0 of the second, 128), the lowest head height at row 0, all heights of a take at least 1e-3 apart.

Conditions (check_conditions; build() refuses takes that break them).  Each is a discontinuity of the reference, so no fp32 code can be held to it:
  no joint difference within 0.02 rad of an odd multiple of pi; no root turn within 0.01 rad of pi; every relative rotation between consecutive rows (root
  and the 23 joint quaternions) exactly 0, at most 1e-4 rad or at least 1e-3 rad (the cut-off 1 - |w| < 1e-8 sits at 2.8e-4); sqrt(w^2 + z^2) >= 0.05.

Tolerances (bounds): from the oracle alone.  get_expert on N_COPIES copies of the rows, every coordinate moved by an independent uniform amount within half
an fp32 ulp and the root renormalised; the per-entry spread (max - min) is what fp32 input rounding alone does to the reference.
    bound = 8 * spread + 8 * 2^-24 * (|value| + |largest operand| / dt)
8 for the roughly ten fp32 operations between the input and the table, each rounding like one more input rounding; the second term a floor for entries the
perturbation happens not to move (operands: the positions for the linear tables, the joint angles for the joint tables, 1 for a quaternion component; the
tables that are no finite difference take no 1 / dt).  Entries whose reference value is an exact 0 of a finite-difference table take no bound: they are
compared exactly (a cut-off that misses leaves 1e-4 / dt there).

Caps (caps): every bound is at most a tenth of the error of the nearest wrong branch of that entry:
  joints of qvel, rlinv   0.2 (a missing clamp lets 0.34 * 30 through; a missing unwrap is 2 pi / dt, 20 after the clamp, and larger)
  rangv                   the smallest of 0.2 (clamp), 2 pi / dt (a missing wrap) and |rangv| of the pair (a cut-off that takes a turn it should not)
  bangvel                 per body the smaller of 2 pi / dt (a wrap where the reference has none) and |bangvel| (the same cut-off)
  rlinv_local             0.2, and on the catalogued pairs of root_turns / root_sign |v| * |sin(turn)|: the wrong frame
  com, ee_pos, rq_rmh     1e-3: a tenth of it is a tenth of a millimetre (1e-4 of a unit quaternion), three orders above fp32 at these magnitudes and
                          far below any wrong formula (the un-normalised heading of upside_down is wrong by 0.9)
A difference that reaches across a take boundary is wrong by the difference between the adjacent takes' rows over dt; the CPU test checks that against the
bounds of each take's first row.
"""
import functools
import math
import os

import numpy as np

from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
from oracle import np_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20261
NAMES = ("still", "joint_wrap", "root_turns", "root_sign", "upside_down", "len63", "len64", "len65", "len129")
EDGE = NAMES[:5]                                              # the takes that are also built at dt = 1 s
LENS = {"still": 2, "joint_wrap": 3, "root_turns": 10, "root_sign": 10, "upside_down": 6, "len63": 63, "len64": 64, "len65": 65, "len129": 129}
STEPS = (math.pi - 0.05, -(math.pi - 0.05), math.pi + 0.05, -(math.pi + 0.05), 2 * math.pi + 0.1, -7.0, 9.5, 0.25, -0.25, 0.34, 1e-4, 0.0)
TURNS = (1e-4, 1e-3, 1e-2, 0.3, 3.0, math.pi - 0.02, math.pi + 0.02, 3.3, 2 * math.pi - 0.01)
DERIVED = ("qvel", "rlinv_local", "rq_rmh", "com", "ee_pos", "bangvel")       # what the fixture stores per take; rlinv / rangv are qvel[:, :3] / [:, 3:6]
FD = ("qvel", "rlinv_local", "bangvel")                       # the finite differences: row 0 repeats row 1, identical rows give exact zeros
N_COPIES = 16
U = 2.0 ** -24
ROOT_DZ, HEAD_DZ = 1.25e-3, 1.25e-3                            # the len takes: the root sinks and the head rises by this much per row

_KPM = read_kpm(DEFAULT_KPM)
MODEL = (_KPM["body_pos"].reshape(24, 3), _KPM["body_ipos"].reshape(24, 3), _KPM["body_parent"], _KPM["body_mass"])


def _std():
    return np.load(os.path.join(GOLD, "standing_neutral.npz"))["qpos"].reshape(-1)[:76].astype(np.float64)


def _axis(rng):
    """a unit axis with no component under 0.2: not aligned with a coordinate axis"""
    while True:
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        if np.abs(a).min() >= 0.2:
            return a


def _yaw(a):
    return np.array([math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)])


def _hn(q):
    return math.hypot(q[0], q[3]) / np.linalg.norm(q)


def _still(rng, std):
    row = std.copy(); row[7:] += rng.uniform(-0.3, 0.3, 69)
    row[3:7] = O.quaternion_multiply(O.quaternion_about_axis(0.4, _axis(rng)), std[3:7])
    return np.stack([row, row])


def _joint_wrap(rng, std, steps=STEPS):
    r0 = std.copy(); r0[7:] = rng.uniform(-3.1, 3.1, 69)
    st = np.array([steps[j % len(steps)] for j in range(69)])
    r1 = r0.copy(); r1[7:] = r0[7:] + st
    r2 = r1.copy(); r2[7:] = r1[7:] - st
    return np.stack([r0, r1, r2])


def _root_turns(rng, std, flip):
    rows = [std.copy()]
    rows[0][7:] += rng.uniform(-0.3, 0.3, 69)
    for i, turn in enumerate(TURNS):
        prev = rows[-1]
        while True:                                           # redraw the axis until the heading divisor stays away from 0
            q = O.quaternion_multiply(O.quaternion_about_axis(turn, _axis(rng)), prev[3:7])
            if _hn(q) >= 0.1:
                break
        d = _axis(rng) * (0.5 if i % 2 == 0 else 0.2)
        r = prev.copy(); r[:3] = prev[:3] + d; r[3:7] = q
        r[7:] = prev[7:] + rng.uniform(0.01, 0.03, 69) * rng.choice([-1.0, 1.0], 69)
        rows.append(r)
    rows = np.stack(rows)
    if flip:
        rows[1::2, 3:7] *= -1.0
    return rows


def _upside_down(rng, std):
    roll = O.quaternion_about_axis(math.pi - 0.2, [1.0, 0.0, 0.0])
    tilt = O.quaternion_about_axis(0.2, [0.0, 1.0, 0.0])
    quats = [roll, O.quaternion_multiply(_yaw(0.3), roll), O.quaternion_multiply(_yaw(math.pi - 5e-4), tilt), O.quaternion_multiply(_yaw(-math.pi + 5e-4), tilt),
             O.quaternion_multiply(_yaw(0.5), std[3:7]), O.quaternion_multiply(_yaw(0.55), std[3:7])]
    rows = np.tile(std, (6, 1))
    rows[:, 7:] += rng.uniform(-0.3, 0.3, 69)
    for i, q in enumerate(quats):
        rows[i, 3:7] = q
        rows[i, :2] += 0.01 * i
        rows[i, 7:] += 0.02 * i * np.sign(rows[0, 7:] - std[7:])
    return rows


def _smooth(rng, std, T):
    """joints drift one way each by 2e-3 .. 5.2e-3 rad a row, the root yaws by about 0.015 rad a row and sinks by ROOT_DZ; a tilt about the world x axis is
    then solved per row so that the head rises by HEAD_DZ: height of the head above the root = rho cos(tilt - phi), (rho, phi) from the untilted row's FK"""
    t = np.arange(T)[:, None]
    rate = rng.uniform(0.002, 0.004, 69) * rng.choice([-1.0, 1.0], 69)
    ph = rng.uniform(0, 2 * math.pi, 69)
    inc = rate * (1 + 0.3 * np.sin(0.2 * t + ph))
    rows = np.tile(std, (T, 1))
    rows[:, 7:] += rng.uniform(-0.1, 0.1, 69) + np.cumsum(inc, 0) - inc[0]
    rows[:, :2] = np.cumsum(rng.uniform(0.005, 0.015, (T, 2)), 0)
    rows[:, 2] = 0.95 + ROOT_DZ * (T - 1 - t[:, 0])
    yaw = np.cumsum(rng.uniform(0.01, 0.02, T))
    a_prev, f0 = -1.35, None
    for i in range(T):
        q0 = O.quaternion_multiply(_yaw(yaw[i]), std[3:7])
        flat = rows[i].copy(); flat[:3] = 0; flat[3:7] = q0
        p = O.qpos_fk(flat, *MODEL[:3])["wbpos"][13]
        rho, phi = math.hypot(p[1], p[2]), math.atan2(p[1], p[2])          # z after a tilt a about x: p_y sin a + p_z cos a = rho cos(a - phi)
        if f0 is None:
            f0 = rho * math.cos(a_prev - phi)
        target = f0 + (ROOT_DZ + HEAD_DZ) * i
        if not target < 0.98 * rho:
            raise ValueError(f"take_edges: the head of a {T}-row take cannot rise to {target:.3f} m above the root")
        a = phi - math.acos(target / rho)
        rows[i, 3:7] = O.quaternion_multiply(O.quaternion_about_axis(a, [1.0, 0.0, 0.0]), q0)
        a_prev = a
    return rows


def _take(name, rng, std):
    if name == "still":
        return _still(rng, std)
    if name == "joint_wrap":
        return _joint_wrap(rng, std)
    if name in ("root_turns", "root_sign"):
        return _root_turns(rng, std, name == "root_sign")
    if name == "upside_down":
        return _upside_down(rng, std)
    return _smooth(rng, std, LENS[name])


def rows_for_reference(rows):
    """what both fp64 references read: the fp32 values of the rows, the root quaternion renormalised in fp64"""
    r = np.asarray(rows).astype(np.float32).astype(np.float64)
    r[:, 3:7] /= np.linalg.norm(r[:, 3:7], axis=1, keepdims=True)
    return r


def _rel_angle(q1, q0):
    """(rotation angle in [0, pi], w) of q1 (x) q0^-1"""
    d = O.quaternion_multiply(q1, O.quaternion_inverse(q0))
    d = d / np.linalg.norm(d)
    return 2 * math.atan2(np.linalg.norm(d[1:]), abs(d[0])), d[0]


def pair_rotations(rows):
    """per consecutive pair of one take: ([T - 1, 24] rotation angles in [0, pi], [T - 1, 24] w of the relative quaternions)"""
    bq = np.stack([O.get_body_quat(r) for r in rows]).reshape(len(rows), 24, 4)
    ang, w = np.zeros((len(rows) - 1, 24)), np.zeros((len(rows) - 1, 24))
    for i in range(len(rows) - 1):
        for b in range(24):
            ang[i, b], w[i, b] = _rel_angle(bq[i + 1, b], bq[i, b])
    return ang, w


def check_conditions(rows, take_off):
    """the conditions on the inputs, in fp64 on the rows as built (rounding them to fp32 moves an angle by under 1e-6 rad, against margins of 1e-2 and a
    band from 1e-4 to 1e-3); ValueError names the first one broken"""
    ref = np.array(rows, np.float64)
    ref[:, 3:7] /= np.linalg.norm(ref[:, 3:7], axis=1, keepdims=True)
    if not np.isfinite(ref).all():
        raise ValueError("take_edges: a row is not finite")
    hn = np.hypot(ref[:, 3], ref[:, 6])
    if hn.min() < 0.05:
        raise ValueError(f"take_edges: row {int(hn.argmin())} has sqrt(w^2 + z^2) = {hn.min():.3g} < 0.05")
    for k in range(len(take_off) - 1):
        tk = ref[take_off[k]:take_off[k + 1]]
        if len(tk) < 2:
            raise ValueError(f"take_edges: take {k} has fewer than 2 rows")
        d = np.diff(tk[:, 7:], axis=0)
        off = np.abs(np.abs(d) / math.pi - (2 * np.floor(np.abs(d) / (2 * math.pi)) + 1)) * math.pi           # distance to the nearest odd multiple of pi
        if off.min() < 0.02:
            i, j = np.unravel_index(off.argmin(), off.shape)
            raise ValueError(f"take_edges: take {k} pair {i} joint {j}: a difference of {d[i, j]:.6f} is within 0.02 rad of an odd multiple of pi")
        ang, w = pair_rotations(tk)
        full = np.where(w[:, 0] < 0, 2 * math.pi - ang[:, 0], ang[:, 0])                                     # 2 acos(w), what the root's wrap sees
        if np.abs(full - math.pi).min() < 0.01:
            raise ValueError(f"take_edges: take {k} pair {int(np.abs(full - math.pi).argmin())}: a root turn within 0.01 rad of pi")
        same = (tk[1:, 7:] == tk[:-1, 7:]).reshape(len(tk) - 1, 23, 3).all(-1)
        same = np.concatenate([(tk[1:, 3:7] == tk[:-1, 3:7]).all(-1)[:, None], same], 1)
        bad = ~same & (ang > 1e-4 * (1 + 1e-9)) & (ang < 1e-3 * (1 - 1e-9))                # identical quaternions turn by exactly 0
        if bad.any():
            i, b = np.argwhere(bad)[0]
            raise ValueError(f"take_edges: take {k} pair {i} body {b}: a relative rotation of {ang[i, b]:.3g} rad is neither 0, <= 1e-4 nor >= 1e-3 (the cut-off sits at 2.8e-4)")


def _heights(rows32):
    """(root heights, head heights) of fp32-valued rows, in fp64"""
    r = rows_for_reference(rows32)
    return r[:, 2], np.array([O.qpos_fk(x, *MODEL[:3])["wbpos"][13][2] for x in r])


def check_minima(rows, take_off):
    """the len takes: lowest root height at the last row, lowest head height at row 0, every two heights of a take at least 1e-3 apart"""
    for k, name in enumerate(NAMES):
        if not name.startswith("len"):
            continue
        z, hz = _heights(rows[take_off[k]:take_off[k + 1]])
        if int(z.argmin()) != CATALOGUE[name]["min_root_row"] or int(hz.argmin()) != CATALOGUE[name]["min_head_row"]:
            raise ValueError(f"take_edges: {name}: minima at rows {int(z.argmin())} / {int(hz.argmin())}, not where the catalogue says")
        if np.diff(np.sort(z)).min() < 1e-3 or np.diff(np.sort(hz)).min() < 1e-3:
            raise ValueError(f"take_edges: {name}: two heights closer than 1e-3")


CATALOGUE = {n: {"len": LENS[n]} for n in NAMES}
for _n in ("len63", "len64", "len65", "len129"):
    CATALOGUE[_n].update(min_root_row=LENS[_n] - 1, min_head_row=0)
for _n in ("root_turns", "root_sign"):
    CATALOGUE[_n].update(turns=TURNS, cutoff_pair=0)          # pair i = rows i -> i + 1; pair 0 (1e-4 rad) falls under the cut-off: table rows 0 and 1


def assemble(takes):
    """(rows, take_off) of a list of per-take row arrays, conditions checked"""
    rows = np.concatenate(takes, 0)
    take_off = np.concatenate([[0], np.cumsum([len(t) for t in takes])]).astype(np.int32)
    check_conditions(rows, take_off)
    return rows, take_off


@functools.lru_cache(maxsize=None)
def _build(seed):
    std = _std()
    takes = [_take(name, np.random.default_rng([seed, k]), std) for k, name in enumerate(NAMES)]
    rows, take_off = assemble(takes)
    assert [int(b - a) for a, b in zip(take_off[:-1], take_off[1:])] == [LENS[n] for n in NAMES]
    check_minima(rows, take_off)
    return rows, take_off


def build(seed=SEED):
    """(rows [R, 76] fp64, take_off [10] int32) of the nine takes"""
    rows, take_off = _build(seed)
    return rows.copy(), take_off.copy()


def broken_take():
    """joint_wrap with a step of exactly pi: assemble() must refuse it"""
    return _joint_wrap(np.random.default_rng([SEED, 1]), _std(), steps=(math.pi,) + STEPS[1:])


def take_slice(take_off, names=NAMES):
    return {n: slice(int(take_off[k]), int(take_off[k + 1])) for k, n in enumerate(names)}


def oracle_tables(ref_rows, dt):
    """oracle.np_oracle.get_expert on one take's reference rows"""
    ex = O.get_expert(np.array(ref_rows, np.float64), *MODEL, dt=dt)
    out = {t: np.asarray(ex[t], np.float64) for t in DERIVED}
    out["height_lb"], out["head_height_lb"] = float(ex["height_lb"]), float(ex["head_height_lb"])
    return out


def perturbed(rows, rng):
    """one copy of the reference rows with every coordinate moved within half an fp32 ulp of its fp32 value"""
    r32 = np.asarray(rows).astype(np.float32)
    r = r32.astype(np.float64) + rng.uniform(-0.5, 0.5, r32.shape) * np.spacing(np.abs(r32)).astype(np.float64)
    r[:, 3:7] /= np.linalg.norm(r[:, 3:7], axis=1, keepdims=True)
    return r


def load_fixture():
    return np.load(os.path.join(GOLD, "uhc_take_edges.npz"))


def fixture_dts(g):
    return [float(x) for x in g["dts"]]


def fixture_key(di, name, table):
    return f"d{di}_{name}_{table}"


def _pairs(a):
    """per-pair values [T - 1, ...] laid out per table row [T, ...]: row r holds pair r - 1, row 0 pair 0"""
    return np.concatenate([a[:1], a], 0)


def _operands(tk, dt):
    """the floor's |largest operand| / dt per table, for one take's reference rows [T, 76]"""
    T = len(tk)
    pos = _pairs(np.maximum(np.abs(tk[1:, :3]), np.abs(tk[:-1, :3])))
    jnt = _pairs(np.maximum(np.abs(tk[1:, 7:]), np.abs(tk[:-1, 7:])))
    body = np.concatenate([np.ones((T, 1)), np.maximum(1.0, jnt.reshape(T, 23, 3).max(-1))], 1)
    reach = np.abs(tk[:, :3]).max(1, keepdims=True) + 1.0
    return {"qvel": np.concatenate([pos, np.ones((T, 3)), jnt], 1) / dt, "rlinv_local": np.repeat(pos.max(1, keepdims=True), 3, 1) / dt,
            "bangvel": np.repeat(body, 3, 1) / dt, "rq_rmh": np.ones((T, 4)), "com": np.repeat(reach, 3, 1), "ee_pos": np.repeat(reach, 15, 1)}


def spreads(rows, take_off, names, dt, seed, n=N_COPIES):
    """per take and table: (min, max) over n perturbed copies of the oracle's tables"""
    sl = take_slice(take_off)
    rng = np.random.default_rng([SEED, seed])
    lo, hi = {}, {}
    for _ in range(n):
        p = perturbed(rows, rng)
        for name in names:
            tab = oracle_tables(p[sl[name]], dt)
            for t in DERIVED:
                key = (name, t)
                lo[key] = tab[t] if key not in lo else np.minimum(lo[key], tab[t])
                hi[key] = tab[t] if key not in hi else np.maximum(hi[key], tab[t])
    return lo, hi


@functools.lru_cache(maxsize=None)
def _bounds(dt, names, seed):
    rows, take_off = _build(SEED)
    ref = rows_for_reference(rows)
    sl = take_slice(take_off)
    lo, hi = spreads(rows, take_off, names, dt, seed)
    out = {}
    for name in names:
        val = oracle_tables(ref[sl[name]], dt)
        op = _operands(ref[sl[name]], dt)
        for t in DERIVED:
            out[(name, t)] = 8 * (hi[(name, t)] - lo[(name, t)]) + 8 * U * (np.abs(val[t]) + op[t])
    return out


def bounds(dt, names=NAMES, seed=1):
    """{(take, table): per-entry absolute bound}, from the oracle alone (module docstring)"""
    return _bounds(float(dt), tuple(names), seed)


def exact_zero(name, table, want):
    """the entries compared exactly: exact zeros of a finite-difference table"""
    return (want == 0) if table in FD else np.zeros(want.shape, bool)


def caps(dt, names=NAMES):
    """{(take, table): per-entry cap on the bound}: a tenth of the error of the nearest wrong branch (module docstring); inf where the entry is an exact 0"""
    rows, take_off = _build(SEED)
    ref = rows_for_reference(rows)
    sl = take_slice(take_off)
    out = {}
    with np.errstate(divide="ignore"):
        for name in names:
            tk = ref[sl[name]]
            T = len(tk)
            val = oracle_tables(tk, dt)
            wrap = 2 * math.pi / dt
            rang = np.linalg.norm(val["qvel"][:, 3:6], axis=1, keepdims=True)
            c = np.full((T, 75), 0.2)
            c[:, 3:6] = np.minimum(np.minimum(0.2, wrap), np.where(rang > 0, rang, np.inf))
            out[(name, "qvel")] = 0.1 * c
            bv = np.linalg.norm(val["bangvel"].reshape(T, 24, 3), axis=2)
            out[(name, "bangvel")] = 0.1 * np.repeat(np.minimum(wrap, np.where(bv > 0, bv, np.inf)), 3, 1)
            c = np.full((T, 3), 0.2)
            if "turns" in CATALOGUE[name]:
                v = np.linalg.norm(val["qvel"][:, :3], axis=1)
                c = np.minimum(c, (v * _pairs(np.abs(np.sin(np.array(TURNS)))))[:, None])
            out[(name, "rlinv_local")] = 0.1 * c
            for t, w in (("rq_rmh", 4), ("com", 3), ("ee_pos", 15)):
                out[(name, t)] = np.full((T, w), 1e-4)
    return out
