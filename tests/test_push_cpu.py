"""Impulse pushes without a GPU: the exported entry point, the PushSchedule on the CPU device, the scripts' flags, and the fp64 reference
tests/push_oracle.py held to closed forms that use OracleSim only (momentum, power, the root push)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import push_oracle as PO
from kinpoly_amd import build as kpbuild
from oracle.kpo import OracleSim

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
M_TOTAL = 80.2914


def test_apply_impulse_is_exported():
    if not os.path.exists(kpbuild.LIB):
        kpbuild.build_native()
    L = ctypes.CDLL(kpbuild.LIB)
    assert hasattr(L, "kp_sim_apply_impulse")
    L.kp_sim_apply_impulse.restype = ctypes.c_int
    L.kp_sim_apply_impulse.argtypes = [ctypes.c_void_p] * 6
    L.kp_last_error.restype = ctypes.c_char_p
    assert L.kp_sim_apply_impulse(None, None, None, None, None, None) == -1 and b"kp_sim_apply_impulse: null argument" in L.kp_last_error()
    from kinpoly_amd.sim import ABI_SYMBOLS
    assert "kp_sim_apply_impulse" in ABI_SYMBOLS
    assert "kp_sim_apply_impulse(" in open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()


def _schedule(**kw):
    from kinpoly_amd.push import PushSchedule
    return PushSchedule(**{**dict(n_envs=64, device="cpu", interval=3, bodies=("Chest", "Head", "L_Knee"), impulse=(10.0, 30.0), seed=5), **kw})


def test_schedule_draws():
    from kinpoly_amd.env import SMPL_BODY_NAMES
    a, b, c = _schedule(), _schedule(), _schedule(seed=6)
    ids = {SMPL_BODY_NAMES.index(x) for x in ("Chest", "Head", "L_Knee")}
    differs = False
    for t in range(1, 13):
        cur_t = torch.full((64,), t, dtype=torch.int32); cur_t[::2] += 1          # two episode clocks in the batch
        (ea, ia, oa), (eb, ib, _), (ec, ic, _) = a.draw(cur_t), b.draw(cur_t), c.draw(cur_t)
        assert torch.equal(ea, eb) and torch.equal(ia, ib) and oa is None          # one seed, identical draws
        differs |= not torch.equal(ia, ic)
        due = cur_t % 3 == 0
        assert torch.equal(ea >= 0, due)                                           # prob = 1: a push exactly on the multiples of the interval
        assert set(ea[due].tolist()) <= ids and (ea[~due] == -1).all() and not ia[~due].any()
        mag = ia[due, :3].norm(dim=1)
        assert ((mag > 10.0 - 1e-4) & (mag < 30.0 + 1e-4)).all()
        assert not ia[:, 2].any() and not ia[:, 3:].any()                          # horizontal: p_z = 0, l = 0
    assert differs and int(a.count) == sum(int(((torch.full((64,), t) + (torch.arange(64) % 2 == 0)) % 3 == 0).sum()) for t in range(1, 13))
    s = _schedule(horizontal=False, interval=1, n_envs=4096)
    _, imp, _ = s.draw(torch.ones(4096, dtype=torch.int32))
    assert imp[:, 2].abs().max() > 5 and abs(float(imp[:, 2].mean())) < 1.5 and not imp[:, 3:].any()      # on the sphere: p_z = mag x uniform(-1, 1)
    half = _schedule(prob=0.5, interval=1, n_envs=4096)
    ent, _, _ = half.draw(torch.ones(4096, dtype=torch.int32))
    assert 0.45 < float((ent >= 0).float().mean()) < 0.55
    alive = torch.arange(64) % 4 != 0
    ent, imp, off = _schedule(interval=1, offset=(0.0, 0.1, 0.2)).draw(torch.ones(64, dtype=torch.int32), alive)
    assert torch.equal(ent >= 0, alive) and not imp[~alive].any() and tuple(off.shape) == (64, 3) and torch.equal(off[7], torch.tensor([0.0, 0.1, 0.2]))


def test_schedule_refusals():
    with pytest.raises(ValueError, match="unknown body 'Tail'"):
        _schedule(bodies=("Chest", "Tail"))
    with pytest.raises(ValueError, match="interval"):
        _schedule(interval=0)
    with pytest.raises(ValueError, match="prob"):
        _schedule(prob=1.5)
    with pytest.raises(ValueError, match="impulse"):
        _schedule(impulse=(30.0, 10.0))


@pytest.mark.parametrize("script", ["train_uhc", "eval_uhc", "train_ar_policy", "eval_ar_policy"])
def test_script_flags(script):
    spec = importlib.util.spec_from_file_location("push_flags_" + script, os.path.join(ROOT, "scripts", script + ".py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    off = mod.build_parser().parse_args([])
    assert off.push_impulse is None                                               # off unless asked for
    from kinpoly_amd.push import schedule_from_args
    assert schedule_from_args(off, 4, "cpu") is None
    on = mod.build_parser().parse_args(["--push_impulse", "10", "30", "--push_interval", "5", "--push_prob", "0.5", "--push_bodies", "Chest,Head", "--push_seed", "3"])
    s = schedule_from_args(on, 4, "cpu")
    assert (s.lo, s.hi, s.interval, s.prob, s.body_names) == (10.0, 30.0, 5, 0.5, ("Chest", "Head"))
    one = schedule_from_args(mod.build_parser().parse_args(["--push_impulse", "20"]), 4, "cpu")
    assert (one.lo, one.hi, one.interval) == (20.0, 20.0, 30)


# ---------------------------------------------------------------------------------------------------------------- the reference against closed forms

def _poses(n, seed):
    rng = np.random.default_rng(seed)
    q = np.tile(STD["qpos"], (n, 1))
    q[:, 7:] = rng.uniform(-1.2, 1.2, (n, 69))
    d = rng.normal(size=(n, 4)); q[:, 3:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return q


@pytest.fixture(scope="module")
def oracle():
    return OracleSim(contact=False, limits=False)


def test_total_mass(oracle):
    oracle.reset(STD["qpos"], np.zeros(75)); oracle.forward()
    assert abs(oracle.fullM()[0, 0] - M_TOTAL) < 1e-3


def test_reference_conserves_linear_momentum(oracle):
    """m_total dv_com = p for every body and random offsets: the centre-of-mass velocity is the directional derivative of subtree_com along dv"""
    rng = np.random.default_rng(2)
    qs = _poses(24, 1)
    for b in range(24):
        off = rng.uniform(-0.15, 0.15, 3)
        imp = np.concatenate([rng.normal(size=3) * 30, rng.normal(size=3) * 3])
        dv = PO.delta_qvel(oracle, qs[b], b, off, imp)
        m = oracle.fullM()[0, 0]
        vcom = PO.com_velocity(oracle, qs[b], dv)
        assert np.abs(m * vcom - imp[:3]).max() < 1e-8 * np.abs(imp[:3]).max(), (b, m * vcom, imp[:3])


def test_reference_power_identity(oracle):
    """g^T dv = w^T (J dv) > 0: the work of the impulse is the kinetic energy it creates, twice"""
    rng = np.random.default_rng(3)
    qs = _poses(6, 4)
    for e, b in enumerate((0, 4, 11, 13, 18, 22)):
        off = rng.uniform(-0.15, 0.15, 3)
        w = np.concatenate([rng.normal(size=3) * 30, rng.normal(size=3) * 3])
        Jp, _ = PO.point_jacobian(oracle, qs[e], b, off)
        g = Jp.T @ w
        dv = oracle.solveM(g)
        M = oracle.fullM()
        assert np.abs(M @ dv - g).max() < 1e-9 * np.abs(g).max()
        assert g @ dv > 0 and abs(g @ dv - w @ (Jp @ dv)) < 1e-12 * abs(g @ dv) and abs(g @ dv - dv @ M @ dv) < 1e-9 * abs(g @ dv)


def test_reference_root_push(oracle):
    """A pure p at the root origin of the straight standing pose: the root's linear dofs are world translations, so g is p on them and zero on the root's
    rotations; the root moves faster than the whole body would (dv_root > p / m_total: the limbs lag behind on their joints) and slower than the pelvis
    alone would (p / m_pelvis), while the centre of mass takes exactly p / m_total."""
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    m_pelvis = float(read_kpm(DEFAULT_KPM)["body_mass"][0])
    q = STD["qpos"].copy(); q[7:] = 0.0; q[3:7] = [1, 0, 0, 0]
    p = np.array([25.0, 0.0, 0.0])
    imp = np.concatenate([p, np.zeros(3)])
    g = PO.generalised_impulse(oracle, q, 0, np.zeros(3), imp)
    assert np.abs(g[:3] - p).max() < 1e-12 and np.abs(g[3:6]).max() < 1e-12
    dv = PO.delta_qvel(oracle, q, 0, np.zeros(3), imp)
    m = oracle.fullM()[0, 0]
    assert p[0] / m < dv[0] < p[0] / m_pelvis
    assert np.abs(m * PO.com_velocity(oracle, q, dv) - p).max() < 1e-8 * 25.0
    assert not PO.delta_qvel(oracle, q, 24, np.zeros(3), imp).any() and not PO.delta_qvel(oracle, q, -1, np.zeros(3), imp).any()


def test_object_reference_closed_form():
    """A free body pushed through its centre of mass only translates, with p / m: that holds for the object's inertia without the free joint's armature
    (which sits on the diagonal of object_dyn's M), and checks both the oracle's M and the reference's generalised impulse g."""
    from kinpoly_amd.model_compiler import STEP_KPM, read_kpm
    kpm = read_kpm(STEP_KPM)
    quat = np.array([0.8, 0.2, -0.4, 0.3]); quat /= np.linalg.norm(quat)
    p = np.array([3.0, -2.0, 1.0])
    for oi in (0, 1, 3):                                         # chair, box, Can
        inert = kpm["obj_inertial"].reshape(-1, 13)[oi]
        mass, c, arm = inert[0], inert[1:4], inert[12]
        pose = np.concatenate([[0.3, -0.2, 0.9], quat])
        o = OracleSim(kpm=STEP_KPM)
        o.set_object(0, kpm, oi, pose)
        q = STD["qpos"].copy(); q[0] += 30
        o.reset(q, np.zeros(75))
        imp = np.concatenate([p, np.zeros(3)])
        M = o.object_dyn(0)[0]
        dv = PO.object_delta_qvel(o, 0, pose, c, imp)
        g = M @ dv
        assert np.abs(g[:3] - p).max() < 1e-9 * np.abs(p).max()
        free = np.linalg.solve(M - arm * np.eye(6), g)           # the same impulse on the body without the joint's armature
        R = PO._rot(quat)
        assert np.abs(free[3:]).max() < 1e-9 * np.abs(p).max() / mass, oi
        assert np.abs(free[:3] + np.cross(R @ free[3:], R @ c) - p / mass).max() < 1e-9 * np.abs(p).max() / mass, oi
