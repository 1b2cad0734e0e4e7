"""The proof behind tests/np_rigid.py: every helper there against each copy it replaced, np.array_equal of the outputs on 1000 seeded random inputs
with the degenerate ones each copy guards mixed in; and the same comparison for the copies that were NOT merged, to record that they differ.

    python profiles/rows_call/helpers_equal.py <tests directory of the parent commit>

Exits 0 when every merged pair is equal on every input."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [sys.argv[1], ROOT]
spec = importlib.util.spec_from_file_location("np_rigid", os.path.join(ROOT, "tests", "np_rigid.py"))
NR = importlib.util.module_from_spec(spec); spec.loader.exec_module(NR)

import body_motion_oracle as BM  # noqa: E402  (the parent's copies)
import contact_estimate_oracle as CE  # noqa: E402
import contact_force_oracle as CF  # noqa: E402
import fit_pose_oracle as FP  # noqa: E402
import inverse_dynamics_oracle as ID  # noqa: E402
import known_answers as KA  # noqa: E402
import push_oracle as PO  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM  # noqa: E402

assert os.path.samefile(os.path.dirname(BM.__file__), sys.argv[1]), "the copies must come from the parent's tests"
N = 1000
rng = np.random.default_rng(2024)


def unit(v):
    return v / np.linalg.norm(v)


def quats():
    """random quaternions: unit and non-unit, every fourth with w < 0, some with w = 0 exactly, the identity and its negative"""
    out = []
    for i in range(N):
        q = rng.normal(size=4)
        q = unit(q) if i % 2 else q * rng.uniform(0.1, 3.0)
        q[0] = -abs(q[0]) if i % 4 == 0 else q[0]
        out.append(q)
    out[1], out[2], out[3] = np.array([1.0, 0, 0, 0]), np.array([-1.0, 0, 0, 0]), np.array([0.0, 0, 1.0, 0])
    return out


def normals():
    """random unit normals, with +-z, +-x, +-y and normals on either side of the |n_y| = 0.5 switch"""
    out = [unit(rng.normal(size=3)) for _ in range(N)]
    out[:6] = [np.array(v, float) for v in ([0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0])]
    for i, ny in enumerate((0.5, -0.5, np.nextafter(0.5, 0), np.nextafter(0.5, 1))):
        out[6 + i] = np.array([np.sqrt(1 - ny * ny), ny, 0.0])
    return out


def equal(name, new, old, inputs):
    same = sum(np.array_equal(np.asarray(new(*x)), np.asarray(old(*x))) for x in inputs)
    print(f"{name}: equal on {same} of {len(inputs)} inputs")
    return same == len(inputs)


Q, NRM = quats(), normals()
assert sum(q[0] < 0 for q in Q) >= N // 4
pairs = [(a, b) for a, b in zip(Q, Q[1:] + Q[:1])]
vals = [(rng.normal(size=rng.integers(1, 80)) * 10.0 ** rng.integers(-8, 8),) for _ in range(N)]
ok = True
print("merged into tests/np_rigid.py:")
ok &= equal("qmul = body_motion_oracle.qmul", NR.qmul, BM.qmul, pairs)
ok &= equal("qmul = fit_pose_oracle.qmul", NR.qmul, FP.qmul, pairs)
ok &= equal("quat_matrix = contact_estimate_oracle.quat_matrix", NR.quat_matrix, CE.quat_matrix, [(q,) for q in Q])
ok &= equal("quat_matrix = push_oracle._rot", NR.quat_matrix, PO._rot, [(q,) for q in Q])
ok &= equal("make_frame = contact_force_oracle.make_frame", NR.make_frame, CF.make_frame, [(n,) for n in NRM])
ok &= equal("make_frame = contact_estimate_oracle.make_frame", NR.make_frame, CE.make_frame, [(n,) for n in NRM])
for M in (BM, FP, ID):
    ok &= equal(f"f32 = {M.__name__}.f32", NR.f32, M.f32, vals)
# oracle(kpm_path): the same constructor call; compared by what the oracles compute (positions, orientations, centres of mass of 1000 random poses)
o_new, o_bm, o_fp = NR.oracle(DEFAULT_KPM), BM.oracle(DEFAULT_KPM), FP.oracle(DEFAULT_KPM)
poses = []
for q in Q:
    p = np.concatenate([rng.normal(size=3), q, rng.uniform(-3.0, 3.0, 69)])
    poses.append((p,))


def kin(o):
    def f(p):
        o.reset(p, np.zeros(75))
        return np.concatenate([o.get("xpos"), o.get("xquat"), o.get("xipos")])
    return f


ok &= equal("oracle = body_motion_oracle.oracle", kin(o_new), kin(o_bm), poses)
ok &= equal("oracle = fit_pose_oracle.oracle", kin(o_new), kin(o_fp), poses)
print("left separate (they differ):")
equal("quat_matrix vs body_motion_oracle.qmat (1 - 2 (y^2 + z^2) on the diagonal)", NR.quat_matrix, BM.qmat, [(q,) for q in Q])
equal("make_frame vs known_answers.make_frame (normalises n, returns a tuple)", NR.make_frame, lambda n: np.stack(KA.make_frame(n)), [(n,) for n in NRM])
equal("body_motion_oracle.fk vs fit_pose_oracle.fk, positions only (reset against set_state_raw of the normalised pose; R and xipos against xquat)",
      lambda p: BM.fk(o_bm, p)[0], lambda p: FP.fk(o_fp, p)[0], poses[:100])
sys.exit(0 if ok else 1)
