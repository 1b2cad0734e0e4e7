"""The chunk loop of the rows launchers (launch_rows, kp_readout.hip) on a real MI355X: with KP_ROWS_CHUNK = 64 a call of 67 rows is two launches, the
second with row0 = 64 and three rows -- the smallest call that has row0 > 0 and a ragged last chunk.  Every rows kernel must give the bits of the
one-launch call, and rows 64..66 the bits of those rows computed alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import inverse_dynamics_oracle as ID  # noqa: E402
import rows_harness as H  # noqa: E402
from rows_harness import STD, dev, handle  # noqa: E402
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm  # noqa: E402

R = 67


@pytest.fixture(scope="module")
def kp():
    return H.gpu_module()


def rows(scene):
    """q, v, a, blk (None on the floor) of 67 rows: the named floor states in turn, or the sit state, each row with its own seeded qacc"""
    named = ID.named_states(read_kpm(DEFAULT_KPM), read_kpm(STEP_KPM), STD["qpos"], STD["qvel"])
    sts = named[:-1] if scene == "floor" else named[-1:]
    pick = [sts[e % len(sts)] for e in range(R)]
    a = ID.f32(np.random.default_rng(11).normal(size=(R, 75)) * 30.0)
    blk = None if scene == "floor" else dev(np.stack([s["blk"] for s in pick]))
    return dev(np.stack([s["q"] for s in pick])), dev(np.stack([s["v"] for s in pick])), dev(a), blk


def calls(kp, scene):
    """name -> f(rows lo..hi) -> dict of device outputs, for every rows kernel the scene reaches"""
    sim = handle(kp, DEFAULT_KPM if scene == "floor" else STEP_KPM)
    q, v, a, blk = rows(scene)
    cut = lambda t, s: None if t is None else t[s].contiguous()  # noqa: E731
    out = {"inverse_dynamics": lambda s: sim.inverse_dynamics(q[s], v[s], a[s], cut(blk, s), want=tuple(kp.INVDYN_OUTPUTS)),
           "estimate_contacts": lambda s: sim.estimate_contacts(q[s], v[s], a[s], cut(blk, s), want=tuple(kp.ESTIMATE_OUTPUTS))}
    if scene == "floor":
        body = dev(np.arange(R) % 24, torch.int32)
        off = dev(ID.f32(np.random.default_rng(12).uniform(-0.2, 0.2, (R, 3))))
        tgt = sim.fk(dev(np.roll(q.cpu().numpy(), 1, axis=0)))["wbpos"].view(R, 24, 3)          # the next state's body positions
        cfg = kp.KpFitCfg.default()
        cfg.n_iters = 4
        out["body_motion"] = lambda s: sim.body_motion(q[s], v[s], a[s])
        out["point_jacobian"] = lambda s: {"J": sim.point_jacobian(q[s], body[s], off[s])}
        out["fit_pose"] = lambda s: sim.fit_pose(q[s], tgt[s].contiguous(), cfg=cfg, want_dq=True)
    return out


@pytest.mark.parametrize("scene", ["floor", "g_sit"])
def test_chunked_launches_equal_one_launch(kp, scene, monkeypatch):
    every, tail = slice(0, R), slice(64, R)
    for name, f in calls(kp, scene).items():
        monkeypatch.delenv("KP_ROWS_CHUNK", raising=False)
        whole, alone = f(every), f(tail)
        monkeypatch.setenv("KP_ROWS_CHUNK", "64")
        chunked = f(every)
        assert set(chunked) == set(whole) and len(whole) > 0
        for k in whole:
            assert whole[k].shape[0] == R and alone[k].shape[0] == 3, (name, k)
            assert torch.equal(chunked[k].view(torch.int32), whole[k].view(torch.int32)), f"{name}: {k} in two launches against one"
            assert torch.equal(chunked[k][tail].view(torch.int32), alone[k].view(torch.int32)), f"{name}: {k}, rows 64..66 against those rows alone"
        assert all(bool(t.isfinite().all()) for t in whole.values()) and any(bool(t.any()) for t in whole.values()), f"{name}: the outputs are filled"
