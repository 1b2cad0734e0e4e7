"""What the GPU tests of the rows tools share (test_gpu_inverse_dynamics, test_gpu_contact_estimate, test_gpu_body_motion, test_gpu_fit_pose,
test_gpu_contact_force, test_gpu_rows_chunk): test infrastructure, imported like the *_oracle modules.  Nothing here chooses a case or a tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

import contact_force_oracle as CF
import inverse_dynamics_oracle as ID
from kinpoly_amd.model_compiler import DEFAULT_KPM, STEP_KPM, read_kpm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))


def gpu_module():
    """kinpoly_amd.sim, behind the test modules' `kp` fixtures: a GPU test without a device fails, it does not skip"""
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    return kpsim


def dev(a, dt=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


class Measured(dict):
    """running maxima of named figures: what a module prints beside its tolerances"""

    def note(self, key, v, *also):
        """also: further dicts that keep their own maximum of the figure (a test's local ones)"""
        for d in (self, *also):
            d[key] = max(d.get(key, 0.0), float(v))


_SIMS = {}


def handle(kp, blob=DEFAULT_KPM, n=1, **opts):
    """one handle per (blob, envs, options), kept for the session"""
    key = (blob, n, tuple(sorted(opts.items())))
    if key not in _SIMS:
        _SIMS[key] = kp.KpSim(kp.KpModel(blob, **opts), n)
    return _SIMS[key]


def same_bits(a, b, keys=None):
    """the 32-bit numpy outputs a[k] and b[k] are equal bit for bit"""
    for k in a if keys is None else keys:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def sentinel(table, struct, rows=5):
    """output buffers of an outputs table filled with 7 and the C struct that points at them"""
    bufs = {k: torch.full((rows, *shape), 7, dtype=dt, device="cuda") for k, (shape, dt) in table.items()}
    return bufs, struct(*[ctypes.c_void_p(b.data_ptr()) for b in bufs.values()])


def refused_calls_wrote_nothing(*bufs):
    """after the refused calls: every sentinel buffer (tensors, or sentinel()'s dicts) still holds its 7s"""
    torch.cuda.synchronize()
    for b in bufs:
        for k, t in (b.items() if isinstance(b, dict) else [("", b)]):
            assert bool((t == 7).all()), f"a refused call launched nothing: {k}"


def step_pair(kp, scene, floor=None):
    """Two equal 67-env handles on 16 wave slots (the job queue; the lean layout on the floor handle) and an action for them.  scene: floor -- the states
    `floor` (dicts with q, v; default the first five of inverse_dynamics_oracle.named_states) in turn -- or h_push."""
    if scene == "floor":
        floor = ID.named_states(read_kpm(DEFAULT_KPM), read_kpm(STEP_KPM), STD["qpos"], STD["qvel"])[:5] if floor is None else floor
        sts = [dict(q=floor[e % 5]["q"], v=floor[e % 5]["v"], blk=None) for e in range(67)]
    else:
        q, v, blk, _ = CF.object_scenes(read_kpm(STEP_KPM), STD["qpos"])["h_push"]
        sts = [dict(q=ID.f32(q), v=ID.f32(v), blk=ID.f32(blk)) for _ in range(67)]
    sims = []
    for _ in range(2):
        sim = kp.KpSim(kp.KpModel(DEFAULT_KPM if scene == "floor" else STEP_KPM, queue_slots=16), 67)
        if sts[0]["blk"] is not None:
            sim.set_objects(dev(np.stack([s["blk"] for s in sts])))
        sim.set_state(dev(np.stack([s["q"] for s in sts])), dev(np.stack([s["v"] for s in sts])))
        sim.set_target(dev(np.tile(ID.f32(STD["qpos"]), (67, 1))))
        sims.append(sim)
    return sims, dev(np.random.default_rng(3).normal(size=(67, 75)) * 0.3)


def control_step_untouched(kp, scene, between, floor=None, pair=None):
    """Three control steps on two equal handles, between(sims[0]) before each of them on the first handle only: every stored field and kp_sim_diag end
    bit-identical.  pair: the caller's own (handles, action) in place of step_pair(kp, scene, floor)."""
    sims, act = step_pair(kp, scene, floor) if pair is None else pair
    for _ in range(3):
        between(sims[0])
        for s in sims:
            s.step_ctrl(act, 15)
    assert sims[0].queue_counters()["claimed"] > 0
    for k in kp.FIELDS:
        try:
            x = sims[0].get(k)
        except kp.KinPolyNativeError:
            with pytest.raises(kp.KinPolyNativeError):
                sims[1].get(k)
            continue
        assert torch.equal(x.view(torch.int32), sims[1].get(k).view(torch.int32)), k
    assert np.array_equal(sims[0].diag(), sims[1].diag())
