"""On the device: the step kernels read their argument block from the kernarg segment at the site of use and carry the phase profiler as a compile-time
property.  Neither changes arithmetic: the three launch forms (lean job queue, full-layout job queue, one workgroup per env) and the overflow kernel
agree word for word on a small batch with contacts and joint limits active, and a profiled handle reports cycles for every env and leaves the unprofiled states."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
STD = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
N = 128


@pytest.fixture(scope="module")
def kp():
    from kinpoly_amd import sim as kpsim
    return kpsim


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def _scene(n, seed):
    """standing poses with perturbed joints; every third env lies on the floor at a seeded heading (contacts all along the body, joints at their limits)"""
    rng = np.random.default_rng(seed)
    qpos = np.tile(STD["qpos"], (n, 1)); qpos[:, 7:] += np.clip(rng.normal(size=(n, 69)) * 0.2, -np.pi, np.pi)
    qvel = rng.normal(size=(n, 75)) * 0.5
    c = np.cos(np.pi / 4)
    for e in range(0, n, 3):
        a = rng.uniform(-np.pi, np.pi) / 2
        qpos[e, 3:7] = [np.cos(a) * c, np.cos(a) * c, np.sin(a) * c, np.sin(a) * c]      # heading a about z after 90 degrees about x
        qpos[e, 2] = rng.uniform(0.12, 0.2)
        qpos[e, 7:] = STD["qpos"][7:] + rng.normal(size=69) * 0.05
        qvel[e] *= 0.2
    return qpos, qvel, rng.normal(size=(n, 75)) * 0.1


def _run(kp, n, scene, steps, **opts):
    """everything get() returns for a floor scene, plus diag(), after `steps` control steps"""
    qpos, qvel, act = scene
    sim = kp.KpSim(kp.KpModel(**opts), n)
    sim.set_state(dev(qpos[:n]), dev(qvel[:n])); sim.set_target(dev(np.tile(STD["qpos"], (n, 1))))
    a = dev(act[:n])
    for _ in range(steps):
        sim.step_ctrl(a, 15)
    out = {k: sim.get(k).cpu().numpy() for k in kp.FIELDS if not k.startswith("obj_")}      # a floor scene has no object rows
    out["diag"] = sim.diag()
    return out, sim


def _same_words(a, b):
    return [k for k in a if not np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k])]


@pytest.fixture(scope="module")
def scene():
    return _scene(N, 91)


@pytest.fixture(scope="module")
def per_env(kp, scene):
    """the reference of both schedule tests: one workgroup per env"""
    out, sim = _run(kp, N, scene, 3, substeps_per_job=0)
    maxcon = out["diag"][:, 3] & 255
    print("envs above 8 contacts:", int((maxcon > 8).sum()), "max contacts", int(maxcon.max()))
    # what the overflow case needs of the scene: at least one env beyond the lowered limit of 8 contacts (and most within it)
    assert (maxcon > 8).sum() >= 1 and (maxcon <= 8).sum() >= N // 2 and (out["diag"][:, 2] & 255).max() == 0
    return out


@pytest.mark.parametrize("overflow", [False, True], ids=["lean", "lean+overflow"])
def test_launch_forms_agree_word_for_word(kp, scene, per_env, overflow):
    """128 envs on 24 wave slots, 3 control steps: the lean job queue (with lean_max_contacts = 8: the lying envs' jobs go through kp_step_overflow_kernel), the
    full-layout job queue and one workgroup per env."""
    extra = dict(lean_max_contacts=8, lean_adaptive=0) if overflow else {}
    lean, sim = _run(kp, N, scene, 3, lean_queue=1, queue_slots=24, **extra)
    c = sim.queue_counters()
    assert c["lean_layout_next_launch"], c
    assert (c["lean_overflow_jobs"] >= 1) if overflow else (c["lean_overflow_jobs"] == 0), c
    assert int(sim.status_tensor()[2]) == 0
    full, fsim = _run(kp, N, scene, 3, lean_queue=0, queue_slots=24)
    assert not fsim.queue_counters()["lean_layout_next_launch"]
    assert _same_words(lean, full) == []
    assert _same_words(lean, per_env) == []


def test_profiled_handle_reports_every_env_and_leaves_the_states(kp, scene, monkeypatch):
    """64 envs, 2 control steps under KP_PROFILE=1 (the profiling instantiation of the one-workgroup-per-env kernel): every env reports cycles for the control step,
    its phases sum to at most that total, and the states are those of the unprofiled handle."""
    n = 64
    plain, _ = _run(kp, n, scene, 2)
    monkeypatch.setenv("KP_PROFILE", "1")
    prof, sim = _run(kp, n, scene, 2)
    pe = sim.phase_cycles_env()
    monkeypatch.delenv("KP_PROFILE")
    assert pe.shape == (n, 8)
    assert (pe[:, 7] > 0).all() and (pe[:, :7].sum(1) > 0).all(), "every env reports non-zero cycles"
    assert (pe[:, :7].sum(1) <= pe[:, 7]).all()
    mean = sim.phase_cycles()
    assert mean["total"] > 0 and abs(mean["total"] - pe[:, 7].mean()) <= 1e-9 * mean["total"]
    assert _same_words(prof, plain) == []
    with pytest.raises(kp.KinPolyNativeError, match="KP_PROFILE=1"):
        kp.KpSim(kp.KpModel(), 8).phase_cycles()
